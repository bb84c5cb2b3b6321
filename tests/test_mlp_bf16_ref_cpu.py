"""CPU: the reference of the fused bf16 producer tests (tests/mlp_bf16_ref.py) checked on its own — against torch's CPU bf16
modules, an independent summation order, and against the closed-form answers of its two known-answer constructions."""
import numpy as np
import pytest
import torch
from torch import nn

import mlp_bf16_ref as R


def test_bf16_rounding_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e-39, 65280.0, 3.4e38, 0.0, -0.0])
    assert np.array_equal(R.bf16_rne(v)[:3], [1.0, 1.0, 1.015625])  # ties go to the even neighbour
    assert np.isinf(R.bf16_rne(np.array([3.4e38])))[0] and np.isnan(R.bf16_rne(np.array([np.nan])))[0]
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy().astype(np.float64)  # (f32 inputs: torch rounds once too)
    assert np.array_equal(R.bf16_rne(x.astype(np.float64)), want)
    bits = np.arange(0x0080, 0x7F80, 37, dtype=np.uint16)
    assert np.array_equal(R.to_bits(R.from_bits(bits)), bits)
    assert np.array_equal(R.ulp_bf16(np.array([1.0, 1.5, 2.0, 255.0])), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0])
    assert np.array_equal(R.plus_zero(np.array([0x8000, 0x0000, 0x8001], np.uint16)), [0, 0, 0x8001])


@pytest.mark.parametrize("T,E,h,O", R.TORCH_SHAPES)
def test_ref_against_torch_cpu_bf16_modules(T, E, h, O):
    X = R.random_x(T, E, R.seed_of(T, E))
    (A, a, B, b), = R.random_params(E, [(h, O)], seed=T + h)
    net = nn.Sequential(nn.Linear(E, h), nn.GELU(), nn.Linear(h, O)).bfloat16()
    with torch.no_grad():
        for p, v in zip((net[0].weight, net[0].bias, net[2].weight, net[2].bias), (A, a, B, b)):
            p.copy_(torch.from_numpy(v))
        got = net(torch.from_numpy(X).to(torch.bfloat16)).double().numpy()
    _, _, y, dy = R.ref(X, A, a, B, b)
    R.assert_close(got, y, dy, f"torch cpu bf16 {T}x{E}x{h}x{O}")


def test_the_envelope_rejects_real_defects():
    T, E, h, O = 300, 32, 33, 15
    X = R.random_x(T, E, 1)
    (A, a, B, b), = R.random_params(E, [(h, O)], seed=2)
    _, _, y, dy = R.ref(X, A, a, B, b)
    for what, bad in (("a dropped bias", R.ref(X, A, np.zeros(h), B, b)[2]),
                      ("a missing k-step", R.ref(np.where(np.arange(E) < 16, X, 0.0), A, a, B, b)[2]),
                      ("a swapped pair of hidden rows", R.ref(X, A, a, B[:, np.r_[1, 0, 2:h]], b)[2])):
        worst, share = R.compare(bad, y, dy)
        assert worst > 1.0 and share > R.MAX_DIFFERING, what


@pytest.mark.parametrize("kind", sorted(R.KINDS))
@pytest.mark.parametrize("T,E,layers", R.SHAPES, ids=[f"{T}x{E}" for T, E, _ in R.SHAPES])
def test_known_answer_constructions_are_exact(kind, T, E, layers):
    make, check = R.KINDS[kind]
    X, params, answers = make(T, E, layers, R.seed_of(T, E))
    check(X, params, answers)  # grid and partial-sum bounds / tie margins
    assert X.shape == (T, E) and len(params) == len(layers)
    seen = set()
    for (A, a, B, b), want, (h, O) in zip(params, answers, layers):
        assert A.shape == (h, E) and B.shape == (O, h) and want.shape == (T, O)
        for t in (X, A, a, B, b, want):
            R.to_bits(t)  # every operand and every answer is a bf16 value
        key = (A.tobytes(), B.tobytes())
        if key in seen:
            continue  # (the shapes repeat their link MLPs' sizes, not their weights — kept for safety)
        seen.add(key)
        _, _, y, _ = R.ref(X, A, a, B, b)
        assert np.array_equal(R.plus_zero(R.to_bits(y)), R.plus_zero(R.to_bits(want)))


def test_select_margin_is_asserted():
    vals = R.select_values()
    assert np.all(R.gelu_margin_ok(vals)) and np.all(np.abs(vals) <= 1.0)
    # a z whose GELU sits on a rounding boundary of h (0.375 + 2^-10: the spacing in [0.25, 0.5) is 2^-9) is refused
    lo, hi = 0.5, 0.6
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if R.gelu64(np.array([mid]))[0] < 0.375 + 2.0 ** -10 else (lo, mid)
    assert not R.gelu_margin_ok(np.array([lo]))[0]
    assert R.gelu_margin_ok(np.array([lo + 1e-4]))[0]  # and one a fifth of the spacing away from it is accepted
