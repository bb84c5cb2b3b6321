"""CPU: the reference and the known-answer constructions of the bf16 producer backward (tests/mlp_bf16_bwd_ref.py) check
themselves — every construction passes its own exactness conditions and equals the contract evaluated in float64, PyTorch's CPU
bf16 autograd of the stacked form lies inside the envelope (a second summation order), and each emulated kernel defect changes
an exact answer."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_bf16_bwd_ref as BR
import mlp_bf16_ref as R

IDS = [f"{T}x{E}x{len(layers)}" for T, E, layers in BR.SHAPES]


@functools.lru_cache(maxsize=None)
def case_of(kind, idx):
    T, E, layers = BR.SHAPES[idx]
    return BR.KINDS[kind][0](T, E, layers, BR.seed_of(T, E))


def same(a, b):
    return all(np.array_equal(x, y) for (_, x), (_, y) in zip(BR.bits_of(a), BR.bits_of(b)))


@pytest.mark.parametrize("kind", sorted(BR.KINDS))
@pytest.mark.parametrize("idx", range(len(BR.SHAPES)), ids=IDS)
def test_known_answers_pass_their_checks_and_equal_the_contract(kind, idx):
    case = case_of(kind, idx)
    BR.KINDS[kind][1](case)
    assert same(BR.contract(case.X, case.params, case.dYs), case.answers)


def test_round_once_case():
    case = BR.make_round_once(63)
    BR.check_linear(case)
    assert case.answers["dX"][61, 0] == 256.0
    assert same(BR.contract(case.X, case.params, case.dYs), case.answers)


def test_dy_reaches_every_tile_of_at_least_one_shape():
    assert BR.check_linear(case_of("linear", 1)) and BR.check_select(case_of("select", 1))  # 257 tokens: nine tiles


def test_shapes_cover_the_kernels_boundaries():
    Ts = {T for T, _, _ in BR.SHAPES}
    assert 31 in Ts and 8 * 32 + 1 in Ts and 16 * 8 * 32 + 1 in Ts and {4088 * 32, 4088 * 32 + 1} <= Ts
    assert {8, 24, 32} <= {E for _, E, _ in BR.SHAPES}
    assert {5, 32, 33, 128} <= {h for _, _, l in BR.SHAPES for h, _ in l}
    assert {1, 15, 16, 17, 32} <= {O for _, _, l in BR.SHAPES for _, O in l}
    assert {1, 15, 32} <= {len(l) for _, _, l in BR.SHAPES}


def stacked_autograd(X, params, dYs):
    """PyTorch's CPU bf16 autograd of the stacked form: one Linear(E, sum h), GELU, one Linear per MLP on its slice."""
    bf = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16)
    x = bf(X).requires_grad_(True)
    ps = [[bf(p).requires_grad_(True) for p in mlp] for mlp in params]
    hidden = F.gelu(F.linear(x, torch.cat([p[0] for p in ps], 0), torch.cat([p[1] for p in ps], 0)))
    parts = hidden.split([p[0].shape[0] for p in ps], dim=-1)
    ys = [F.linear(part, p[2], p[3]) for part, p in zip(parts, ps)]
    torch.autograd.backward(ys, [bf(dy) for dy in dYs])
    val = lambda t: t.grad.float().numpy().astype(np.float64)
    return {"dX": val(x), "grads": [tuple(val(t) for t in p) for p in ps]}


@pytest.mark.parametrize("T,E,layers", BR.RANDOM, ids=[f"{T}x{E}x{len(l)}" for T, E, l in BR.RANDOM])
def test_torch_bf16_autograd_lies_inside_the_envelope(T, E, layers):
    X = R.random_x(T, E, R.seed_of(T, E))
    params = R.random_params(E, layers, seed=T + 7 * E)
    dYs = BR.random_dys(T, layers, seed=T + 11 * E)
    want, env = BR.ref_bwd(X, params, dYs)
    worst, where = BR.worst_in_envelope(stacked_autograd(X, params, dYs), want, env)
    print(f"{T}x{E}: worst |err| / envelope = {worst:.4f} in {where}")
    assert worst <= 1.0
    # the true gradient is inside it too (the roundings the contract makes are what the envelope is made of)
    assert BR.worst_in_envelope(BR.true_grad(X, params, dYs), want, env)[0] <= 1.0


# defect -> the exact cases it must change: (kind, index into SHAPES) or "round_once"
DEFECT_CASES = {
    "drop_tile": [("linear", 1), ("select", 1)],
    "drop_unit": [("linear", 2), ("select", 2)],
    "db_every_unit": [("linear", 2), ("select", 2)],
    "dx_per_mlp": ["round_once"],
    "skip_last_token": [("linear", 0), ("select", 1), ("linear", 2)],
    "ignore_o16": [("linear", 2), ("select", 2)],
}


def test_at_least_six_defects():
    assert set(DEFECT_CASES) == set(BR.DEFECTS) and len(BR.DEFECTS) >= 6


@pytest.mark.parametrize("defect", BR.DEFECTS)
def test_an_emulated_defect_changes_an_exact_answer(defect):
    for which in DEFECT_CASES[defect]:
        case = BR.make_round_once(63) if which == "round_once" else case_of(*which)
        assert same(BR.contract(case.X, case.params, case.dYs), case.answers)
        assert not same(BR.contract(case.X, case.params, case.dYs, defect=defect), case.answers), f"{defect} goes unnoticed on {which}"
