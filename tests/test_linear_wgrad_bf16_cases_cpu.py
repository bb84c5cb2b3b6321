"""CPU: the known-answer cases of linear_wgrad_bf16_cases.py are what they claim to be — checked against a second evaluation
(int64 / float64 sums, torch's own float32 -> bfloat16 conversion for the rounding) before any GPU test relies on them."""
import numpy as np
import pytest
import torch

import linear_wgrad_bf16_cases as C


def _torch_rne(a64: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.asarray(a64, np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float32).numpy()


def _is_bf16(a) -> bool:
    a = np.asarray(a, np.float32)
    return bool(np.all(a.view(np.uint32) & 0xFFFF == 0))


def test_rne_bf16_rounds_to_nearest_even():
    vals = np.array([256, 257, 258, 259, 260, 261, 300, 511, 513, 1023, 16384, -257, -259, 0.5, 3.0], np.float64)
    assert np.array_equal(C.rne_bf16(vals), _torch_rne(vals))
    assert list(C.rne_bf16(np.array([257.0, 259.0, 261.0, -257.0]))) == [256.0, 260.0, 260.0, -256.0]


def test_plan_cuts_whole_tiles():
    for T, m, n in ((1, 1, 1), (33, 32, 32), (4096, 128, 128), (70001, 32, 32), (70001, 128, 128), (40 * 16384, 32, 32)):
        p = C.plan(T, m, n)
        assert p["rows_per_wave"] % C.TILE_ROWS == 0 and p["rows_per_wave"] >= C.TILE_ROWS
        assert (p["nwaves"] - 1) * p["rows_per_wave"] < T <= p["nwaves"] * p["rows_per_wave"]
        assert p["nparts"] == -(-p["nwaves"] // 4) and p["workspace_bytes"] <= (32 << 20) + 4 * p["nparts"] * 128
    assert C.plan(70001, 32, 32)["rows_per_wave"] == 32 and C.plan(70001, 128, 128)["rows_per_wave"] == 64


@pytest.mark.parametrize("shape", C.PROBE_SHAPES, ids=str)
def test_probes_cover_the_edges(shape):
    T, m, n = shape
    ps = list(C.probes(T, m, n))
    rpw = C.plan(T, m, n)["rows_per_wave"]
    assert {p.t for p in ps} >= {0, 7, 8, 15, 16, T - 1, rpw, 2 * rpw - 1}
    assert {p.i for p in ps} == set(C.tile_corners(m)) and {p.j for p in ps} == set(C.tile_corners(n))
    assert len(ps) == len({(p.t, p.i, p.j) for p in ps})
    for p in ps[:: max(1, len(ps) // 16)]:
        x, dy = p.x().astype(np.float64), p.dy().astype(np.float64)
        assert np.count_nonzero(x) == 1 and np.count_nonzero(dy) == 1
        dWt, db = p.expected()
        assert np.array_equal(dWt, dy.T @ x) and np.array_equal(db, dy.sum(0)) and _is_bf16(dWt) and _is_bf16(db)


@pytest.mark.parametrize("case", C.DENSE, ids=lambda c: c.id)
def test_dense_cases_are_exact_in_any_order(case):
    x, dy = case.x(), case.dy()
    assert case.T <= 4096 and x.shape == (case.T, case.m) and dy.shape == (case.T, case.n)
    assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(dy)) <= {-2, -1, 0, 1, 2}
    assert float((np.abs(dy).T.astype(np.float64) @ np.abs(x).astype(np.float64)).max()) < 2 ** 24  # every partial sum is exact in f32
    exact_W, exact_b = dy.astype(np.float64).T @ x.astype(np.float64), dy.astype(np.float64).sum(0)
    iW, ib = case.exact()
    assert np.array_equal(iW, exact_W) and np.array_equal(ib, exact_b)
    dWt, db = case.expected()
    assert np.array_equal(dWt, _torch_rne(exact_W)) and np.array_equal(db, _torch_rne(exact_b)) and _is_bf16(dWt) and _is_bf16(db)


def test_dense_cases_exercise_the_rounding():
    inexact = [c.id for c in C.DENSE if not np.array_equal(c.expected()[0].astype(np.float64), c.exact()[0].astype(np.float64))]
    assert len(inexact) >= 3, inexact  # sums that are no bf16 values: the store rounds
    ties = 0
    for c in C.DENSE:
        if c.kind == "tie":
            a = np.abs(c.exact()[0]).astype(np.int64)
            step = 2 ** (np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) - 7)  # spacing of bf16 at a
            ties += int(((step >= 2) & (a % step == step // 2)).sum())
            assert {257, 259, 261} <= set(np.unique(a)) and {256.0, 260.0} <= set(np.unique(c.expected()[0]))
    assert ties > 0


@pytest.mark.parametrize("case", C.AFFINE, ids=lambda c: c.id)
def test_affine_cases_are_exact(case):
    x, w, b = case.x(), case.w(), case.b()
    assert 1 <= case.K <= 3 and x.shape == (case.T, case.K) and w.shape == (case.E, case.K) and case.E % 8 == 0
    assert _is_bf16(x) and _is_bf16(w) and (b is None or _is_bf16(b))
    ref = x.astype(np.float64) @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
    want = case.expected()
    assert np.array_equal(want.astype(np.float64), ref) and _is_bf16(want)  # exact: no rounding anywhere on the way
    assert not np.any(np.signbit(want) & (want == 0))
    if case.kind == "ints":
        bound = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T + (0.0 if b is None else np.abs(b))
        assert float(bound.max()) <= 256


def test_affine_cases_cover_k_and_bias():
    assert {(c.K, c.bias) for c in C.AFFINE} >= {(K, b) for K in (1, 2, 3) for b in (True, False)}
    assert {c.E for c in C.AFFINE} >= {8, 1024}
