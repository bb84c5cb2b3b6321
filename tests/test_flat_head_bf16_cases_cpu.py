"""CPU: the known-answer cases of flat_head_bf16_cases.py are what they claim — nothing here touches the library.

Every expectation is recomputed in float64 numpy from the case's operands, is an integer whose partial sums all stay at or below
256, and survives a round trip through bf16 unchanged (numpy's emulation and torch's cast agree); every operand is a bf16 value;
the probes sit where the kernels' documented boundaries are.
"""
import numpy as np
import pytest
import torch

import flat_head_bf16_cases as C


def _is_bf16(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return torch.equal(t.to(torch.bfloat16).float(), t)


def test_the_numpy_round_trip_is_torchs_cast():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.standard_normal(4096) * 100, np.arange(-300, 301), [257.0, 258.0, 259.0, 0.0, -0.0, 1e-30, 3.0e38]])
    want = torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).double().numpy()
    assert np.array_equal(C.bf16_round_trip(a), want)
    assert C.bf16_round_trip(np.array([257.0]))[0] == 256.0 and C.bf16_round_trip(np.array([259.0]))[0] == 260.0  # 8 bits
    with pytest.raises(AssertionError):
        C.as_bf16(np.array([257.0]))
    with pytest.raises(AssertionError):
        C.as_bf16(np.array([0.5]))


@pytest.mark.parametrize("case", C.FWD, ids=lambda c: c.id)
def test_forward_case_is_exact_in_bf16(case):
    x, w, b = case.x(), case.w(), case.b()
    assert x.shape == (case.B, case.K) and w.shape == (case.J, case.K) and case.K % 4 == 0 and 1 <= case.J <= 8
    assert all(_is_bf16(a) for a in (x, w)) and (b is None or _is_bf16(b))
    assert case.bound() <= C.LIMIT
    want = x.astype(np.float64) @ w.astype(np.float64).T + (0 if b is None else b.astype(np.float64))
    got = case.expected()
    assert np.array_equal(got, want)
    assert np.array_equal(C.bf16_round_trip(got), got) and _is_bf16(C.as_bf16(got))
    if case.kind == "probe":
        pos = case.positions()
        assert case.B == len(pos) and pos[0] == 0 and pos[-1] == case.K - 1
        for r, p in enumerate(pos):
            assert np.count_nonzero(x[r]) == 1 and abs(x[r, p]) in (1.0, 2.0) and np.all(w[:, p] != 0)
        # every output is its one product (plus the bias): a probe read elsewhere, dropped or doubled gives another integer
        assert np.all(got - (0 if b is None else b) != 0)
    else:
        assert np.all(np.count_nonzero(x, axis=1) == case.nnz)


def test_forward_probes_reach_every_boundary():
    reached = set()
    for case in C.FWD:
        if case.kind == "probe":
            reached.update(case.positions())
    for edge in C.FWD_BOUNDARIES:
        assert {edge - 1, edge} <= reached, edge
    assert C.FWD_BOUNDARIES == (4, 1024, 4096)
    ks = {c.K for c in C.FWD}
    assert any(k % 1024 for k in ks) and any(k > 4096 and k % 4096 for k in ks)       # ragged last chunks of both lengths
    assert any(c.B % 8 for c in C.FWD) and any(not c.bias for c in C.FWD) and {1, 3, 8} <= {c.J for c in C.FWD}


@pytest.mark.parametrize("case", C.BWD, ids=lambda c: c.id)
def test_backward_case_is_exact_in_bf16(case):
    dy, x, w = case.dy(), case.x(), case.w()
    assert dy.shape == (case.B, case.J) and x.shape == (case.B, case.K) and w.shape == (case.J, case.K)
    assert case.K % 4 == 0 and 1 <= case.J <= 16 and 1 <= case.B <= 1024 and (case.want_dx or case.want_dw)
    assert all(_is_bf16(a) for a in (dy, x, w))
    assert case.bound() <= C.LIMIT
    dX, dW = case.expected()
    assert np.array_equal(dX, dy.astype(np.float64) @ w.astype(np.float64))
    assert np.array_equal(dW, dy.astype(np.float64).T @ x.astype(np.float64))
    for a in (dX, dW):
        assert np.array_equal(C.bf16_round_trip(a), a) and _is_bf16(C.as_bf16(a))
    if case.kind == "probe":
        pos = case.positions()
        assert case.B == len(pos) and pos[0] == 0 and pos[-1] == case.K - 1
        for r, p in enumerate(pos):
            assert np.count_nonzero(x[r]) == 1 and np.count_nonzero(dy[r]) == 1
            j = int(np.flatnonzero(dy[r])[0])
            assert dW[j, p] == float(dy[r, j]) * float(x[r, p]) != 0     # the one product, at the probe and nowhere else
            assert np.all(dX[r, list(pos)] != 0)                          # dX at every boundary column is a nonzero product
        assert np.count_nonzero(dW) == len(pos)


def test_backward_probes_reach_every_boundary():
    reached = set()
    for case in C.BWD:
        if case.kind == "probe":
            reached.update(case.positions())
    for edge in C.BWD_BOUNDARIES:
        assert {edge - 1, edge} <= reached, edge
    assert C.BWD_BOUNDARIES == (4, 256)
    assert any(c.want_dx and not c.want_dw for c in C.BWD) and any(c.want_dw and not c.want_dx for c in C.BWD)
    assert any(c.B % 8 for c in C.BWD) and any(c.B > 8 for c in C.BWD) and {1, 16} <= {c.J for c in C.BWD}
    assert any(c.K % 256 for c in C.BWD)
