"""CPU self-tests of the cases of test_gpu_chain_bwd_lds.py (tests/chain_bwd_cases.py).

Without a GPU they show three things. Reach: the lists hold every (L, G = 1, RES) instance and the limits they are there for,
computed from the rules bwd_chain_lds.h documents. Agreement: the kernel's documented order, restated in plain numpy float32
(plain_backward), has the oracle's bits on every case — so "the oracle's bits" is the right verdict for this kernel, dW
included. Sensitivity: seven emulated defects each change dV0 or some dW_m, in bits, in every case they apply to — so a kernel
with one of them cannot pass.
"""
import numpy as np
import pytest

import chain_bwd_cases as cc

NORMAL = sorted(set(cc.ONE_LAUNCH), key=cc.ONE_LAUNCH.index)  # every one-launch case on normal operands, once


def test_grid_holds_every_instance_of_one_channel_group():
    want = {(L, 1, res) for L in range(2, 21) for res in (False, True)}
    assert len(want) == 38
    assert {cc.instance(c) for c in cc.GRID} == want and len(cc.GRID) == 38
    for c in cc.GRID:
        B, N, M, _L, C, _res, off = c
        assert (B, N, M, C, off) == (2, 67, 2, 4, None) and cc.covered(c)
    assert -(-67 // 64) == 2 and 2 * 64 - 67 == 61  # two waves, 61 idle lanes


def test_limit_list_reaches_what_it_claims():
    lim = cc.LIMITS
    assert len(lim) == 12 and all(cc.covered(c) for c in cc.ONE_LAUNCH)
    # the dynamic-LDS maximum: N = 1024, L = 20 at C = 8
    top = [c for c in lim if c[1] == 1024 and c[3] == 20 and c[4] == 8]
    assert top and cc.lds_bytes(top[0]) == 2 * 2 * 1024 * 16 + 1024 * 21 * 4 == 151552
    assert max(cc.lds_bytes(c) for c in cc.ONE_LAUNCH) == 151552
    # a C = 4 launch beyond 48 KB: N (L | 1) > 4096
    assert any(c[4] == 4 and c[1] * (c[3] | 1) > 4096 and cc.lds_bytes(c) > cc.LDS_FREE for c in lim)
    assert all(cc.lds_bytes(c) <= cc.LDS_FREE for c in cc.GRID)
    assert any(c[2] == cc.MAX_STEPS == 64 for c in lim)
    assert {c[1] for c in lim} >= {1, 2, 3, 63, 64, 65, 1023, 1024}
    # offsets that repeat mod N: 14 self links at N = 64, L = 20
    assert any(c[1] == 64 and c[3] == 20 and cc.offsets_of(c).count(0) == 14 for c in lim)
    explicit = [c for c in lim if c[6] is not None]
    assert explicit and any(min(c[6]) < 0 and max(c[6]) >= c[1] for c in explicit)
    assert cc.offsets_of(explicit[0]) == [0, 5, 255, 44, 255, 128]
    assert {c[5] for c in lim} == {False, True} and {c[4] for c in lim} == {4, 8}


def test_the_raise_happens_between_launches_of_one_instance():
    a, b, c = cc.RAISE_BETWEEN
    assert cc.instance(a) == cc.instance(b) == cc.instance(c) and a[4] == 4
    assert cc.lds_bytes(a) <= cc.LDS_FREE < cc.lds_bytes(b) and a == c


def test_the_other_lists_are_what_the_entry_documents():
    assert [cc.covered(c) for c in cc.LIBRARY_STEPS] == [False] * 4 and not cc.covered(cc.UNSUPPORTED)
    # N, C, L and M each leave the kernel's range once
    assert [c[1] > cc.ROWS for c in cc.LIBRARY_STEPS] == [True, False, False, False]
    assert [c[4] not in (4, 8) for c in cc.LIBRARY_STEPS] == [False, True, False, False]
    assert [c[3] > cc.L_MAX for c in cc.LIBRARY_STEPS] == [False, False, True, False]
    assert [c[2] > cc.MAX_STEPS for c in cc.LIBRARY_STEPS] == [False, False, False, True]
    # the residual sum inside the library takes at most 32 terms of a multiple of 4 elements
    for B, N, M, _L, C, res, _off in cc.LIBRARY_STEPS:
        assert not res or (M + 1 <= 32 and (B * N * C) % 4 == 0)
    assert cc.UNSUPPORTED[5] and cc.UNSUPPORTED[2] + 1 > 32
    assert {c[:5] for c in cc.BANDS} == {(2, 67, 3, 5, 8), (2, 1024, 2, 11, 4), (3, 130, 2, 20, 8)} and len(cc.BANDS) == 6
    assert cc.WIDE[0] * cc.WIDE_COPIES == 600 > 256  # more workgroups than the 256 CUs


@pytest.mark.parametrize("case", NORMAL, ids=cc.case_id)
def test_documented_order_has_the_oracles_bits_and_every_defect_shows(case):
    _W, _V0, _dOut, _X, want_dV0, want_dW = cc.problem(case)
    assert np.isfinite(want_dV0).all() and all(np.isfinite(d).all() for d in want_dW)
    dV0, dW = cc.plain_backward(case)
    assert cc.same_bits(dV0, want_dV0), "dV0"
    for m, (a, b) in enumerate(zip(dW, want_dW)):
        assert cc.same_bits(a, b), f"dW_{m}"
    for defect in cc.DEFECTS:
        if not cc.applies(defect, case):
            continue
        dV0, dW = cc.plain_backward(case, defect)
        changed = not cc.same_bits(dV0, want_dV0) or any(not cc.same_bits(a, b) for a, b in zip(dW, want_dW))
        assert changed, f"{defect} leaves every bit of dV0 and dW as it was"


def test_defects_apply_everywhere_but_where_stated():
    """Which cases a defect cannot apply to: N = 1 and N = 2 for the offset's sign, N = 1 for the wrap, M = 1 or no residual for
    the order of the residual sum, M = 1 for the contracted product (bf16 x bf16 is exact)."""
    for case in NORMAL:
        _B, N, M, _L, _C, res, _off = case
        want = {"plus_offset": N > 2, "no_wrap": N > 1, "last_link_dropped": True, "dw_next_x": True, "dw_leaving_gradient": True,
                "reverse_residual_sum": res and M >= 2, "dw_contracted": M >= 2}
        assert {d: cc.applies(d, case) for d in cc.DEFECTS} == want, case


def test_same_bits_tells_the_sign_of_zero_and_a_last_bit():
    one = np.array([1.0, 0.0], dtype=np.float32)
    assert cc.same_bits(one, one.copy())
    assert not cc.same_bits(one, np.array([1.0, -0.0], dtype=np.float32))
    assert not cc.same_bits(one, np.array([np.nextafter(np.float32(1), np.float32(2)), 0.0], dtype=np.float32))
