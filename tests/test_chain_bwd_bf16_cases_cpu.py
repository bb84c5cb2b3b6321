"""CPU self-tests of the cases of test_gpu_chain_bwd_lds_bf16.py (tests/chain_bwd_bf16_cases.py).

Without a GPU they show three things. Reach: the lists hold every (L, G, RES) instance and the limits they are there for,
computed from the rules bwd_chain_lds_bf16.h documents. Agreement: the documented contract, restated in numpy float32
(plain_backward_bf16), gives the dV0 bits of the stepwise oracle recipe — oc.spmul_bwd per step on the widened operands, every g
rounded to bf16 (be.rne_bits) before the next step reads it, the residual terms summed in f32 and rounded once — on every case,
and for C = 8 the dW bits of bf16_rne(oracle dW). (At C = 16 the contract's dW is the rounded sum of two 8-channel partials,
which the oracle's one running sum is not: variant (c) below.) Sensitivity: each of three wrong variants changes bits on at
least one listed case it applies to — so the GPU comparison can see those mistakes.
"""
import numpy as np
import pytest

import bf16_edges as be
import chain_bwd_bf16_cases as cb
from oracle import chord_oracle as oc

NORMAL = [c for c in sorted(set(cb.ONE_LAUNCH), key=cb.ONE_LAUNCH.index) if c not in cb.SPECIAL or c == cb.GRAPH]


def test_grid_holds_every_instance():
    want = {(L, G, res) for L in range(2, 21) for G in (1, 2) for res in (False, True)}
    assert len(want) == 76
    assert {cb.instance(c) for c in cb.GRID} == want and len(cb.GRID) == 76
    for B, N, M, L, C, _res, off in cb.GRID:
        assert (B, N, M, off) == (2, 67, 2, None) and C in (8, 16) and cb.covered(N, L, C, M)
    assert -(-67 // 64) == 2 and 2 * 64 - 67 == 61  # two waves, 61 idle lanes


def test_the_shape_rule():
    assert cb.covered(1024, 20, 16, 64) and cb.covered(1, 2, 8, 1) and cb.covered(128, 8, 8, 14)
    for N, L, C, M in ((1025, 8, 8, 2), (128, 8, 4, 2), (128, 8, 12, 2), (128, 8, 24, 2), (128, 1, 8, 2), (128, 21, 8, 2), (128, 8, 8, 0),
                       (128, 8, 8, 65), (0, 8, 8, 2)):
        assert not cb.covered(N, L, C, M), (N, L, C, M)
    assert all(cb.covered(c[1], c[3], c[4], c[2]) for c in cb.ONE_LAUNCH)
    assert [cb.covered(c[1], c[3], c[4], c[2]) for c in cb.DECLINED] == [False, False]
    assert cb.DECLINED[0][1] == 1025 and cb.DECLINED[1][4] == 12
    assert not cb.covered(*(cb.AUTOGRAD_FALLBACK[i] for i in (1, 3, 4, 2))) and cb.AUTOGRAD_FALLBACK[1] == 1025
    assert [s for s in cb.AUTOGRAD] == [(2, 128, 14, 8, 8), (2, 1024, 5, 11, 16)]
    assert all(cb.covered(N, L, C, M) for _B, N, M, L, C in cb.AUTOGRAD)


def test_limit_list_reaches_what_it_claims():
    lim = cb.LIMITS
    assert len(lim) == 12
    # the dynamic-LDS maximum: N = 1024, L = 20 at C = 16 — the f32 kernel's footprint at the same G
    top = [c for c in lim if c[1] == 1024 and c[3] == 20 and c[4] == 16]
    assert top and cb.lds_bytes(top[0]) == 2 * 2 * 1024 * 16 + 1024 * 21 * 4 == 151552 <= 160 * 1024
    assert max(cb.lds_bytes(c) for c in cb.ONE_LAUNCH) == 151552
    assert any(c[4] == 8 and cb.lds_bytes(c) > cb.LDS_FREE for c in lim)  # G = 1 beyond 48 KB
    assert any(c[2] == cb.MAX_STEPS == 64 for c in lim)
    assert {c[1] for c in lim} >= {1, 2, 3, 63, 64, 65, 1023, 1024}
    assert any(c[1] == 64 and c[3] == 20 and cb.offsets_of(c).count(0) == 14 for c in lim)
    explicit = [c for c in lim if c[6] is not None]
    assert explicit and cb.offsets_of(explicit[0]) == [0, 5, 255, 44, 255, 128]
    assert {c[5] for c in lim} == {False, True} and {c[4] for c in lim} == {8, 16}


def test_the_raise_happens_between_launches_of_one_instance():
    a, b, c = cb.RAISE_BETWEEN
    assert cb.instance(a) == cb.instance(b) == cb.instance(c) and a == c
    assert cb.lds_bytes(a) <= cb.LDS_FREE < cb.lds_bytes(b)


def test_the_other_lists():
    assert {c[:5] for c in cb.BANDS} == {(2, 67, 3, 5, 8), (2, 1024, 2, 11, 16), (3, 130, 2, 20, 8)} and len(cb.BANDS) == 6
    assert {c[3] % 2 for c in cb.BANDS} == {0, 1} and cb.W_SHIFTS == (0, 1, 3)  # odd and even L; shifts off the dword too
    assert cb.STALE == [(2, 37, 4, 5, 8, True, None), (2, 100, 3, 7, 16, True, None), (5, 777, 3, 10, 8, False, None)]
    assert cb.lds_bytes(cb.STALE_FIRST) == 151552
    assert cb.SPECIAL == [(2, 128, 3, 8, 8, False, None), (2, 128, 3, 8, 8, True, None)] and cb.GRAPH == (2, 128, 3, 8, 8, True, None)
    # the per-step route the GPU tests compare with sums at most 32 residual terms of a multiple of 8 elements: only the
    # two M = 64 residual cases are beyond it
    beyond = [c for c in cb.ONE_LAUNCH if c[5] and (c[2] + 1 > 32 or (c[0] * c[1] * c[4]) % 8)]
    assert sorted(set(beyond)) == sorted({(1, 1024, 64, 2, 8, True, None), (2, 65, 64, 5, 16, True, None)})


def _oracle_recipe(case):
    """(dV0 bits, [oracle dW_m in f32]) stepwise: oc.spmul_bwd on the widened operands, every g rounded before the next step."""
    _B, _N, M, _L, _C, res, off = case
    W, _V0, dOut, X = cb.problem(case)
    g, terms, dW = np.array(dOut), [], [None] * M
    for m in range(M - 1, -1, -1):
        terms.append(g)
        dW[m], dv = oc.spmul_bwd(g, np.array(W[m]), np.array(X[m]), off)
        g = be.as_bf16(dv)
    if res:
        acc = terms[0]
        for t in terms[1:] + [g]:
            acc = (acc + t).astype(np.float32)
        g = acc
    return be.rne_bits(g), dW


@pytest.mark.parametrize("case", NORMAL, ids=cb.case_id)
def test_contract_has_the_stepwise_oracle_bits(case):
    W, V0, dOut, X = cb.problem(case)
    for a in (*W, V0, dOut, *X):  # bf16 values, finite
        assert np.isfinite(a).all() and np.array_equal(be.as_bf16(a), a)
    dV0, dW = cb.plain_backward_bf16(case)
    want_dV0, oracle_dW = _oracle_recipe(case)
    assert np.isfinite(be.bits_f32(dV0)).all()
    assert np.array_equal(dV0, want_dV0), "dV0"
    if case[4] == 8:
        for m, (a, b) in enumerate(zip(dW, oracle_dW)):
            assert np.array_equal(a, be.rne_bits(b)), f"dW_{m}"


def _changed(case, variant):
    dV0, dW = cb.plain_backward_bf16(case)
    v_dV0, v_dW = cb.plain_backward_bf16(case, variant)
    return not np.array_equal(dV0, v_dV0) or any(not np.array_equal(a, b) for a, b in zip(dW, v_dW))


@pytest.mark.parametrize("variant", cb.VARIANTS)
def test_each_wrong_variant_shows_on_a_listed_case(variant):
    cases = [c for c in NORMAL if cb.applies(variant, c)]
    assert len(cases) >= 10
    shown = [c for c in cases if _changed(c, variant)]
    assert shown, f"{variant} leaves every bit of every case as it was"
    # (g_kept_f32 and residual_bf16_adds show on every case they apply to. An f32 difference in the last place survives the
    # rounding to bf16 about once in 2^16 elements: dw_one_running_sum shows on one of its 46 cases, the largest, and the GPU
    # test's other reference, the per-step route, computes the two-partial sum itself)
    if variant != "dw_one_running_sum":
        assert shown == cases
    for c in NORMAL:
        if not cb.applies(variant, c):
            assert not _changed(c, variant), (variant, c)


def test_the_one_16_channel_sum_is_the_oracles_and_not_the_contracts():
    """Variant (c) restated: at C = 16 the oracle's running sum over all channels equals variant dw_one_running_sum, bit for
    bit — the kernel's two-partial sum is what the per-step bf16 kernels compute instead."""
    case = (2, 67, 2, 9, 16, True, None)
    assert case in cb.GRID
    W, _V0, dOut, X = cb.problem(case)
    M = case[2]
    oracle_last, _dv = oc.spmul_bwd(np.array(dOut), np.array(W[M - 1]), np.array(X[M - 1]), None)
    _dV0, v_dW = cb.plain_backward_bf16(case, "dw_one_running_sum")
    assert np.array_equal(v_dW[M - 1], be.rne_bits(oracle_last))
