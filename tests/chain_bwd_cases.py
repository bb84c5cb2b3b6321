"""Cases, operands and expected answers for the one-launch backward chain (csrc/bwd_chain_lds.h: chord_chain_bwd_lds_k<L, G, RES>
behind psf_chord_chain_bwd_f32), used by test_gpu_chain_bwd_lds.py and checked without a GPU by test_chain_bwd_cases_cpu.py.

A case is (B, N, M, L, C, residual, offsets); offsets is None (the chord pattern 0, 1, 2, 4, ... mod N) or a tuple of L integers.
Operands are tests/bf16_edges.normal_case: W_m scaled by 0.4 (seed 81 + m), V0 (seed 80) and dOut (seed 79) at 1.0, as in
test_gpu_launch_table._bwd_chain_case. The expected answer is that function's recipe on the CPU oracle: X_m by oc.spmul_fwd
(plus V0 with the residual), gradients by oc.spmul_bwd per step, the residual terms summed ((g_M + g_{M-1}) + ... + g_1) + g_0
in float32. The GPU tests feed X_steps from this CPU forward, so the backward is tested on its own.

``plain_backward`` restates the kernel's documented order in plain numpy float32 (products and sums rounded separately, channels
and links ascending, every accumulator starting at +0) and can emulate seven defects; the CPU test shows that it has the
oracle's bits without a defect and other bits with each one, on every case the defect applies to.

The shape rules below (instance = (L, C / 4, residual); dynamic LDS = 2 G 1024 16 + N (L | 1) 4 bytes; 48 KB raise) are the ones
bwd_chain_lds.h and bwd_chain_lds_inst.hip document. They serve to ASSERT what the lists reach, never to compute an answer.
"""
from __future__ import annotations

import functools

import numpy as np

import bf16_edges as be
from oracle import chord_oracle as oc

ROWS = 1024       # kChainBwdRows: rows a workgroup holds, and the channel-group stride in LDS
MAX_STEPS = 64    # kChainMaxSteps
L_MIN, L_MAX = 2, 20
LDS_FREE = 48 * 1024   # dynamic LDS a kernel may ask for without the launcher raising its limit

# a. every C = 4 instance: two waves, 61 idle lanes
GRID = [(2, 67, 2, L, 4, res, None) for L in range(L_MIN, L_MAX + 1) for res in (False, True)]

# b. limits
LIMITS = [
    (2, 1024, 3, 20, 8, True, None),    # the dynamic-LDS maximum, 151 552 bytes
    (2, 1024, 2, 20, 4, False, None),   # G = 1 beyond 48 KB
    (2, 1023, 2, 19, 8, True, None),    # one idle lane in the last wave
    (1, 1024, 64, 2, 4, True, None),    # M = kChainMaxSteps at the smallest L, all 1024 threads
    (2, 65, 64, 5, 8, True, None),      # M = kChainMaxSteps, two waves with 63 idle lanes
    (3, 1, 1, 2, 4, False, None),       # one row: every link a self link
    (2, 2, 3, 20, 8, True, None),
    (2, 3, 2, 4, 4, True, None),
    (2, 64, 2, 20, 8, True, None),      # 14 duplicate self links (2^k mod 64 = 0 from k = 6 on)
    (2, 63, 1, 7, 8, True, None),
    (2, 63, 1, 7, 8, False, None),
    (2, 256, 3, 6, 4, True, (0, 5, 255, 300, -1, 128)),
]

# the same C = 4 instance below 48 KB, above it, below it again
RAISE_BETWEEN = [(2, 64, 2, 9, 4, True, None), (2, 1024, 2, 9, 4, True, None), (2, 64, 2, 9, 4, True, None)]

# c. bands and alignment (each with and without the residual)
BANDS = [(B, N, M, L, C, res, None) for (B, N, M, L, C) in ((2, 67, 3, 5, 8), (2, 1024, 2, 11, 4), (3, 130, 2, 20, 8)) for res in (False, True)]
W_SHIFTS = (0, 1, 3)   # floats off a 16-byte boundary, W_m and dW_m alike

# d. stale LDS
STALE = [(2, 37, 4, 5, 8, True, None), (2, 100, 3, 7, 4, True, None), (5, 777, 3, 10, 8, False, None)]

# e. special values (operands from test_gpu_parity._special, not from here)
SPECIAL = [(2, 128, 3, 8, 8, False, None), (2, 128, 3, 8, 8, True, None), (2, 300, 2, 9, 4, True, None)]

# f. more workgroups than CUs: three sequences, each repeated 200 times
WIDE = (3, 64, 2, 7, 8, True, None)
WIDE_COPIES = 200

# g. shapes the one launch does not take: the library issues the per-step kernels (needs dX_steps) ...
LIBRARY_STEPS = [(2, 1025, 2, 11, 8, True, None), (2, 100, 2, 9, 12, True, None), (2, 100, 2, 21, 8, False, None),
                 (2, 100, 65, 5, 8, False, None)]
# ... or says PSF_E_UNSUPPORTED: a residual chain of more than 31 steps is beyond psf_sum_tensors_f32
UNSUPPORTED = (2, 100, 65, 5, 8, True, None)

# h. graph capture
GRAPH = (2, 128, 3, 8, 8, True, None)

ONE_LAUNCH = GRID + LIMITS + RAISE_BETWEEN[:2] + BANDS + STALE + [WIDE, GRAPH]


def case_id(case) -> str:
    B, N, M, L, C, res, off = case
    return f"B{B}-N{N}-M{M}-L{L}-C{C}-{'res' if res else 'plain'}{'-offsets' if off is not None else ''}"


# ---------------------------------------------------------------- what a case reaches (documented rules)
def covered(case) -> bool:
    """chain_bwd_lds_fits of bwd_chain_lds_inst.hip."""
    _B, N, M, L, C, _res, _off = case
    return 1 <= N <= ROWS and C in (4, 8) and L_MIN <= L <= L_MAX and 1 <= M <= MAX_STEPS


def instance(case):
    """(L, G, RES) of chord_chain_bwd_lds_k."""
    _B, _N, _M, L, C, res, _off = case
    return L, C // 4, bool(res)


def lds_bytes(case) -> int:
    _B, N, _M, L, C, _res, _off = case
    return 2 * (C // 4) * ROWS * 16 + N * (L | 1) * 4


def offsets_of(case):
    """The L link offsets reduced into [0, N)."""
    _B, N, _M, L, _C, _res, off = case
    if off is None:
        return be.chord_offsets(N, L)
    assert len(off) == L
    return [int(o) % N for o in off]


# ---------------------------------------------------------------- operands and the oracle's answer
def operands(case):
    """(W, V0, dOut): M arrays [B, N, L], and two of [B, N, C]."""
    B, N, M, L, C, _res, _off = case
    return [be.normal_case((B, N, L), 81 + m, 0.4) for m in range(M)], be.normal_case((B, N, C), 80), be.normal_case((B, N, C), 79)


def forward(W, V0, residual, offsets=None):
    """[X_0 = V0, X_1, ..., X_M] by the oracle, stored in float32 after every step."""
    X = [V0]
    for Wm in W:
        nxt = oc.spmul_fwd(Wm, X[-1], offsets)
        X.append((nxt + V0).astype(np.float32) if residual else nxt)
    return X


def oracle_backward(W, X, dOut, residual, offsets=None):
    """(dV0, [dW_0 .. dW_{M-1}]): oc.spmul_bwd per step, the residual terms summed ((g_M + g_{M-1}) + ... + g_1) + g_0."""
    M = len(W)
    g, dW, terms = dOut, [None] * M, []
    for m in range(M - 1, -1, -1):
        terms.append(g)
        dW[m], g = oc.spmul_bwd(g, W[m], X[m], offsets)
    if residual:
        acc = terms[0]
        for t in terms[1:] + [g]:
            acc = (acc + t).astype(np.float32)
        g = acc
    return g, dW


@functools.lru_cache(maxsize=None)
def problem(case):
    """(W, V0, dOut, X, dV0, dW) of a case: computed once, shared, never written to."""
    _B, _N, _M, _L, _C, res, off = case
    W, V0, dOut = operands(case)
    X = forward(W, V0, res, off)
    dV0, dW = oracle_backward(W, X, dOut, res, off)
    for a in (*W, V0, dOut, *X, dV0, *dW):
        a.setflags(write=False)
    return W, V0, dOut, X, dV0, dW


# ---------------------------------------------------------------- the kernel's order in plain numpy, and its defects
DEFECTS = ("plus_offset", "no_wrap", "last_link_dropped", "dw_next_x", "dw_leaving_gradient", "reverse_residual_sum", "dw_contracted")


def applies(defect, case) -> bool:
    """Whether the defect can change anything in the case, from the shape alone.

    plus_offset           dV gathered from p + off: needs a link with off != -off mod N (none at N = 1 and N = 2)
    no_wrap               the source row clamped into [0, N) instead of taken mod N: needs a link with off != 0 (none at N = 1)
    last_link_dropped     always
    dw_next_x             always (X_{m+1} is another array than X_m)
    dw_leaving_gradient   always
    reverse_residual_sum  needs the residual and three or more terms: at M = 1 the sum g_1 + g_0 is commutative
    dw_contracted         needs a dW product that is inexact in f32. The operands are bf16 values, so at the last step
                          (g = dOut, and X_{M-1} = V0 when M = 1) every product of two 8-bit significands is exact and
                          a fused multiply-add returns the same bits: M = 1 cannot show it, M >= 2 (f32 g, f32 X) can
    """
    _B, N, M, _L, _C, res, _off = case
    off = offsets_of(case)
    if defect == "plus_offset":
        return any((2 * o) % N for o in off)
    if defect == "no_wrap":
        return any(off)
    if defect == "reverse_residual_sum":
        return bool(res) and M >= 2
    if defect == "dw_contracted":
        return M >= 2
    assert defect in DEFECTS
    return True


def plain_backward(case, defect=None):
    """(dV0, [dW_m]) from the case's W, X and dOut in the order bwd_chain_lds.h documents. Every operation is a numpy float32
    operation on whole arrays (one rounding each); `defect` swaps in one departure from it."""
    assert defect is None or defect in DEFECTS
    _B, N, M, L, C, res, _off = case
    W, _V0, dOut, X, _dV0, _dW = problem(case)
    off = offsets_of(case)
    f32, rows = np.float32, np.arange(N)

    def wrap(idx):
        return np.clip(idx, 0, N - 1) if defect == "no_wrap" else idx % N

    g, terms, dW = dOut, [dOut], [None] * M
    for m in range(M - 1, -1, -1):
        # g_m[q, :] = sum_k W_m[(q - off_k) mod N, k] * g_{m+1}[(q - off_k) mod N, :], links ascending
        acc = np.zeros_like(g)
        for k in range(L - 1 if defect == "last_link_dropped" else L):
            src = wrap(rows + off[k] if defect == "plus_offset" else rows - off[k])
            acc = acc + W[m][:, src, k, None] * g[:, src, :]
        assert acc.dtype == f32
        # dW_m[p, k] = sum_d g_{m+1}[p, d] * X_m[(p + off_k) mod N, d], channels ascending
        gin = acc if defect == "dw_leaving_gradient" else g
        Xm = X[m + 1] if defect == "dw_next_x" else X[m]
        dw = np.empty(W[m].shape, dtype=f32)
        for k in range(L):
            src = wrap(rows + off[k])
            a = np.zeros(gin.shape[:2], dtype=f32)
            for d in range(C):
                if defect == "dw_contracted":  # the product kept exact (float64 holds it) and rounded once with the add
                    a = (a.astype(np.float64) + gin[:, :, d].astype(np.float64) * Xm[:, src, d].astype(np.float64)).astype(f32)
                else:
                    a = a + gin[:, :, d] * Xm[:, src, d]
            dw[:, :, k] = a
        dW[m], g = dw, acc
        terms.append(g)
    if res:
        order = terms[::-1] if defect == "reverse_residual_sum" else terms
        g = order[0]
        for t in order[1:]:
            g = g + t
        assert g.dtype == f32
    return g, dW


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
