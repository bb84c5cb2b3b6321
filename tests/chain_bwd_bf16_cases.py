"""Cases, operands and expected answers for the one-launch bf16 backward chain (csrc/bwd_chain_lds_bf16.h:
chord_chain_bwd_lds_k<bf16, L, G, RES> behind psf_chord_chain_bwd_lds_bf16), used by test_gpu_chain_bwd_lds_bf16.py and checked
without a GPU by test_chain_bwd_bf16_cases_cpu.py.

A case is (B, N, M, L, C, residual, offsets); offsets is None (the chord pattern 0, 1, 2, 4, ... mod N) or a tuple of L integers.
Operands are tests/bf16_edges.normal_case, rounded to bf16 and carried as the f32 values they stand for: W_m scaled by 0.4
(seed 81 + m), V0 (seed 80) and dOut (seed 79) at 1.0 — the seed recipe of chain_bwd_cases.py. Every product then stays inside
f32's normal range, where a fused multiply-add of bf16 operands equals the exact product followed by one rounded sum.

``plain_backward_bf16`` restates the kernel's documented contract in numpy float32:
  g_m     per element an f32 sum from +0, links ascending, each term exact-product-then-add; rounded to bf16 ONCE
          (be.rne_bits), and that rounded value enters the next step;
  dW_m    per 8-channel group a running sum over the channels ascending from +0; C = 8 rounds it, C = 16 rounds the f32 sum
          of the two partials;
  dV0     ((g_M + g_{M-1}) + ... + g_1) + g_0 over the rounded g_m in f32, rounded once; g_0 without the residual.
The product of two bf16 values has at most 16 significant bits, so ``a * b`` in float32 is exact and ``acc + a * b`` is one
rounding: the fused multiply-add. It can emulate three wrong variants; the CPU test shows each gives other bits.

The shape rules below (covered; dynamic LDS = 2 G 1024 16 + N (L | 1) 4 bytes with G = C / 8; 48 KB raise) are the ones
bwd_chain_lds_bf16.h and bwd_chain_lds_bf16_inst.hip document. They serve to ASSERT what the lists reach, never to compute an
answer.
"""
from __future__ import annotations

import functools

import numpy as np

import bf16_edges as be

ROWS = 1024       # kChainBwdRows
MAX_STEPS = 64    # kChainMaxSteps
L_MIN, L_MAX = 2, 20
LDS_FREE = 48 * 1024

# 1. every instance: L = 2..20 x residual at C = 8 (G = 1) and at C = 16 (G = 2); two waves, 61 idle lanes
GRID = [(2, 67, 2, L, C, res, None) for C in (8, 16) for L in range(L_MIN, L_MAX + 1) for res in (False, True)]

# 2. limits
LIMITS = [
    (2, 1024, 3, 20, 16, True, None),   # the dynamic-LDS maximum, 151 552 bytes
    (2, 1024, 2, 20, 8, False, None),   # G = 1 beyond 48 KB
    (2, 1023, 2, 19, 16, True, None),   # one idle lane in the last wave
    (1, 1024, 64, 2, 8, True, None),    # M = kChainMaxSteps at the smallest L, all 1024 threads
    (2, 65, 64, 5, 16, True, None),     # M = kChainMaxSteps, two waves with 63 idle lanes
    (3, 1, 1, 2, 8, False, None),       # one row: every link a self link
    (2, 2, 3, 20, 16, True, None),
    (2, 3, 2, 4, 8, True, None),
    (2, 64, 2, 20, 8, True, None),      # 14 duplicate self links (2^k mod 64 = 0 from k = 6 on)
    (2, 63, 1, 7, 8, True, None),
    (2, 63, 1, 7, 8, False, None),
    (2, 256, 3, 6, 8, True, (0, 5, 255, 300, -1, 128)),
]

# one instance below 48 KB of dynamic LDS, above it, below it again
RAISE_BETWEEN = [(2, 64, 2, 9, 8, True, None), (2, 1024, 2, 9, 8, True, None), (2, 64, 2, 9, 8, True, None)]

# 3. bands and alignment (each with and without the residual); odd L and even L
BANDS = [(B, N, M, L, C, res, None) for (B, N, M, L, C) in ((2, 67, 3, 5, 8), (2, 1024, 2, 11, 16), (3, 130, 2, 20, 8)) for res in (False, True)]
W_SHIFTS = (0, 1, 3)   # bf16 elements off a 16-byte boundary, W_m and dW_m alike

# 4. stale LDS: a large case first, then these
STALE_FIRST = (2, 1024, 2, 20, 16, True, None)
STALE = [(2, 37, 4, 5, 8, True, None), (2, 100, 3, 7, 16, True, None), (5, 777, 3, 10, 8, False, None)]

# 5. special values (operands from be.special_operands, not from here)
SPECIAL = [(2, 128, 3, 8, 8, False, None), (2, 128, 3, 8, 8, True, None)]

# 6. declines
DECLINED = [(2, 1025, 2, 11, 8, True, None), (2, 100, 2, 9, 12, True, None)]
MISALIGNED = (2, 67, 3, 5, 8, True, None)

# 7. autograd route: (B, N, M, L, C), residual on; the last one falls back to the per-step route
AUTOGRAD = [(2, 128, 14, 8, 8), (2, 1024, 5, 11, 16)]
AUTOGRAD_FALLBACK = (2, 1025, 3, 11, 8)

# graph capture
GRAPH = (2, 128, 3, 8, 8, True, None)

ONE_LAUNCH = GRID + LIMITS + RAISE_BETWEEN[:2] + BANDS + [STALE_FIRST] + STALE + SPECIAL + [MISALIGNED, GRAPH]


def case_id(case) -> str:
    B, N, M, L, C, res, off = case
    return f"B{B}-N{N}-M{M}-L{L}-C{C}-{'res' if res else 'plain'}{'-offsets' if off is not None else ''}"


# ---------------------------------------------------------------- what a case reaches (documented rules)
def covered(N, L, C, M) -> bool:
    """chain_bwd_lds_bf16_fits of bwd_chain_lds_bf16_inst.hip."""
    return 1 <= N <= ROWS and C in (8, 16) and L_MIN <= L <= L_MAX and 1 <= M <= MAX_STEPS


def instance(case):
    """(L, G, RES) of chord_chain_bwd_lds_k<bf16>."""
    _B, _N, _M, L, C, res, _off = case
    return L, C // 8, bool(res)


def lds_bytes(case) -> int:
    _B, N, _M, L, C, _res, _off = case
    return 2 * (C // 8) * ROWS * 16 + N * (L | 1) * 4


def offsets_of(case):
    """The L link offsets reduced into [0, N)."""
    _B, N, _M, L, _C, _res, off = case
    if off is None:
        return be.chord_offsets(N, L)
    assert len(off) == L
    return [int(o) % N for o in off]


# ---------------------------------------------------------------- operands and the forward (bf16 values as f32 arrays)
def operands(case):
    """(W, V0, dOut): M arrays [B, N, L], and two of [B, N, C]; every value a bf16 value."""
    B, N, M, L, C, _res, _off = case
    return [be.normal_case((B, N, L), 81 + m, 0.4) for m in range(M)], be.normal_case((B, N, C), 80), be.normal_case((B, N, C), 79)


def forward_bf16(W, V0, residual, offsets):
    """[X_0 = V0, X_1, ..., X_M]: the bf16 forward chain's contract — f32 sum from +0, links ascending, then the residual, one
    rounding to bf16 per step. (The backward tests only need SOME bf16 X_m; this is the one a forward would have saved.)"""
    N = V0.shape[1]
    rows = np.arange(N)
    X = [V0]
    with np.errstate(all="ignore"):
        for Wm in W:
            acc = np.zeros_like(V0)
            for k, o in enumerate(offsets):
                src = (rows + o) % N
                acc = acc + Wm[:, :, k, None] * X[-1][:, src, :]
            if residual:
                acc = acc + V0
            X.append(be.as_bf16(acc))
    return X


# ---------------------------------------------------------------- the kernel's contract in plain numpy, and three departures
VARIANTS = ("g_kept_f32", "residual_bf16_adds", "dw_one_running_sum")


def applies(variant, case) -> bool:
    """Whether the variant can change a bit in the case, from the shape alone.

    g_kept_f32           needs a reader of the unrounded g: a second step (M >= 2) or the residual sum
    residual_bf16_adds   needs the residual and three terms or more: at M = 1 the one sum g_1 + g_0 is rounded once either way
    dw_one_running_sum   needs two channel groups: C = 16
    """
    _B, _N, M, _L, C, res, _off = case
    if variant == "g_kept_f32":
        return M >= 2 or bool(res)
    if variant == "residual_bf16_adds":
        return bool(res) and M >= 2
    assert variant == "dw_one_running_sum"
    return C == 16


def backward_from(case, W, X, dOut, variant=None):
    """(dV0 bits, [dW_m bits]) as uint16 arrays, from bf16-valued f32 operands, in the order bwd_chain_lds_bf16.h documents.
    Every operation is a numpy float32 operation on whole arrays; `variant` swaps in one departure from the contract."""
    assert variant is None or variant in VARIANTS
    _B, N, M, L, C, res, _off = case
    off = offsets_of(case)
    f32, rows = np.float32, np.arange(N)
    g, terms, dW = dOut, [dOut], [None] * M
    with np.errstate(all="ignore"):
        for m in range(M - 1, -1, -1):
            # dW_m[p, k]: per 8-channel group a running sum over the channels, then the groups added, then one rounding.
            # (with g_kept_f32 the dW operand is what the step READS, the unrounded g)
            dw = np.empty(W[m].shape, dtype=f32)
            for k in range(L):
                src = (rows + off[k]) % N
                if variant == "dw_one_running_sum":
                    a = np.zeros(g.shape[:2], dtype=f32)
                    for d in range(C):
                        a = a + g[:, :, d] * X[m][:, src, d]
                else:
                    parts = []
                    for c0 in range(0, C, 8):
                        a = np.zeros(g.shape[:2], dtype=f32)
                        for d in range(c0, c0 + 8):
                            a = a + g[:, :, d] * X[m][:, src, d]
                        parts.append(a)
                    a = parts[0] if len(parts) == 1 else parts[0] + parts[1]
                assert a.dtype == f32
                dw[:, :, k] = a
            dW[m] = be.rne_bits(dw)
            # g_m[q, :] = sum_k W_m[(q - off_k) mod N, k] * g_{m+1}[(q - off_k) mod N, :], links ascending, ONE rounding
            acc = np.zeros_like(g)
            for k in range(L):
                src = (rows - off[k]) % N
                acc = acc + W[m][:, src, k, None] * g[:, src, :]
            assert acc.dtype == f32
            g = acc if variant == "g_kept_f32" else be.as_bf16(acc)
            terms.append(g)
        if res:
            if variant == "residual_bf16_adds":
                s = terms[0]
                for t in terms[1:]:
                    s = be.as_bf16(s + t)
            else:
                s = terms[0]
                for t in terms[1:]:
                    s = s + t
                assert s.dtype == f32
            g = s
    return be.rne_bits(g), dW


@functools.lru_cache(maxsize=None)
def problem(case):
    """(W, V0, dOut, X) of a case: computed once, shared, never written to."""
    _B, _N, _M, _L, _C, res, _off = case
    W, V0, dOut = operands(case)
    X = forward_bf16(W, V0, res, offsets_of(case))
    for a in (*W, V0, dOut, *X):
        a.setflags(write=False)
    return W, V0, dOut, X


@functools.lru_cache(maxsize=None)
def plain_backward_bf16(case, variant=None):
    """(dV0 bits, (dW_m bits, ...)) of the case's own operands: computed once per (case, variant), shared, read-only."""
    W, _V0, dOut, X = problem(case)
    dV0, dW = backward_from(case, W, X, dOut, variant)
    for a in (dV0, *dW):
        a.setflags(write=False)
    return dV0, tuple(dW)
