"""Cases and CPU references for the attention-map queries (sparsefactorization_amd/attention_map.py, psf_chord_chain_tr_*).

The transposed chain  Y_M = Q;  Y_m[b,q,c] = sum_k W_m[b,(q-off_k) mod N,k] * Y_{m+1}[b,(q-off_k) mod N,c]  for m = M-1 .. 0.
With a one-hot column (a 1 at row r) the result's column is row r of A_b = W_{M-1} ... W_0.

References, none of which reads anything the GPU produced:
  tr_chain_f64     the chain in numpy float64 (the "exact" value of the accuracy bounds; |W| gives their absolute-value product)
  dense_map_f64    A_b as a product of dense N x N matrices (the identity the queries rest on; small N only)
  oracle_f32       M applications of the CPU oracle's dV (oracle_spmul_bwd_dv_f32): the BITS the f32 entry must return
  oracle_bf16      the same step on the upcast operands, rounded to bf16 (nearest even) after every step: the bf16 entry's bits

Bounds (stated in the issue): per element |got - exact| <= gamma * (|W_{M-1}| ... |W_0|)[row, :] with
  f32   gamma_n = n u / (1 - n u), n = M (L + 1), u = 2^-24
  bf16  M L roundings at 2^-24 (the f32 accumulator) and M roundings at 2^-9 (one per step): n u -> M L 2^-24 + M 2^-9
"""
import functools

import numpy as np

U32, U16 = 2.0 ** -24, 2.0 ** -9


def covered(N, L, R, M, elem_bytes):
    """psf_chord_chain_tr_supported, restated: where the entry runs one launch."""
    return (elem_bytes in (2, 4) and 1 <= N <= 1024 and 2 <= L <= 20 and 1 <= M <= 64 and R >= 1 and R % (16 // elem_bytes) == 0)


def workgroup_groups(R, elem_bytes):
    """The launcher's split of a sequence's 16-byte column groups over workgroups, restated: chunks = ceil(CG / 4) workgroups
    of G = ceil(CG / chunks) groups, the last one with what is left. Returns (G, [groups per workgroup])."""
    CG = R // (16 // elem_bytes)
    chunks = -(-CG // 4)
    G = -(-CG // chunks)
    return G, [min(G, CG - c * G) for c in range(chunks)]


def chord_offsets(L):
    return [0] + [1 << (k - 1) for k in range(1, L)]


def tr_step_f64(W, Y, offsets=None):
    B, N, L = W.shape
    off = chord_offsets(L) if offsets is None else list(offsets)
    out = np.zeros_like(Y, dtype=np.float64)
    q = np.arange(N)
    for k in range(L):
        src = (q - off[k]) % N
        out += W[:, src, k, None].astype(np.float64) * Y[:, src, :]
    return out


def tr_chain_f64(Ws, Q, offsets=None):
    Y = np.asarray(Q, dtype=np.float64)
    for W in reversed(list(Ws)):
        Y = tr_step_f64(np.asarray(W, dtype=np.float64), Y, offsets)
    return Y


def dense_map_f64(Ws, offsets=None):
    """A_b = W_{M-1} ... W_0 with dense factors D_m[p, (p + off_k) mod N] += W_m[p, k] — [B, N, N]."""
    Ws = [np.asarray(W, dtype=np.float64) for W in Ws]
    B, N, L = Ws[0].shape
    off = chord_offsets(L) if offsets is None else list(offsets)
    A = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    p = np.arange(N)
    for W in Ws:  # A <- D_m A, m ascending
        D = np.zeros((B, N, N))
        for k in range(L):
            np.add.at(D, (slice(None), p, (p + off[k]) % N), W[:, :, k])
        A = D @ A
    return A


def gamma(M, L, elem_bytes=4):
    n = M * (L + 1) * U32 if elem_bytes == 4 else M * L * U32 + M * U16
    return n / (1.0 - n)


def one_hot(rows, N, dtype=np.float32):
    """rows [B, R] -> Q [B, N, R]"""
    rows = np.asarray(rows)
    B, R = rows.shape
    Q = np.zeros((B, N, R), dtype=dtype)
    Q[np.arange(B)[:, None], rows, np.arange(R)[None, :]] = 1
    return Q


def rne_bf16(a):
    """f32 -> the nearest bf16 (ties to even, NaN kept), returned as f32"""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def oracle_f32(Ws, Q, offsets=None):
    from oracle import chord_oracle as oc
    y = np.ascontiguousarray(Q, dtype=np.float32)
    for W in reversed(list(Ws)):
        y = oc.spmul_bwd(y, W, y, offsets)[1]
    return y


def oracle_bf16(Ws, Q, offsets=None):
    """Ws, Q: f32 arrays of bf16-representable values"""
    from oracle import chord_oracle as oc
    y = np.ascontiguousarray(Q, dtype=np.float32)
    for W in reversed(list(Ws)):
        y = rne_bf16(oc.spmul_bwd(y, W, y, offsets)[1])
    return y


def same_bits(got, want):
    """number of elements whose bits differ; a NaN matches any NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return int((~ok).sum())


# (name, B, N, L, M, R, offsets, special): special in None, "dense" (a random Q that is not one-hot), "nan", "inf" (in W)
# N crosses 1 | 2 | 3, 63 | 64 | 65 and 1023 | 1024 (one launch) and 1025, 4097 (per step); L = 2, 12 at N = 1024 (2^10 mod N:
# the duplicate self link), 20; M = 1, 2, 11, 64; R = 4, 8, 12 (one workgroup of one, two, three full groups), 64 (four full
# workgroups per sequence), and the RAGGED splits 20 (five groups: workgroups of 3 + 2) and 52 (thirteen: 4 + 4 + 4 + 1), whose
# last workgroup repeats its last group in the idle slots and must not store it; B = 1, 3.
F32_CASES = [
    ("n1", 1, 1, 2, 2, 4, None, None),
    ("n2", 3, 2, 2, 1, 8, None, "dense"),
    ("n3_l20", 1, 3, 20, 2, 12, None, None),
    ("n63", 3, 63, 7, 11, 12, None, None),
    ("n64_r64", 1, 64, 7, 2, 64, None, "dense"),
    ("n65_m64", 1, 65, 8, 64, 4, None, None),
    ("n1023_l20", 1, 1023, 20, 2, 8, None, None),
    ("pathfinder", 3, 1024, 12, 11, 64, None, None),
    ("n1024_l20", 1, 1024, 20, 1, 12, None, None),
    ("n1024_l2_m64", 1, 1024, 2, 64, 4, None, None),
    ("n1025", 3, 1025, 12, 2, 8, None, None),
    ("imdb", 2, 4097, 13, 12, 4, None, None),
    ("explicit", 2, 100, 5, 3, 8, (0, 3, 7, 50, 99), None),
    ("negative", 2, 100, 4, 3, 4, (-1, 0, 5, -37), None),
    ("ragged_r20", 2, 65, 7, 3, 20, None, "dense"),
    ("ragged_r52", 1, 1024, 12, 2, 52, None, None),
    ("nan", 1, 65, 5, 3, 4, None, "nan"),
    ("inf", 1, 65, 5, 3, 4, None, "inf"),
]
# (64: eight groups of eight, two full workgroups per sequence; 40: five groups, 3 + 2; 56: seven groups, 4 + 3)
_BF16_R = {4: 8, 8: 16, 12: 24, 64: 64, 20: 40, 52: 56}
BF16_CASES = [(name, B, N, L, M, _BF16_R[R], off, sp) for name, B, N, L, M, R, off, sp in F32_CASES]
BF16_ODD_W = ("odd_w_l15", 2, 200, 15, 3, 8, None, None)  # every W_m at an odd 2-byte offset, 30-byte rows


@functools.lru_cache(maxsize=None)
def operands(case, bf16=False):
    """(Ws [M] of [B,N,L] f32, Q [B,N,R] f32, rows [B,R] or None). bf16: the values are bf16-representable. Cached: do not write."""
    name, B, N, L, M, R, _off, special = case
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + N)  # (hash() of a str changes from run to run)
    # |W| around 1 / sqrt(L): the products neither grow nor vanish over 64 steps
    Ws = [(rng.standard_normal((B, N, L)) / np.sqrt(L)).astype(np.float32) for _ in range(M)]
    rows = None
    if special == "dense":
        Q = rng.standard_normal((B, N, R)).astype(np.float32)
    else:
        rows = rng.integers(0, N, size=(B, R))
        rows[:, 0] = 0
        rows[:, -1] = N - 1
        Q = one_hot(rows, N)
    if special in ("nan", "inf"):
        Ws[M // 2][0, N // 3, 1] = np.nan if special == "nan" else np.inf
        Ws[0][0, N - 1, L - 1] = np.nan if special == "nan" else -np.inf
    if bf16:
        Ws, Q = [rne_bf16(W) for W in Ws], rne_bf16(Q)
    for a in (*Ws, Q):
        a.setflags(write=False)
    return tuple(Ws), Q, rows


@functools.lru_cache(maxsize=None)
def expected(case, bf16=False):
    """The bits the entry must return for ``operands(case, bf16)``. Cached: do not write."""
    Ws, Q, _rows = operands(case, bf16)
    want = (oracle_bf16 if bf16 else oracle_f32)(Ws, Q, case[6])
    want.setflags(write=False)
    return want
