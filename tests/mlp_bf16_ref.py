"""Reference and known-answer inputs for the fused bf16 producer forward (psf_mlp_fwd_bf16, csrc/mlp_fwd_bf16.hip).

The contract (include/psf_chord.h): every operand and result is bf16, and for each MLP

    z = bf16_rne(f32(X A^T + a)),   h = bf16_rne(GELU_f32(z)),   y = bf16_rne(f32(h B^T + b))

with exact products and f32 sums in an unspecified order. ``ref`` evaluates that in float64 (the sums exact to 2^-53, far
below an f32 rounding) and returns an envelope: what any f32 summation order can produce through flipped bf16 ties. A
result outside the envelope is wrong; on random inputs at most ``MAX_DIFFERING`` of the elements may differ from ``ref`` at
all (flips need an f32 sum within ~(E + 1) 2^-24 relative of a tie: about one element in 2^16 / (E + 1)).

Two constructions make the order irrelevant, so the answer is exact to the bit (compare after mapping -0 to +0: the GELU's
dead regime returns -0):

  "linear"  small integers everywhere, every live pre-activation an integer in [16, 256] and every dead one <= -32, where
            the kernels' GELU returns exactly x or 0 (x3_exact.gelu_regime_ok); every y an integer of magnitude <= 256.
  "select"  one nonzero +-2^s per row of A and of B, zero biases: z = +-2^s X comes from a list of bf16 values whose GELU
            lies further than 4e-7 (|z| + 1) from every bf16 rounding boundary, so h is determined, and Y = +-2^s h.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from x3_exact import gelu_regime_ok

MAX_DIFFERING = 0.01  # a cap, not a measurement


# ---------------------------------------------------------------- bf16 on float64 arrays
def _exp2_floor(v):
    """floor(log2 |v|) for nonzero finite v, clamped to bf16's normal range (subnormals share the smallest normal's ulp)."""
    _, e = np.frexp(np.abs(v))
    return np.clip(e - 1, -126, 127)


def ulp_bf16(v) -> np.ndarray:
    """The spacing of bf16 values at |v| (8 significant bits)."""
    v = np.asarray(v, np.float64)
    return np.ldexp(1.0, (_exp2_floor(np.where(v == 0, 1e-300, v)) - 7).astype(np.int64))


def bf16_rne(v) -> np.ndarray:
    """float64 -> the nearest bf16 value (ties to even), as float64; one rounding, not via f32."""
    v = np.asarray(v, np.float64)
    q = ulp_bf16(v)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(v / q) * q  # np.rint rounds halves to even
        r = np.where(np.abs(r) > 3.3895313892515355e38, np.copysign(np.inf, v), r)
    return np.where(np.isfinite(v), r, v)


def to_bits(v) -> np.ndarray:
    """bf16-valued floats -> uint16 bit patterns."""
    f = np.ascontiguousarray(v, np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(v, np.float64), equal_nan=True)
    bits = f.view(np.uint32)
    assert not np.any(bits & np.uint32(0xFFFF)), "not a bf16 value"
    return (bits >> np.uint32(16)).astype(np.uint16)


def from_bits(b) -> np.ndarray:
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def plus_zero(bits) -> np.ndarray:
    """bf16 bit patterns with -0 mapped to +0."""
    bits = np.asarray(bits, np.uint16)
    return np.where(bits == 0x8000, np.uint16(0), bits)


def erf64(v):
    """float64 erf (numpy has none; torch's CPU double erf, elementwise)."""
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v, np.float64))).numpy()


def gelu64(z):
    z = np.asarray(z, np.float64)
    return 0.5 * z * (1.0 + erf64(z / np.sqrt(2.0)))


# ---------------------------------------------------------------- the reference
def ref(X, A, a, B, b):
    """(z, h, y, dy): the three-rounding contract in float64 and the per-element envelope of y.
    dz = ulp(z); dh = ulp(h) + 1.13 dz + 2e-7 (|z| + 1) (1.13 bounds |GELU'|, 2e-7 covers Phi); dy = ulp(y) + |B| dh."""
    X, A, a, B, b = (np.asarray(t, np.float64) for t in (X, A, a, B, b))
    z = bf16_rne(X @ A.T + a)
    h = bf16_rne(gelu64(z))
    y = bf16_rne(h @ B.T + b)
    dz = ulp_bf16(z)
    dh = ulp_bf16(h) + 1.13 * dz + 2e-7 * (np.abs(z) + 1.0)
    dy = ulp_bf16(y) + dh @ np.abs(B).T
    return z, h, y, dy


def compare(got, y, dy) -> Tuple[float, float]:
    """(largest |got - y| / dy, share of elements that differ from y at all) of a result given as bf16-valued floats."""
    got = np.asarray(got, np.float64)
    assert got.shape == y.shape and np.all(np.isfinite(got))
    err = np.abs(got - y)
    return float(np.max(err / dy)) if err.size else 0.0, float(np.mean(err != 0)) if err.size else 0.0


def assert_close(got, y, dy, what=""):
    worst, share = compare(got, y, dy)
    print(f"{what}: worst |err| / envelope = {worst:.4f}, differing share = {share:.3e}")
    assert worst <= 1.0, f"{what}: outside the envelope ({worst:.3f} of it)"
    assert share <= MAX_DIFFERING, f"{what}: {share:.3%} of the elements differ from the reference"


# ---------------------------------------------------------------- random inputs
def random_params(E: int, layers: Sequence[Tuple[int, int]], seed: int, scale: float = 1.0):
    """nn.Linear-initialised (A, a, B, b) per MLP, rounded to bf16, as float64 arrays; ``scale`` multiplies the weights."""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, O in layers:
        ps = []
        for rows, cols in ((h, E), (O, h)):
            bound = 1.0 / np.sqrt(cols)
            w = (torch.rand(rows, cols, generator=g, dtype=torch.float64) * 2 - 1) * bound * scale
            c = (torch.rand(rows, generator=g, dtype=torch.float64) * 2 - 1) * bound
            ps += [bf16_rne(w.numpy()), bf16_rne(c.numpy())]
        out.append(tuple(ps))
    return out


def random_x(T: int, E: int, seed: int):
    return bf16_rne(np.random.default_rng(seed).standard_normal((T, E)))


# ---------------------------------------------------------------- known answers
def _row_rank(h, O):
    """Hidden row j is read by output j % O; its rank among that output's rows alternates the sign of its weight."""
    return np.arange(h) % O, np.arange(h) // O


def _dead(h, j):
    return h > 2 and j != h - 1 and j % 7 == 5


def make_linear(T: int, E: int, layers: Sequence[Tuple[int, int]], seed: int = 0):
    """(X, params, answers): the "linear" construction and its closed-form Y per MLP (exact integers)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-1, 2, size=(T, E)).astype(np.float64)
    X[-1, :] = np.where(np.arange(E) % 2 == 0, 1.0, -1.0)  # the last token (of a ragged last tile) is nonzero everywhere
    X[:, -1] = np.where(X[:, -1] == 0, 1.0, X[:, -1])      # and so is the last column of E
    params, answers = [], []
    for h, O in layers:
        A = np.zeros((h, E))
        a = np.zeros(h)
        for j in range(h):
            cols = {(E - 1 - 5 * j) % E, (E - 2 - 5 * j - (E // 2) * (j % 2)) % E}  # row 0 reads the last column
            for c in cols:
                A[j, c] = rng.choice([-1.0, 1.0])
            a[j] = -48.0 if _dead(h, j) else 20.0 + (j % 5) + 3 * (j == h - 1)  # the last hidden row stands out
        B = np.zeros((O, h))
        out_of, rank = _row_rank(h, O)
        for j in range(h):
            B[out_of[j], j] = 1.0 if rank[j] % 2 == 0 else -1.0
        b = rng.integers(-8, 9, size=O).astype(np.float64)
        pre = X @ A.T + a
        live = np.where(pre > 0, pre, 0.0)
        params.append((A, a, B, b))
        answers.append(live @ B.T + b)
    return X, params, answers


def check_linear(X, params, answers):
    """The construction's own exactness conditions (grids, GELU regime, partial sums, magnitudes)."""
    for (A, a, B, b), y in zip(params, answers):
        for t in (X, A, a, B, b):
            assert np.array_equal(t, np.rint(t)) and np.max(np.abs(t)) <= 256  # small integers: bf16-exact
        pre = X @ A.T + a
        live = pre > 0
        assert np.all((pre[live] >= 16) & (pre[live] <= 256)) and np.all(pre[~live] <= -32)
        assert gelu_regime_ok(pre.astype(np.float32))  # gelu2 returns exactly x or 0 there
        assert np.max(np.abs(X) @ np.abs(A).T + np.abs(a)) < 2.0 ** 24  # every partial sum of GEMM1 is exact in f32
        hp = np.where(live, pre, 0.0)
        assert np.max(hp @ np.abs(B).T + np.abs(b)) < 2.0 ** 24           # and of GEMM2
        assert np.array_equal(y, np.rint(y)) and np.max(np.abs(y)) <= 256, "y must be an integer of magnitude <= 256"
        assert np.all(np.abs(A).sum(1) > 0) and np.all(np.abs(B).sum(0) > 0) and np.all(np.abs(B).sum(1) > 0)
        assert A[0, -1] != 0 and np.all(X[-1] != 0) and np.all(X[:, -1] != 0)
        assert np.any(y[-1] != 0)


# bf16 values in [-1, 1]; with the scales 2^-1 .. 2^2 of A every z lies in [-4, 4]
_SELECT_BASE = [v / 128.0 for v in range(-128, 129) if v % 3]
_A_SCALES = (-1, 0, 1, 2)
_B_SCALES = (-1, 0, 1, 2)


def gelu_margin_ok(z) -> np.ndarray:
    """Per value: float64 GELU(z) lies further than 4e-7 (|z| + 1) from every bf16 rounding boundary."""
    z = np.asarray(z, np.float64)
    g = gelu64(z)
    r = bf16_rne(g)
    assert np.all(r != 0)
    mag = to_bits(np.abs(r)).astype(np.int64)  # the neighbours of |r| on the bf16 grid are the bit patterns +- 1
    up, dn = from_bits((mag + 1).astype(np.uint16)), from_bits((mag - 1).astype(np.uint16))
    dist = np.minimum(np.abs(np.abs(g) - (np.abs(r) + up) / 2), np.abs(np.abs(g) - (np.abs(r) + dn) / 2))
    return dist > 4e-7 * (np.abs(z) + 1.0)


def select_values() -> np.ndarray:
    """The base list: bf16 values v in [-1, 1] all of whose scalings +-2^s v pass the margin."""
    base = np.array(_SELECT_BASE)
    ok = np.ones(base.shape, bool)
    for s in _A_SCALES:
        for sign in (-1.0, 1.0):
            ok &= gelu_margin_ok(sign * np.ldexp(base, s))
    vals = base[ok]
    assert vals.size >= 32 and np.any(vals < 0) and np.any(vals > 0)
    return vals


def make_select(T: int, E: int, layers: Sequence[Tuple[int, int]], seed: int = 0):
    """(X, params, answers): the "select" construction and its closed-form Y = +-2^s h[row the output names]."""
    rng = np.random.default_rng(seed)
    vals = select_values()
    X = vals[rng.integers(0, vals.size, size=(T, E))]
    params, answers = [], []
    for h, O in layers:
        A = np.zeros((h, E))
        cols = (E - 1 - 5 * np.arange(h)) % E  # row 0 reads the last column
        A[np.arange(h), cols] = rng.choice([-1.0, 1.0], size=h) * np.ldexp(1.0, rng.choice(_A_SCALES, size=h))
        B = np.zeros((O, h))
        rows = (h - 1 - 3 * np.arange(O)) % h  # output 0 reads the last hidden row
        B[np.arange(O), rows] = rng.choice([-1.0, 1.0], size=O) * np.ldexp(1.0, rng.choice(_B_SCALES, size=O))
        z = X[:, cols] * A[np.arange(h), cols]
        hh = bf16_rne(gelu64(z))
        params.append((A, np.zeros(h), B, np.zeros(O)))
        answers.append(hh[:, rows] * B[np.arange(O), rows])
    return X, params, answers


def check_select(X, params, answers):
    for (A, a, B, b), y in zip(params, answers):
        assert not a.any() and not b.any()
        assert np.all((A != 0).sum(1) == 1) and np.all((B != 0).sum(1) == 1)
        for t in (A, B):
            nz = np.abs(t[t != 0])
            assert np.array_equal(nz, np.ldexp(1.0, np.round(np.log2(nz)).astype(np.int64)))  # powers of two
        z = X @ A.T
        assert np.array_equal(z, bf16_rne(z)) and np.max(np.abs(z)) <= 4.0
        assert np.all(gelu_margin_ok(z)), "a GELU value too close to a bf16 rounding boundary"
        assert np.array_equal(y, bf16_rne(y)) and np.all(np.isfinite(y))
        assert A[0, -1] != 0 and B[0, -1] != 0


KINDS = {"linear": (make_linear, check_linear), "select": (make_select, check_select)}

# (T, E, [(h, O), ...]) of the GPU known-answer tests
ADDING = [(32, 8)] + [(32, 15)] * 14
SHAPES = [
    (31, 8, [(5, 3)]),                                  # under one tile
    (257, 32, ADDING),                                  # two blocks plus one token, the Adding MLPs, odd O
    (4097, 32, [(128, 32)] + [(128, 13)] * 12),         # four units per MLP
    (1000, 64, [(96, 32), (33, 1), (128, 20)]),         # E = 64, ragged units, O = 1
    (130, 24, [(7, 2), (40, 31)]),                      # E % 16 == 8
    (129, 16, [(16, 11)] * 32),                         # K = 32
]
# (T, E, h, O) of the CPU check of the envelope against torch's own bf16 modules
TORCH_SHAPES = [(4097, 32, 32, 15), (1000, 64, 128, 32), (555, 8, 7, 2), (3000, 16, 16, 11)]


def seed_of(T: int, E: int) -> int:
    return T + 3 * E
