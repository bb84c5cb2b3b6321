"""Tools of the bf16 edge tests (test_gpu_bf16_edges.py; checked themselves, without a GPU, by test_bf16_edges_host.py).

numpy only. bf16 values travel as raw bits (uint16) or as the f32 values they stand for.

* ``rne_bits`` / ``trunc_bits``: f32 -> bf16 by round-to-nearest-even (what the kernels must do) and by truncation (a defect).
* ``rne64``: float64 -> the nearest bf16 value directly, without the double rounding of a detour through f32.
* ``int_case``: dZ and V of integers in [-15, 15]. Every product and every partial sum of sum_c dZ V is an exact f32 integer
  (|sum| <= 225 C < 2^24 for C <= 1024), so the only correct dW is rne_bits(exact sum), bit for bit, whatever the order.
* ``dw_sums`` and ``dw_bracket``: for random data, exact = sum_c dZ V in float64 and e = C 2^-24 sum_c |dZ V|, the standard
  bound of an f32 sum of C exact terms in any order or tree (bf16 x bf16 is exact in f32). A correct dW is bf16_rne of an f32
  value within e of exact, and rounding is monotone: rne64(exact - e) <= dW <= rne64(exact + e). No other tolerance.
* ``band_report``: what a kernel did to the NaN-pattern arena around and inside an output.
* ``special_case``: operands with NaN, Inf, signed zeros and magnitudes at the ends of f32's product range.
* ``decide_rows``: the verdict of the 2 GB cases on rows sampled in float64.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = 2.0 ** -126
SENTINEL = 0x7FC1   # a quiet-NaN bit pattern other than the canonical 0x7FC0
BAND = 128          # elements of two bytes: 256 bytes on either side


# ---------------------------------------------------------------- conversions
def rne_bits(a):
    """bf16 bits of f32 values, rounded to nearest even; a NaN stays a NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> 16) & 1))) >> 16).astype(np.uint16)  # (wraps only for NaNs, set below)
    nan = np.isnan(a)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def trunc_bits(a):
    """bf16 bits of f32 values by dropping the low 16 bits (round toward zero): the defect rne_bits is told from."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bits_f32(b):
    """The f32 values of bf16 bits."""
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def as_bf16(a):
    """f32 values rounded once to bf16, as f32 (bf16-representable inputs for the oracle and the kernels alike)."""
    return bits_f32(rne_bits(a))


def rne64(x):
    """float64 -> nearest bf16 value (ties to even), returned as f32. Direct: 8 significant bits in the normal range, the
    grid 2^-133 below 2^-126, infinity from 2^128 (1 - 2^-9) on."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        m, e = np.frexp(x)
        y = np.ldexp(np.rint(m * 256.0), e - 8)
        y = np.where(np.abs(x) < FLT_MIN, np.rint(x * 2.0 ** 133) * 2.0 ** -133, y)
        y = np.where(np.abs(y) >= 2.0 ** 128, np.copysign(np.inf, x), y)
        return y.astype(np.float32)


def same_bits(got_bits, want_bits):
    """Number of elements that differ: NaN must meet NaN (any payload), everything else bit for bit (the sign of zero too)."""
    got_bits, want_bits = np.asarray(got_bits).view(np.uint16), np.asarray(want_bits).view(np.uint16)
    gn, wn = np.isnan(bits_f32(got_bits)), np.isnan(bits_f32(want_bits))
    return int(((gn != wn) | (~gn & (got_bits != want_bits))).sum())


# ---------------------------------------------------------------- operands
def normal_case(shape, seed, scale=1.0):
    """Standard normals rounded to bf16 (f32 array)."""
    return as_bf16(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))


def int_case(shape, seed):
    """Integers in [-15, 15] (f32 array): exact in bf16."""
    return np.random.default_rng(seed).integers(-15, 16, size=shape).astype(np.float32)


# (shape, bwd_fused, broadcast V) of the known-answer dW test: window dW full-tile and edge instances, generic VEC = 8 and
# VEC = 1, the fused step; C in {6, 8, 24, 32, 128, 264}
KNOWN_ANSWER = [
    ((2, 1024, 11, 8), 0, False), ((2, 1025, 11, 8), 0, False), ((2, 515, 9, 24), 0, False), ((2, 256, 9, 32), 0, False),
    ((2, 1025, 11, 32), 0, False), ((2, 64, 6, 128), 0, False), ((2, 67, 6, 128), 0, False), ((2, 777, 22, 8), 0, False),
    ((1, 300, 12, 264), 0, False), ((2, 300, 9, 6), 0, False), ((2, 1024, 11, 8), 2, False), ((2, 256, 9, 32), 2, False),
    ((2, 64, 6, 128), 2, False), ((3, 1024, 11, 8), 0, True), ((3, 1024, 11, 8), 2, True),
]


def known_answer_operands(shape, broadcast):
    """(dZ, V) of a known-answer case."""
    B, N, L, C = shape
    return int_case((B, N, C), 50 + C), int_case((N, C) if broadcast else (B, N, C), 51 + C)


def rounding_classes(exact):
    """Counts of the ways bf16_rne treats exact f32 values: representable, tie (to the even neighbour, away from zero or
    toward it), and the plain roundings up and down in magnitude."""
    exact = np.asarray(exact, dtype=np.float32)
    mag = np.abs(exact).astype(np.float64)
    down = bits_f32(trunc_bits(np.abs(exact))).astype(np.float64)
    up = bits_f32(trunc_bits(np.abs(exact)) + np.uint16(1)).astype(np.float64)
    got = np.abs(bits_f32(rne_bits(exact))).astype(np.float64)
    rep = mag == down
    tie = ~rep & (mag - down == up - mag)
    return {"exact": int(rep.sum()), "tie_up": int((tie & (got == up)).sum()), "tie_down": int((tie & (got == down)).sum()),
            "up": int((~rep & ~tie & (got == up)).sum()), "down": int((~rep & ~tie & (got == down)).sum()), "n": int(exact.size)}


SPECIAL_TAME = [np.nan, np.inf, -np.inf, 0.0, -0.0]
SPECIAL_BIG = [2.0 ** 126, -2.0 ** 126]
SPECIAL_TINY = [2.0 ** -126, -2.0 ** -126]


def special_case(shape, seed, values, frac=0.02):
    """Random sign times [1, 2) rounded to bf16, `frac` of the elements replaced by `values` (at least one of each)."""
    rng = np.random.default_rng(seed)
    x = as_bf16(rng.choice([-1.0, 1.0], size=shape) * (1.0 + rng.random(shape))).astype(np.float32)
    x = np.where(np.abs(x) >= 2.0, np.sign(x) * np.float32(1.9921875), x).astype(np.float32)  # 2 - 2^-7: [1, 2) after rounding
    flat = x.reshape(-1)
    n = max(len(values), int(frac * flat.size))
    idx = rng.choice(flat.size, n, replace=False)
    vals = np.asarray(values, dtype=np.float32)
    pick = np.concatenate([np.arange(len(values)), rng.integers(0, len(values), n - len(values))])
    flat[idx] = vals[pick]
    return x


SPECIAL_SHAPES = [(2, 1024, 11, 8), (2, 1025, 11, 32), (2, 300, 9, 24), (2, 300, 9, 6), (2, 64, 6, 128)]
SPECIAL_RUNS = ["w", "dz", "dz_tame"]


def special_operands(B, N, L, C, run):
    """(W, V, R, dZ). NaN, Inf and signed zeros go anywhere; the ends of the product range, +-2^126 and +-2^-126, only into W
    (run "w": the forward and dV products W V and W dZ) or only into dZ (run "dz": the dW products dZ V; run "dz_tame":
    2^-126 without 2^126, so that no dW sum can overflow)."""
    tame = SPECIAL_TAME
    wide = tame + SPECIAL_BIG + SPECIAL_TINY
    vals = {"w": (wide, tame, tame), "dz": (tame, tame, wide), "dz_tame": (tame, tame, tame + SPECIAL_TINY)}[run]
    W, V = special_case((B, N, L), 61, vals[0]), special_case((B, N, C), 62, vals[1])
    return W, V, special_case((B, N, C), 63, tame), special_case((B, N, C), 64, vals[2])


def product_range_ok(a, b):
    """Whether every nonzero finite product of an element of `a` with an element of `b` lies in [2^-126, FLT_MAX]: the
    condition under which the kernels' fused multiply-add gives the bits of the rounded product followed by the rounded sum
    (checked over ALL pairs, which covers the pairs that meet)."""
    mags = []
    for t in (a, b):
        t = np.abs(np.asarray(t, dtype=np.float64))
        t = t[np.isfinite(t) & (t > 0)]
        if t.size == 0:
            return True
        mags.append((t.min(), t.max()))
    return bool(mags[0][0] * mags[1][0] >= FLT_MIN and mags[0][1] * mags[1][1] <= FLT_MAX)


# ---------------------------------------------------------------- dW
def chord_offsets(N, L):
    return [0] + [(1 << k) % N for k in range(L - 1)]


def dw_sums(dZ, V, L, offsets=None):
    """(exact, absum), both [B, N, L] float64: sum_c dZ[b,n,c] V[b,(n+off_k) mod N,c] and the same of |dZ V|. V may be [N, C]."""
    dZ = np.asarray(dZ, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    B, N, _ = dZ.shape
    off = chord_offsets(N, L) if offsets is None else [int(o) % N for o in offsets]
    exact, absum = np.empty((B, N, L)), np.empty((B, N, L))
    aZ, aV = np.abs(dZ), np.abs(V)  # |dZ V| = |dZ| |V|, exactly
    with np.errstate(all="ignore"):
        for k, o in enumerate(off):
            exact[:, :, k] = np.einsum("...c,...c->...", dZ, np.roll(V, -o, axis=-2))
            absum[:, :, k] = np.einsum("...c,...c->...", aZ, np.roll(aV, -o, axis=-2))
    return exact, absum


def dw_bracket(exact, absum, C):
    """(lo, hi) as f32: the bf16 values a correct dW lies between, ends included."""
    e = C * 2.0 ** -24 * np.asarray(absum, dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (Inf - Inf where the operands hold infinities: no bracket there)
        return rne64(exact - e), rne64(exact + e)


def bracket_report(got_bits, exact, absum, C, where=None):
    """(violations, loose share): elements of `got_bits` outside their bracket, and the share of brackets that hold more than
    one value. `where` restricts both to a mask."""
    lo, hi = dw_bracket(exact, absum, C)
    got = bits_f32(got_bits).reshape(lo.shape)
    with np.errstate(invalid="ignore"):
        bad = ~((lo <= got) & (got <= hi))
        loose = lo != hi
    if where is not None:
        bad, loose = bad[where], loose[where]
    return int(bad.sum()), float(loose.mean()) if loose.size else 0.0


MAX_LOOSE = 0.25  # the bracket must pin most elements to one value, or it tests little


def assert_dw_bracket(got_bits, dZ, V, L, offsets=None, what="dW"):
    C = np.asarray(dZ).shape[-1]
    exact, absum = dw_sums(dZ, V, L, offsets)
    bad, loose = bracket_report(got_bits, exact, absum, C)
    assert loose <= MAX_LOOSE, f"{what}: {loose:.1%} of the brackets hold more than one bf16 value"
    assert bad == 0, f"{what}: {bad} of {exact.size} elements outside bf16_rne(exact -+ C 2^-24 sum|dZ V|)"


# ---------------------------------------------------------------- guard bands
def arena_span(n, shift):
    """(total elements, lo, hi) of an arena for n elements at element shift `shift` (0..8): at least BAND on either side, lo
    16-byte aligned for shift 0 when the arena itself is."""
    assert 0 <= shift <= 8
    return n + 2 * BAND + 8, BAND + shift, BAND + shift + n


def band_report(arena_bits, lo, hi):
    """(stray elements below, stray elements above, elements inside still holding the sentinel)."""
    a = np.asarray(arena_bits).view(np.uint16)
    s = np.uint16(SENTINEL)
    return int((a[:lo] != s).sum()), int((a[hi:] != s).sum()), int((a[lo:hi] == s).sum())


# ---------------------------------------------------------------- the 2 GB cases: sampled rows in float64
def sample_rows(N):
    return [0, 1, 255, 256, N // 2 - 1, N // 2, N - 257, N - 1]


def decide_rows(got_bits, exact, slack):
    """(wrong, decidable share). `exact` is the float64 value of each sampled element, `slack` a bound on how far the
    kernel's f32 accumulator may be from it. Where bf16_rne(exact - slack) == bf16_rne(exact + slack) the element is
    decidable and must have exactly those bits. Elsewhere exact is within slack of a rounding boundary and the result must
    be one of the boundary's two neighbours, bf16_rne(exact - slack) or bf16_rne(exact + slack); where sums cancel, slack can
    span several boundaries of the fine grid near zero, and then rounding being monotone allows just the values between
    those two, ends included."""
    lo, hi = rne64(exact - slack), rne64(exact + slack)
    got_bits = np.asarray(got_bits).view(np.uint16).reshape(lo.shape)
    got = bits_f32(got_bits)
    decidable = rne_bits(lo) == rne_bits(hi)
    with np.errstate(invalid="ignore"):
        ok = np.where(decidable, got_bits == rne_bits(lo), (lo <= got) & (got <= hi))
    return int((~ok).sum()), float(decidable.mean())


MIN_DECIDABLE = 0.90
