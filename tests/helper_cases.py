"""Known-answer inputs for the token-wise helper kernels: the token embedding, its table gradient and the affine input rows
(csrc/embed.hip), the FLATTEN head and its backward (csrc/flat_head.hip) and the Linear weight gradient (csrc/linear_wgrad.hip).

Every operand is a small integer stored as f32 (seeded numpy), so every product is an integer, and for every output the sum
of the |terms| stays below 2^24: every partial sum of every subset of the terms is then an integer below 2^24, exact in f32 in
any order, with or without FMA. The right answer is therefore bit-exact whatever order a kernel sums in; no order is
restated here. Expected answers are computed in int64 / float64, checked to be integers below 2^24 (``as_f32``) and cast.

Bounds, per operator (``bound()`` of each case returns the left-hand side, LIMIT = 2^24 the right):

* embedding gradient  dTable[v] = sum of dOut[t] over idx[t] == v:  |dOut| <= 4, so sum |terms| <= 4 T < 2^24 (T <= 300 001)
* embedding forward   table[idx[t]] + pos[t mod N]:  |table|, |pos| <= 2000, one add, 4000 < 2^24
* affine rows         x W^T + b with K <= 3:  |x|, |w|, |b| <= 7, so 49 K + 7 <= 154 < 2^24
* head forward        b_j + sum_i X[b,i] W[j,i]:  |x|, |w| <= 2, integer |bias| <= 100, so 4 K + |b| < 2^24 (K <= 258 060)
* head backward       dW = dY^T X, dX = dY W:  |dY|, |x|, |w| <= 3, so 9 B <= 9216 and 9 J <= 144
* weight gradient     dWt = dY^T X, db = sum dY:  |X| <= 3, |dY| <= 2, so 6 T < 2^24 (T <= 100 003)

The data are asymmetric: every value depends on its token, its column and its row (seeded draws, no symmetry), so a
transposed, permuted or dropped tile cannot pass; the last token of an embedding gradient carries the largest magnitude.

The shape rules quoted below (sub-tables, slices, chunk lengths, grid caps) are the ones the kernels' headers and comments
document; they are used to ASSERT that the lists reach what they claim to reach (test_helper_cases_cpu.py), never to compute
an expected value.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

LIMIT = 1 << 24


def as_f32(a) -> np.ndarray:
    """An exact integer answer below 2^24 in magnitude, as f32 (asserts both)."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        assert np.array_equal(a, np.rint(a)), "expected answer is not integral"
    assert a.size == 0 or int(np.abs(a).max()) < LIMIT, "expected answer leaves the exact range of f32"
    out = a.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), a.astype(np.float64))
    return out


def _rng(tag, *key):
    return np.random.default_rng([tag, *[int(k) for k in key]])


def _ints(rng, bound, shape) -> np.ndarray:
    """Uniform integers in [-bound, bound] as f32."""
    return rng.integers(-bound, bound + 1, size=shape, dtype=np.int16).astype(np.float32)


def _amax(a) -> int:
    return int(np.abs(a).max()) if a.size else 0


# ------------------------------------------------------------------------------------------ embedding gradient
# documented in csrc/embed.hip: one wave per (slice of 128 tokens, 64-column chunk), at most 2048 slices (longer slices beyond
# that); rows narrower than 64 put 64 / E' tokens side by side in sub-tables, E' = E rounded up to a power of two; the LDS
# table is V * 256 bytes, and beyond 48 KB the launcher raises the kernel's dynamic-LDS limit
EMB_TOKENS_PER_SLICE, EMB_SLICES_MAX, EMB_CHUNK = 128, 2048, 64
EMB_PATTERNS = ("uniform", "one_row", "missing", "ends")


def emb_subtables(E: int) -> int:
    ep = 1
    while ep < min(E, EMB_CHUNK):
        ep *= 2
    return EMB_CHUNK // ep


def emb_slices(T: int) -> int:
    return min(max(-(-T // EMB_TOKENS_PER_SLICE), 1), EMB_SLICES_MAX)


def emb_slice_len(T: int) -> int:
    return -(-T // emb_slices(T))


def emb_lds_bytes(V: int) -> int:
    return V * EMB_CHUNK * 4


@dataclass(frozen=True)
class EmbGrad:
    T: int
    V: int
    E: int
    pattern: str

    @property
    def id(self):
        return f"T{self.T}-V{self.V}-E{self.E}-{self.pattern}"

    def idx(self) -> np.ndarray:
        rng = _rng(1, self.T, self.V, self.E, EMB_PATTERNS.index(self.pattern))
        T, V = self.T, self.V
        if self.pattern == "uniform":
            return rng.integers(0, V, T, dtype=np.int64)
        if self.pattern == "one_row":
            return np.full(T, V // 2, dtype=np.int64)
        if self.pattern == "missing":  # even rows only: every odd row must come out +0.0
            return 2 * rng.integers(0, (V + 1) // 2, T, dtype=np.int64)
        assert self.pattern == "ends"
        return np.where(rng.integers(0, 2, T) == 1, V - 1, 0).astype(np.int64)

    def dout(self) -> np.ndarray:
        """[T, E], |.| <= 3; the last token +-4 in every column (the sign depends on the column)."""
        d = _ints(_rng(2, self.T, self.V, self.E), 3, (self.T, self.E))
        d[-1] = np.where((np.arange(self.E) * 5 // 3) % 2 == 0, 4.0, -4.0)
        return d

    def bound(self) -> int:
        return 4 * self.T

    def expected(self, idx=None, dout=None, keep=None) -> np.ndarray:
        """int64 [V, E]. ``keep``: a boolean mask of the tokens that count (the emulated defects of the CPU self-tests)."""
        idx = self.idx() if idx is None else idx
        d = (self.dout() if dout is None else dout).astype(np.int64)
        if keep is not None:
            idx, d = idx[keep], d[keep]
        out = np.zeros((self.V, self.E), dtype=np.int64)
        np.add.at(out, idx, d)
        return out


def _eg(T, V, E, pattern):
    return EmbGrad(T, V, E, pattern)


EMB_GRAD = [
    _eg(1, 6, 1, "uniform"), _eg(999, 193, 1, "missing"),
    _eg(127, 6, 2, "ends"), _eg(4096, 225, 2, "uniform"),
    _eg(128, 6, 3, "missing"), _eg(999, 192, 3, "uniform"),
    _eg(129, 6, 5, "one_row"), _eg(4096, 193, 5, "ends"),
    _eg(127, 225, 8, "missing"), _eg(999, 1, 8, "uniform"),
    _eg(128, 192, 12, "ends"), _eg(4096, 6, 12, "missing"),
    _eg(1, 6, 16, "one_row"), _eg(999, 225, 16, "uniform"),
    _eg(129, 6, 17, "uniform"), _eg(4096, 192, 17, "one_row"),
    _eg(127, 193, 32, "uniform"), _eg(4096, 6, 32, "ends"),
    _eg(128, 6, 33, "missing"), _eg(999, 225, 33, "ends"),
    _eg(129, 6, 64, "missing"), _eg(4096, 512, 64, "uniform"), _eg(4096, 512, 64, "missing"),
    _eg(127, 6, 65, "uniform"), _eg(999, 193, 65, "missing"),
    _eg(128, 225, 100, "uniform"), _eg(4096, 6, 100, "one_row"),
    # E = 4096 (64 chunks) at V = 4: T = 300 and, so that this width too sees two T, a slice that is one token short
    _eg(300, 4, 4096, "uniform"), _eg(127, 4, 4096, "missing"),
    # beyond 2048 slices of 128 tokens: the last full one, then longer slices with empty ones at the end
    _eg(262144, 6, 4, "uniform"), _eg(262145, 6, 4, "missing"), _eg(300001, 6, 4, "ends"), _eg(300001, 6, 4, "one_row"),
]


# ------------------------------------------------------------------------------------------ embedding forward
# documented in csrc/embed.hip: a thread writes one float4; at most 8192 workgroups of 256 threads, a grid-stride loop beyond
STRIDE_GRID, STRIDE_THREADS = 8192, 256


@dataclass(frozen=True)
class EmbFwd:
    B: int
    N: int
    V: int
    E: int
    pos: bool

    @property
    def id(self):
        return f"B{self.B}-N{self.N}-V{self.V}-E{self.E}-{'pos' if self.pos else 'nopos'}"

    @property
    def T(self):
        return self.B * self.N

    def vectors(self) -> int:
        return self.T * self.E // 4

    def idx(self) -> np.ndarray:
        return _rng(3, self.B, self.N, self.V).integers(0, self.V, self.T, dtype=np.int64)

    def table(self) -> np.ndarray:
        return _ints(_rng(4, self.V, self.E), 2000, (self.V, self.E))

    def pos_rows(self) -> Optional[np.ndarray]:
        return _ints(_rng(5, self.N, self.E), 2000, (self.N, self.E)) if self.pos else None

    def bound(self) -> int:
        return _amax(self.table()) + (_amax(self.pos_rows()) if self.pos else 0)

    def expected(self, idx=None) -> np.ndarray:
        idx = self.idx() if idx is None else idx
        out = self.table().astype(np.int64)[idx]
        if self.pos:
            out = out + self.pos_rows().astype(np.int64)[np.arange(self.T) % self.N]
        return out


EMB_FWD = [EmbFwd(1, 1, 1, 4, False), EmbFwd(3, 7, 6, 4, True), EmbFwd(7, 10000, 6, 128, True), EmbFwd(2, 2049, 512, 32, False)]


# ------------------------------------------------------------------------------------------ affine rows
@dataclass(frozen=True)
class Affine:
    T: int
    K: int
    E: int
    bias: bool

    @property
    def id(self):
        return f"T{self.T}-K{self.K}-E{self.E}-{'bias' if self.bias else 'nobias'}"

    def positions_per_workgroup(self) -> int:
        return STRIDE_THREADS // (self.E // 4)

    def x(self) -> np.ndarray:
        return _ints(_rng(6, self.T, self.K, self.E), 7, (self.T, self.K))

    def w(self) -> np.ndarray:
        return _ints(_rng(7, self.K, self.E), 7, (self.E, self.K))

    def b(self) -> Optional[np.ndarray]:
        return _ints(_rng(8, self.K, self.E), 7, (self.E,)) if self.bias else None

    def bound(self) -> int:
        return int((np.abs(self.x()).astype(np.int64) @ np.abs(self.w()).astype(np.int64).T).max()) + (_amax(self.b()) if self.bias else 0)

    def expected(self) -> np.ndarray:
        out = self.x().astype(np.int64) @ self.w().astype(np.int64).T
        return out + self.b().astype(np.int64) if self.bias else out


AFFINE = [
    Affine(85, 1, 4, True), Affine(86, 3, 4, False), Affine(85, 2, 12, False), Affine(86, 1, 12, True),
    Affine(1, 3, 256, True), Affine(86, 2, 256, False),
    Affine(1, 2, 516, True), Affine(85, 3, 516, False), Affine(86, 1, 516, True), Affine(8193, 2, 516, False),
    Affine(1, 1, 1024, False), Affine(85, 2, 1024, True), Affine(86, 3, 1024, False), Affine(8193, 3, 1024, True),
    # 600 000 positions: at E = 4 a workgroup takes 256 of them (8192 x 256 > T, one trip); at E = 16 it takes 64, and
    # 8192 x 64 < T sends the first workgroups round the stride loop a second time with more than one position each
    Affine(600000, 2, 4, True), Affine(600000, 3, 16, True),
]


# ------------------------------------------------------------------------------------------ head forward
# documented in include/psf_chord.h and csrc/flat_head.hip: a workgroup owns a chunk of K and 8 batch rows; the chunk is 4096
# floats, or 1024 when 4096-float chunks would leave fewer than 1024 workgroups
HEAD_ROWS = 8


def head_chunk(B: int, K: int) -> int:
    return 4096 if -(-K // 4096) * -(-B // HEAD_ROWS) >= 1024 else 1024


@dataclass(frozen=True)
class HeadFwd:
    B: int
    K: int
    J: int
    bias: bool = True
    rows_of: int = 0  # > 0: X is the first B rows of the X of the case with this many rows (same K, same W)

    @property
    def id(self):
        return f"B{self.B}-K{self.K}-J{self.J}" + ("" if self.bias else "-nobias")

    def chunk(self) -> int:
        return head_chunk(self.B, self.K)

    def x(self) -> np.ndarray:
        rows = max(self.B, self.rows_of)
        return _ints(_rng(9, rows, self.K), 2, (rows, self.K))[:self.B]

    def w(self) -> np.ndarray:
        return _ints(_rng(10, self.K, self.J), 2, (self.J, self.K))

    def b(self) -> Optional[np.ndarray]:
        return _ints(_rng(11, self.K, self.J), 100, (self.J,)) if self.bias else None

    def bound(self) -> int:
        return 4 * self.K + (_amax(self.b()) if self.bias else 0)

    def expected(self, x=None, w=None, cols=None) -> np.ndarray:
        """float64 [B, J]. ``cols``: only these columns of K count (the emulated defect of the CPU self-tests)."""
        x = (self.x() if x is None else x).astype(np.float64)
        w = (self.w() if w is None else w).astype(np.float64)
        if cols is not None:
            x, w = x[:, cols], w[:, cols]
        out = x @ w.T
        return out + self.b().astype(np.float64) if self.bias else out


_KBIG = 63 * 4096 + 12
HEAD_FWD = [
    HeadFwd(1, 4, 1), HeadFwd(9, 4, 3, bias=False), HeadFwd(8, 1020, 3), HeadFwd(9, 1020, 8), HeadFwd(9, 1024, 8), HeadFwd(1, 1024, 3),
    HeadFwd(1, 1028, 8), HeadFwd(8, 1028, 1, bias=False), HeadFwd(9, 4096 + 12, 3), HeadFwd(8, 4096 + 12, 1),
    HeadFwd(128, _KBIG, 3), HeadFwd(120, _KBIG, 3, rows_of=128), HeadFwd(128, _KBIG, 1), HeadFwd(1024, 7 * 4096 + 4, 8),
]
HEAD_FWD_LARGE_CHUNK = [(128, _KBIG, 3), (128, _KBIG, 1), (1024, 7 * 4096 + 4, 8)]  # (B, K, J) on the 4096-float side
HEAD_FWD_ACROSS = ((128, _KBIG, 3), (120, _KBIG, 3))  # the same rows on both sides of the rule


# ------------------------------------------------------------------------------------------ head backward
HEAD_BWD_MAX_B, HEAD_BWD_MAX_J = 1024, 16  # include/psf_chord.h; dY is staged in B * J * 4 bytes of LDS


@dataclass(frozen=True)
class HeadBwd:
    B: int
    K: int
    J: int
    want_dx: bool
    want_dw: bool

    @property
    def id(self):
        return f"B{self.B}-K{self.K}-J{self.J}-{'dX' if self.want_dx else ''}{'dW' if self.want_dw else ''}"

    def dy(self) -> np.ndarray:
        return _ints(_rng(12, self.B, self.K, self.J), 3, (self.B, self.J))

    def x(self) -> np.ndarray:
        return _ints(_rng(13, self.B, self.K, self.J), 3, (self.B, self.K))

    def w(self) -> np.ndarray:
        return _ints(_rng(14, self.B, self.K, self.J), 3, (self.J, self.K))

    def bound(self) -> int:
        return 9 * max(self.B, self.J)

    def expected(self, rows=None):
        """(dX [B, K], dW [J, K]) in float64. ``rows``: only these batch rows are visited (the emulated defect of the CPU
        self-tests): the others add nothing to dW and their dX stays unwritten (NaN)."""
        dy, x, w = self.dy().astype(np.float64), self.x().astype(np.float64), self.w().astype(np.float64)
        dX = dy @ w
        if rows is not None:
            seen = np.zeros(self.B, dtype=bool)
            seen[rows] = True
            dX[~seen] = np.nan
            dy, x = dy[seen], x[seen]
        return dX, dy.T @ x


def _hb(B, K, J, what):
    return HeadBwd(B, K, J, "x" in what, "w" in what)


HEAD_BWD = [
    _hb(1, 4, 1, "xw"), _hb(7, 252, 5, "xw"), _hb(8, 256, 16, "x"), _hb(9, 260, 1, "w"), _hb(9, 4096, 5, "x"), _hb(8, 260, 16, "w"),
    _hb(7, 4, 16, "xw"), _hb(1, 256, 5, "w"), _hb(9, 252, 1, "x"), _hb(1024, 260, 1, "xw"), _hb(1024, 4096, 16, "xw"),
]


# ------------------------------------------------------------------------------------------ weight gradient
@dataclass(frozen=True)
class WGrad:
    T: int
    m: int
    n: int
    strided: bool  # X and dY are column slices of arrays with ldx = m + 3, ldy = n + 5 columns, the rest NaN
    need_bias: bool

    @property
    def id(self):
        return f"T{self.T}-m{self.m}-n{self.n}-{'slices' if self.strided else 'dense'}-{'db' if self.need_bias else 'nodb'}"

    X_OFF, DY_OFF = 2, 3  # first column of the slice inside the wide array

    @property
    def ldx(self):
        return self.m + 3 if self.strided else self.m

    @property
    def ldy(self):
        return self.n + 5 if self.strided else self.n

    def x(self) -> np.ndarray:
        return _ints(_rng(15, self.T, self.m, self.n), 3, (self.T, self.m))

    def dy(self) -> np.ndarray:
        return _ints(_rng(16, self.T, self.m, self.n), 2, (self.T, self.n))

    def wide(self):
        """(X wide [T, ldx], dY wide [T, ldy]): the slices at columns X_OFF.. / DY_OFF.., NaN everywhere else."""
        assert self.strided
        xw = np.full((self.T, self.ldx), np.nan, dtype=np.float32)
        yw = np.full((self.T, self.ldy), np.nan, dtype=np.float32)
        xw[:, self.X_OFF:self.X_OFF + self.m] = self.x()
        yw[:, self.DY_OFF:self.DY_OFF + self.n] = self.dy()
        return xw, yw

    def bound(self) -> int:
        return 6 * self.T

    def expected(self):
        """(dWt [n, m], db [n]) in float64."""
        dy = self.dy().astype(np.float64)
        return dy.T @ self.x().astype(np.float64), dy.sum(0)


WGRAD = [
    WGrad(1, 1, 1, False, True), WGrad(2, 1, 128, True, True), WGrad(15, 128, 1, False, False), WGrad(17, 128, 128, False, True),
    WGrad(31, 33, 65, True, False), WGrad(4097, 32, 15, False, True), WGrad(100003, 33, 65, False, True),
    WGrad(100003, 128, 128, True, True), WGrad(1, 128, 128, False, False), WGrad(2, 33, 65, False, True),
    WGrad(15, 32, 15, True, True), WGrad(17, 1, 1, True, False), WGrad(31, 1, 128, False, False), WGrad(4097, 128, 1, True, True),
    WGrad(4097, 128, 128, False, False), WGrad(100003, 1, 1, False, False),
]


# ------------------------------------------------------------------------------------------ ids outside the table
CLAMP_BAND_ROWS = 4           # NaN rows on either side of the table in the clamping tests: a missing clamp reads NaN, in bounds


def with_out_of_range_ids(idx: np.ndarray, V: int, seed: int) -> np.ndarray:
    """``idx`` with about 1 % of its positions, the first and the last always among them, replaced by -2, -1, V or V + 1."""
    rng = _rng(17, seed, V, idx.size)
    flat = idx.reshape(-1).copy()
    hit = rng.random(flat.size) < 0.01
    hit[0] = hit[-1] = True
    which = rng.integers(0, 4, flat.size)
    which[0], which[-1] = 1, 2  # -1 at the first token, V at the last
    bad = np.array([-2, -1, V, V + 1], dtype=np.int64)[which]
    flat[hit] = bad[hit]
    return flat.reshape(idx.shape)


EMB_GRAD_CLAMPED = [EmbGrad(999, 6, 8, "uniform"), EmbGrad(4096, 193, 65, "uniform")]
EMB_FWD_CLAMPED = [EmbFwd(3, 700, 6, 32, True), EmbFwd(2, 1025, 225, 16, False)]
