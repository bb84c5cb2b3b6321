"""Known-answer inputs for psf_linear_wgrad_bf16 (csrc/linear_wgrad_bf16.hip) and psf_affine_rows_bf16 (csrc/embed.hip), built on
the CPU alone, with their expected bits.

    dWt[j, i] = rne_bf16(sum_t dY[t, j] X[t, i])        db[j] = rne_bf16(sum_t dY[t, j])

* Position probes: ONE non-zero in X at (t, i) and one in dY at (t, j), values +-1 / +-2. The answer is one product at
  dWt[j, i], one value at db[j], zero elsewhere — a probe that is staged to the wrong plane, transposed wrongly, dropped at a
  slab or tile edge or counted twice gives something else. t runs over {0, 7, 8, 15, 16, T - 1} (the halves of an 8-token
  fragment and of a 16-token matrix step) plus the first and last row of the SECOND wave's slab; (i, j) over the corners of
  every 32-wide tile. The slab length is the kernel's plan, mirrored in ``plan`` (the GPU test checks the mirror against
  psf_linear_wgrad_bf16_workspace).
* Dense small-integer cases: operands in {-2..2}, T <= 4096, so every partial sum of every subset of the terms is an integer
  of magnitude <= 4 * 4096 < 2^24: exact in f32 in any order. The one correct answer is rne_bf16 of the exact integer — sums
  beyond 256 are mostly no bf16 values, so the single rounding at the store is exercised; ``TIE`` puts exact ties there.
* Affine rows: small integers (every sum <= 256 in magnitude: exact in bf16) and single powers of two, K = 1, 2, 3, with and
  without a bias.

Expected answers come from int64 / float64 arithmetic and ``rne_bf16``; test_linear_wgrad_bf16_cases_cpu.py checks them
against a second evaluation.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

TILE_ROWS = 32      # tokens per LDS tile of the kernel: slabs are whole tiles
MAX_WAVES = 8192    # slabs of a launch, before the partial-tile budget
BUDGET_FLOATS = (32 << 20) // 4


def plan(T: int, m: int, n: int) -> dict:
    """The kernel's plan (make_plan of csrc/linear_wgrad_bf16.hip): rows per wave (slab), waves, partial tiles, workspace bytes."""
    tj, ti = -(-n // 32), -(-m // 32)
    tile = tj * ti * 1024
    nw = MAX_WAVES
    if nw // 4 * tile > BUDGET_FLOATS:
        nw = 4 * (BUDGET_FLOATS // tile)
    rpw = -(-T // nw)
    rpw = -(-rpw // TILE_ROWS) * TILE_ROWS
    nw = -(-T // rpw)
    nparts = -(-nw // 4)
    return {"rows_per_wave": rpw, "nwaves": nw, "nparts": nparts, "workspace_bytes": 4 * nparts * (tile + tj * 32)}


def rne_bf16(a) -> np.ndarray:
    """float64 (exactly representable in f32) -> the nearest bf16 value, ties to even, as f32."""
    f = np.asarray(a, dtype=np.float64).astype(np.float32)
    assert np.array_equal(f.astype(np.float64), np.asarray(a, dtype=np.float64)), "not exact in f32"
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(f.shape)


def tile_corners(width: int) -> Tuple[int, ...]:
    """First and last column of every 32-wide tile of ``width`` columns."""
    out = set()
    for c0 in range(0, width, 32):
        out.update((c0, min(c0 + 31, width - 1)))
    return tuple(sorted(out))


def probe_rows(T: int, m: int, n: int) -> Tuple[int, ...]:
    rpw = plan(T, m, n)["rows_per_wave"]
    rows = {0, 7, 8, 15, 16, T - 1, rpw, 2 * rpw - 1}
    assert 2 * rpw - 1 < T, "the case has no complete second slab"
    return tuple(sorted(r for r in rows if r < T))


_PROBE_VALUES = (1.0, -2.0, 2.0, -1.0)


@dataclass(frozen=True)
class Probe:
    T: int
    m: int
    n: int
    t: int
    i: int
    j: int
    vx: float
    vy: float

    def x(self):
        a = np.zeros((self.T, self.m), np.float32)
        a[self.t, self.i] = self.vx
        return a

    def dy(self):
        a = np.zeros((self.T, self.n), np.float32)
        a[self.t, self.j] = self.vy
        return a

    def expected(self):
        dWt, db = np.zeros((self.n, self.m), np.float32), np.zeros(self.n, np.float32)
        dWt[self.j, self.i] = self.vx * self.vy
        db[self.j] = self.vy
        return dWt, db


def probes(T: int, m: int, n: int):
    k = 0
    for t in probe_rows(T, m, n):
        for i in tile_corners(m):
            for j in tile_corners(n):
                yield Probe(T, m, n, t, i, j, _PROBE_VALUES[k % 4], _PROBE_VALUES[(k // 4 + 1) % 4])
                k += 1


#: (T, m, n) of the probe sets: four slabs of 32 rows with a ragged last one; every tile count in one dimension, one in the other
PROBE_SHAPES = ((100, 128, 128), (70, 33, 40), (97, 2, 32))


@dataclass(frozen=True)
class Dense:
    kind: str  # "ints": operands uniform in {-2..2}; "biased": mostly positive, so the sums leave the exact range of bf16;
    T: int     # "tie": counted columns whose sums are exact ties between two bf16 values
    m: int
    n: int
    seed: int = 0

    @property
    def id(self):
        return f"{self.kind}-T{self.T}-m{self.m}-n{self.n}"

    def _rng(self, tag):
        return np.random.default_rng([tag, self.T, self.m, self.n, self.seed])

    def x(self):
        if self.kind == "tie":
            return np.ones((self.T, self.m), np.float32)
        r = self._rng(1)
        if self.kind == "biased":
            return r.choice(np.array([-1, 1, 2, 2], np.float32), size=(self.T, self.m))
        return r.integers(-2, 3, size=(self.T, self.m)).astype(np.float32)

    def dy(self):
        if self.kind == "tie":
            a = np.zeros((self.T, self.n), np.float32)
            for j in range(self.n):
                a[:TIE_COUNTS[j % len(TIE_COUNTS)], j] = 1.0
            return a
        r = self._rng(2)
        if self.kind == "biased":
            return r.choice(np.array([-1, 1, 1, 2], np.float32), size=(self.T, self.n))
        return r.integers(-2, 3, size=(self.T, self.n)).astype(np.float32)

    def exact(self):
        x, dy = self.x().astype(np.int64), self.dy().astype(np.int64)
        return dy.T @ x, dy.sum(0)

    def expected(self):
        dWt, db = self.exact()
        return rne_bf16(dWt.astype(np.float64)), rne_bf16(db.astype(np.float64))


#: rows set to one in a column of dY of a "tie" case: 257 -> 256, 259 -> 260, 261 -> 260 (ties, to the even neighbour), 300 (a value)
TIE_COUNTS = (257, 259, 261, 300)

DENSE = (
    Dense("ints", 1, 3, 8), Dense("ints", 33, 15, 31), Dense("ints", 4096, 32, 32), Dense("ints", 4096, 128, 128),
    Dense("ints", 1000, 2, 32), Dense("ints", 4095, 33, 33),
    Dense("biased", 4096, 32, 8), Dense("biased", 4001, 64, 64), Dense("biased", 3000, 127, 128),
    Dense("tie", 300, 4, 4), Dense("tie", 333, 33, 36),
)


# ------------------------------------------------------------------------------------------------------ affine rows
@dataclass(frozen=True)
class Affine:
    kind: str  # "ints": x in {-4..4}, W in {-3..3}, bias in {-8..8} (|sum| <= 44); "pow2": K = 1, one power of two each
    T: int
    K: int
    E: int
    bias: bool

    @property
    def id(self):
        return f"{self.kind}-T{self.T}-K{self.K}-E{self.E}-{'bias' if self.bias else 'nobias'}"

    def _rng(self, tag):
        return np.random.default_rng([tag, self.T, self.K, self.E, int(self.bias)])

    def x(self):
        r = self._rng(3)
        if self.kind == "pow2":
            return (r.choice([-1.0, 1.0], size=(self.T, 1)) * 2.0 ** r.integers(-20, 21, size=(self.T, 1))).astype(np.float32)
        return r.integers(-4, 5, size=(self.T, self.K)).astype(np.float32)

    def w(self):
        r = self._rng(4)
        if self.kind == "pow2":
            return (r.choice([-1.0, 1.0], size=(self.E, 1)) * 2.0 ** r.integers(-20, 21, size=(self.E, 1))).astype(np.float32)
        return r.integers(-3, 4, size=(self.E, self.K)).astype(np.float32)

    def b(self):
        return self._rng(5).integers(-8, 9, size=self.E).astype(np.float32) if self.bias else None

    def expected(self):
        out = self.x().astype(np.float64) @ self.w().astype(np.float64).T
        if self.bias:
            out = out + self.b().astype(np.float64)
        return rne_bf16(out) + np.float32(0.0)  # (a zero is +0: the chain ends in an add of the bias, or of +0)


AFFINE = tuple(Affine("ints", T, K, E, bias) for K in (1, 2, 3) for bias in (True, False) for T, E in ((37, 8), (300, 40))) + (
    Affine("pow2", 64, 1, 8, False), Affine("pow2", 257, 1, 1024, False), Affine("ints", 5, 2, 1024, True))
