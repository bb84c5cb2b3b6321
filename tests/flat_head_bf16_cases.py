"""Known-answer inputs for the bf16 FLATTEN head and its backward (psf_flat_head_bf16, psf_flat_head_bwd_bf16; csrc/flat_head.hip).

The pattern of helper_cases.py, one precision down: every operand is a small integer (exact in bf16), every product is an integer,
and for every output the sum of the |terms| stays at or below LIMIT = 256 = 2^8. Every partial sum of every subset of the terms
is then an integer of magnitude <= 256: exact in f32 in any order, with or without FMA, and — bf16 has 8 significant bits, so
every integer up to 256 is a bf16 value — unchanged by the one rounding at the store. The right answer is therefore exact bits
whatever order a kernel sums in; no order is restated here. Expected answers are computed in float64 and checked by ``as_bf16``.

* Position probes: each row of X (forward) or of dY (backward) has one nonzero, +-1 or +-2, so each output is one product (plus
  the bias). The probe sits at the first and last element of K and on both sides of every boundary the kernels have inside K:
  3/4 (a thread's group of four), 1023/1024 and 4095/4096 (the two chunk lengths of the forward), 255/256 (one workgroup of
  64 threads x 4 of the backward). A probe that is read by the wrong thread, dropped at a chunk edge or counted twice gives
  another integer.
* Dense small-integer cases: X (or dY) has few nonzeros per row, so that sum |terms| <= 256 although K is in the thousands.

The boundaries are the ones include/psf_chord.h and csrc/flat_head.hip document; they place the probes and are asserted by
test_flat_head_bf16_cases_cpu.py, never used to compute an expected value.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

LIMIT = 256  # every integer of magnitude <= 2^8 is a bf16 value

FWD_BOUNDARIES = (4, 1024, 4096)  # first element behind the boundary: thread group, short chunk, long chunk
BWD_BOUNDARIES = (4, 256)         # thread group, one workgroup (64 threads x 4)


def bf16_round_trip(a: np.ndarray) -> np.ndarray:
    """float64 -> f32 -> bf16 (round to nearest even on the f32 bits) -> float64, in numpy alone."""
    f = np.asarray(a, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(f.shape)


def as_bf16(a) -> np.ndarray:
    """An exact integer answer of magnitude <= 256, as f32 holding bf16 values (asserts integrality, range, and the round trip)."""
    a = np.asarray(a, dtype=np.float64)
    assert np.array_equal(a, np.rint(a)), "expected answer is not integral"
    assert a.size == 0 or float(np.abs(a).max()) <= LIMIT, "expected answer leaves the exact range of bf16"
    assert np.array_equal(bf16_round_trip(a), a), "expected answer is not a bf16 value"
    return a.astype(np.float32)


def _rng(tag, *key):
    return np.random.default_rng([tag, *[int(k) for k in key]])


def _ints(rng, bound, shape) -> np.ndarray:
    return rng.integers(-bound, bound + 1, size=shape, dtype=np.int16).astype(np.float32)


def probe_positions(K: int, boundaries) -> Tuple[int, ...]:
    """First and last element of K and both sides of every boundary inside K, ascending, without repeats."""
    pos = {0, K - 1}
    for b in boundaries:
        if b < K:
            pos.update((b - 1, b))
    return tuple(sorted(pos))


_PROBE_VALUES = (1.0, -2.0, 2.0, -1.0)


# ------------------------------------------------------------------------------------------------------ forward
@dataclass(frozen=True)
class FwdCase:
    kind: str  # "probe": row r of X is _PROBE_VALUES[r % 4] at positions()[r]; "dense": nnz nonzeros of +-1 / +-2 per row
    B: int
    K: int
    J: int
    bias: bool = True
    nnz: int = 0

    @property
    def id(self):
        return f"fwd-{self.kind}-B{self.B}-K{self.K}-J{self.J}" + ("" if self.bias else "-nobias")

    def positions(self) -> Tuple[int, ...]:
        return probe_positions(self.K, FWD_BOUNDARIES)

    def x(self) -> np.ndarray:
        x = np.zeros((self.B, self.K), dtype=np.float32)
        if self.kind == "probe":
            for r, p in enumerate(self.positions()):
                x[r, p] = _PROBE_VALUES[r % 4]
            return x
        rng = _rng(21, self.B, self.K, self.J)
        for r in range(self.B):
            at = rng.choice(self.K, size=self.nnz, replace=False)
            x[r, at] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), size=self.nnz)
        return x

    def w(self) -> np.ndarray:
        """[J, K] in -3..3, never zero at a probe (a probe that meets a zero weight shows nothing)."""
        w = _ints(_rng(22, self.K, self.J), 3, (self.J, self.K))
        if self.kind == "probe":
            for p in self.positions():
                col = w[:, p]
                col[col == 0] = 3.0
        return w

    def b(self) -> Optional[np.ndarray]:
        return _ints(_rng(23, self.K, self.J), 100, (self.J,)) if self.bias else None

    def bound(self) -> float:
        """max over outputs of |bias| + sum |x||w|: what every partial sum stays below."""
        t = np.abs(self.x().astype(np.float64)) @ np.abs(self.w().astype(np.float64)).T
        return float(t.max() + (np.abs(self.b()).max() if self.bias else 0))

    def expected(self) -> np.ndarray:
        out = self.x().astype(np.float64) @ self.w().astype(np.float64).T
        return out + self.b().astype(np.float64) if self.bias else out


def _probe_fwd(K, J, bias=True):
    return FwdCase("probe", len(probe_positions(K, FWD_BOUNDARIES)), K, J, bias)


FWD = [
    _probe_fwd(4, 1), _probe_fwd(8, 3, bias=False), _probe_fwd(1028, 8), _probe_fwd(4100, 3), _probe_fwd(8192, 1),
    _probe_fwd(2 * 4096 + 12, 8, bias=False),
    FwdCase("dense", 9, 1028, 3, True, nnz=8), FwdCase("dense", 7, 4096 + 12, 8, True, nnz=12), FwdCase("dense", 1, 1020, 1, False, nnz=40),
]


# ------------------------------------------------------------------------------------------------------ backward
@dataclass(frozen=True)
class BwdCase:
    """dW = dY^T X, dX = dY W. "probe": X has one nonzero per row at positions()[r] (dW there is one product, exact zeros elsewhere
    in that row's sum) and dY one nonzero per row (dX is one product per element); "dense": small integers with few nonzero rows."""
    kind: str
    B: int
    K: int
    J: int
    want_dx: bool = True
    want_dw: bool = True

    @property
    def id(self):
        return f"bwd-{self.kind}-B{self.B}-K{self.K}-J{self.J}-{'dX' if self.want_dx else ''}{'dW' if self.want_dw else ''}"

    def positions(self) -> Tuple[int, ...]:
        return probe_positions(self.K, BWD_BOUNDARIES)

    def dy(self) -> np.ndarray:
        if self.kind == "probe":
            dy = np.zeros((self.B, self.J), dtype=np.float32)
            for r in range(self.B):
                dy[r, (3 * r + 1) % self.J] = _PROBE_VALUES[(r + 1) % 4]
            return dy
        return _ints(_rng(31, self.B, self.K, self.J), 2, (self.B, self.J))

    def x(self) -> np.ndarray:
        if self.kind == "probe":
            x = np.zeros((self.B, self.K), dtype=np.float32)
            for r, p in enumerate(self.positions()):
                x[r, p] = _PROBE_VALUES[r % 4]
            return x
        return _ints(_rng(32, self.B, self.K, self.J), 3, (self.B, self.K))

    def w(self) -> np.ndarray:
        w = _ints(_rng(33, self.B, self.K, self.J), 3, (self.J, self.K))
        if self.kind == "probe":
            for p in self.positions():
                col = w[:, p]
                col[col == 0] = -3.0
        return w

    def bound(self) -> float:
        dy, x, w = (np.abs(a.astype(np.float64)) for a in (self.dy(), self.x(), self.w()))
        return float(max((dy.T @ x).max(), (dy @ w).max()))

    def expected(self):
        dy, x, w = self.dy().astype(np.float64), self.x().astype(np.float64), self.w().astype(np.float64)
        return dy @ w, dy.T @ x


def _probe_bwd(K, J, what="xw"):
    return BwdCase("probe", len(probe_positions(K, BWD_BOUNDARIES)), K, J, "x" in what, "w" in what)


BWD = [
    _probe_bwd(4, 1), _probe_bwd(8, 16), _probe_bwd(260, 5), _probe_bwd(516, 7, "w"), _probe_bwd(260, 16, "x"),
    # dense: |dY| <= 2, |x|, |w| <= 3: sums of at most 6 B (dW) and 6 J (dX) <= 256
    BwdCase("dense", 9, 260, 7), BwdCase("dense", 40, 252, 1, want_dx=False), BwdCase("dense", 17, 256, 16, want_dw=False),
    BwdCase("dense", 42, 1028, 4),
]
