"""Known-answer inputs for the split-bf16 producer kernels (the MLPBlock forward and backward, csrc/mlp_x3_common.h).

Every f32 operand of those kernels is split exactly into three bf16 terms t1 + t2 + t3 by truncation, and each product
keeps six of the nine term products (csrc/mlp_x3_common.h). The kernels' summation order is fixed but not specified
here. The inputs built below make that order irrelevant, so the right answer is bit-exact:

* Linear GELU regime: every live pre-activation is >= LIVE and every dead one <= DEAD. There the kernels' GELU returns
  exactly x or 0 and its derivative exactly 1 or 0 (checked by ``gelu_regime_ok`` on numpy f32 ports of the formulas).
* Grids: every tensor is on a grid k 2^s. For every output of every GEMM the sum of |terms| stays below 2^24 units of the
  coarsest grid that all its terms share, so every partial sum is exact in f32 whatever the order (``check_exact``).
* Split: in every product x w the three dropped term products t2 t3', t3 t2', t3 t3' are zero, i.e. the split levels
  (number of nonzero terms) add up to at most 4, while some operands do carry a nonzero third term (``coverage``).

Three constructions, each exact on its own; together every split operand of every GEMM carries third terms:

  "x"  : X with 17 significant bits (and 9-bit values against 9-bit weights: the t2 t2' product); A, B, dY small
         integers or powers of two. Third terms in X (forward, recompute, dA) and H (second layer, dB).
  "w"  : X and dY small integers; A with 17-bit values in every other hidden row, B with 17-bit values on the outputs
         that read the integer rows. Third terms in A (forward, dX), B (second layer, dHpost) and G (dA, dX).
  "dy" : X, A, B integers; dY with 17-bit values on a few tokens. Third terms in dY (dHpost, dB) and G (dA, dX).

dY is nonzero on a few tokens per output, the last token of the (ragged) last tile always among them; the last hidden
row, the last column of E and the last output always carry the construction's hard values.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

LIVE, DEAD = 16.0, -32.0
UNITS = 2.0 ** 24


# ---------------------------------------------------------------- the split (numpy port of psf_x3::split3)
def split3(v):
    """(t1, t2, t3) of f32 values: t1 = v with the low 16 bits cleared, t2 = the same of v - t1, t3 = the rest."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    t1 = (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = (v - t1).astype(np.float32)
    t2 = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    t3 = (r1 - t2).astype(np.float32)
    return t1, t2, t3


def level(v) -> np.ndarray:
    """Number of nonzero split terms: 0 for zero, 1 for bf16 values, 2 when t3 = 0, else 3 (t2 = 0 implies t3 = 0)."""
    t1, t2, t3 = split3(v)
    return np.where(t3 != 0, 3, np.where(t2 != 0, 2, np.where(t1 != 0, 1, 0))).astype(np.int8)


def grid_exp(v) -> np.ndarray:
    """Elementwise s of the largest 2^s that divides v (a large sentinel for zeros)."""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2(np.maximum(mi & -mi, 1).astype(np.float64)).astype(np.int64)
    return np.where(v != 0, e - 53 + low, 1 << 20)


def out_grid_exp(P, Q) -> np.ndarray:
    """For C = P Q: per output, s of the coarsest grid 2^s that every nonzero term P[i,k] Q[k,j] lies on (a min-plus
    product of the entries' grid exponents, over the few distinct exponents)."""
    gp, gq = grid_exp(P), grid_exp(Q)
    out = np.full((gp.shape[0], gq.shape[1]), 1 << 20, dtype=np.int64)
    for s in np.unique(gp[gp < (1 << 20)]):
        ms = (gp == s).astype(np.float32)
        for r in np.unique(gq[gq < (1 << 20)]):
            hit = (ms @ (gq == r).astype(np.float32)) > 0
            out = np.where(hit, np.minimum(out, s + r), out)
    return out


# ---------------------------------------------------------------- GELU ports (f32, as the kernels evaluate them)
def _f(x):
    return np.float32(x)


def gelu_as(x):
    """gelu2 / gelu_and_grad (csrc/mlp_x3_image.h, mlp_bwd.hip, mlp_wide.hip, x3_gemm.h): Phi by A&S 26.2.17, x Phi and
    dy/dx = fma(x 0.39894, E, Phi). The reciprocal is exact here where the kernels use v_rcp_f32: it only feeds q, which
    the vanishing E multiplies."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        t = (_f(1.0) / (np.abs(x) * _f(0.2316419) + _f(1.0))).astype(np.float32)
        p = _f(0.53070271) * t + _f(-0.72657602)
        p = p * t + _f(0.71070687)
        p = p * t + _f(-0.14224837)
        p = p * t + _f(0.12741479)
        p = (p * t).astype(np.float32)
        E = np.exp2((x * x) * _f(-0.72134752044448170368)).astype(np.float32)
        dlt = np.copysign((_f(0.5) - p * E).astype(np.float32), x)
        phi = (_f(0.5) + dlt).astype(np.float32)
        y = (x * phi).astype(np.float32)
        dydx = ((x.astype(np.float64) * np.float64(_f(0.39894228040143267794))) * E + phi).astype(np.float32)
    return y, dydx


def gelu_erf(x):
    """gelu_erf (csrc/mlp_fwd.hip, the f32-MFMA forward variants): 0.5 x (1 + erf(x / sqrt 2)), erf by A&S 7.1.26."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        z = (x * _f(0.70710678118654752440)).astype(np.float32)
        ax = np.abs(z)
        t = (_f(1.0) / (_f(0.3275911) * ax + _f(1.0))).astype(np.float32)
        p = _f(1.061405429) * t + _f(-1.453152027)
        p = p * t + _f(1.421413741)
        p = p * t + _f(-0.284496736)
        p = p * t + _f(0.254829592)
        e = np.exp(-ax * ax).astype(np.float32)
        erf = np.copysign((_f(1.0) - (p * t) * e).astype(np.float32), z)
        return (_f(0.5) * x * (_f(1.0) + erf)).astype(np.float32)


def gelu_regime_ok(h) -> bool:
    """Every value of ``h`` is in the linear regime, where both GELU forms give exactly x or 0 and the derivative 1 or 0."""
    h = np.asarray(h, dtype=np.float32).ravel()
    if not np.all((h >= LIVE) | (h <= DEAD)):
        return False
    y, d = gelu_as(h)
    ye = gelu_erf(h)
    want = np.where(h > 0, h, np.float32(0))
    return bool(np.array_equal(y, want) and np.array_equal(ye, want) and np.array_equal(d, (h > 0).astype(np.float32)))


# ---------------------------------------------------------------- the constructions
@dataclass
class Case:
    kind: str
    X: np.ndarray                                    # [T, E] f32
    params: List[Tuple[np.ndarray, ...]]             # per MLP (A [h, E], a [h], B [O, h], b [O]) f32
    dYs: List[np.ndarray]                            # per MLP [T, O] f32
    _ref: Optional[Dict[str, object]] = field(default=None, repr=False)

    @property
    def T(self):
        return self.X.shape[0]

    def reference(self):
        """The float64 results (exact in f32 for a valid construction): Y_k, Hpre_k, G_k, dX, (dA, da, dB, db)_k."""
        if self._ref is None:
            X = self.X.astype(np.float64)
            ys, hs, gs, grads = [], [], [], []
            dX = np.zeros_like(X)
            for (A, a, B, b), dY in zip(self.params, self.dYs):
                A, a, B, b, dY = (t.astype(np.float64) for t in (A, a, B, b, dY))
                H = X @ A.T + a
                Hp = np.where(H > 0, H, 0.0)
                G = np.where(H > 0, dY @ B, 0.0)
                ys.append(Hp @ B.T + b)
                hs.append(H)
                gs.append(G)
                dX += G @ A
                grads.append((G.T @ X, G.sum(0), dY.T @ Hp, dY.sum(0)))
            self._ref = {"Y": ys, "H": hs, "G": gs, "dX": dX, "grads": grads}
        return self._ref


def _hard(rng, n, base, grid_exp, bits=17):
    """±(base + r 2^grid_exp): values of ``bits`` significant bits when base = 2^(grid_exp + bits - 1)."""
    r = rng.integers(1, 2 ** (bits - 1), size=n)
    r |= 1 | 1 << (bits - 9)  # the bits just below t1 and the lowest one: the rest after t1 spans 9 bits, t3 != 0
    return (rng.choice([-1.0, 1.0], size=n) * (base + r * 2.0 ** grid_exp)).astype(np.float32)


def _ints(rng, shape, lo, hi, zero_frac=0.0):
    v = rng.integers(lo, hi + 1, size=shape).astype(np.float32)
    if zero_frac:
        v[rng.random(shape) < zero_frac] = 0
    return v


def _row_map(h, O):
    """j*(o): the one hidden row output o reads; output 0 reads the last row."""
    return [(h - 1 - 3 * o) % h for o in range(O)]


def _dead(h, j):
    return h > 2 and j != h - 1 and j % 7 == 5


def make_case(kind: str, T: int, E: int, layers, seed: int = 0, per_col: int = 3, row_cap: int = 12,
              tok_cap: int = 24) -> Case:
    """A known-answer case of construction ``kind`` ("x", "w" or "dy") for MLPs Linear(E, h) -> GELU -> Linear(h, O)."""
    assert kind in ("x", "w", "dy") and E % 4 == 0
    rng = np.random.default_rng(seed)
    mid = np.arange(E) % 4 == 1  # kind "x": 9-bit X against 9-bit weights (the t2 t2' product)
    if kind == "x":
        X = _hard(rng, T * E, 256.0, -8).reshape(T, E)              # 17 bits in [256, 512)
        Xm = (rng.choice([-1.0, 1.0], size=(T, E)) * (256.0 + (rng.integers(0, 128, size=(T, E)) * 2 + 1))).astype(np.float32)
        X[:, mid] = Xm[:, mid]                                        # 9 bits
        # patterns with zero bytes inside: 256 + 2^-8 (t2 far below t1) and 256 + 1 + 2^-8 (t2 = 1, t3 = 2^-8)
        X[-1, -1] = 256.0 + 2.0 ** -8
        X[-1, E - 2] = -(256.0 + 1.0 + 2.0 ** -8)
        X[0, -1] = 511.0 + 255 * 2.0 ** -8  # 17 ones
    else:
        X = _ints(rng, (T, E), -2, 2, 0.3)
    params, dYs = [], []
    tok_load = np.zeros(T, np.int64)
    for (h, O) in layers:
        A = np.zeros((h, E), np.float32)
        a = np.zeros(h, np.float32)
        jmap = _row_map(h, O)
        for j in range(h):
            hard_row = (h - 1 - j) % 2 == 0  # kind "w": 17-bit weights in the last row and every other one
            if kind == "x":
                cols = [E - 1 - (7 * j) % E]
                if mid[cols[0]]:
                    A[j, cols[0]] = (rng.choice([-1.0, 1.0]) * 2.0 ** -5 * (1 + (2 * rng.integers(0, 128) + 1) * 2.0 ** -8))
                else:
                    A[j, cols[0]] = rng.choice([-1.0, 1.0]) * 2.0 ** -5
                    c2 = (E - 1 - (7 * j) % E - 1 - 4 * (j % 3)) % E
                    if not mid[c2] and c2 != cols[0] and j % 2:
                        A[j, c2] = rng.choice([-1.0, 1.0]) * 2.0 ** -5
                a[j] = 48.0
            else:
                cols = [E - 1 - (5 * j) % E, (E - 1 - (5 * j) % E - 1 - 16 * (j % 2)) % E]
                for c in dict.fromkeys(cols):
                    if kind == "w" and hard_row:
                        A[j, c] = _hard(rng, 1, 1.0, -16)[0]
                    else:
                        A[j, c] = rng.choice([-1.0, 1.0])
                a[j] = 24.0
            if _dead(h, j):
                a[j] = -80.0 if kind == "x" else -48.0
        B = np.zeros((O, h), np.float32)
        for o, j in enumerate(jmap):
            if kind == "w" and (h - 1 - j) % 2 == 1:
                B[o, j] = _hard(rng, 1, 1.0, -16)[0]
            else:
                B[o, j] = rng.choice([-2.0, -1.0, 1.0, 2.0])
        b = _ints(rng, O, -8, 8)
        # dY: up to per_col tokens per output; the last token for every fourth output and the last one, the last tile's
        # first token for others; loads per hidden row and per token capped (the sums of dA and dX)
        dY = np.zeros((T, O), np.float32)
        row_load = np.zeros(h, np.int64)
        for o in range(O):
            j = jmap[o]
            cands = ([T - 1] if (o % 4 == 0 or o == O - 1) else []) + ([max(T - 32, 0)] if o % 4 == 2 else [])
            cands += rng.integers(0, T, size=2 * per_col).tolist()
            toks = []
            for t in cands:
                if len(toks) < per_col and row_load[j] < row_cap and t not in toks and tok_load[t] < tok_cap:
                    toks.append(t)
                    row_load[j] += 1
                    tok_load[t] += 1
            for t in toks:
                dY[t, o] = _hard(rng, 1, 1.0, -16)[0] if kind == "dy" else rng.choice([-1.0, 1.0])
        if kind == "dy" and T > 1:
            # zero middle byte: 1 + 2^-16 (t1 = 1, t2 = 2^-16) and 1 + 2^-8 + 2^-16 (t2 = 2^-8, t3 = 2^-16), in the last tile
            for o, v in ((0, 1.0 + 2.0 ** -16), (O - 1, -(1.0 + 2.0 ** -8 + 2.0 ** -16))):
                nz = np.flatnonzero(dY[:, o])
                if nz.size:
                    dY[nz[-1], o] = v
        params.append((A, a, B, b))
        dYs.append(dY)
    return Case(kind, X, params, dYs)


# ---------------------------------------------------------------- the checks
def _ind(m):
    return m.astype(np.float32)  # indicator matrices: counts far below 2^24, BLAS products


def _gemms(case: Case):
    """(name, P, Q, bias) of every GEMM C = P Q + bias of the forward and backward, per MLP; dX summed over MLPs."""
    ref = case.reference()
    X = case.X.astype(np.float64)
    out = []
    dx_terms = []
    for k, ((A, a, B, b), dY) in enumerate(zip(case.params, case.dYs)):
        H = ref["H"][k]
        Hp = np.where(H > 0, H, 0.0)
        G = ref["G"][k]
        ones = np.ones((1, case.T))
        out += [(f"H[{k}]", X, A.T, a), (f"Y[{k}]", Hp, B.T, b), (f"dHpost[{k}]", dY, B, None),
                (f"dB[{k}]", dY.T, Hp, None), (f"dA[{k}]", G.T, X, None), (f"da[{k}]", ones, G, None),
                (f"db[{k}]", ones, dY, None)]
        dx_terms.append((G, A))
    out.append(("dX", np.concatenate([g for g, _ in dx_terms], 1), np.concatenate([a for _, a in dx_terms], 0), None))
    return out


def check_exact(case: Case) -> Dict[str, float]:
    """Asserts that the construction is exact: f32 inputs and results, the linear GELU regime, the split condition and
    sum |terms| < 2^24 grid units for every output of every GEMM. Returns the largest sum in grid units per GEMM."""
    for t in [case.X] + [p for ps in case.params for p in ps] + case.dYs:
        assert t.dtype == np.float32 and np.all(np.isfinite(t))
    ref = case.reference()
    for k, H in enumerate(ref["H"]):
        assert gelu_regime_ok(H.astype(np.float32)), f"MLP {k}: pre-activation outside the linear GELU regime"
        assert np.array_equal(H.astype(np.float32).astype(np.float64), H)
    used = {}
    for name, P, Q, bias in _gemms(case):
        P = np.asarray(P, np.float64)
        Q = np.asarray(Q, np.float64)
        gexp = out_grid_exp(P, Q)
        absum = np.abs(P) @ np.abs(Q)
        if bias is not None:
            bias = np.broadcast_to(np.asarray(bias, np.float64), absum.shape)
            gexp = np.minimum(gexp, grid_exp(bias))
            absum = absum + np.abs(bias)
        units = float(np.max(absum * 2.0 ** -np.minimum(gexp, 1000).astype(np.float64))) if absum.size else 0.0
        assert units < UNITS, f"{name}: sum |terms| reaches {units:.3e} grid units (>= 2^24)"
        used[name] = units
        lp, lq = level(P.astype(np.float32)), level(Q.astype(np.float32))
        bad = _ind(lp == 3) @ _ind(lq >= 2) + _ind(lp >= 2) @ _ind(lq == 3)
        assert not bad.any(), f"{name}: {int((bad > 0).sum())} outputs hold a product whose dropped split terms are nonzero"
    for name, v in [("Y", ref["Y"]), ("G", ref["G"]), ("dX", [ref["dX"]])] + [("grad", list(g)) for g in ref["grads"]]:
        for t in v:
            assert np.array_equal(np.asarray(t).astype(np.float32).astype(np.float64), t), f"{name} not exact in f32"
    return used


def coverage(case: Case) -> Dict[str, int]:
    """Per (GEMM, operand): the number of products whose operand has a nonzero third term and whose partner is nonzero."""
    cov = {}
    for name, P, Q, _ in _gemms(case):
        base = name.split("[")[0]
        lp, lq = level(np.asarray(P, np.float32)), level(np.asarray(Q, np.float32))
        cov[base + ".P"] = cov.get(base + ".P", 0) + int((_ind(lp == 3) @ _ind(lq > 0)).sum(dtype=np.float64))
        cov[base + ".Q"] = cov.get(base + ".Q", 0) + int((_ind(lp > 0) @ _ind(lq == 3)).sum(dtype=np.float64))
    return cov


# what each GEMM's operands are (C = P Q): the split operands that must carry third terms across the constructions
OPERANDS = {"H.P": "X", "H.Q": "A", "Y.P": "H", "Y.Q": "B", "dHpost.P": "dY", "dHpost.Q": "B", "dB.P": "dY",
            "dB.Q": "H", "dA.P": "G", "dA.Q": "X", "dX.P": "G", "dX.Q": "A"}


# ---------------------------------------------------------------- emulated defects
TERMS = [(0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0)]  # mfma6's six term products (P term, Q term), smallest first


def _x3(P, Q, drop=None, t3_zero=False, p_two=False):
    """P Q with the kernels' split arithmetic (exact products, float64 sums) and an optional defect: ``drop`` one of the
    six term products, ``t3_zero`` both operands' third terms, ``p_two`` P's third term (G from two bf16 planes)."""
    ps = [t.astype(np.float64) for t in split3(P)]
    qs = [t.astype(np.float64) for t in split3(Q)]
    if t3_zero or p_two:
        ps[2] = np.zeros_like(ps[2])
    if t3_zero:
        qs[2] = np.zeros_like(qs[2])
    return sum(ps[i] @ qs[j] for n, (i, j) in enumerate(TERMS) if n != drop)


def emulate(case: Case, drop=None, t3_zero=False, g_two=False):
    """Forward and backward of the case with the split arithmetic and a defect; same keys as ``Case.reference``."""
    X = case.X
    ys, gs, grads = [], [], []
    dX = 0.0
    kw = dict(drop=drop, t3_zero=t3_zero)
    for (A, a, B, b), dY in zip(case.params, case.dYs):
        H = _x3(X, A.T, **kw) + a
        Hp = np.where(H > 0, H, 0.0).astype(np.float32)
        ys.append(_x3(Hp, B.T, **kw) + b)
        G = np.where(H > 0, _x3(dY, B, **kw), 0.0).astype(np.float32)
        gs.append(G)
        dX = dX + _x3(G, A, p_two=g_two, **kw)
        grads.append((_x3(G.T, X, p_two=g_two, **kw), G.astype(np.float64).sum(0), _x3(dY.T, Hp, **kw),
                      dY.astype(np.float64).sum(0)))
    return {"Y": ys, "G": gs, "dX": dX, "grads": grads}


def differs(case: Case, got) -> bool:
    """Whether any output of ``got`` (an ``emulate`` result) differs from the exact reference."""
    ref = case.reference()
    pairs = list(zip(ref["Y"], got["Y"])) + [(ref["dX"], got["dX"])]
    pairs += [(r, g) for rs, gs in zip(ref["grads"], got["grads"]) for r, g in zip(rs, gs)]
    return any(not np.array_equal(np.asarray(r).astype(np.float32), np.asarray(g).astype(np.float32)) for r, g in pairs)


# ---------------------------------------------------------------- the shapes of the GPU tests (test_gpu_x3_exact.py)
# (T, E, [(h, O), ...]) within the narrow kernels' limits (E <= 32, O <= 32): token counts around the 32-token tile, every
# hidden-width boundary of the 32-row units, outputs around the 16-output boundary; the model widths of MLP_CASES at a
# shorter T
NARROW = [
    (257, 32, [(33, 17), (128, 12), (1, 1), (97, 32), (127, 1)]),
    (4097, 4, [(127, 12), (1, 32), (128, 17)]),
    (31, 28, [(128, 1), (33, 12)]),
    (1, 32, [(33, 12), (97, 32)]),
    (255, 16, [(16, 16)] + [(16, 11)] * 10),            # CIFAR-10 widths
    (4097, 32, [(32, 8)] + [(32, 15)] * 14),            # Adding / Order: g + 14 link MLPs
    (1025, 32, [(128, 32)] + [(128, 13)] * 12),         # IMDb / Pathfinder widths
    (257, 32, [(33, 12)] + [(32, 12)] * 30 + [(128, 1)]),  # K = 32, the narrow kernels' limit: one launch
]
# the f32-MFMA variant with LDS-resident weights needs all K weight images in LDS
RESIDENT = [(4097, 32, [(32, 8)] + [(32, 12)] * 11), (31, 4, [(5, 3), (32, 17)]), (257, 28, [(1, 1), (32, 32)])]

# (T, E, [(h, O), ...]) within the wide kernels' limits (E a multiple of 16, O <= 128, K <= 24)
WIDE = [
    (257, 512, [(128, 128), (100, 127)]),
    (4097, 48, [(96, 33), (33, 1), (128, 20)]),
    (255, 272, [(1, 17), (127, 12), (33, 128)]),
    (31, 16, [(5, 3), (97, 33)]),
    (1, 64, [(64, 12)] * 24),
    (1031, 512, [(128, 128)] + [(128, 12)] * 11),       # reference ListOps widths at a shorter T
]
# every MLP 97..128 hidden rows: the narrow-output second layers can run in the first GEMM's epilogue (wide_fuse = 1)
WIDE_FUSE = [(777, 128, [(128, 96), (128, 12), (100, 15), (128, 32), (97, 1)]), (4097, 48, [(127, 17), (97, 1), (128, 33)])]


# (name, B, N, E, h, C, L, M, residual, mixer_lds values). With mixer_lds = 1 a shape runs on the single-launch mixer only
# where its plan allows (csrc/mixer_lds_inst.hip, plan_mixer_lds: C 4 or 8, N a multiple of 32, at most two token tiles per
# wave, the images of up to four hidden units in LDS); the test asserts psf_mixer_fwd_plan before every run. lds_*: the
# single launch (and the per-step kernels where they also cover the shape), steps_*: the per-step kernels only.
MIXER = [
    ("lds_cfg1", 4, 128, 32, 32, 8, 8, 7, True, (1,)),                 # the per-step kernels do not cover N = 128, C = 8
    ("lds_n512_h100", 2, 512, 32, 100, 8, 10, 4, True, (1, 0)),        # three full 32-row units and a ragged one
    ("lds_n256_c4_h128", 3, 256, 16, 128, 4, 9, 6, False, (1,)),       # four full units
    ("lds_n64_e28_h33", 5, 64, 28, 33, 8, 7, 6, True, (1,)),           # one full unit and a one-row unit
    ("steps_n512_c4_h128", 2, 512, 16, 128, 4, 9, 4, False, (0,)),     # 16 token tiles on 4 waves: steps only
    ("steps_odd", 2, 600, 12, 40, 12, 9, 5, True, (0,)),
    ("steps_imdb", 1, 4097, 32, 128, 32, 13, 3, True, (0,)),
]


def seed(path, T, E):
    """The seed of a GPU test's case, shared with its CPU self-test."""
    return {"narrow": T + 3 * E, "resident": 2 * T + E, "wide": T + 5 * E, "wide_fuse": T + 7 * E}[path]


def mixer_case(kind, B, N, E, h, C, L, M, seed):
    """A forward case for g (h -> C) and M link MLPs (h -> L) on B x N tokens, second layers scaled by 2^-11 so that
    |W| L < 2 and the chain does not grow (a power of two keeps every value exact)."""
    case = make_case(kind, B * N, E, [(h, C)] + [(h, L)] * M, seed=seed)
    case.params = [(A, a, (Bm * 2.0 ** -11).astype(np.float32), (b * 2.0 ** -11).astype(np.float32))
                   for A, a, Bm, b in case.params]
    return case
