"""Reference and known-answer inputs for the fused bf16 producer backward (psf_mlp_bwd_bf16, csrc/mlp_bwd_bf16.hip).

The contract (include/psf_chord.h): every operand and result is bf16, and for each MLP k, with z and hh as in the forward's
contract (tests/mlp_bf16_ref.py),

    g  = bf16_rne(f32(dY B))            d  = bf16_rne(f32(g) GELU'_f32(z))
    dA = bf16_rne(f32(d^T X))           da = bf16_rne(f32(sum_t d))
    dB = bf16_rne(f32(dY^T hh))         db = bf16_rne(f32(sum_t dY))
    dX = bf16_rne(f32(sum_k d_k A_k))   one rounding over all K MLPs

with exact products and f32 sums in an unspecified order. ``contract`` evaluates that in float64 (optionally with an emulated
defect), ``ref_bwd`` adds the per-element envelope of what any f32 summation order can produce through flipped bf16 ties, and
``true_grad`` is the same gradient with no intermediate rounding at all.

Two constructions make the order irrelevant, so the answer is exact to the bit (compare after mapping -0 to +0):

  "linear"  mlp_bf16_ref.make_linear's forward (small integers, every pre-activation in x3_exact's linear regime, where the
            derivative is exactly 1 or 0) with dY = +-1 on five tokens per output: every partial sum is a small integer and
            every gradient an integer with <= 8 significant bits. ``make_round_once`` is a hand-made member of the family in
            which one MLP's share of a dX element is 257 and another's -1: rounded per MLP the element is 255, rounded once 256.
  "select"  one nonzero +-2^s per row of A and of B, zero first-layer bias, dY = +-2^s on ONE token per output, no token used
            twice: g, d and every element of every gradient is a single product (or zero), rounded once. X only holds values
            whose GELU and GELU' lie further than 4e-7 (|z| + 1) from every bf16 rounding boundary at every scale of A, so hh
            and d are determined; ``check_select`` verifies with x3_exact.gelu_as, the f32 port of the kernels' formula, that
            every value lands on the expected side.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import mlp_bf16_ref as R
from mlp_bf16_ref import bf16_rne, ulp_bf16
from x3_exact import gelu_as, gelu_regime_ok

TILE = 32
GRAD_MARGIN = 4e-7  # the forward's gelu_margin_ok margin, per unit of (|z| + 1) |g|


def gelu_grad64(z):
    """GELU'(z) = Phi(z) + z phi(z) in float64."""
    z = np.asarray(z, np.float64)
    return 0.5 * (1.0 + R.erf64(z / np.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


@dataclass
class Case:
    kind: str
    X: np.ndarray                              # [T, E] bf16-valued float64
    params: List[Tuple[np.ndarray, ...]]       # per MLP (A [h, E], a [h], B [O, h], b [O])
    dYs: List[np.ndarray]                      # per MLP [T, O]
    answers: Optional[Dict[str, object]] = field(default=None, repr=False)  # {"dX": [T, E], "grads": [(dA, da, dB, db)]}

    @property
    def T(self):
        return self.X.shape[0]

    @property
    def E(self):
        return self.X.shape[1]


# ---------------------------------------------------------------- the contract, the envelope, the true gradient
DEFECTS = ("drop_tile", "drop_unit", "db_every_unit", "dx_per_mlp", "skip_last_token", "ignore_o16")


def contract(X, params, dYs, defect: Optional[str] = None, keep: bool = False):
    """The contract in float64: {"dX", "grads": [(dA, da, dB, db)]} (and the intermediates per MLP with ``keep``).
    ``defect``: one of DEFECTS — what a kernel with that bug would return (for the CPU self-test)."""
    assert defect is None or defect in DEFECTS
    X = np.asarray(X, np.float64)
    T = X.shape[0]
    use = np.ones(T, bool)  # tokens whose rows reach the sums
    if defect == "drop_tile":
        use[TILE * ((T - 1) // TILE // 2):][:TILE] = False  # the middle tile (the only one when T <= 32)
    if defect == "skip_last_token" and T % TILE:
        use[-1] = False
    grads, inter = [], []
    dX = np.zeros_like(X)
    for (A, a, B, *_), dY in zip(params, dYs):
        A, a, B, dY = (np.asarray(t, np.float64) for t in (A, a, B, dY))
        h = A.shape[0]
        if defect == "ignore_o16":
            dY = np.where(np.arange(dY.shape[1]) < 16, dY, 0.0)
        dY = np.where(use[:, None], dY, 0.0)
        z = bf16_rne(X @ A.T + a)
        hh = bf16_rne(R.gelu64(z))
        g = bf16_rne(dY @ B)
        d = bf16_rne(g * gelu_grad64(z))
        if defect == "drop_unit" and h > TILE:
            d[:, TILE:2 * TILE] = 0.0
            hh = hh.copy()
            hh[:, TILE:2 * TILE] = 0.0
        units = (h + TILE - 1) // TILE if defect == "db_every_unit" else 1
        grads.append((bf16_rne(d.T @ X), bf16_rne(d.sum(0)), bf16_rne(dY.T @ hh), bf16_rne(units * dY.sum(0))))
        share = d @ A
        dX += bf16_rne(share) if defect == "dx_per_mlp" else share
        inter.append((z, hh, g, d, dY))
    out = {"dX": bf16_rne(dX), "grads": grads}
    if keep:
        out["inter"] = inter
    return out


def ref_bwd(X, params, dYs):
    """(reference, envelope): ``contract`` and, in the same layout, the per-element bound of |result - reference| for any f32
    summation order. Three parts: the ulp of the result (its own rounding may flip); the envelopes of z, hh, g and d pushed
    through |B|, |A|, |X| and |dY| (ez = ulp(z); eh = ulp(hh) + 1.13 ez + 2e-7 (|z| + 1), the forward's; eg = ulp(g);
    ed = ulp(d) + |GELU'| eg + |g| (0.8 ez + 4e-7 (|z| + 1)): 0.8 bounds |GELU''|, 4e-7 covers the f32 evaluation of Phi
    and phi); and n 2^-24 sum |terms| for the f32 accumulation of a sum of n terms."""
    X = np.asarray(X, np.float64)
    T = X.shape[0]
    want = contract(X, params, dYs, keep=True)
    acc = 2.0 ** -24
    env_grads = []
    e_dx = np.zeros_like(X)
    n_dx, abs_dx = 0, np.zeros_like(X)
    for (A, a, B, *_), (z, hh, g, d, dY), (dA, da, dB, db) in zip(params, want["inter"], want["grads"]):
        A, B = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(B, np.float64))
        ez = ulp_bf16(z)
        eh = ulp_bf16(hh) + 1.13 * ez + 2e-7 * (np.abs(z) + 1.0)
        eg = ulp_bf16(g) + B.shape[0] * acc * (np.abs(dY) @ B)
        ed = ulp_bf16(d) + np.abs(gelu_grad64(z)) * eg + np.abs(g) * (0.8 * ez + GRAD_MARGIN * (np.abs(z) + 1.0))
        aX, aY, ad = np.abs(X), np.abs(dY), np.abs(d)
        env_grads.append((ulp_bf16(dA) + ed.T @ aX + T * acc * (ad.T @ aX),
                          ulp_bf16(da) + ed.sum(0) + T * acc * ad.sum(0),
                          ulp_bf16(dB) + aY.T @ eh + T * acc * (aY.T @ np.abs(hh)),
                          ulp_bf16(db) + T * acc * aY.sum(0)))
        e_dx += ed @ A
        abs_dx += ad @ A
        n_dx += A.shape[0]
    env = {"dX": ulp_bf16(want["dX"]) + e_dx + n_dx * acc * abs_dx, "grads": env_grads}
    return {"dX": want["dX"], "grads": want["grads"]}, env


def true_grad(X, params, dYs):
    """The same gradients in float64 with no intermediate rounding."""
    X = np.asarray(X, np.float64)
    dX = np.zeros_like(X)
    grads = []
    for (A, a, B, *_), dY in zip(params, dYs):
        A, a, B, dY = (np.asarray(t, np.float64) for t in (A, a, B, dY))
        z = X @ A.T + a
        d = (dY @ B) * gelu_grad64(z)
        grads.append((d.T @ X, d.sum(0), dY.T @ R.gelu64(z), dY.sum(0)))
        dX += d @ A
    return {"dX": dX, "grads": grads}


NAMES = ("dA", "da", "dB", "db")


def tensors(result) -> List[Tuple[str, np.ndarray]]:
    """[(name, array)] of a result in a fixed order: dX, then dA, da, dB, db per MLP."""
    return [("dX", result["dX"])] + [(f"{n}[{k}]", t) for k, g in enumerate(result["grads"]) for n, t in zip(NAMES, g)]


def worst_in_envelope(got, want, env) -> Tuple[float, str]:
    """(largest |got - want| / envelope, the tensor it is in)."""
    worst, where = 0.0, ""
    for (name, g), (_, w), (_, e) in zip(tensors(got), tensors(want), tensors(env)):
        g = np.asarray(g, np.float64)
        assert g.shape == w.shape, name
        assert np.all(np.isfinite(g)), f"{name} is not finite"
        r = float(np.max(np.abs(g - w) / e)) if g.size else 0.0
        if r > worst:
            worst, where = r, name
    return worst, where


def rms_errors(got, true) -> Dict[str, float]:
    return {name: float(np.sqrt(np.mean((np.asarray(g, np.float64) - t) ** 2))) for (name, g), (_, t) in zip(tensors(got), tensors(true))}


def random_dys(T: int, layers: Sequence[Tuple[int, int]], seed: int):
    rng = np.random.default_rng(seed)
    return [bf16_rne(rng.standard_normal((T, O))) for _, O in layers]


# ---------------------------------------------------------------- "linear"
def _spread_tokens(T: int, n: int, start: int, rng) -> List[int]:
    """n distinct tokens, the i-th in tile (start + i) mod tiles: a running ``start`` visits every tile in turn."""
    tiles = (T + TILE - 1) // TILE
    toks: List[int] = []
    i = 0
    while len(toks) < n:
        t0 = TILE * ((start + i) % tiles)
        t = t0 + int(rng.integers(0, min(TILE, T - t0)))
        if t not in toks:
            toks.append(t)
        i += 1
    return toks


def make_linear(T: int, E: int, layers: Sequence[Tuple[int, int]], seed: int = 0) -> Case:
    X, params, _ = R.make_linear(T, E, layers, seed)
    rng = np.random.default_rng(seed + 1)
    per_col = 5 if T >= 5 else 1  # odd: a sum of +-1 over them is never zero
    dYs, n = [], 0
    for h, O in layers:
        dY = np.zeros((T, O))
        for o in range(O):
            toks = _spread_tokens(T, per_col, n, rng)
            n += per_col
            if o % 4 == 0 or o == O - 1:
                toks[0] = T - 1 if T - 1 not in toks else toks[0]  # the last token of the (ragged) last tile
            dY[toks, o] = rng.choice([-1.0, 1.0], size=len(toks))
        dYs.append(dY)
    return _with_linear_answers(Case("linear", X, params, dYs))


def make_round_once(T: int, E: int = 8) -> Case:
    """Two MLPs whose shares of dX[T - 2, 0] are 257 and -1 (see the module docstring); everything else as "linear"."""
    X = np.zeros((T, E))
    X[:, 0] = 1.0
    X[:, E - 1] = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
    t = T - 2
    A0 = np.zeros((2, E)); A0[:, 0] = 1.0; A0[1, E - 1] = 1.0
    A1 = np.zeros((2, E)); A1[0, 0] = 1.0; A1[1, 1] = 1.0
    eye = np.eye(2)
    dY0 = np.zeros((T, 2)); dY0[t] = (256.0, 1.0); dY0[T - 1] = (0.0, 1.0)
    dY1 = np.zeros((T, 2)); dY1[t] = (-1.0, 0.0); dY1[T - 1] = (1.0, -1.0)
    params = [(A0, np.full(2, 20.0), eye, np.zeros(2)), (A1, np.full(2, 21.0), eye, np.zeros(2))]
    return _with_linear_answers(Case("linear", X, params, [dY0, dY1]))


def _with_linear_answers(case: Case) -> Case:
    X = case.X
    dX = np.zeros_like(X)
    grads = []
    for (A, a, B, b), dY in zip(case.params, case.dYs):
        H = X @ A.T + a
        live = H > 0
        G = np.where(live, dY @ B, 0.0)
        grads.append((G.T @ X, G.sum(0), dY.T @ np.where(live, H, 0.0), dY.sum(0)))
        dX += G @ A
    case.answers = {"dX": dX, "grads": grads}
    return case


def check_linear(case: Case):
    """The construction's own exactness conditions."""
    X, T = case.X, case.T
    covered = np.zeros((T + TILE - 1) // TILE, bool)
    abs_dx = np.zeros_like(X)
    for (A, a, B, b), dY, (dA, da, dB, db) in zip(case.params, case.dYs, case.answers["grads"]):
        for t in (X, A, a, B, dY):
            assert np.array_equal(t, np.rint(t)) and np.max(np.abs(t)) <= 256  # small integers: bf16-exact
        pre = X @ A.T + a
        live = pre > 0
        assert np.all((pre[live] >= 16) & (pre[live] <= 256)) and np.all(pre[~live] <= -32)
        assert gelu_regime_ok(pre.astype(np.float32))  # GELU is exactly x or 0 there, its derivative exactly 1 or 0
        G = np.abs(dY) @ np.abs(B)
        assert np.max(G) <= 256                        # g, d: integers of <= 9 bits ... and bf16 values:
        assert np.array_equal(bf16_rne(dY @ B), dY @ B)
        sums = [np.abs(X) @ np.abs(A).T + np.abs(a), G.T @ np.abs(X), np.abs(dY).T @ np.abs(np.where(live, pre, 0.0)), np.abs(dY).sum(0)]
        assert all(np.max(s) < 2.0 ** 24 for s in sums)  # every partial sum is an exact f32 integer in any order
        abs_dx += G @ np.abs(A)
        for t in (dA, da, dB, db):
            assert np.array_equal(t, np.rint(t)) and np.array_equal(bf16_rne(t), t), "a gradient with more than 8 significant bits"
        assert dY[-1].any() and dY[:, -1].any() and dA[-1].any() and dA[:, -1].any() and db[-1] != 0 and dB[-1].any() and dB[:, -1].any()
        covered |= np.add.reduceat(np.abs(dY).sum(1), np.arange(0, T, TILE)) > 0
    dX = case.answers["dX"]
    assert np.max(abs_dx) < 2.0 ** 24 and np.array_equal(dX, np.rint(dX)) and np.array_equal(bf16_rne(dX), dX)
    assert dX[-1].any() and dX[:, -1].any()
    return bool(covered.all())


# ---------------------------------------------------------------- "select"
_A_SCALES = (-1, 0, 1, 2)
_Y_SCALES = (-2, -1, 0, 1, 2)


def _margin_ok(v, z) -> np.ndarray:
    """Per value: v lies further than GRAD_MARGIN (|z| + 1) from every bf16 rounding boundary."""
    v, z = np.asarray(v, np.float64), np.asarray(z, np.float64)
    r = bf16_rne(v)
    assert np.all(r != 0)
    mag = R.to_bits(np.abs(r)).astype(np.int64)
    up, dn = R.from_bits((mag + 1).astype(np.uint16)), R.from_bits((mag - 1).astype(np.uint16))
    dist = np.minimum(np.abs(np.abs(v) - (np.abs(r) + up) / 2), np.abs(np.abs(v) - (np.abs(r) + dn) / 2))
    return dist > GRAD_MARGIN * (np.abs(z) + 1.0)


@functools.lru_cache(maxsize=None)
def select_values() -> np.ndarray:
    """mlp_bf16_ref.select_values (the GELU's margin) narrowed to values whose GELU' also keeps the margin at every scaling."""
    base = R.select_values()
    ok = np.ones(base.shape, bool)
    for s in _A_SCALES:
        for sign in (-1.0, 1.0):
            z = sign * np.ldexp(base, s)
            ok &= _margin_ok(gelu_grad64(z), z)
    vals = base[ok]
    assert vals.size >= 32 and np.any(vals < 0) and np.any(vals > 0)
    return vals


def _select_rows(h: int, O: int) -> np.ndarray:
    """The hidden row each output reads: distinct rows, output 0 reads the last one."""
    assert O <= h, "select needs a hidden row of its own for every output"
    rows = (h - 1 - 3 * np.arange(O)) % h
    return rows if len(set(rows.tolist())) == O else (h - 1 - np.arange(O)) % h


def make_select(T: int, E: int, layers: Sequence[Tuple[int, int]], seed: int = 0) -> Case:
    rng = np.random.default_rng(seed)
    vals = select_values()
    X = vals[rng.integers(0, vals.size, size=(T, E))]
    n_out = sum(O for _, O in layers)
    assert n_out <= T, "select needs a token of its own for every output of every MLP"
    # tokens: the last one, then one per tile, then whatever is left, each used once; the LAST output of the last MLP gets T - 1
    tiles = (T + TILE - 1) // TILE
    per_tile = [TILE * i + int(rng.integers(0, min(TILE, T - TILE * i))) for i in range(tiles)]
    order = list(dict.fromkeys([T - 1] + [t for t in per_tile if t != T - 1]))
    taken = set(order)
    rest = [t for t in rng.permutation(T).tolist() if t not in taken]
    tokens = (order + rest)[:n_out][::-1]  # reversed: the last (k, o) takes T - 1
    params, dYs, grads = [], [], []
    dX = np.zeros((T, E))
    n = 0
    for h, O in layers:
        A = np.zeros((h, E))
        cols = (E - 1 - 5 * (h - 1 - np.arange(h))) % E  # the last hidden row reads the last column
        A[np.arange(h), cols] = rng.choice([-1.0, 1.0], size=h) * np.ldexp(1.0, rng.choice(_A_SCALES, size=h))
        rows = _select_rows(h, O)
        B = np.zeros((O, h))
        B[np.arange(O), rows] = rng.choice([-1.0, 1.0], size=O) * np.ldexp(1.0, rng.choice(_A_SCALES, size=O))
        dY = np.zeros((T, O))
        toks = np.array(tokens[n:n + O])
        n += O
        dY[toks, np.arange(O)] = rng.choice([-1.0, 1.0], size=O) * np.ldexp(1.0, rng.choice(_Y_SCALES, size=O))
        z = X[:, cols] * A[np.arange(h), cols]              # [T, h], single products
        hh = bf16_rne(R.gelu64(z))
        g_sel = dY[toks, np.arange(O)] * B[np.arange(O), rows]  # per output o: g at (toks[o], rows[o])
        d_sel = bf16_rne(g_sel * gelu_grad64(z[toks, rows]))
        dA, da = np.zeros((h, E)), np.zeros(h)
        dA[rows] = bf16_rne(d_sel[:, None] * X[toks])
        da[rows] = d_sel
        dB = bf16_rne(dY[toks, np.arange(O)][:, None] * hh[toks])  # [O, h]: row o = dY[t_o, o] hh[t_o, :]
        db = dY[toks, np.arange(O)].copy()
        dX[toks, cols[rows]] = bf16_rne(d_sel * A[rows, cols[rows]])
        params.append((A, np.zeros(h), B, np.zeros(O)))
        dYs.append(dY)
        grads.append((dA, da, dB, db))
    return Case("select", X, params, dYs, {"dX": dX, "grads": grads})


def check_select(case: Case):
    X, T = case.X, case.T
    used = np.zeros(T, np.int64)
    for (A, a, B, b), dY, (dA, da, dB, db) in zip(case.params, case.dYs, case.answers["grads"]):
        assert not a.any()
        assert np.all((A != 0).sum(1) == 1) and np.all((B != 0).sum(1) == 1) and np.all((B != 0).sum(0) <= 1)
        assert np.all((dY != 0).sum(0) == 1)
        for t in (A, B, dY):
            nz = np.abs(t[t != 0])
            assert np.array_equal(nz, np.ldexp(1.0, np.round(np.log2(nz)).astype(np.int64)))  # powers of two
        used += (dY != 0).sum(1)
        z = X @ A.T
        assert np.array_equal(z, bf16_rne(z)) and np.max(np.abs(z)) <= 4.0
        assert np.all(R.gelu_margin_ok(z)) and np.all(_margin_ok(gelu_grad64(z), z)), "a value too close to a bf16 rounding boundary"
        # the f32 port of the kernels' formula lands every hh and every d on the expected side
        y32, dd32 = gelu_as(z.astype(np.float32))
        assert np.array_equal(bf16_rne(y32.astype(np.float64)), bf16_rne(R.gelu64(z)))
        g = dY @ B
        assert np.array_equal(bf16_rne(g * dd32.astype(np.float64)), bf16_rne(g * gelu_grad64(z)))
        for t in (dA, da, dB, db):
            assert np.array_equal(t, bf16_rne(t)) and np.all(np.isfinite(t))
        assert dA[-1].any() and dA[:, -1].any() and db[-1] != 0 and dB[-1].any() and dB[:, -1].any()
    assert used.max() == 1, "a token carries the dY of two outputs: dX would be a sum"
    assert case.dYs[-1][-1, -1] != 0, "the last output of the last MLP reads the last token"
    dX = case.answers["dX"]
    assert np.array_equal(dX, bf16_rne(dX)) and dX[-1].any() and dX[:, -1].any()
    return bool(np.all(np.add.reduceat(used, np.arange(0, T, TILE)) > 0))


KINDS = {"linear": (make_linear, check_linear), "select": (make_select, check_select)}

# (T, E, [(h, O), ...]) of the GPU known-answer tests. The kernel: 32-token tiles, 32-row hidden units, eight waves per
# workgroup and partial-sum slot, one tile per wave below 4 089 tiles and two from there on, a stage-1 slice per 16 slots.
ADDING = [(32, 8)] + [(32, 15)] * 14
SHAPES = [
    (31, 8, [(5, 3)]),                                       # under one tile; K = 1; h = 5
    (257, 32, ADDING),                                       # one token past one workgroup's tiles; K = 15; odd O
    (4097, 24, [(128, 32), (33, 17), (33, 1), (128, 16)]),   # 17 partial slots = two stage-1 slices; E = 24; O = 32, 17, 1, 16
    (385, 16, [(16, 11)] * 32),                              # K = 32
    (130816, 8, [(33, 17)]),                                 # 4 088 tiles: the last size with one tile per wave
    (130817, 8, [(33, 17)]),                                 # 4 089 tiles: two tiles per wave
]
# (T, E, layers) of the random-input tests, GPU and CPU
RANDOM = [(4097, 32, ADDING), (1000, 24, [(96, 32), (33, 1), (128, 20)]), (555, 8, [(7, 2)])]


def seed_of(T: int, E: int) -> int:
    return T + 3 * E


def bits_of(result) -> List[Tuple[str, np.ndarray]]:
    """[(name, uint16 bits with -0 mapped to +0)] of a result of bf16-valued arrays."""
    return [(n, R.plus_zero(R.to_bits(t))) for n, t in tensors(result)]
