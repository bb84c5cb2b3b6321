"""Componentwise accuracy and 2^k scaling laws for the split-bf16 producer MLPs: cases, float64 reference, per-element
error scales, the kernels' arithmetic restated with f32 sums, and emulated defects (used by test_x3_scaled_cpu.py without a
GPU and by test_gpu_x3_scaled.py on one). tests/x3_exact.py holds the split (``split3``) and the six kept term products
(``TERMS``); everything here runs in torch on the device it is given, so the GPU tests evaluate it next to the kernels.

    Y_k = GELU(X A_k^T + a_k) B_k^T + b_k          dHpost_k = dY_k B_k        G_k = dHpost_k . GELU'(H_k)
    dX = sum_k G_k A_k     dA_k = G_k^T X     da_k = sum_t G_k     dB_k = dY_k^T GELU(H_k)     db_k = sum_t dY_k

The cases (``make_case``). Dense randn X and dY, A ~ N(0, 1/E), B ~ N(0, 1/h), biases 0.1 randn: pre-activations mostly in
|h| < 4, the curved part of GELU. One ``kind`` of seeded power-of-two scaling, exponents in [-EXT, EXT] = [-12, 12] (within
the +-20 at which even a third split term of a product of three scaled operands stays a normal f32 and bf16 number):
"rows" tokens of X and, independently, tokens of dY; "cols" columns of X; "hidden" rows of A with a; "outs" rows of B with
b and, independently, columns of dY; "flat" nothing. The last token, column, hidden row and output carry +-EXT.

The per-element scale S (``reference``), in units of u = 2^-24, is the first-order bound on what f32 arithmetic may leave
in that element: for a GEMM C = P Q + c every kept or dropped term product and every f32 sum is within u |p||q| of exact
per term, so the GEMM's own share is sum |p||q| + |c|; an operand that is itself a result carries its own scale through
the same |Q|. With D1 = GELU' = Phi + x phi and D2 = GELU'' = phi (2 - x^2):

    S_H   = |X||A|^T + |a|
    dHp   = |D1(H)| S_H + e_Phi |H|                      what S_H and the kernels' approximation of Phi leave in GELU(H)
    S_Y   = |GELU(H)||B|^T + |b| + dHp |B|^T
    S_dH  = |dY||B|                                       dHpost
    S_G   = |D1| S_dH + |dHpost| (|D2| S_H + e_D1) + |G|  e_D1 = e_Phi + |H| phi(H) (H^2 + 3): Phi's error, and x phi from
                                                          exp2 of a twice-rounded argument (relative error H^2 u) and three
                                                          roundings of the products
    S_dX  = sum_k (|G_k| + S_G_k) |A_k|        S_dA = (|G| + S_G)^T |X|        S_da = sum_t (|G| + S_G)
    S_dB  = |dY|^T (|GELU(H)| + dHp)           S_db = sum_t |dY|

e_Phi is the kernels' documented bound on Phi in units of u: 7.5e-8 / 2^-24 for Abramowitz & Stegun 26.2.17 (mlp_x3_image.h,
mlp_bwd.hip, mlp_wide.hip, x3_gemm.h) and for the erf form of mlp_fwd.hip, whose erf by A&S 7.1.26 is within 1.5e-7, i.e.
Phi = (1 + erf) / 2 within 7.5e-8 as well. An element with S = 0 has only zero terms and must be exact (``ratio``).

The ratio of a result is |got - float64 reference| / (u S), maximised per output family. The bar it is held to is NOT taken
from a kernel: ``arith`` restates the documented arithmetic — three-way truncation split, the six kept products exact, f32
sums left to right over the matrix instructions (blocks of 16 contraction indices, per block the six term pairs smallest
first; one instruction adds the exact sum of its 16 products to the f32 accumulator in ONE rounding: ``gemm32``), the
kernels' GELU formulas in f32 — once with every f32 operation rounded to nearest and once with every one rounded toward
zero (the accumulation rounding of the matrix pipe is not pinned here, and v_rcp_f32 / v_exp_f32 are 1-ulp instructions:
rounding every GELU operation toward zero leaves as much), and ``thresholds`` is 2 x the larger of the two modes' ratios per family over all
cases of a path; the 2 is for summation orders other than left to right. (One rounding per single product instead of per
instruction makes the round-toward-zero ratio grow like the square root of the number of adds, to 25 - 650 at these
shapes, above the 2^-16 / u / 3 = 85 that G from two planes can leave at all; the matrix instruction is the unit in which
mlp_x3_common.h documents the arithmetic.) ``DEFECTS`` are the same arithmetic with one thing wrong;
test_x3_scaled_cpu.py asserts each of them lands at least 2 x above the bar.

Scaling laws (``law_a``, ``law_b``, ``law_c``): a power of two commutes with truncation, with exact products and with f32
rounding, so absent under/overflow they hold bit for bit in any fixed summation order.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import x3_exact as xe

U = 2.0 ** -24
EXT = 12
E_PHI = 7.5e-8 / U      # A&S 26.2.17, and (1 + erf) / 2 with erf by A&S 7.1.26 (1.5e-7 / 2), in units of u
FAMILIES = ("Y", "dX", "dA", "da", "dB", "db")
KINDS = ("flat", "rows", "cols", "hidden", "outs")
MODES = ("rn", "rz")


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    kind: str
    X: np.ndarray                                    # [T, E] f32
    params: List[Tuple[np.ndarray, ...]]             # per MLP (A [h, E], a [h], B [O, h], b [O]) f32
    dYs: List[np.ndarray]                            # per MLP [T, O] f32
    name: str = ""
    _cache: Dict = field(default_factory=dict, repr=False, compare=False)

    def operands(self):
        return [self.X] + [p for ps in self.params for p in ps] + list(self.dYs)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def pow2(rng, n, ext=EXT, last=None):
    """n seeded powers of two with exponents in [-ext, ext]; the last one is 2^last (default: +-ext)."""
    k = rng.integers(-ext, ext + 1, size=n)
    k[-1] = (ext if rng.integers(0, 2) else -ext) if last is None else last
    return np.exp2(k.astype(np.float64)).astype(np.float32)


def make_case(kind: str, T: int, E: int, layers, seed: int = 0) -> Case:
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    X = rng.standard_normal((T, E))
    params, dYs = [], []
    for h, O in layers:
        params.append([rng.standard_normal((h, E)) / math.sqrt(E), 0.1 * rng.standard_normal(h),
                       rng.standard_normal((O, h)) / math.sqrt(h), 0.1 * rng.standard_normal(O)])
        dYs.append(rng.standard_normal((T, O)))
    if kind == "rows":
        X = X * pow2(rng, T)[:, None]
        sd = pow2(rng, T)[:, None]
        dYs = [d * sd for d in dYs]
    elif kind == "cols":
        X = X * pow2(rng, E)[None, :]
    elif kind == "hidden":
        for p in params:
            s = pow2(rng, p[0].shape[0])
            p[0], p[1] = p[0] * s[:, None], p[1] * s
    elif kind == "outs":
        for p, k in zip(params, range(len(dYs))):
            s = pow2(rng, p[2].shape[0])
            p[2], p[3] = p[2] * s[:, None], p[3] * s
            dYs[k] = dYs[k] * pow2(rng, p[2].shape[0])[None, :]
    return Case(kind, _f32(X), [tuple(_f32(t) for t in p) for p in params], [_f32(d) for d in dYs],
                name=f"{kind}:T{T}E{E}K{len(layers)}")


def check_normal(case: Case):
    """Every operand's three split terms are zero or normal f32 (= bf16 exponent range) numbers, none infinite."""
    tiny = np.float32(2.0 ** -126)
    for v in case.operands():
        assert np.all(np.isfinite(v))
        for t in xe.split3(v):
            assert not np.any((t != 0) & (np.abs(t) < tiny)), case.name


# ---------------------------------------------------------------- float64 reference and scales
def _t64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).double()


def _phi(H):
    return torch.exp(-0.5 * H * H) / math.sqrt(2.0 * math.pi)


def reference(case: Case, dev="cpu", backward=True):
    """({family: [tensor per MLP] or tensor}, the same of scales S in units of u), float64 on ``dev``; true erf-GELU."""
    key = ("ref", str(dev), backward)
    if key in case._cache:
        return case._cache[key]
    X = _t64(case.X, dev)
    aX = X.abs()
    out = {"Y": [], "dA": [], "da": [], "dB": [], "db": [], "dX": torch.zeros_like(X)}
    S = {"Y": [], "dA": [], "da": [], "dB": [], "db": [], "dX": torch.zeros_like(X)}
    for (A, a, B, b), dY in zip(case.params, case.dYs):
        A, a, B, b, dY = (_t64(t, dev) for t in (A, a, B, b, dY))
        H = X @ A.T + a
        Phi = 0.5 * torch.special.erfc(-H / math.sqrt(2.0))
        phi = _phi(H)
        Hp = H * Phi
        D1 = Phi + H * phi
        S_H = aX @ A.abs().T + a.abs()
        dHp = D1.abs() * S_H + E_PHI * H.abs()
        out["Y"].append(Hp @ B.T + b)
        S["Y"].append(Hp.abs() @ B.abs().T + b.abs() + dHp @ B.abs().T)
        if not backward:
            continue
        D2 = phi * (2.0 - H * H)
        dH = dY @ B
        G = dH * D1
        S_G = D1.abs() * (dY.abs() @ B.abs()) + dH.abs() * (D2.abs() * S_H + E_PHI + H.abs() * phi * (H * H + 3.0)) + G.abs()
        GS = G.abs() + S_G
        out["dX"] += G @ A
        S["dX"] += GS @ A.abs()
        out["dA"].append(G.T @ X)
        S["dA"].append(GS.T @ aX)
        out["da"].append(G.sum(0))
        S["da"].append(GS.sum(0))
        out["dB"].append(dY.T @ Hp)
        S["dB"].append(dY.abs().T @ (Hp.abs() + dHp))
        out["db"].append(dY.sum(0))
        S["db"].append(dY.abs().sum(0))
    case._cache[key] = (out, S)
    return out, S


def ratio(got, ref, S):
    """(max over elements of |got - ref| / (u S), flat index of the worst). Every element counts; where S is 0 the element
    must equal the reference exactly (ratio 0), else the ratio is infinite."""
    err = (got.double() - ref).abs()
    r = torch.where(S > 0, err / (U * torch.where(S > 0, S, torch.ones_like(S))),
                    torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if r.numel() == 0:
        return 0.0, 0
    i = int(torch.argmax(r))
    return float(r.reshape(-1)[i]), i


def ratios(case: Case, got, dev="cpu", families=FAMILIES):
    """{family: (worst ratio, "k=.. index=..")} of a result ``got`` (same layout as ``reference``'s outputs)."""
    ref, S = reference(case, dev, backward=any(f != "Y" for f in families))
    res = {}
    for f in families:
        if f not in got or got[f] is None:
            continue
        if f == "dX":
            r, i = ratio(got[f], ref[f], S[f])
            res[f] = (r, f"element {np.unravel_index(i, tuple(ref[f].shape))}")
            continue
        worst = (-1.0, "")
        for k, (g, r_, s_) in enumerate(zip(got[f], ref[f], S[f])):
            r, i = ratio(g, r_, s_)
            if r > worst[0]:
                worst = (r, f"MLP {k} element {np.unravel_index(i, tuple(r_.shape))}")
        res[f] = worst
    return res


# ---------------------------------------------------------------- the documented arithmetic with f32 sums
_MASK29 = -(1 << 29)


def _round(mode):
    """The f32 rounding of a float64 tensor holding an (almost) exact result: to nearest, or toward zero (the low 29
    bits of the float64 pattern cleared: valid in f32's normal range, which the cases stay in)."""
    if mode == "rn":
        return lambda x: x.float().double()
    return lambda x: (x.contiguous().view(torch.int64) & _MASK29).view(torch.float64)


def split3_t(v):
    """``x3_exact.split3`` on a float64 tensor holding f32 values; three float64 tensors."""
    v32 = v.float().contiguous()
    t1 = (v32.view(torch.int32) & -65536).view(torch.float32)
    r1 = v32 - t1
    t2 = (r1.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return [t1.double(), t2.double(), (r1 - t2).double()]


KB = 16       # the contraction depth of one v_mfma_f32_32x32x16_bf16
KB_F32 = 2    # ... and of one v_mfma_f32_32x32x2_f32 (mlp_fwd.hip)


def gemm32(P, Q, mode, split=True, drop=None, t3_zero=False, p_two=False):
    """P [M, K] Q [K, N] as the matrix pipe sums it: left to right over blocks of KB = 16 contraction indices, and per block
    the six kept term products smallest first (``xe.TERMS``, mfma6 of mlp_x3_common.h); one matrix instruction adds the
    exact sum of its 16 exact products to the f32 accumulator in ONE rounding (``mode``). split False: unsplit operands,
    one instruction per block of KB_F32 = 2 (the f32 matrix instruction of mlp_fwd.hip). The defects of ``x3_exact._x3``: one term
    dropped, both operands' third terms zero, P's third term zero."""
    M, K = P.shape
    N = Q.shape[1]
    if split:
        ps, qs = split3_t(P), split3_t(Q)
        if t3_zero or p_two:
            ps[2] = torch.zeros_like(ps[2])
        if t3_zero:
            qs[2] = torch.zeros_like(qs[2])
        terms = [(ps[i], qs[j]) for n, (i, j) in enumerate(xe.TERMS) if n != drop]
    else:
        terms = [(P, Q)]
    kb = KB if split else KB_F32
    r = _round(mode)
    acc = torch.zeros(M, N, dtype=torch.float64, device=P.device)
    for k0 in range(0, K, kb):
        for p, q in terms:
            acc = r(acc + p[:, k0:k0 + kb] @ q[k0:k0 + kb])
    return acc


def colsum32(P):
    """sum over rows of P [T, N] in f32, first row first (db). Vector adds (v_add_f32) round to nearest in either mode."""
    r = _round("rn")
    acc = torch.zeros(P.shape[1], dtype=torch.float64, device=P.device)
    for t in range(P.shape[0]):
        acc = r(acc + P[t])
    return acc


def _c(v):
    return float(np.float32(v))


def gelu_as(x, r):
    """gelu_and_grad of the kernels (x3_exact.gelu_as) with every f32 operation rounded by ``r``: (x Phi, Phi + x phi)."""
    t = r(1.0 / r(r(x.abs() * _c(0.2316419)) + 1.0))
    p = r(r(_c(0.53070271) * t) + _c(-0.72657602))
    for c in (0.71070687, -0.14224837, 0.12741479):
        p = r(r(p * t) + _c(c))
    p = r(p * t)
    E = r(torch.exp2(r(r(x * x) * _c(-0.72134752044448170368))))
    dlt = torch.copysign(r(0.5 - r(p * E)), x)
    Phi = r(0.5 + dlt)
    return r(x * Phi), r(r(x * _c(0.39894228040143267794)) * E + Phi)


def gelu_erf(x, r):
    """gelu_erf of mlp_fwd.hip (x3_exact.gelu_erf) with every f32 operation rounded by ``r``."""
    z = r(x * _c(0.70710678118654752440))
    ax = z.abs()
    t = r(1.0 / r(r(_c(0.3275911) * ax) + 1.0))
    p = r(r(_c(1.061405429) * t) + _c(-1.453152027))
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = r(r(p * t) + _c(c))
    e = r(torch.exp(-r(ax * ax)))
    erf = torch.copysign(r(1.0 - r(r(p * t) * e)), z)
    return r(r(0.5 * x) * r(1.0 + erf))


DEFECTS = [("drop", n) for n in range(6)] + [("t3_zero", None), ("g_two", None), ("mag", None)]
MAG = 1e-7   # the magnitude-dependent defect: MAG max|tensor| added to every element


def arith(case: Case, mode="rn", dev="cpu", backward=True, erf_f32=False, defect=None):
    """The producers' arithmetic as documented (module docstring), f32 results as float64 tensors in ``reference``'s layout.
    ``erf_f32``: the f32-matrix-instruction forward of mlp_fwd.hip (no split, erf form of GELU; forward only).
    ``defect``: one of ``DEFECTS``."""
    kind, arg = defect if defect else (None, None)
    kw = dict(split=not erf_f32, drop=arg if kind == "drop" else None, t3_zero=kind == "t3_zero")
    g_two = kind == "g_two"
    r = _round(mode)
    X = _t64(case.X, dev)
    Ps = [[_t64(t, dev) for t in p] for p in case.params]
    hs = [p[0].shape[0] for p in Ps]
    Hcat = gemm32(X, torch.cat([p[0] for p in Ps], 0).T, mode, **kw)  # stacked first layers: each output is its own sum
    out = {"Y": [], "dA": [], "da": [], "dB": [], "db": [], "dX": None}
    Gs, j0 = [], 0
    for (A, a, B, b), h, dY in zip(Ps, hs, case.dYs):
        H = r(Hcat[:, j0:j0 + h] + a)
        j0 += h
        if erf_f32:
            Hp, D1 = gelu_erf(H, r), None
        else:
            Hp, D1 = gelu_as(H, r)
        out["Y"].append(r(gemm32(Hp, B.T, mode, **kw) + b))
        if not backward:
            continue
        dY = _t64(dY, dev)
        Gs.append(r(gemm32(dY, B, mode, **kw) * D1))
        out["dB"].append(gemm32(dY.T, Hp, mode, **kw))
        out["db"].append(colsum32(dY))
    if backward:
        Gcat = torch.cat(Gs, 1)
        out["dX"] = gemm32(Gcat, torch.cat([p[0] for p in Ps], 0), mode, p_two=g_two, **kw)
        dAcat = gemm32(Gcat.T, X, mode, p_two=g_two, **kw)
        # da = G^T 1 on the matrix pipe (mlp_bwd.hip: G's three terms against a fragment of ones, smallest first)
        dacat = gemm32(Gcat.T, torch.ones(X.shape[0], 1, dtype=torch.float64, device=X.device), mode)[:, 0]
        j0 = 0
        for h in hs:
            out["dA"].append(dAcat[j0:j0 + h])
            out["da"].append(dacat[j0:j0 + h])
            j0 += h
    if kind == "mag":
        for f, v in out.items():
            if isinstance(v, list):
                out[f] = [t + MAG * float(t.abs().max()) for t in v]
            elif v is not None:
                out[f] = v + MAG * float(v.abs().max())
    return out


# ---------------------------------------------------------------- shapes, paths, thresholds
# (T, E, [(h, O), ...], kinds): the smallest shapes that cross each tile boundary of the kernels. Which kinds run on which
# shape is chosen by what the bar has to resolve. A sum over tokens (dA, dB) of token-scaled rows is dominated by one early
# token; every later add then truncates against it in round-toward-zero mode, so that mode's ratio grows with T (13 at
# T = 257, 44 at 777, 59 at 1100), while the most G from two planes can leave is 2^-16 / u / 3 = 85. "rows" therefore runs
# where T <= 300 — 300 tokens still cross the 32-token tiles and the 256-token GEMM tile —, and "cols" / "hidden" stay off
# the widest contractions (E = 512, 528 ("cols"), 1024, J = 1536) for the same reason in dX. "flat", which has no dominant
# term, runs at every wide width. Every kind runs at least twice per path. Not run (shape x kind): narrow T = 1025 rows;
# wide E = 512 cols, hidden; T = 1000 rows; E = 144 outs; E = 1024 cols, hidden; E = 528 rows, cols; K = 24 rows, hidden,
# outs; wide-fused T = 777 rows (the T = 257 shape runs it) and T = 257 flat, cols, outs.
NARROW = [
    (257, 32, [(33, 17), (128, 12), (1, 1), (97, 32)], KINDS),
    (1025, 32, [(128, 32)] + [(128, 13)] * 3, ("flat", "cols", "hidden", "outs")),
    (31, 28, [(128, 1), (33, 12)], KINDS),
]
WIDE = [
    (257, 512, [(128, 128), (100, 127)], ("flat", "rows", "outs")),
    (1000, 48, [(96, 33), (33, 1), (128, 20)], ("flat", "cols", "hidden", "outs")),
    (300, 144, [(64, 12), (127, 33)], ("flat", "rows", "cols", "hidden")),  # the first width on the 256 x 256 GEMM configuration
    (300, 1024, [(128, 12), (64, 128)], ("flat", "rows", "outs")),             # E_pad = 1024: four column tiles in dX / dAcat
    (257, 528, [(100, 17)], ("flat", "hidden", "outs")),
    (1100, 64, [(64, 12)] * 24, ("flat", "cols")),                          # K = 24 and split-K above 1
]
# the second shape: one-output MLPs (dHpost is a single product, so G's own scale is smallest) at a T where "rows" is sharp
WIDE_FUSE = [(777, 128, [(128, 96), (128, 12), (100, 15), (128, 32), (97, 1)], ("flat", "cols", "hidden", "outs")),
             (257, 16, [(97, 1), (128, 3)], ("rows", "hidden"))]
MIXER_NAMES = ("lds_cfg1", "lds_n512_h100", "steps_odd")
MIXER_KINDS = ("flat", "rows", "cols", "hidden")   # ("outs" would scale W itself by 2^+-12 per link: the chain then overflows)
MIXER = [m for m in xe.MIXER if m[0] in MIXER_NAMES]

# the shapes of "narrow_f32" whose K weight images fit in LDS together (mlp_variant 2; the others are refused by the library)
RESIDENT_FITS = (2, 3)

# path -> what runs there. "narrow_f32": the f32-matrix-instruction forwards (mlp_variant 1 and 2), forward only.
PATHS = {
    "narrow": dict(shapes=NARROW, backward=True, erf_f32=False),
    "narrow_f32": dict(shapes=NARROW + [(257, 28, [(1, 1), (32, 32)], KINDS)], backward=False, erf_f32=True),
    "wide": dict(shapes=WIDE, backward=True, erf_f32=False),
    "wide_fuse": dict(shapes=WIDE_FUSE, backward=True, erf_f32=False),
    "mixer": dict(shapes=[(B * N, E, [(h, C)] + [(h, L)] * M, MIXER_KINDS) for _, B, N, E, h, C, L, M, _, _ in MIXER],
                  backward=False, erf_f32=False),
}


def seed(path, T, E):
    return {"narrow": 11, "narrow_f32": 11, "wide": 23, "wide_fuse": 37, "mixer": 41}[path] + T + 3 * E


@functools.lru_cache(maxsize=None)
def case_of(path, i, kind) -> Case:
    T, E, layers, kinds = PATHS[path]["shapes"][i]
    assert kind in kinds
    c = make_case(kind, T, E, layers, seed=seed(path, T, E))
    return replace(c, name=f"{path}[{i}] {c.name}")


def cases(path):
    return [(i, k) for i, s in enumerate(PATHS[path]["shapes"]) for k in s[3]]


def families(path):
    return FAMILIES if PATHS[path]["backward"] else ("Y", "V") if path == "mixer" else ("Y",)


# ---------------------------------------------------------------- the mixer: V_m = spmm(chord, W_m, V_{m-1}) (+ V_0)
def _chord(N, L):
    from oracle import chord_oracle as oc
    rows, cols = oc.chord_indices(N, L)
    assert np.array_equal(rows, np.repeat(np.arange(N), L))  # entry (n, l) of W_m multiplies row cols[n L + l] of V
    return np.stack([rows, cols]), cols.reshape(N, L)


def mixer_reference(case: Case, spec, dev="cpu"):
    """(V_1 .. V_M [M, B, N, C], their scales) of the mixer ``spec`` (an entry of ``x3_exact.MIXER``) on the case's MLPs:
    V_0 = g(X), W_m = fs[m](X) and the chain in float64 (the oracle's float64 chain). A step's scale is its own sum |w||v|
    plus what W's and V's scales leave in it: S_m = (|W_m| + S_W_m) |V_{m-1}| + |W_m| S_{m-1} (+ S_0 with the residual),
    gathered as the step gathers."""
    key = ("mixer", str(dev))
    if key in case._cache:
        return case._cache[key]
    from oracle import chord_oracle as oc
    _, B, N, E, h, C, L, M, residual, _ = spec
    ref, S = reference(case, dev, backward=False)
    Y = [y.cpu().numpy().reshape(B, N, -1) for y in ref["Y"]]
    SY = [y.cpu().numpy().reshape(B, N, -1) for y in S["Y"]]
    index, cols = _chord(N, L)
    steps = oc.chain(index, np.stack(Y[1:]), Y[0], residual)
    V, SV, scales = Y[0], SY[0], []
    for m in range(M):
        W, SW = np.abs(Y[1 + m]), SY[1 + m]
        SV = (np.einsum("bnl,bnlc->bnc", W + SW, np.abs(V)[:, cols, :]) + np.einsum("bnl,bnlc->bnc", W, SV[:, cols, :])
              + (SY[0] if residual else 0.0))
        scales.append(SV)
        V = steps[m]
    out = (torch.from_numpy(steps), torch.from_numpy(np.stack(scales)))
    case._cache[key] = out
    return out


def mixer_chain_f32(ys, spec):
    """The oracle's f32 chain (the arithmetic of the fused step: test_gpu_x3_exact.py), every step [M, B, N, C], on f32
    outputs ``ys`` of the MLPs. The chord step's own sums are the oracle's, rounded to nearest in either mode: the chord
    kernels are held bit for bit elsewhere; here they only carry W's error to V."""
    from oracle import chord_oracle as oc
    _, B, N, E, h, C, L, M, residual, _ = spec
    Y = [np.ascontiguousarray(y.cpu().numpy(), dtype=np.float32).reshape(B, N, -1) for y in ys]
    return torch.from_numpy(oc.chain(_chord(N, L)[0], np.stack(Y[1:]), Y[0], residual))


def mixer_ratio(case: Case, spec, steps, dev="cpu"):
    """The worst ratio over every step output V_1 .. V_M (``steps``: [M, B, N, C] or a list of M tensors)."""
    ref, S = mixer_reference(case, spec, dev)
    if isinstance(steps, (list, tuple)):
        steps = torch.stack([v.detach().cpu() for v in steps])
    r, i = ratio(steps.detach().cpu().reshape(ref.shape), ref, S)
    m, b, n, c = np.unravel_index(i, tuple(ref.shape))
    return r, f"step {m + 1} element {(b, n, c)}"


@functools.lru_cache(maxsize=None)
def arith_ratios(path, i, kind, mode, dev="cpu", defect=None):
    """{family: worst ratio} of the restated arithmetic (or one defect of it) on one case."""
    p = PATHS[path]
    case = case_of(path, i, kind)
    got = arith(case, mode, dev, backward=p["backward"], erf_f32=p["erf_f32"], defect=defect)
    res = {f: v[0] for f, v in ratios(case, got, dev, families(path)).items()}
    if path == "mixer":
        V = mixer_chain_f32(got["Y"], MIXER[i])
        if defect and defect[0] == "mag":
            V = V.double() + MAG * V.abs().amax(dim=(1, 2, 3), keepdim=True).double()
        res["V"] = mixer_ratio(case, MIXER[i], V, dev)[0]
    return res


@functools.lru_cache(maxsize=None)
def thresholds(path, dev="cpu"):
    """{family: 2 x the largest ratio of the restated arithmetic over both rounding modes and all cases of the path}."""
    worst = {f: 0.0 for f in families(path)}
    for i, kind in cases(path):
        for mode in MODES:
            for f, v in arith_ratios(path, i, kind, mode, dev).items():
                worst[f] = max(worst[f], v)
    return {f: 2.0 * v for f, v in worst.items()}


def defect_applies(path, defect):
    """G from two planes needs a backward; the f32-matrix-instruction forwards have no split to get wrong."""
    if defect[0] == "mag":
        return True
    if PATHS[path]["erf_f32"]:
        return False
    return PATHS[path]["backward"] or defect[0] != "g_two"


def defect_margin(path, defect, dev="cpu", stop_at=2.0):
    """The largest (defect's ratio / threshold) over families and cases of the path; cases in order, cheapest shapes first,
    until one reaches ``stop_at`` (None: all of them)."""
    thr = thresholds(path, dev)
    best = 0.0
    order = sorted(cases(path), key=lambda c: _cost(PATHS[path]["shapes"][c[0]]))
    for i, kind in order:
        got = arith_ratios(path, i, kind, "rn", dev, defect)
        best = max(best, max(got[f] / thr[f] for f in thr))
        if stop_at is not None and best >= stop_at:
            break
    return best


def _cost(shape):
    T, E, layers, _ = shape
    return T * E * sum(h for h, _ in layers)


# ---------------------------------------------------------------- scaling laws
def law_a(case: Case, rng):
    """X[:, e] 2^k(e) with A[:, e] 2^-k(e): H and every Y bit-identical."""
    s = pow2(rng, case.X.shape[1], ext=6)
    params = [(_f32(A / s[None, :]), a, B, b) for A, a, B, b in case.params]
    return Case(case.kind, _f32(case.X * s[None, :]), params, case.dYs, name=case.name + " law a")


def law_b(case: Case, rng):
    """B_k[o, :] 2^k, b_k[o] 2^k, dY_k[:, o] 2^-k: Y_k[:, o] scales by 2^k, dX, dA, da stay, dB_k[o, :] and db_k[o] scale by
    2^-k. Returns (case, [scale vector per MLP])."""
    ss = [pow2(rng, B.shape[0], ext=6) for _, _, B, _ in case.params]
    params = [(A, a, _f32(B * s[:, None]), _f32(b * s)) for (A, a, B, b), s in zip(case.params, ss)]
    dYs = [_f32(d / s[None, :]) for d, s in zip(case.dYs, ss)]
    return Case(case.kind, case.X, params, dYs, name=case.name + " law b"), ss


def law_c(case: Case, rng):
    """dY[t, :] 2^k(t) in every MLP: dX[t, :] scales by 2^k(t). Returns (case, scale vector)."""
    s = pow2(rng, case.X.shape[0], ext=6)
    return Case(case.kind, case.X, case.params, [_f32(d * s[:, None]) for d in case.dYs], name=case.name + " law c"), s


def same(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def check_laws(case: Case, run, laws=("a", "b", "c"), seed=5):
    """Asserts the scaling laws, bit for bit, on ``run(case) -> outputs`` (``reference``'s layout). With law "c" asked for
    the run must return dX and the weight gradients (their absence is a failure); without it, a forward-only run is
    checked on Y alone. Each transformed case is checked to stay normal."""
    rng = np.random.default_rng(seed)
    base = run(case)
    if "c" in laws:
        assert base.get("dX") is not None and len(base.get("dB") or []) == len(case.params), f"no gradients ({case.name})"
    has = lambda o, f: o.get(f) is not None and (f == "dX" or len(o[f]) > 0)  # noqa: E731
    if "a" in laws:
        c = law_a(case, rng)
        check_normal(c)
        got = run(c)
        for k, (y, y0) in enumerate(zip(got["Y"], base["Y"])):
            assert same(y, y0), f"law a: Y[{k}] changes under X 2^k, A 2^-k ({case.name})"
    if "b" in laws:
        c, ss = law_b(case, rng)
        check_normal(c)
        got = run(c)
        for k, s in enumerate(ss):
            st = torch.from_numpy(s).to(base["Y"][k].device).to(base["Y"][k].dtype)
            assert same(got["Y"][k], base["Y"][k] * st), f"law b: Y[{k}] is not scaled exactly ({case.name})"
            if has(base, "dB"):
                assert same(got["dB"][k], base["dB"][k] / st[:, None]), f"law b: dB[{k}] ({case.name})"
                assert same(got["db"][k], base["db"][k] / st), f"law b: db[{k}] ({case.name})"
                assert same(got["dA"][k], base["dA"][k]) and same(got["da"][k], base["da"][k]), f"law b: dA / da[{k}] ({case.name})"
        if has(base, "dX"):
            assert same(got["dX"], base["dX"]), f"law b: dX changes ({case.name})"
    if "c" in laws and has(base, "dX"):
        c, s = law_c(case, rng)
        check_normal(c)
        got = run(c)
        st = torch.from_numpy(s).to(base["dX"].device).to(base["dX"].dtype)
        assert same(got["dX"], base["dX"] * st[:, None]), f"law c: dX is not scaled exactly by the token's 2^k ({case.name})"


# ---------------------------------------------------------------- the record (profiles/x3_componentwise.md)
def report(dev="cpu") -> str:
    """Markdown: per path and family the restated arithmetic's worst ratios in both rounding modes and the threshold, and
    per path every defect's best ratio / threshold (the mildest one first)."""
    lines = []
    for path in PATHS:
        thr = thresholds(path, dev)
        lines += [f"### {path}", "", "| family | round to nearest | round toward zero | threshold |", "|---|---|---|---|"]
        for f in thr:
            worst = {m: max(arith_ratios(path, i, k, m, dev)[f] for i, k in cases(path)) for m in MODES}
            lines.append(f"| {f} | {worst['rn']:.2f} | {worst['rz']:.2f} | {thr[f]:.2f} |")
        marg = sorted((defect_margin(path, d, dev, stop_at=None), d) for d in DEFECTS if defect_applies(path, d))
        lines += ["", "defect ratio / threshold, best family and case: "
                  + ", ".join(f"{d[0]}{'' if d[1] is None else ' ' + str(xe.TERMS[d[1]])} {m:.3g}" for m, d in marg), ""]
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
