"""Reference, error envelope and float32 emulation of psf_adam_step_f32 (csrc/adam.hip), used by test_gpu_adam.py and checked
without a GPU by test_adam_cases_cpu.py. numpy only.

The update the header documents, with c1 = 1 - beta1, c2 = 1 - beta2 (both exact in f32: Sterbenz), t the step count:

    m' = m + (g - m) c1                  v' = beta2 v + (c2 g) g
    s  = lr / (1 - beta1^t)              q  = sqrt(1 - beta2^t)
    D  = s * (m' / (sqrt(v') / q + eps))           p' = p - D

``reference`` evaluates it in float64 on the float32 VALUES of the hyperparameters (float(np.float32(0.999)), not 0.999: the
kernel receives floats, and 1 - beta2 differs by 1.3e-5 between the two).

The envelope (``bounds``). Every float32 operation is allowed one ulp, U = 2^-23 relative — twice the unit roundoff 2^-24 of a
correctly rounded operation, because powf, sqrtf and the division of a GPU's math library are specified to 1 ulp, not to
correct rounding. The IEEE operations are given the same U: a correct kernel then keeps a factor 2 in hand (a single
rounding reaches its 2^-24 on some element of a large array, so a bound of 2^-24 per operation would be met, not undercut).
To first order in U:

  m'   sub, mul, add: U c1 |g - m| twice, U |m'| once; |g - m| <= |m| + |g| and |m'| <= |m| + |g|, so
           |dm'| <= (2 c1 + 1) U (|m| + |g|)                                     absolute
  v'   both terms are >= 0, so relative errors do not amplify: beta2 v one rounding, (c2 g) g two, the sum one:
           |dv'| <= 4 U v'                                                        relative
  s    beta1^t to 1 ulp is U beta1^t absolute, against 1 - beta1^t that is U r1 with r1 = beta1^t / (1 - beta1^t); the
       subtraction and the division add U each:                 U (r1 + 2)
  q    likewise U (r2 + 1) for 1 - beta2^t with r2 = beta2^t / (1 - beta2^t), halved by the root, plus the root's U:
                                                                  U (r2 / 2 + 1.5)
       r2 / 2 is the large term: 249.5 at t = 2 with beta2 = 0.999, i.e. 3.0e-5 of the update, and it is not the kernel's to
       avoid: a float cannot hold 0.998001 more precisely, and 1 - x divides that by 0.002
  sqrt(v') / q + eps   half of v's 4 U plus the root's U, q's bound, the division and the addition (eps > 0 only shrinks the
       relative error of the sum):                               U (r2 / 2 + 6.5)
  D    s, the denominator, the division m' / . and the product:  R = U (r1 + r2 / 2 + 10.5)   relative, m' taken as exact
       and m's own error enters as s |dm'| / (sqrt(v') / q + eps)
  p'   |dp'| <= |D| R + s (2 c1 + 1) U (|m| + |g|) / (sqrt(v') / q + eps) + U |p'|

With p = 0 the last term vanishes with respect to D (p' = -D exactly), so half of the elements start from p = 0: there the
update itself is compared, relatively.

``emulate`` restates the formula in numpy float32, one rounding per operation, in the uncontracted form and in the form a
compiler may contract it to (m' and p' as one fused multiply-add each, v' as fma(beta2, v, (c2 g) g)); a fused multiply-add
is the exact float64 product added in float64 and rounded to float32. It also takes three defects. The CPU test shows both
forms inside the envelope with a factor 2 to spare at every t, and each defect outside it.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -23
STEPS = (1, 2, 3, 10, 1000, 100000)
DEFAULTS = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
DEFECTS = ("no_bias_correction_2", "eps_inside_sqrt", "beta1_for_v")


def f32_value(x) -> float:
    """The float32 value of a hyperparameter, as a Python float (what the kernel receives)."""
    return float(np.float32(x))


def hyper(**kw):
    h = {**DEFAULTS, **kw}
    return {k: f32_value(v) for k, v in h.items()}


def operands(t, n=1 << 15, seed=0):
    """(p, g, m, v) float32: |g| log-uniform over 1e-4 .. 1e2 with random signs; states to match (m within +-|g|, v within
    (0, 2] g^2), a sixteenth of them the true first-step state m = v = 0; p = 0 for every second element, N(0, 1) elsewhere."""
    rng = np.random.default_rng([seed, t])
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 2, n)).astype(np.float32)
    m = (g * rng.uniform(-1, 1, n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(1e-3, 2, n)).astype(np.float32)
    m[::16], v[::16] = 0, 0
    p = rng.standard_normal(n).astype(np.float32)
    p[::2] = 0
    return p, g, m, v


def reference(p, g, m, v, h, t):
    """(p', m', v', D, denominator) in float64."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = h["beta1"], h["beta2"]
    m1 = m + (g - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g * g
    s, q = h["lr"] / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)
    den = np.sqrt(v1) / q + h["eps"]
    D = s * (m1 / den)
    return p - D, m1, v1, D, den


def bounds(p, g, m, v, h, t):
    """(reference p', m', v'; bounds E_p, E_m absolute and E_v absolute = 4 U v') as documented above."""
    p1, m1, v1, D, den = reference(p, g, m, v, h, t)
    b1, b2 = h["beta1"], h["beta2"]
    c1 = 1.0 - b1
    r1, r2 = b1 ** t / (1.0 - b1 ** t), b2 ** t / (1.0 - b2 ** t)
    s = h["lr"] / (1.0 - b1 ** t)
    E_m = (2 * c1 + 1) * U * (np.abs(np.float64(m)) + np.abs(np.float64(g)))
    E_v = 4 * U * v1
    R = U * (r1 + r2 / 2 + 10.5)
    E_p = np.abs(D) * R + s * E_m / den + U * np.abs(p1)
    return (p1, m1, v1), (E_p, E_m, E_v)


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def emulate(p, g, m, v, h, t, contracted=False, defect=None):
    """(p', m', v') in float32, one rounding per operation (per fused multiply-add when contracted)."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    lr, b1, b2, eps = (f(h[k]) for k in ("lr", "beta1", "beta2", "eps"))
    powf = lambda b: f(np.float64(b) ** np.float64(f(t)))  # noqa: E731  (correctly rounded; the envelope allows 1 ulp)
    bc1, bc2 = f(1) - powf(b1), f(1) - powf(b2)
    s, q = lr / bc1, np.sqrt(bc2)
    if defect == "no_bias_correction_2":
        q = f(1)
    c1, c2 = f(1) - b1, f(1) - b2
    bv = b1 if defect == "beta1_for_v" else b2
    cv = c1 if defect == "beta1_for_v" else c2
    if contracted:
        m1 = _fma(g - m, c1, m)
        v1 = _fma(v, bv, (cv * g) * g)
    else:
        m1 = m + (g - m) * c1
        v1 = bv * v + cv * g * g
    den = np.sqrt(v1 + eps) / q if defect == "eps_inside_sqrt" else np.sqrt(v1) / q + eps
    ratio = m1 / den
    p1 = _fma(ratio, -s, p) if contracted else p - s * ratio
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def worst(got, want, E):
    """max over the elements of |got - want| / E, per quantity (p, m, v); 0 / 0 counts as 0."""
    out = []
    for a, w, e in zip(got, want, E):
        err = np.abs(np.asarray(a, dtype=np.float64) - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / e)
        out.append(float(ratio.max()))
    return tuple(out)


def measured(got, ops, want):
    """The plain maxima that DESIGN.md records: v' relative, and the update relative on the elements in the true first-step
    state (p = 0, so p' = -D exactly; m = v = 0, so m' = c1 g has no cancellation to magnify its rounding)."""
    (p1, _m1, v1w), (gp, _gm, gv), (p0, _g, m0, v0) = want, got, ops
    with np.errstate(divide="ignore", invalid="ignore"):
        v_rel = np.max(np.where(v1w > 0, np.abs(np.float64(gv) - v1w) / v1w, 0.0))
        first = (p0 == 0) & (m0 == 0) & (v0 == 0)
        upd = np.max(np.abs(np.float64(gp)[first] - p1[first]) / np.abs(p1[first]))
    return float(v_rel), float(upd)


# ---------------------------------------------------------------- exact known answers (Adam's first-step rule)
KNOWN = dict(lr=2.0 ** -7, beta1=0.5, beta2=0.75, eps=0.0)


def known_answer(zero_gradient=False):
    """(p, g, m, v, hyper, p', m', v') with every intermediate exact in float32, contracted or not: m = v = 0, t = 1,
    g = +-2k for k = 1..1024 (signs and order shuffled), p multiples of 2^-7 below 1024. Then m' = g / 2, v' = g^2 / 4,
    1 - beta1 = 1/2, sqrt(1 - beta2) = 1/2, the denominator 2 |k| / (1/2) ... = 2 |g| / 2 = |g|, m' / |g| = +-1/2, s = 2^-6 and
    p' = p - 2^-7 sign(g). With g = 0 and eps = 2^-10 nothing moves and nothing is NaN (0 / 2^-10 = 0)."""
    rng = np.random.default_rng(7)
    k = np.arange(1, 1025, dtype=np.float64)
    g = np.concatenate([2 * k, -2 * k])
    rng.shuffle(g)
    n = g.size
    p = rng.integers(-(1 << 17) + 1, 1 << 17, n).astype(np.float64) * 2.0 ** -7
    assert np.abs(p).max() < 1024
    h = dict(KNOWN)
    if zero_gradient:
        g = np.zeros(n)
        h["eps"] = 2.0 ** -10
        want = (p, np.zeros(n), np.zeros(n))
    else:
        want = (p - 2.0 ** -7 * np.sign(g), g / 2, g * g / 4)
    to32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    for a in (p, g, *want):
        assert np.array_equal(to32(a).astype(np.float64), a)  # exact in float32
    return (to32(p), to32(g), np.zeros(n, np.float32), np.zeros(n, np.float32), h, *(to32(w) for w in want))
