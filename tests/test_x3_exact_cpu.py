"""CPU self-tests of the known-answer constructions of test_gpu_x3_exact.py (tests/x3_exact.py).

They show, without a GPU, that the GPU tests' expected values are right and that those tests can tell the shipped
arithmetic from its likely defects: the inputs are exact on their grids with sum |terms| < 2^24 units, the thresholds put
both GELU forms in their linear regime, every split operand of every GEMM carries third bf16 terms, and emulations of
three defects (third terms forced to zero, one of the six term products dropped, G from two bf16 planes) change at least
one expected result.
"""
import numpy as np
import pytest

import x3_exact as xe

KINDS = ("x", "w", "dy")


def test_split3_port():
    v = np.array([1 + 2.0 ** -20, 1 + 2.0 ** -8 + 2.0 ** -16, -(256 + 1 + 2.0 ** -8), 3.0, 0.0, 511 + 255 * 2.0 ** -8],
                 np.float32)
    t1, t2, t3 = xe.split3(v)
    assert t1.tolist() == [1.0, 1.0, -256.0, 3.0, 0.0, 510.0]
    assert t2.tolist() == [2.0 ** -20, 2.0 ** -8, -1.0, 0.0, 0.0, 1 + 254 * 2.0 ** -8]
    assert t3.tolist() == [0.0, 2.0 ** -16, -2.0 ** -8, 0.0, 0.0, 2.0 ** -8]
    assert xe.level(v).tolist() == [2, 3, 3, 1, 0, 3]
    rng = np.random.default_rng(0)
    r = (rng.standard_normal(100000) * np.exp2(rng.integers(-40, 40, 100000))).astype(np.float32)
    t1, t2, t3 = xe.split3(r)
    assert np.array_equal(t1.astype(np.float64) + t2 + t3, r.astype(np.float64))
    for t in (t1, t2):
        assert not np.any(t.view(np.uint32) & 0xFFFF)
    assert np.all(np.abs(t3) < np.abs(r) * 2.0 ** -14)  # two truncations to 8 significant bits


def test_linear_gelu_regime_of_both_gelu_forms():
    """At and beyond the thresholds GELU is exactly x or 0 and its derivative exactly 1 or 0, in the kernels' f32
    formulas; just inside them it is not (the ports are not trivially exact)."""
    live = np.concatenate([np.float32(xe.LIVE) + np.arange(0, 2 ** 14, dtype=np.float32) * np.float32(2.0 ** -9),
                           np.geomspace(16, 3e38, 5000).astype(np.float32)])
    dead = -np.concatenate([np.float32(-xe.DEAD) + np.arange(0, 2 ** 14, dtype=np.float32) * np.float32(2.0 ** -8),
                            np.geomspace(32, 3e38, 5000).astype(np.float32)])
    assert xe.gelu_regime_ok(live) and xe.gelu_regime_ok(dead)
    y, d = xe.gelu_as(live)
    assert np.array_equal(y, live) and np.all(d == 1)
    y, d = xe.gelu_as(dead)
    assert np.all(y == 0) and np.all(d == 0)
    assert np.all(xe.gelu_erf(live) == live) and np.all(xe.gelu_erf(dead) == 0)
    near = np.array([4.0, -4.0, 1.0], np.float32)
    assert not xe.gelu_regime_ok(near)
    assert not np.array_equal(xe.gelu_as(np.float32([4.0]))[0], np.float32([4.0]))
    assert not np.array_equal(xe.gelu_erf(np.float32([-3.0])), np.float32([0.0]))


def _all_cases():
    out = []
    for path, shapes in (("narrow", xe.NARROW), ("wide", xe.WIDE), ("wide_fuse", xe.WIDE_FUSE)):
        for T, E, layers in shapes:
            for kind in KINDS:
                out.append((path, kind, T, E, layers))
    for T, E, layers in xe.RESIDENT:
        for kind in KINDS[:2]:
            out.append(("resident", kind, T, E, layers))
    return out


@pytest.mark.parametrize("path,kind,T,E,layers", _all_cases())
def test_constructions_are_exact(path, kind, T, E, layers):
    """Inputs and results f32-exact, linear regime, split condition, sum |terms| < 2^24 grid units (check_exact), and the
    construction's hard values where the kernels' tiles end."""
    case = xe.make_case(kind, T, E, layers, seed=xe.seed(path, T, E))
    units = xe.check_exact(case)
    assert max(units.values()) < xe.UNITS
    lx = xe.level(case.X)
    if kind == "x":
        assert (lx[-1] == 3).any() and (lx[:, -1] == 3).any()          # last token, last column of E
    for (A, a, B, b), dY in zip(case.params, case.dYs):
        assert a[-1] > 0 and A[-1].any() and B[0, -1] != 0               # the last hidden row is live and read
        if kind == "w":
            assert (xe.level(A[-1]) == 3).any()
    assert any(dY[-1].any() for dY in case.dYs)                          # the last token carries gradient
    if kind == "dy":
        assert any((xe.level(dY[-1]) == 3).any() for dY in case.dYs)


@pytest.mark.parametrize("shapes", ["narrow", "wide", "resident"])
def test_every_split_operand_carries_third_terms(shapes):
    """Across the constructions of a path, every split operand of every GEMM has products with a nonzero third term."""
    lst = {"narrow": xe.NARROW, "wide": xe.WIDE, "resident": xe.RESIDENT}[shapes]
    total = {}
    for T, E, layers in lst:
        for kind in KINDS:
            for k, v in xe.coverage(xe.make_case(kind, T, E, layers, seed=xe.seed(shapes, T, E))).items():
                total[k] = total.get(k, 0) + v
    missing = [f"{k} ({xe.OPERANDS[k]})" for k in xe.OPERANDS if not total.get(k)]
    assert not missing, missing


def test_the_mixer_cases_are_exact():
    for B, N, E, h, C, L, M in [m[1:8] for m in xe.MIXER]:
        for kind in KINDS[:2]:
            case = xe.mixer_case(kind, B, N, E, h, C, L, M, seed=N + E + h)
            xe.check_exact(case)
            ys = case.reference()["Y"]
            assert max(np.abs(y).max() for y in ys[1:]) * L < 2  # |W| L < 2: the chain does not grow


DEFECT_SHAPES = [(257, 32, [(33, 17), (128, 12), (1, 1)]), (31, 16, [(5, 3), (97, 33)]), (33, 48, [(127, 12), (1, 128)])]


@pytest.mark.parametrize("T,E,layers", DEFECT_SHAPES)
def test_emulated_defects_change_the_expected_results(T, E, layers):
    """The split arithmetic emulated exactly reproduces the expected results; each defect changes at least one:
    t3 forced to 0 (every construction), G from two bf16 planes (the constructions with third terms in G) and each of
    the six term products dropped (at least one construction per term)."""
    cases = {k: xe.make_case(k, T, E, layers, seed=T + E) for k in KINDS}
    for k, c in cases.items():
        xe.check_exact(c)
        assert not xe.differs(c, xe.emulate(c)), k
        assert xe.differs(c, xe.emulate(c, t3_zero=True)), k
    for k in ("w", "dy"):
        assert xe.differs(cases[k], xe.emulate(cases[k], g_two=True)), k
    for term in range(6):
        assert any(xe.differs(c, xe.emulate(c, drop=term)) for c in cases.values()), xe.TERMS[term]
    # the one the GPU mutation drops (w.t2 x.t2) is seen by the "x" construction alone
    assert xe.differs(cases["x"], xe.emulate(cases["x"], drop=1))
