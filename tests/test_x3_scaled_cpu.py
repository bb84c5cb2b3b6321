"""CPU self-tests of the componentwise-accuracy and scaling-law tests of test_gpu_x3_scaled.py (tests/x3_scaled.py).

They show, without a GPU, that those tests can tell the shipped arithmetic from its likely defects: the thresholds come
from the documented arithmetic restated with f32 sums in both rounding modes (never from a kernel), every emulated defect
lands at least 2 x above them on every path, every output element is compared, elements with a zero scale must be exact,
every scaled operand keeps all three split terms normal, and the restated arithmetic obeys the three scaling laws bit for
bit in both rounding modes.
"""
import math

import numpy as np
import pytest
import torch

import x3_exact as xe
import x3_scaled as xs

ALL_CASES = [(p, i, k) for p in xs.PATHS for i, k in xs.cases(p)]


@pytest.mark.parametrize("path,i,kind", ALL_CASES)
def test_scaled_operands_stay_normal_and_carry_the_extremes(path, i, kind):
    case = xs.case_of(path, i, kind)
    xs.check_normal(case)
    for v in case.operands():
        assert v.dtype == np.float32
    # the case's float64 results and scales are finite, the scales non-negative: nothing under- or overflows on the way
    ref, S = xs.reference(case, backward=xs.PATHS[path]["backward"])
    for f in xs.families(path):
        if f == "V":
            continue
        for r, s in zip(*(([ref[f]], [S[f]]) if f == "dX" else (ref[f], S[f]))):
            assert torch.isfinite(r).all() and torch.isfinite(s).all() and (s >= 0).all()
    # the last token, column, hidden row and output carry the extreme exponent of their kind
    T, E, layers = xs.PATHS[path]["shapes"][i][:3]
    again = xs.make_case(kind, T, E, layers, seed=xs.seed(path, T, E))
    assert all(np.array_equal(u, v) for u, v in zip(again.operands(), case.operands()))  # seeded: the same case every time
    # the kind's scaling is there: the largest |value| per token / column / row spans most of the exponent range
    def spread(v, axis):
        return np.log2(np.abs(v).max(axis=axis))
    if kind == "rows":
        assert np.ptp(spread(case.X, 1)) > xs.EXT and np.ptp(spread(case.dYs[0], 1)) > xs.EXT
        assert abs(spread(case.X, 1)[-1]) > xs.EXT - 4
    elif kind == "cols":
        assert np.ptp(spread(case.X, 0)) > xs.EXT / 2 and abs(spread(case.X, 0)[-1]) > xs.EXT - 4
    elif kind == "hidden":
        A = max((p[0] for p in case.params), key=lambda a: a.shape[0])
        assert np.ptp(spread(A, 1)) > xs.EXT / 2
    elif kind == "outs":
        Bm = max((p[2] for p in case.params), key=lambda b: b.shape[0])
        assert Bm.shape[0] == 1 or np.ptp(spread(Bm, 1)) > xs.EXT / 2


def test_pow2_scales_are_powers_of_two_within_the_exponent_range():
    rng = np.random.default_rng(3)
    s = xs.pow2(rng, 1000)
    m, e = np.frexp(s)
    assert np.all(m == 0.5) and np.all(np.abs(e - 1) <= xs.EXT) and abs(int(e[-1]) - 1) == xs.EXT
    assert xs.EXT <= 20
    # all five kinds differ from the flat case only by such factors
    flat = xs.make_case("flat", 9, 16, [(5, 3)], seed=1)
    assert all(np.all(np.abs(v) < 8) for v in flat.operands())


def test_ratio_counts_every_element_and_demands_exactness_where_the_scale_is_zero():
    ref = torch.tensor([1.0, 0.0, -2.0, 0.0], dtype=torch.float64)
    S = torch.tensor([1.0, 0.0, 4.0, 0.0], dtype=torch.float64)
    assert xs.ratio(ref.float(), ref, S) == (0.0, 0)
    got = ref.clone()
    got[2] += 8 * xs.U  # 8 u against a scale of 4: ratio 2, at the worst element
    assert xs.ratio(got, ref, S) == (2.0, 2)
    got[3] = 1e-30    # zero scale: any error at all is infinite
    r, i = xs.ratio(got, ref, S)
    assert math.isinf(r) and i == 3
    got[3] = float("nan")
    assert math.isinf(xs.ratio(got, ref, S)[0])
    # a single wrong element of a whole case is seen by its family
    case = xs.case_of("narrow", 2, "flat")
    out, _ = xs.reference(case)
    got = {f: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for f, v in out.items()}
    assert all(v[0] == 0 for v in xs.ratios(case, got).values())
    got["dB"][1][-1, -1] += 1.0
    got["dX"][0, 0] += 1.0
    res = xs.ratios(case, got)
    assert res["dB"][0] > 1e4 and res["dX"][0] > 1e4 and res["Y"][0] == 0 and "MLP 1" in res["dB"][1]


def test_zero_rows_have_zero_scale_and_the_arithmetic_is_exact_there():
    """A token of zeros in dY and a zero row of B: dX of that token, and dB / db of that output, have scale 0 and the
    restated arithmetic returns exact zeros (ratio 0, not infinity)."""
    case = xs.make_case("flat", 40, 16, [(33, 5)], seed=4)
    case.dYs[0][7] = 0
    case.dYs[0][:, 2] = 0
    _, S = xs.reference(case)
    assert float(S["dX"][7].abs().max()) == 0 and float(S["db"][0][2]) == 0 and float(S["dB"][0][2].abs().max()) == 0
    for mode in xs.MODES:
        res = xs.ratios(case, xs.arith(case, mode))
        assert all(math.isfinite(v[0]) for v in res.values()), res


def test_split_port_equals_x3_exact():
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(50000) * np.exp2(rng.integers(-40, 40, 50000))).astype(np.float32)
    for a, b in zip(xe.split3(v), xs.split3_t(torch.from_numpy(v).double())):
        assert np.array_equal(a.astype(np.float64), b.numpy())


def test_gelu_ports_round_to_nearest_equal_x3_exact_closely_and_toward_zero_is_below():
    """The rounded-per-operation GELU in round-to-nearest mode is x3_exact's f32 port (up to the fused last step of the
    derivative and the double rounding of exp2: a few ulps), within the documented bound of the true GELU."""
    x = torch.linspace(-9, 9, 20001, dtype=torch.float64).float().double()
    y, d = xs.gelu_as(x, xs._round("rn"))
    y0, d0 = xe.gelu_as(x.float().numpy())
    assert np.max(np.abs(y.numpy() - y0)) <= 4e-7 and np.max(np.abs(d.numpy() - d0)) <= 4e-7
    Phi = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    for mode in xs.MODES:
        r = xs._round(mode)
        y, d = xs.gelu_as(x, r)
        assert float((y - x * Phi).abs().max()) <= 9 * 1.5e-7  # |x| (7.5e-8 + roundings)
        assert float((d - (Phi + x * xs._phi(x))).abs().max()) <= 1e-6
        ye = xs.gelu_erf(x, r)
        assert float((ye - x * Phi).abs().max()) <= 9 * 2.5e-7
        assert torch.equal(y.float().double(), y) and torch.equal(ye.float().double(), ye)  # f32 values
    assert np.max(np.abs(xs.gelu_erf(x, xs._round("rn")).numpy() - xe.gelu_erf(x.float().numpy()))) <= 4e-7


def test_rounding_modes():
    x = torch.tensor([1 + 2.0 ** -24 + 2.0 ** -40, -(1 + 2.0 ** -24 + 2.0 ** -40), 1 + 2.0 ** -23, 3.0, 0.0], dtype=torch.float64)
    assert xs._round("rn")(x).tolist() == [1 + 2.0 ** -23, -(1 + 2.0 ** -23), 1 + 2.0 ** -23, 3.0, 0.0]
    assert xs._round("rz")(x).tolist() == [1.0, -1.0, 1 + 2.0 ** -23, 3.0, 0.0]


def test_gemm32_without_rounding_error_equals_the_exact_split_product():
    """17-bit integers against integers up to 3: every term and partial sum is an integer below 2^24, so both modes give
    x3_exact._x3 (float64 sums) exactly — with and without each defect, some of which change the result."""
    rng = np.random.default_rng(2)
    P = (rng.integers(2 ** 16, 2 ** 17, (7, 37)) * rng.choice([-1, 1], (7, 37))).astype(np.float32)
    Q = rng.integers(-3, 4, (37, 5)).astype(np.float32)
    assert (xe.level(P) == 3).any()
    Pt, Qt = torch.from_numpy(P).double(), torch.from_numpy(Q).double()
    clean = xe._x3(P, Q)
    assert np.array_equal(clean, P.astype(np.float64) @ Q.astype(np.float64))
    changed = 0
    for kw in [dict(), dict(drop=2), dict(drop=4), dict(drop=5), dict(t3_zero=True), dict(p_two=True)]:
        want = xe._x3(P, Q, **kw)
        changed += not np.array_equal(want, clean)
        for mode in xs.MODES:
            assert np.array_equal(xs.gemm32(Pt, Qt, mode, **kw).numpy(), want), (kw, mode)
    assert changed == 5
    assert np.array_equal(xs.gemm32(Pt, Qt, "rz", split=False).numpy(), clean)


@pytest.mark.parametrize("path", list(xs.PATHS))
def test_thresholds_come_from_the_restated_arithmetic_and_every_defect_clears_them_twice(path):
    thr = xs.thresholds(path)
    assert set(thr) == set(xs.families(path))
    for f, v in thr.items():
        assert 0 < v < 64, (f, v)   # above 2^-16 / u / 3 = 85 no split defect could be seen
    for d in xs.DEFECTS:
        if xs.defect_applies(path, d):
            m = xs.defect_margin(path, d)
            assert m >= 2.0, f"{path}: defect {d} reaches only {m:.2f} x the threshold"
    assert sum(xs.defect_applies(path, d) for d in xs.DEFECTS) >= (1 if path == "narrow_f32" else 8)


def test_the_mixer_sees_every_defect_in_its_final_output_alone():
    """The GPU test of the mixer sees V_M only (W never reaches memory): every defect clears 2 x the threshold there."""
    thr = xs.thresholds("mixer")["V"]
    for d in xs.DEFECTS:
        if xs.defect_applies("mixer", d):
            best = max(xs.arith_ratios("mixer", i, k, "rn", "cpu", d)["V"] for i, k in xs.cases("mixer"))
            assert best >= 2.0 * thr, (d, best, thr)


def test_every_kind_runs_on_every_path_and_the_new_widths_are_there():
    for path, p in xs.PATHS.items():
        kinds = {k for _, k in xs.cases(path)}
        assert kinds == set(xs.MIXER_KINDS if path == "mixer" else xs.KINDS), path
    assert {144, 528, 1024} <= {s[1] for s in xs.WIDE}
    assert max(len(s[2]) for s in xs.WIDE) == 24


LAW_CASES = [("narrow", 2, "flat"), ("narrow", 0, "rows"), ("wide", 2, "hidden"), ("wide_fuse", 1, "rows"), ("narrow", 2, "outs")]


@pytest.mark.parametrize("mode", xs.MODES)
@pytest.mark.parametrize("path,i,kind", LAW_CASES)
def test_the_restated_arithmetic_obeys_the_scaling_laws_bit_for_bit(path, i, kind, mode):
    case = xs.case_of(path, i, kind)
    xs.check_laws(case, lambda c: xs.arith(c, mode))


def test_the_scaling_laws_are_not_vacuous():
    """A run that rounds one product before scaling breaks law (a); the checker notices."""
    case = xs.case_of("narrow", 2, "flat")

    def broken(c):
        out = xs.arith(c, "rn", backward=False)
        out["Y"] = [y + torch.from_numpy(c.X[:, :1]).double() * 2.0 ** -20 for y in out["Y"]]  # depends on X's scale
        return out

    with pytest.raises(AssertionError, match="law a"):
        xs.check_laws(case, broken, laws=("a",))
