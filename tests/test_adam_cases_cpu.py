"""CPU half of the Adam envelope of test_gpu_adam.py (tests/adam_cases.py): the float32 emulation of the documented formula,
contracted and not, sits inside the envelope with a factor 2 to spare at every step count; three emulated defects leave it;
the known-answer cases are exact in both forms."""
import numpy as np
import pytest

import adam_cases as ac


@pytest.mark.parametrize("t", ac.STEPS)
def test_emulation_sits_inside_the_envelope_with_a_factor_two_to_spare(t):
    h = ac.hyper()
    ops = ac.operands(t)
    want, E = ac.bounds(*ops, h, t)
    for contracted in (False, True):
        wp, wm, wv = ac.worst(ac.emulate(*ops, h, t, contracted), want, E)
        print(f"t={t} contracted={contracted}: p {wp:.3f} m {wm:.3f} v {wv:.3f} of the bound")
        assert max(wp, wm, wv) <= 0.5, (t, contracted, wp, wm, wv)


def test_operands_span_what_they_claim():
    p, g, m, v = ac.operands(3)
    assert np.abs(g).min() < 2e-4 and np.abs(g).max() > 50 and (g < 0).any() and (g > 0).any()
    assert (p == 0).sum() == p.size // 2 and ((m == 0) & (v == 0)).sum() >= p.size // 16 and (v >= 0).all()
    h = ac.hyper()
    assert h["beta2"] == float(np.float32(0.999)) != 0.999 and abs((1 - h["beta2"]) / (1 - 0.999) - 1) > 1e-5


# the step counts at which a defect is visible at all: once beta2^t has underflowed against 1, sqrt(1 - beta2^t) = 1 and leaving
# the second bias correction out changes nothing
VISIBLE = {"no_bias_correction_2": (1, 2, 3, 10, 1000), "eps_inside_sqrt": ac.STEPS, "beta1_for_v": ac.STEPS}


@pytest.mark.parametrize("defect", ac.DEFECTS)
def test_every_defect_leaves_the_envelope(defect):
    h = ac.hyper()
    for t in VISIBLE[defect]:
        ops = ac.operands(t)
        want, E = ac.bounds(*ops, h, t)
        for contracted in (False, True):
            assert max(ac.worst(ac.emulate(*ops, h, t, contracted, defect), want, E)) > 1.0, (defect, t, contracted)


def test_reference_on_float_hyperparameters_is_another_operation_than_on_decimal_ones():
    """The envelope at t = 1000 is about 1e-6 of the update; 0.999 in place of float(0.999) moves v' by 1.3e-5 of its new term."""
    t = 1000
    ops = ac.operands(t)
    want, E = ac.bounds(*ops, ac.hyper(), t)
    off = ac.reference(*ops, dict(ac.DEFAULTS), t)[:3]
    assert max(ac.worst(off, want, E)) > 1.0


@pytest.mark.parametrize("zero_gradient", [False, True])
def test_known_answers_are_exact_in_both_forms(zero_gradient):
    p, g, m, v, h, wp, wm, wv = ac.known_answer(zero_gradient)
    assert p.size == 2048 and set(np.abs(g)) == ({0.0} if zero_gradient else set(np.arange(2.0, 2049.0, 2.0)))
    for contracted in (False, True):
        got = ac.emulate(p, g, m, v, ac.hyper(**h), 1, contracted)
        for a, w in zip(got, (wp, wm, wv)):
            assert np.array_equal(a.view(np.uint32), w.view(np.uint32))
    if not zero_gradient:
        assert np.array_equal(wp, p - np.float32(2.0 ** -7) * np.sign(g)) and (wp != p).all()
