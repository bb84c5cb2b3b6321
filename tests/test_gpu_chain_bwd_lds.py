"""GPU: the one-launch backward chain (csrc/bwd_chain_lds.h: chord_chain_bwd_lds_k<L, G, RES>) through psf_chord_chain_bwd_f32
itself, at its limits. ctypes tables, dX_steps = NULL wherever the one launch applies, X_steps from the oracle's forward on the
CPU — so the backward stands on its own.

Verdict unless stated otherwise: dV0 and every dW_m carry the oracle's bits (tests/chain_bwd_cases.py; its CPU self-test shows
that the kernel's documented order has exactly those bits, and that seven ways of departing from it have others). Every
operand of every case sits inside 256 bytes of NaN on either side and every output is a NaN-filled view with the same bands:
after each call the bands are still NaN and the outputs fully written.

  a. every instance of one channel group (C = 4): L = 2..20, with and without the residual, two waves with 61 idle lanes
  b. limits: the dynamic-LDS maximum (151 552 bytes), G = 1 beyond 48 KB, M = 64, N = 1, 2, 3, 63, 64, 65, 1023, 1024, repeated and
     explicit offsets; the 48 KB raise between launches of one instance
  c. W_m and dW_m 0, 1 and 3 floats off a 16-byte boundary; PSF_E_ALIGN and PSF_E_ALIAS leave every output byte alone
  d. NaN left in every CU's LDS beforehand
  e. NaN, Inf, denormals, signed zeros, values near FLT_MAX: the oracle's bits or NaN on both sides
  f. 600 workgroups
  g. the entry's other answers: library-issued steps, PSF_E_UNSUPPORTED, B = 0
  h. one call captured into a graph and replayed on operands overwritten in place
"""
import ctypes

import numpy as np
import pytest
import torch

import chain_bwd_cases as cc
from conftest import rel_inf
from test_gpu_guard_bands import _banded, _banded_input

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000  # what torch.full(float("nan")) writes
PSF_E_ALIAS, PSF_E_ALIGN, PSF_E_UNSUPPORTED = -3, -4, -7


def _lib():
    from sparsefactorization_amd import _lib
    return _lib.load()


class _Device:
    """The operands of one call inside NaN bands, and NaN-filled banded outputs. X[0] is V0 (the entry ignores X_steps[0])."""

    def __init__(self, gpu, case, W, V0, dOut, X, w_shift=0, x_shift=0, dout_shift=0, dv0_shift=0, with_dx=False):
        B, N, M, L, C, _res, _off = case
        self.case, self.gpu = case, gpu
        self.W = [_banded_input(np.array(w, dtype=np.float32), gpu, w_shift) for w in W]  # (copies: the shared arrays are read-only)
        self.V0 = _banded_input(np.array(V0, dtype=np.float32), gpu)
        self.X = [self.V0] + [_banded_input(np.array(x, dtype=np.float32), gpu, x_shift) for x in X[1:M]]
        self.dOut = _banded_input(np.array(dOut, dtype=np.float32), gpu, dout_shift)
        self.dW = [_banded((B, N, L), gpu, w_shift) for _ in range(M)]
        self.dV0 = _banded((B, N, C), gpu, dv0_shift)
        self.dX = [torch.empty(B, N, C, device=gpu) for _ in range(M)] if with_dx else None

    def call(self, dW_ptrs=None, B=None, stream=None):
        Bc, N, M, L, C, res, off = self.case
        vp = ctypes.c_void_p
        tab = lambda ptrs: (vp * M)(*ptrs)  # noqa: E731
        offsets = None if off is None else (ctypes.c_int64 * L)(*off)
        s = torch.cuda.current_stream(self.gpu).cuda_stream if stream is None else stream
        return _lib().psf_chord_chain_bwd_f32(
            self.dOut.data_ptr(), tab([w.data_ptr() for w in self.W]), self.V0.data_ptr(), tab([x.data_ptr() for x in self.X]),
            tab([d[1].data_ptr() for d in self.dW] if dW_ptrs is None else dW_ptrs), self.dV0[1].data_ptr(),
            None if self.dX is None else tab([d.data_ptr() for d in self.dX]), M, 1 if res else 0, Bc if B is None else B, N, L, C, offsets, s)

    def outputs(self):
        return [self.dV0] + self.dW

    def refill(self):
        for buf, _view, _span in self.outputs():
            buf.fill_(float("nan"))


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32)


def _assert_untouched(dev, what):
    for i, (buf, _view, _span) in enumerate(dev.outputs()):
        assert bool((_bits(buf) == NAN_BITS).all()), f"{what}: output {i} was written to"


def _assert_bands(dev, what):
    for i, (buf, _view, (lo, hi)) in enumerate(dev.outputs()):
        assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all()), f"{what}: output {i}, a band was written to"


def _same_or_both_nan(got_bits, want):
    want = np.ascontiguousarray(want, dtype=np.float32)
    got = got_bits.view(np.float32)
    return int((~((got_bits == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))).sum())


def _assert_oracle_bits(dev, want_dV0, want_dW, what, nan_meets_nan=False, dw_tol=None):
    """The bands still NaN; every output element written (no NaN left, unless the expectation itself holds NaN) and the oracle's bits."""
    _assert_bands(dev, what)
    for name, (_buf, view, _span), want in [("dV0", dev.dV0, want_dV0)] + [(f"dW_{m}", d, w) for m, (d, w) in enumerate(zip(dev.dW, want_dW))]:
        got = _bits(view)
        if dw_tol is not None and name != "dV0":
            g = got.view(np.float32)
            assert np.isfinite(g).all(), f"{what} {name}"
            assert rel_inf(g, want) <= dw_tol, f"{what} {name}: rel {rel_inf(g, want):.3e}"
            continue
        bad = _same_or_both_nan(got, want) if nan_meets_nan else int((got != np.ascontiguousarray(want).view(np.uint32)).sum())
        assert bad == 0, f"{what} {name}: {bad} of {got.size} elements differ from the oracle's bits"


def _one_launch(gpu, case, **kw):
    """The case on its own operands through the one launch: supported, returns 0, the oracle's bits inside intact bands."""
    _B, N, M, L, C, _res, _off = case
    assert _lib().psf_chord_chain_bwd_supported(N, L, C, M) == 1
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, **kw)
    assert dev.call() == 0, cc.case_id(case)
    _assert_oracle_bits(dev, want_dV0, want_dW, cc.case_id(case))
    return dev


# ---------------------------------------------------------------- a. every C = 4 instance
@pytest.mark.parametrize("case", cc.GRID, ids=cc.case_id)
def test_every_instance_of_one_channel_group(gpu, case):
    _one_launch(gpu, case)


# ---------------------------------------------------------------- b. limits
@pytest.mark.parametrize("case", cc.LIMITS, ids=cc.case_id)
def test_limit_shapes(gpu, case):
    _one_launch(gpu, case)


def test_lds_limit_is_raised_between_launches_of_one_instance(gpu):
    """N = 64 (35 KB of dynamic LDS), N = 1024 (72 KB: the launcher has to raise the kernel's limit now), N = 64 again."""
    for case in cc.RAISE_BETWEEN:
        _one_launch(gpu, case)


# ---------------------------------------------------------------- c. bands and alignment
@pytest.mark.parametrize("shift", cc.W_SHIFTS)
@pytest.mark.parametrize("case", cc.BANDS, ids=cc.case_id)
def test_w_and_dw_need_only_four_byte_alignment(gpu, case, shift):
    """W_m and dW_m `shift` floats off a 16-byte boundary (a W that is a slice of a stacked producer output arrives so): the
    kernel's packed row load and store must cope, and stay inside the row."""
    dev = _one_launch(gpu, case, w_shift=shift)
    assert all(w.data_ptr() % 16 == 4 * shift for w in dev.W) and all(d[1].data_ptr() % 16 == 4 * shift for d in dev.dW)


@pytest.mark.parametrize("which", ["x", "dout", "dv0"])
def test_misaligned_rows_are_refused_and_nothing_is_written(gpu, which):
    case = cc.BANDS[1]
    W, V0, dOut, X, _dV0, _dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, **{f"{which}_shift": 1})
    assert dev.call() == PSF_E_ALIGN
    _assert_untouched(dev, f"{which} 4 bytes off")


def test_dw_aliasing_w_is_refused_and_nothing_is_written(gpu):
    case = cc.BANDS[0]
    W, V0, dOut, X, _dV0, _dW = cc.problem(case)
    for m in range(case[2]):
        dev = _Device(gpu, case, W, V0, dOut, X)
        ptrs = [d[1].data_ptr() for d in dev.dW]
        ptrs[m] = dev.W[m].data_ptr()
        before = [_bits(w) for w in dev.W]
        assert dev.call(dW_ptrs=ptrs) == PSF_E_ALIAS
        _assert_untouched(dev, f"dW_{m} is W_{m}")
        assert all(np.array_equal(a, _bits(w)) for a, w in zip(before, dev.W))


# ---------------------------------------------------------------- d. stale LDS
@pytest.mark.parametrize("case", cc.STALE, ids=cc.case_id)
def test_after_nan_in_every_lds(gpu, case):
    """Threads with tid >= N leave their xs / gs slots unwritten: what earlier kernels left there must not reach a result."""
    from test_gpu_stale_lds import _poison
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X)
    assert _lib().psf_chord_chain_bwd_supported(case[1], case[3], case[4], case[2]) == 1
    _poison(gpu)
    assert dev.call() == 0
    _assert_oracle_bits(dev, want_dV0, want_dW, cc.case_id(case))


# ---------------------------------------------------------------- e. special values
TAME = [np.nan, np.inf, -np.inf, 1e-42, -3e-45, 0.0, -0.0, 1.17549435e-38, 2e-38]  # test_gpu_parity's list


@pytest.mark.parametrize("huge", [False, True], ids=["tame", "near_flt_max"])
@pytest.mark.parametrize("case", cc.SPECIAL, ids=cc.case_id)
def test_special_values_propagate_as_in_the_oracle(gpu, case, huge):
    """NaN, +-Inf, denormals, the smallest normal and +-0 scattered over dOut, every W_m and V0; then the same with +-3e38. The
    kernel sums in the oracle's order (unlike the step kernels' dW), so the overflow patterns agree too: the oracle's bits
    everywhere, or NaN on both sides."""
    from test_gpu_parity import _special
    B, N, M, L, C, res, off = case
    values = TAME + ([3e38, -3e38] if huge else [])
    W = [_special((B, N, L), 11 + m, values) for m in range(M)]
    V0, dOut = _special((B, N, C), 2, values), _special((B, N, C), 4, values)
    with np.errstate(all="ignore"):
        X = cc.forward(W, V0, res, off)
        want_dV0, want_dW = cc.oracle_backward(W, X, dOut, res, off)
    assert np.isnan(want_dV0).any() and not np.isnan(want_dV0).all() and any(np.isinf(w).any() for w in want_dW)
    assert _lib().psf_chord_chain_bwd_supported(N, L, C, M) == 1
    dev = _Device(gpu, case, W, V0, dOut, X)
    assert dev.call() == 0
    _assert_oracle_bits(dev, want_dV0, want_dW, cc.case_id(case), nan_meets_nan=True)


# ---------------------------------------------------------------- f. more workgroups than CUs
def test_more_workgroups_than_cus(gpu):
    """600 sequences, three distinct ones repeated 200 times: every copy equals its original, the originals equal the oracle."""
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(cc.WIDE)
    B, N, M, L, C, res, off = cc.WIDE
    rep = lambda a: np.tile(a, (cc.WIDE_COPIES, 1, 1))  # noqa: E731  (sequence i is original i mod 3)
    case = (B * cc.WIDE_COPIES, N, M, L, C, res, off)
    assert _lib().psf_chord_chain_bwd_supported(N, L, C, M) == 1
    dev = _Device(gpu, case, [rep(w) for w in W], rep(V0), rep(dOut), [rep(x) for x in X])
    assert dev.call() == 0
    _assert_bands(dev, "B = 600")
    for name, (_buf, view, _span), want in [("dV0", dev.dV0, want_dV0)] + [(f"dW_{m}", d, w) for m, (d, w) in enumerate(zip(dev.dW, want_dW))]:
        got = _bits(view)
        assert np.array_equal(got[:B], np.ascontiguousarray(want).view(np.uint32)), f"{name}: the originals"
        assert np.array_equal(got, np.tile(got[:B], (cc.WIDE_COPIES, 1, 1))), f"{name}: a copy differs from its original"


# ---------------------------------------------------------------- g. the entry's other answers
@pytest.mark.parametrize("case", cc.LIBRARY_STEPS, ids=cc.case_id)
def test_uncovered_shapes_run_the_steps_inside_the_library(gpu, case):
    """N, C, L or M outside the kernel's range, dX_steps supplied: the per-step kernels and one psf_sum_tensors_f32 pass. dV0 has
    the oracle's bits (links ascending in every dV kernel, the residual terms left to right); dW sums across lanes in another
    order and meets the project's 1e-5."""
    _B, N, M, L, C, _res, _off = case
    assert _lib().psf_chord_chain_bwd_supported(N, L, C, M) == 0
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, with_dx=True)
    assert dev.call() == 0
    _assert_oracle_bits(dev, want_dV0, want_dW, cc.case_id(case), dw_tol=1e-5)


def test_unsupported_answers_write_nothing(gpu):
    lib = _lib()
    # a residual chain of 65 steps: beyond the one launch and beyond the residual sum, dX_steps or not
    case = cc.UNSUPPORTED
    W, V0, dOut = cc.operands(case)
    X = cc.forward(W, V0, case[5], case[6])
    dev = _Device(gpu, case, W, V0, dOut, X, with_dx=True)
    assert dev.call() == PSF_E_UNSUPPORTED
    _assert_untouched(dev, "65 steps with the residual")
    # an uncovered shape without dX_steps
    case = cc.LIBRARY_STEPS[0]
    W, V0, dOut, X, _dV0, _dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X)
    assert dev.call() == PSF_E_UNSUPPORTED
    _assert_untouched(dev, "N = 1025 without dX_steps")
    # the knob
    import sparsefactorization_amd as sfa
    case = cc.STALE[0]
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, with_dx=True)
    sfa.set_tuning("chain_bwd_fused", 0)
    try:
        assert lib.psf_chord_chain_bwd_supported(case[1], case[3], case[4], case[2]) == 0
        assert dev.call() == PSF_E_UNSUPPORTED
    finally:
        sfa.set_tuning("chain_bwd_fused", 1)
    _assert_untouched(dev, "knob chain_bwd_fused = 0")
    # B = 0: nothing to do, nothing written
    assert dev.call(B=0) == 0
    torch.cuda.synchronize()
    _assert_untouched(dev, "B = 0")
    assert dev.call() == 0  # (and the same buffers with the knob back: the one launch)
    _assert_oracle_bits(dev, want_dV0, want_dW, cc.case_id(case))


# ---------------------------------------------------------------- h. graph capture
def test_one_call_replays_from_a_graph(gpu):
    """The entry issues one stream launch: a graph of a single node. Replayed twice, the operands overwritten in place in
    between (the batch reversed, dOut negated): each replay has the oracle's bits for what the buffers hold then."""
    case = cc.GRAPH
    _B, N, M, L, C, res, off = case
    W, V0, dOut, X, want_dV0, want_dW = cc.problem(case)
    W2, V02, dOut2 = [np.ascontiguousarray(w[::-1]) for w in W], np.ascontiguousarray(V0[::-1]), np.ascontiguousarray(-dOut[::-1])
    X2 = cc.forward(W2, V02, res, off)
    want2_dV0, want2_dW = cc.oracle_backward(W2, X2, dOut2, res, off)
    assert not cc.same_bits(want2_dV0, want_dV0)
    assert _lib().psf_chord_chain_bwd_supported(N, L, C, M) == 1
    dev = _Device(gpu, case, W, V0, dOut, X)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        assert dev.call() == 0  # warm-up outside the capture: the instance's dynamic-LDS limit is raised here
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    _assert_oracle_bits(dev, want_dV0, want_dW, "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert dev.call(stream=torch.cuda.current_stream(gpu).cuda_stream) == 0
    dev.refill()
    graph.replay()
    torch.cuda.synchronize()
    _assert_oracle_bits(dev, want_dV0, want_dW, "first replay")
    for dst, src in zip(dev.W + dev.X + [dev.dOut], W2 + X2[:M] + [dOut2]):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    dev.refill()
    graph.replay()
    torch.cuda.synchronize()
    _assert_oracle_bits(dev, want2_dV0, want2_dW, "second replay")
