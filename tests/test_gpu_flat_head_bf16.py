"""GPU: psf_flat_head_bf16 and psf_flat_head_bwd_bf16 through the raw ABI (csrc/flat_head.hip, include/psf_chord.h).

  known answers   every case of flat_head_bf16_cases.py (position probes at every boundary the kernels have inside K, dense
                  small-integer cases): exact bits, whatever the summation order
  bit for bit     out / dX / dW == rne_bf16(the f32 entry on the widened operands) on the int16 views — the contract of the
                  header: same arithmetic in the same order, one rounding at the store
  accuracy        against a float64 product of the same widened operands, every element:
                      |got - ref| <= 2^-8 |ref| + n 2^-24 sum_i |a_i| |b_i|
                  half a bf16 ulp for the one rounding plus the worst-case f32 accumulation bound over the n summed terms
                  (n = K, + 1 with a bias, forward; B for dW; J for dX). Derived, not tuned; no element is excluded.
  guard bands     out, dX, dW (and the f32 workspace) sit inside larger sentinel-filled allocations: 64 elements before and 64
                  after are unchanged after every call of this file, ragged K and B % 8 != 0 included.

Shapes: forward J in {1, 3, 8}, B in {1, 7, 8, 9} x K in {4, 1020, 1024, 1028, 4096} (the 1024-element chunk form) and
B = 1024 x K in {32768, 32764} (ceil(K / 4096) ceil(B / 8) = 1024: the 4096-element form, the second with a ragged last chunk);
backward J in {1, 7, 16}, B in {1, 8, 9, 1024} x K in {4, 252, 256, 260}, each with dX only, dW only and both.
"""
import numpy as np
import pytest
import torch

import flat_head_bf16_cases as C

pytestmark = pytest.mark.gpu

BAND = 64
SENTINEL = 0x7FA5  # a bf16 NaN no kernel here produces
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _lib_and_stream(gpu):
    from sparsefactorization_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream(gpu).cuda_stream


class Banded:
    """A bf16 array of ``shape`` with BAND sentinel elements on either side (128 bytes: the inner array keeps the allocation's
    alignment)."""

    def __init__(self, shape, gpu):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=torch.int16, device=gpu)
        self.inner = self.buf[BAND:BAND + n].view(BF16).view(*shape)
        assert self.inner.data_ptr() % 8 == 0

    def check(self, what):
        assert bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[-BAND:] == SENTINEL).all()), f"{what}: written outside"
        assert not bool((self.inner.view(torch.int16) == SENTINEL).any()), f"{what}: an element was not written"


def _workspace(nbytes, gpu):
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.full((nbytes // 4 + 2 * BAND,), float("nan"), dtype=F32, device=gpu)
    return buf, buf[BAND:BAND + nbytes // 4]


def _ws_check(buf):
    assert bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[-BAND:]).all()), "workspace: written outside"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_fwd_bf16(gpu, x, w, b):
    _lib, lib, s = _lib_and_stream(gpu)
    (B, K), J = x.shape, w.shape[0]
    assert x.dtype == w.dtype == BF16 and x.is_contiguous() and w.is_contiguous()
    nbytes = lib.psf_flat_head_workspace(B, K, J)
    wsbuf, ws = _workspace(nbytes, gpu)
    out = Banded((B, J), gpu)
    _lib.check(lib.psf_flat_head_bf16(x.data_ptr(), w.data_ptr(), _ptr(b), out.inner.data_ptr(), B, K, J, ws.data_ptr(), nbytes, s),
               "psf_flat_head_bf16")
    out.check(f"out B={B} K={K} J={J}")
    _ws_check(wsbuf)
    return out.inner


def run_fwd_f32(gpu, x, w, b):
    _lib, lib, s = _lib_and_stream(gpu)
    (B, K), J = x.shape, w.shape[0]
    assert x.dtype == w.dtype == F32
    nbytes = lib.psf_flat_head_workspace(B, K, J)
    ws = torch.empty(nbytes // 4, dtype=F32, device=gpu)
    out = torch.empty(B, J, dtype=F32, device=gpu)
    _lib.check(lib.psf_flat_head_f32(x.data_ptr(), w.data_ptr(), _ptr(b), out.data_ptr(), B, K, J, ws.data_ptr(), nbytes, s),
               "psf_flat_head_f32")
    return out


def run_bwd_bf16(gpu, dy, x, w, want_dx, want_dw):
    _lib, lib, s = _lib_and_stream(gpu)
    (B, K), J = x.shape, w.shape[0]
    assert dy.dtype == x.dtype == w.dtype == BF16 and dy.shape == (B, J)
    dX = Banded((B, K), gpu) if want_dx else None
    dW = Banded((J, K), gpu) if want_dw else None
    _lib.check(lib.psf_flat_head_bwd_bf16(dy.data_ptr(), x.data_ptr(), w.data_ptr(), dX.inner.data_ptr() if dX else None,
                                          dW.inner.data_ptr() if dW else None, B, K, J, s), "psf_flat_head_bwd_bf16")
    for band, name in ((dX, "dX"), (dW, "dW")):
        if band is not None:
            band.check(f"{name} B={B} K={K} J={J}")
    return (dX.inner if dX else None), (dW.inner if dW else None)


def run_bwd_f32(gpu, dy, x, w, want_dx, want_dw):
    _lib, lib, s = _lib_and_stream(gpu)
    (B, K), J = x.shape, w.shape[0]
    dX = torch.empty(B, K, dtype=F32, device=gpu) if want_dx else None
    dW = torch.empty(J, K, dtype=F32, device=gpu) if want_dw else None
    _lib.check(lib.psf_flat_head_bwd_f32(dy.data_ptr(), x.data_ptr(), w.data_ptr(), _ptr(dX), _ptr(dW), B, K, J, s), "psf_flat_head_bwd_f32")
    return dX, dW


def within_bound(got, ref, sum_abs, n, what):
    """|got - ref| <= 2^-8 |ref| + n 2^-24 sum |a||b|, every element; prints the worst ratio before it asserts."""
    err = (got.to(F64) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + n * 2.0 ** -24 * sum_abs
    finite = bool(torch.isfinite(got.float()).all())
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}, max |err| = {float(err.max()):.3e}")
    assert finite and bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound (worst ratio {worst:.3f})"


def _randn_bf16(shape, gpu, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(*shape, device=gpu, generator=g).to(BF16)


# ------------------------------------------------------------------------------------------------------- known answers
def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(BF16)


def _want(a, gpu):
    return torch.from_numpy(C.as_bf16(a) + np.float32(0.0)).to(gpu).to(BF16)  # (+ 0.0: a zero is +0, as a sum from +0 is)


@pytest.mark.parametrize("case", C.FWD, ids=lambda c: c.id)
def test_forward_known_answers_are_exact(gpu, case):
    got = run_fwd_bf16(gpu, _dev(case.x(), gpu), _dev(case.w(), gpu), _dev(case.b(), gpu))
    want = _want(case.expected(), gpu)
    assert torch.equal(_bits(got), _bits(want)), (got.float() - want.float()).abs().max()


@pytest.mark.parametrize("case", C.BWD, ids=lambda c: c.id)
def test_backward_known_answers_are_exact(gpu, case):
    dX, dW = run_bwd_bf16(gpu, _dev(case.dy(), gpu), _dev(case.x(), gpu), _dev(case.w(), gpu), case.want_dx, case.want_dw)
    want_dX, want_dW = case.expected()
    if case.want_dx:
        assert torch.equal(_bits(dX), _bits(_want(want_dX, gpu)))
    if case.want_dw:
        assert torch.equal(_bits(dW), _bits(_want(want_dW, gpu)))


# ------------------------------------------------------------------------------------- bit for bit, accuracy, guard bands
FWD_JS, BWD_JS = (1, 3, 8), (1, 7, 16)


def _check_forward(gpu, B, K, J, seed):
    x, w, b = _randn_bf16((B, K), gpu, seed), _randn_bf16((J, K), gpu, seed + 1), _randn_bf16((J,), gpu, seed + 2)
    for bias in (b, None) if (B, J) == (7, 3) else (b,):
        got = run_fwd_bf16(gpu, x, w, bias)
        f32 = run_fwd_f32(gpu, x.float(), w.float(), None if bias is None else bias.float())
        assert torch.equal(_bits(got), _bits(f32.to(BF16))), f"B={B} K={K} J={J}: not the f32 entry's result rounded once"
        x64, w64 = x.to(F64), w.to(F64)
        ref, sum_abs = x64 @ w64.t(), x64.abs() @ w64.abs().t()
        if bias is not None:
            ref, sum_abs = ref + bias.to(F64), sum_abs + bias.to(F64).abs()
        within_bound(got, ref, sum_abs, K + (bias is not None), f"out B={B} K={K} J={J}")


@pytest.mark.parametrize("K", [4, 1020, 1024, 1028, 4096])
def test_forward_small_shapes(gpu, K):
    for B in (1, 7, 8, 9):
        for J in FWD_JS:
            _check_forward(gpu, B, K, J, 1000 * K + 10 * B + J)


@pytest.mark.parametrize("K", [32768, 32764])
def test_forward_four_float4_form(gpu, K):
    """B = 1024: ceil(K / 4096) * ceil(B / 8) = 1024 workgroups, so a thread takes four groups of four; 32764 leaves the last
    chunk ragged."""
    assert -(-K // 4096) * (1024 // 8) == 1024
    for J in FWD_JS:
        _check_forward(gpu, 1024, K, J, K + J)


@pytest.mark.parametrize("B", [1, 8, 9, 1024])
def test_backward_shapes(gpu, B):
    for K in (4, 252, 256, 260):
        for J in BWD_JS:
            seed = 100000 * B + 100 * K + J
            dy, x, w = _randn_bf16((B, J), gpu, seed), _randn_bf16((B, K), gpu, seed + 1), _randn_bf16((J, K), gpu, seed + 2)
            dy64, x64, w64 = dy.to(F64), x.to(F64), w.to(F64)
            ref_dX, abs_dX = dy64 @ w64, dy64.abs() @ w64.abs()
            ref_dW, abs_dW = dy64.t() @ x64, dy64.abs().t() @ x64.abs()
            for want_dx, want_dw in ((True, False), (False, True), (True, True)):
                dX, dW = run_bwd_bf16(gpu, dy, x, w, want_dx, want_dw)
                fX, fW = run_bwd_f32(gpu, dy.float(), x.float(), w.float(), want_dx, want_dw)
                what = f"B={B} K={K} J={J} dx={want_dx} dw={want_dw}"
                if want_dx:
                    assert torch.equal(_bits(dX), _bits(fX.to(BF16))), f"dX {what}: not the f32 entry's result rounded once"
                    within_bound(dX, ref_dX, abs_dX, J, f"dX {what}")
                if want_dw:
                    assert torch.equal(_bits(dW), _bits(fW.to(BF16))), f"dW {what}: not the f32 entry's result rounded once"
                    within_bound(dW, ref_dW, abs_dW, B, f"dW {what}")


def test_results_are_the_same_bits_run_to_run(gpu):
    x, w, b = _randn_bf16((9, 4096 + 12), gpu, 1), _randn_bf16((3, 4096 + 12), gpu, 2), _randn_bf16((3,), gpu, 3)
    assert torch.equal(_bits(run_fwd_bf16(gpu, x, w, b)), _bits(run_fwd_bf16(gpu, x, w, b)))
    dy = _randn_bf16((9, 3), gpu, 4)
    a, c = run_bwd_bf16(gpu, dy, x, w, True, True), run_bwd_bf16(gpu, dy, x, w, True, True)
    assert torch.equal(_bits(a[0]), _bits(c[0])) and torch.equal(_bits(a[1]), _bits(c[1]))
