"""GPU: psf_linear_wgrad_bf16 (csrc/linear_wgrad_bf16.hip) and psf_affine_rows_bf16 (csrc/embed.hip) through the raw ABI.

  known answers   every case of linear_wgrad_bf16_cases.py (position probes at every edge of a fragment, a matrix step, a slab
                  and a 32-wide tile; dense small-integer cases whose one rounding is exercised, ties included): exact bits on
                  the int16 views, whatever the summation order
  accuracy        against a float64 product of the widened operands, EVERY element:
                      |got - ref| <= 2^-8 |ref| + T 2^-24 sum_t |dY[t,j]| |X[t,i]|        (db: the same with |X| = 1)
                  half a bf16 ulp for the one rounding plus the worst-case f32 accumulation bound over the T summed terms —
                  the form of tests/test_gpu_flat_head_bf16.py. Derived, not tuned. Inputs: normal bf16 values of mixed sign.
  shapes          (m, n) in SHAPES x T in TS, one T = 70 001 at (32, 32) (547 partial tiles, a ragged last slab) and one at
                  (128, 128) (slabs of two LDS tiles: the only small size at which a wave walks more than one tile and the
                  register prefetch of the next tile runs); with and without db; contiguous, as column slices whose row stride
                  is a multiple of 8 (16-byte loads, a partial last vector) and as slices with a row stride of m + 3 / n + 5
                  (4-, 2-byte and element loads)
  guard bands     dWt, db and the workspace sit inside sentinel-filled allocations and are unchanged outside after every call;
                  X and dY end flush against a sentinel band of their allocation (bf16 NaNs, like the gaps between the rows
                  of a slice): an over-read lands in memory this test owns and poisons the result. Nothing is set up to fault.
  error codes     PSF_E_ALIGN, PSF_E_SHAPE, PSF_E_NULL and the short workspace are returned before any launch: the outputs keep
                  their sentinels; two calls on the same operands give the same bits
  affine rows     known answers; guard bands at T in {0, 1, 255, 256, 257} x E in {8, 1024}; F.linear in bf16 to one bf16 step.
"""
import numpy as np
import pytest
import torch

import linear_wgrad_bf16_cases as C

pytestmark = pytest.mark.gpu

BAND = 64
SENTINEL = 0x7FA5  # a bf16 NaN no kernel here produces
BF16, F32, F64, I16 = torch.bfloat16, torch.float32, torch.float64, torch.int16
PSF_E_NULL, PSF_E_SHAPE, PSF_E_ALIGN = -1, -2, -4

SHAPES = [(1, 1), (2, 32), (3, 8), (15, 31), (32, 32), (33, 33), (64, 8), (127, 128), (128, 128)]
TS = [1, 2, 15, 16, 17, 33, 4097]
LAYOUTS = ("contiguous", "slice8", "slice_odd")


def _lib_and_stream(gpu):
    from sparsefactorization_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream(gpu).cuda_stream


class Banded:
    """A bf16 array of ``shape`` with BAND sentinel elements on either side."""

    def __init__(self, shape, gpu):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND,), SENTINEL, dtype=I16, device=gpu)
        self.inner = self.buf[BAND:BAND + n].view(BF16).view(*shape)
        self.ptr = self.buf.data_ptr() + 2 * BAND  # the inner array's address, also where it is empty (an empty view has none)

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def check(self, what):
        assert bool((self.buf[:BAND] == SENTINEL).all()) and bool((self.buf[-BAND:] == SENTINEL).all()), f"{what}: written outside"
        assert not bool((self.inner.view(I16) == SENTINEL).any()), f"{what}: an element was not written"


def _ld(width, layout, odd_pad):
    return {"contiguous": width, "slice8": -(-width // 8) * 8 + 8, "slice_odd": width + odd_pad}[layout]


def place(a, ld, gpu):
    """``a`` [T, w] bf16 as a column slice with row stride ``ld`` that ENDS flush against a sentinel band: the elements behind
    a[T-1, w-1], and the gaps between the rows, are bf16 NaNs of this test's own allocation."""
    T, w = a.shape
    span = (T - 1) * ld + w
    buf = torch.full((span + 2 * BAND,), SENTINEL, dtype=I16, device=gpu)
    view = torch.as_strided(buf.view(BF16), (T, w), (ld, 1), BAND)
    view.copy_(a)
    return buf, view


def _workspace(nbytes, gpu):
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.full((nbytes // 4 + 2 * BAND,), float("nan"), dtype=F32, device=gpu)
    return buf, buf[BAND:BAND + nbytes // 4]


def run_wgrad(gpu, x, dy, want_db=True, layout="contiguous"):
    """x [T, m], dy [T, n] bf16 (any layout) -> (dWt [n, m], db [n] or None), every guard band checked."""
    _lib, lib, s = _lib_and_stream(gpu)
    (T, m), n = x.shape, dy.shape[1]
    xb, xv = place(x, _ld(m, layout, 3), gpu)
    yb, yv = place(dy, _ld(n, layout, 5), gpu)
    nbytes = lib.psf_linear_wgrad_bf16_workspace(T, m, n)
    assert nbytes == C.plan(T, m, n)["workspace_bytes"], "the plan mirrored in linear_wgrad_bf16_cases.py is not the kernel's"
    wsbuf, ws = _workspace(nbytes, gpu)
    dWt, db = Banded((n, m), gpu), (Banded((n,), gpu) if want_db else None)
    _lib.check(lib.psf_linear_wgrad_bf16(xv.data_ptr(), xv.stride(0), yv.data_ptr(), yv.stride(0), T, m, n, dWt.inner.data_ptr(),
                                         db.inner.data_ptr() if db else None, ws.data_ptr(), nbytes, s), "psf_linear_wgrad_bf16")
    what = f"T={T} m={m} n={n} {layout}"
    dWt.check(f"dWt {what}")
    if db:
        db.check(f"db {what}")
    assert bool(torch.isnan(wsbuf[:BAND]).all()) and bool(torch.isnan(wsbuf[-BAND:]).all()), f"workspace {what}: written outside"
    return dWt.inner, (db.inner if db else None)


def _bits(t):
    return t.contiguous().view(I16)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(BF16)


def within_bound(got, ref, sum_abs, n, what):
    """|got - ref| <= 2^-8 |ref| + n 2^-24 sum |a||b|, every element; prints the worst ratio before it asserts."""
    err = (got.to(F64) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + n * 2.0 ** -24 * sum_abs
    finite = bool(torch.isfinite(got.float()).all())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f}, max |err| = {float(err.max()):.3e}")
    assert finite and bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} of {err.numel()} elements beyond the bound (worst ratio {worst:.3f})"


def _normal_bf16(shape, gpu, seed):
    """Normal bf16 values of mixed sign: a standard normal pushed away from zero (|v| >= 2^-6)."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    v = torch.randn(*shape, device=gpu, generator=g)
    return (v + torch.copysign(torch.full_like(v, 2.0 ** -6), v)).to(BF16)


# ------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("shape", C.PROBE_SHAPES, ids=str)
def test_position_probes_are_exact(gpu, shape):
    T, m, n = shape
    for k, p in enumerate(C.probes(T, m, n)):
        dWt, db = run_wgrad(gpu, _dev(p.x(), gpu), _dev(p.dy(), gpu), True, LAYOUTS[k % 3] if m > 2 else "contiguous")
        wW, wb = p.expected()
        assert torch.equal(_bits(dWt), _bits(_dev(wW, gpu))) and torch.equal(_bits(db), _bits(_dev(wb, gpu))), (p, dWt.float().nonzero())


@pytest.mark.parametrize("case", C.DENSE, ids=lambda c: c.id)
def test_dense_known_answers_are_exact(gpu, case):
    wW, wb = case.expected()
    for layout in LAYOUTS:
        dWt, db = run_wgrad(gpu, _dev(case.x(), gpu), _dev(case.dy(), gpu), True, layout)
        assert torch.equal(_bits(dWt), _bits(_dev(wW, gpu))), (layout, (dWt.float() - _dev(wW, gpu).float()).abs().max())
        assert torch.equal(_bits(db), _bits(_dev(wb, gpu))), layout


# ------------------------------------------------------------------------------------------------- accuracy, guard bands
def _check(gpu, T, m, n, seed, layouts=LAYOUTS, dbs=(True, False)):
    x, dy = _normal_bf16((T, m), gpu, seed), _normal_bf16((T, n), gpu, seed + 1)
    x64, y64 = x.to(F64), dy.to(F64)
    ref_W, abs_W = y64.t() @ x64, y64.abs().t() @ x64.abs()
    ref_b, abs_b = y64.sum(0), y64.abs().sum(0)
    first = None
    for layout in layouts:
        for want_db in dbs:
            dWt, db = run_wgrad(gpu, x, dy, want_db, layout)
            what = f"T={T} m={m} n={n} {layout} db={want_db}"
            within_bound(dWt, ref_W, abs_W, T, f"dWt {what}")
            if want_db:
                within_bound(db, ref_b, abs_b, T, f"db {what}")
            if first is None:
                first = dWt.clone()
            assert torch.equal(_bits(dWt), _bits(first)), f"{what}: the layout or db changed the bits of dWt"


@pytest.mark.parametrize("mn", SHAPES, ids=lambda s: f"m{s[0]}-n{s[1]}")
def test_shapes_meet_the_bound_with_guard_bands(gpu, mn):
    for T in TS:
        _check(gpu, T, mn[0], mn[1], 1000 * T + 10 * mn[0] + mn[1])


@pytest.mark.parametrize("mn", [(32, 32), (128, 128)], ids=lambda s: f"m{s[0]}-n{s[1]}")
def test_many_partial_tiles_and_a_ragged_last_slab(gpu, mn):
    T = 70001
    p = C.plan(T, *mn)
    assert p["nparts"] > 256 and T % p["rows_per_wave"] != 0 and p["rows_per_wave"] == (32 if mn == (32, 32) else 64)
    _check(gpu, T, mn[0], mn[1], 7, layouts=("contiguous", "slice8"), dbs=(True,))


# ----------------------------------------------------------------------------------------------- repeatability, error codes
def test_two_calls_give_the_same_bits(gpu):
    x, dy = _normal_bf16((4097, 33), gpu, 1), _normal_bf16((4097, 127), gpu, 2)
    a, b = run_wgrad(gpu, x, dy), run_wgrad(gpu, x, dy)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_errors_are_returned_before_any_launch(gpu):
    _lib, lib, s = _lib_and_stream(gpu)
    T, m, n = 64, 32, 32
    x, dy = _normal_bf16((T, m), gpu, 3), _normal_bf16((T, n), gpu, 4)
    nbytes = lib.psf_linear_wgrad_bf16_workspace(T, m, n)
    wsbuf, ws = _workspace(nbytes, gpu)
    dWt, db = Banded((n, m), gpu), Banded((n,), gpu)

    def call(X=x.data_ptr(), ldx=m, DY=dy.data_ptr(), ldy=n, T=T, m=m, n=n, W=dWt.inner.data_ptr(), b=db.inner.data_ptr(),
             ws_ptr=ws.data_ptr(), ws_bytes=nbytes):
        rc = lib.psf_linear_wgrad_bf16(X, ldx, DY, ldy, T, m, n, W, b, ws_ptr, ws_bytes, s)
        torch.cuda.synchronize(gpu)
        assert dWt.untouched() and db.untouched() and bool(torch.isnan(wsbuf).all()), "an error path wrote something"
        return rc

    assert call(X=None) == PSF_E_NULL and call(DY=None) == PSF_E_NULL and call(W=None) == PSF_E_NULL and call(ws_ptr=None) == PSF_E_NULL
    assert call(T=0) == PSF_E_SHAPE and call(m=0) == PSF_E_SHAPE and call(n=129) == PSF_E_SHAPE and call(m=129, ldx=129) == PSF_E_SHAPE
    assert call(ldx=m - 1) == PSF_E_SHAPE and call(ldy=n - 1) == PSF_E_SHAPE
    assert call(ws_bytes=nbytes - 4) == PSF_E_SHAPE
    assert lib.psf_linear_wgrad_bf16_workspace(0, 1, 1) == -1 and lib.psf_linear_wgrad_bf16_workspace(1, 129, 1) == -1
    # alignment: 2 g bytes, g the largest power of two <= 8 dividing the row stride — a stride of 32 wants 16 bytes, 34 wants 4
    assert x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0
    for off in (2, 4, 8):
        assert call(X=x.data_ptr() + off) == PSF_E_ALIGN and call(DY=dy.data_ptr() + off) == PSF_E_ALIGN
    assert call(X=x.data_ptr() + 2, ldx=34) == PSF_E_ALIGN
    assert call(W=dWt.inner.data_ptr() + 1) == PSF_E_ALIGN and call(ws_ptr=ws.data_ptr() + 2) == PSF_E_ALIGN
    assert "psf_linear_wgrad_bf16" in _lib.last_error()
    # and the same operands, unharmed, still give the answer (the offsets above were never dereferenced)
    rc = lib.psf_linear_wgrad_bf16(x.data_ptr(), m, dy.data_ptr(), n, T, m, n, dWt.inner.data_ptr(), db.inner.data_ptr(), ws.data_ptr(), nbytes, s)
    assert rc == 0
    dWt.check("dWt after the error calls")
    within_bound(dWt.inner, dy.to(F64).t() @ x.to(F64), dy.to(F64).abs().t() @ x.to(F64).abs(), T, "dWt after the error calls")


# ------------------------------------------------------------------------------------------------------------ affine rows
def run_affine(gpu, x, w, b, T=None):
    """``T``: the rows to take, x.shape[0] by default (T = 0 wants an x that has an address)."""
    _lib, lib, s = _lib_and_stream(gpu)
    K, E = x.shape[1], w.shape[0]
    T = x.shape[0] if T is None else T
    out = Banded((T, E), gpu)
    _lib.check(lib.psf_affine_rows_bf16(x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), out.ptr, T, K, E, s),
               "psf_affine_rows_bf16")
    if T:
        out.check(f"affine rows T={T} K={K} E={E}")
    else:
        assert out.untouched()
    return out.inner


@pytest.mark.parametrize("case", C.AFFINE, ids=lambda c: c.id)
def test_affine_rows_known_answers_are_exact(gpu, case):
    got = run_affine(gpu, _dev(case.x(), gpu), _dev(case.w(), gpu), None if case.b() is None else _dev(case.b(), gpu))
    assert torch.equal(_bits(got), _bits(_dev(case.expected(), gpu)))


@pytest.mark.parametrize("E", [8, 1024])
def test_affine_rows_guard_bands_and_f_linear(gpu, E):
    for T in (0, 1, 255, 256, 257):
        for K in (1, 2, 3):
            for bias in (True, False):
                x, w = _normal_bf16((max(T, 1), K), gpu, 100 * T + K), _normal_bf16((E, K), gpu, E + K)  # (T = 0: a non-NULL x)
                b = _normal_bf16((E,), gpu, E) if bias else None
                got = run_affine(gpu, x, w, b, T)
                if T == 0:
                    continue
                stock = torch.nn.functional.linear(x, w, b)
                # one bf16 step: the neighbouring bf16 value, i.e. 2^-7 of the larger magnitude (|v| >= 2^e has spacing 2^(e-7))
                step = 2.0 ** -7 * torch.maximum(got.float().abs(), stock.float().abs())
                err = (got.float() - stock.float()).abs()
                print(f"affine rows T={T} K={K} E={E} bias={bias}: {int((err > 0).sum())} of {err.numel()} differ from F.linear")
                assert bool((err <= step).all()), f"T={T} K={K} E={E}: beyond one bf16 step of F.linear"
                ref = x.to(F64) @ w.to(F64).t() + (0 if b is None else b.to(F64))
                mag = x.to(F64).abs() @ w.to(F64).abs().t() + (0 if b is None else b.to(F64).abs())
                within_bound(got, ref, mag, K + 1, f"affine rows T={T} K={K} E={E} bias={bias}")


def test_affine_rows_error_codes(gpu):
    _lib, lib, s = _lib_and_stream(gpu)
    x, w = _normal_bf16((4, 2), gpu, 1), _normal_bf16((8, 2), gpu, 2)
    out = Banded((4, 8), gpu)
    o = out.inner.data_ptr()
    assert lib.psf_affine_rows_bf16(None, w.data_ptr(), None, o, 4, 2, 8, s) == PSF_E_NULL
    assert lib.psf_affine_rows_bf16(x.data_ptr(), w.data_ptr(), None, o, 4, 4, 8, s) == PSF_E_SHAPE
    assert lib.psf_affine_rows_bf16(x.data_ptr(), w.data_ptr(), None, o, 4, 2, 12, s) == PSF_E_SHAPE
    assert lib.psf_affine_rows_bf16(x.data_ptr(), w.data_ptr(), None, o + 2, 4, 2, 8, s) == PSF_E_ALIGN
    torch.cuda.synchronize(gpu)
    assert out.untouched()
