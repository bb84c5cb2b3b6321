"""GPU: the one-launch bf16 backward chain (csrc/bwd_chain_lds_bf16.h: chord_chain_bwd_lds_k<bf16, L, G, RES>) through
psf_chord_chain_bwd_lds_bf16 itself, at its limits. ctypes tables, X_steps from the CPU forward of tests/chain_bwd_bf16_cases.py —
so the backward stands on its own. Every comparison is on bits; any NaN equals any NaN (be.same_bits).

Two references: cb.plain_backward_bf16 (the documented contract in numpy; its CPU self-test shows that three ways of departing
from it give other bits) and psf_chord_chain_bwd_bf16, the per-step route, on the same operands at 16-byte-aligned addresses.
Every dW_m and dV0 is a view into an arena of be.SENTINEL with 256-byte bands on either side: after each call the bands are
intact and the output fully written.

  1. every instance: L = 2..20 x residual at C = 8 and at C = 16
  2. limits: the dynamic-LDS maximum, M = 64, N = 1, 2, 3, 63, 64, 65, 1023, 1024, duplicate and explicit offsets, the 48 KB raise
  3. W_m and dW_m 0, 1 and 3 elements off a 16-byte boundary, odd and even L, W_m ending with its allocation
  4. a small case after a large one
  5. NaN, +-Inf, +-0 against the per-step route
  6. declines write nothing
  7. the autograd route, opt-in, against the default route
"""
import ctypes

import numpy as np
import pytest
import torch

import bf16_edges as be
import chain_bwd_bf16_cases as cb

pytestmark = pytest.mark.gpu

PSF_E_ALIGN, PSF_E_UNSUPPORTED = -4, -7


def _lib():
    from sparsefactorization_amd import _lib
    return _lib.load()


def _up(bits, gpu):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(gpu)


def _down(t):
    return t.detach().cpu().numpy().view(np.uint16)


def _input(a, gpu, shift=0):
    """The bf16 bits of `a` on the device, `shift` elements past a 16-byte boundary, ENDING with their allocation."""
    bits = be.rne_bits(a).reshape(-1)
    buf = torch.empty(shift + bits.size, dtype=torch.int16, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:]
    view.copy_(_up(bits, gpu))
    assert view.data_ptr() + 2 * bits.size == buf.data_ptr() + 2 * buf.numel()
    return view


class _Arena:
    """n output elements at element shift `shift` inside be.SENTINEL."""

    def __init__(self, n, gpu, shift=0):
        total, self.lo, self.hi = be.arena_span(n, shift)
        self.buf = torch.full((total,), be.SENTINEL, dtype=torch.int16, device=gpu)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.hi]

    def report(self):
        return be.band_report(_down(self.buf), self.lo, self.hi)

    def bits(self):
        return _down(self.view)


assert be.SENTINEL < 0x8000  # (fits int16 as it is)


class _Device:
    def __init__(self, gpu, case, W, V0, dOut, X, w_shift=0, dout_shift=0):
        B, N, M, L, C, _res, _off = case
        self.case, self.gpu = case, gpu
        self.W = [_input(w, gpu, w_shift) for w in W]
        self.V0 = _input(V0, gpu)
        self.X = [self.V0] + [_input(x, gpu) for x in X[1:M]]
        self.dOut = _input(dOut, gpu, dout_shift)
        self.dW = [_Arena(B * N * L, gpu, w_shift) for _ in range(M)]
        self.dV0 = _Arena(B * N * C, gpu)

    def _args(self):
        _B, _N, M, L, _C, _res, off = self.case
        tab = lambda ptrs: (ctypes.c_void_p * M)(*ptrs)  # noqa: E731
        offsets = None if off is None else (ctypes.c_int64 * L)(*off)
        return (self.dOut.data_ptr(), tab([w.data_ptr() for w in self.W]), self.V0.data_ptr(), tab([x.data_ptr() for x in self.X]),
                tab([d.view.data_ptr() for d in self.dW]), self.dV0.view.data_ptr()), offsets

    def call(self):
        B, N, M, L, C, res, _off = self.case
        ptrs, offsets = self._args()
        return _lib().psf_chord_chain_bwd_lds_bf16(*ptrs, M, 1 if res else 0, B, N, L, C, offsets,
                                                   torch.cuda.current_stream(self.gpu).cuda_stream)

    def call_steps(self):
        """The per-step route into the same outputs (psf_chord_chain_bwd_bf16 with its M gradient buffers)."""
        B, N, M, L, C, res, _off = self.case
        ptrs, offsets = self._args()
        dX = [torch.empty(B * N * C, dtype=torch.int16, device=self.gpu) for _ in range(M)]
        rc = _lib().psf_chord_chain_bwd_bf16(*ptrs, (ctypes.c_void_p * M)(*[d.data_ptr() for d in dX]), M, 1 if res else 0, B, N, L, C,
                                             offsets, torch.cuda.current_stream(self.gpu).cuda_stream)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return [("dV0", self.dV0)] + [(f"dW_{m}", d) for m, d in enumerate(self.dW)]

    def results(self):
        return [a.bits() for _name, a in self.outputs()]

    def assert_untouched(self, what):
        torch.cuda.synchronize()
        for name, a in self.outputs():
            assert bool((_down(a.buf) == be.SENTINEL).all()), f"{what}: {name} was written to"

    def assert_bands(self, what, written=True):
        torch.cuda.synchronize()
        for name, a in self.outputs():
            below, above, inside = a.report()
            assert below == 0 and above == 0, f"{what}: {name}: {below} elements below and {above} above the output were written to"
            if written:
                assert inside == 0, f"{what}: {name}: {inside} elements were not written"


def _assert_bits(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = be.same_bits(g.reshape(-1), np.asarray(w).reshape(-1))
        assert bad == 0, f"{what}: {'dV0' if i == 0 else f'dW_{i - 1}'}: {bad} of {g.size} elements differ"


def _per_step_bits(gpu, case, W, V0, dOut, X):
    """(dV0, dW_0, ...) of the per-step route at 16-byte-aligned operands, or None where that entry does not take the chain."""
    dev = _Device(gpu, case, W, V0, dOut, X)
    rc = dev.call_steps()
    if rc == PSF_E_UNSUPPORTED:
        return None
    assert rc == 0
    dev.assert_bands(f"{cb.case_id(case)}, per-step route")
    return dev.results()


def _one_launch(gpu, case, steps="where it applies", **kw):
    """The case through the one launch: supported, returns 0, intact bands, the contract's bits and the per-step route's."""
    _B, N, M, L, C, res, _off = case
    what = cb.case_id(case)
    assert _lib().psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 1, what
    W, V0, dOut, X = cb.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, **kw)
    assert dev.call() == 0, what
    dev.assert_bands(what)
    got = dev.results()
    want_dV0, want_dW = cb.plain_backward_bf16(case)
    _assert_bits(got, [want_dV0, *want_dW], f"{what} against the contract")
    per_step = _per_step_bits(gpu, case, W, V0, dOut, X)
    if steps == "must":
        assert per_step is not None, what
    if per_step is None:  # (psf_sum_tensors_bf16's limits: more than 32 residual terms)
        assert res and M + 1 > 32, what
    else:
        _assert_bits(got, per_step, f"{what} against the per-step route")
    return dev, got


# ---------------------------------------------------------------- 1. every instance
@pytest.mark.parametrize("case", cb.GRID, ids=cb.case_id)
def test_every_instance(gpu, case):
    _one_launch(gpu, case, steps="must")


# ---------------------------------------------------------------- 2. limits
@pytest.mark.parametrize("case", cb.LIMITS, ids=cb.case_id)
def test_limit_shapes(gpu, case):
    _one_launch(gpu, case)


def test_lds_limit_is_raised_between_launches_of_one_instance(gpu):
    """N = 64 (35 KB of dynamic LDS), N = 1024 (72 KB: the launcher has to raise the kernel's limit now), N = 64 again."""
    for case in cb.RAISE_BETWEEN:
        _one_launch(gpu, case)


# ---------------------------------------------------------------- 3. bands and alignment
@pytest.mark.parametrize("shift", cb.W_SHIFTS)
@pytest.mark.parametrize("case", cb.BANDS, ids=cb.case_id)
def test_w_and_dw_at_any_two_byte_alignment(gpu, case, shift):
    """W_m and dW_m `shift` bf16 elements off a 16-byte boundary (odd shifts: off their dword too), W_m ending with its
    allocation: the right bits, and nothing written outside dW_m and dV0. The per-step reference runs on aligned copies."""
    dev, _got = _one_launch(gpu, case, w_shift=shift)
    assert all(w.data_ptr() % 16 == 2 * shift for w in dev.W) and all(d.view.data_ptr() % 16 == 2 * shift for d in dev.dW)


# ---------------------------------------------------------------- 4. stale LDS
def test_small_cases_after_a_large_one(gpu):
    """Threads with tid >= N leave their xs / gs slots unwritten, and W_m fills N (L | 1) floats only: what the largest launch
    left in LDS must not reach a result. Each small case gives the bits it gave before the large one, and the contract's."""
    before = [_one_launch(gpu, case)[1] for case in cb.STALE]
    for case, first in zip(cb.STALE, before):
        _one_launch(gpu, cb.STALE_FIRST)
        _dev, got = _one_launch(gpu, case)
        _assert_bits(got, first, f"{cb.case_id(case)} after {cb.case_id(cb.STALE_FIRST)}")


# ---------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("run", ["w", "dz_tame"])
@pytest.mark.parametrize("case", cb.SPECIAL, ids=cb.case_id)
def test_special_values_as_on_the_per_step_route(gpu, case, run):
    """NaN, +-Inf and +-0 anywhere (run "w": +-2^126 and +-2^-126 in W as well). Compared with the per-step GPU route only."""
    B, N, M, L, C, res, _off = case
    Wsp, V0, _R, dOut = be.special_operands(B, N, L, C, run)
    W = [Wsp] + [be.special_case((B, N, L), 70 + m, be.SPECIAL_TAME) for m in range(1, M)]
    X = cb.forward_bf16(W, V0, res, cb.offsets_of(case))
    assert _lib().psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 1
    dev = _Device(gpu, case, W, V0, dOut, X)
    assert dev.call() == 0
    dev.assert_bands(cb.case_id(case), written=False)
    got = dev.results()
    assert np.isnan(be.bits_f32(got[0])).any()
    per_step = _per_step_bits(gpu, case, W, V0, dOut, X)
    assert per_step is not None
    _assert_bits(got, per_step, f"{cb.case_id(case)} {run} against the per-step route")


# ---------------------------------------------------------------- 6. declines
@pytest.mark.parametrize("case", cb.DECLINED, ids=cb.case_id)
def test_uncovered_shapes_are_declined_and_nothing_is_written(gpu, case):
    _B, N, M, L, C, _res, _off = case
    assert _lib().psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 0
    W, V0, dOut = cb.operands(case)
    dev = _Device(gpu, case, W, V0, dOut, [V0] * (M + 1))  # (never read)
    assert dev.call() == PSF_E_UNSUPPORTED
    dev.assert_untouched(cb.case_id(case))


def test_misaligned_dout_is_refused_and_nothing_is_written(gpu):
    case = cb.MISALIGNED
    W, V0, dOut, X = cb.problem(case)
    dev = _Device(gpu, case, W, V0, dOut, X, dout_shift=4)
    assert dev.dOut.data_ptr() % 16 == 8
    assert dev.call() == PSF_E_ALIGN
    dev.assert_untouched("dOut 8 bytes off")


# ---------------------------------------------------------------- 7. the autograd route
def _bf16_tensor(a, gpu):
    return _up(be.rne_bits(a), gpu).view(torch.bfloat16).reshape(a.shape)


def _grads(Ws, V0, dOut):
    import sparsefactorization_amd as sfa
    ws = [w.detach().clone().requires_grad_(True) for w in Ws]
    v0 = V0.detach().clone().requires_grad_(True)
    grads = torch.autograd.grad(sfa.chord_chain(ws, v0, True), [v0, *ws], dOut)
    torch.cuda.synchronize()
    return [_down(t.contiguous().view(torch.int16)) for t in grads]


def _count_calls(monkeypatch, lib, name):
    calls, real = [], getattr(lib, name)

    def counted(*args):
        rc = real(*args)
        calls.append(rc)
        return rc
    monkeypatch.setattr(lib, name, counted, raising=True)
    return calls


@pytest.mark.parametrize("shape", cb.AUTOGRAD + [cb.AUTOGRAD_FALLBACK], ids=lambda s: "B%d-N%d-M%d-L%d-C%d" % s)
def test_autograd_route_gives_the_default_routes_bits(gpu, shape, monkeypatch):
    from sparsefactorization_amd import chord
    B, N, M, L, C = shape
    case = (B, N, M, L, C, True, None)
    Wn, V0n, dOutn = cb.operands(case)
    Ws, V0, dOut = [_bf16_tensor(w, gpu) for w in Wn], _bf16_tensor(V0n, gpu), _bf16_tensor(dOutn, gpu)
    assert chord.bf16_chain_bwd_route == "never"
    calls = _count_calls(monkeypatch, _lib(), "psf_chord_chain_bwd_lds_bf16")
    never = _grads(Ws, V0, dOut)
    assert calls == []  # the default route does not go near the new entry
    chord.bf16_chain_bwd_route = "always"
    try:
        always = _grads(Ws, V0, dOut)
        again = _grads(Ws, V0, dOut)
    finally:
        chord.bf16_chain_bwd_route = "never"
    assert calls == ([0, 0] if cb.covered(N, L, C, M) else [])  # one launch each time, or the fallback without a call
    _assert_bits(always, never, f"{shape}: route 'always' against 'never'")
    for a, b in zip(always, again):
        assert np.array_equal(a, b), f"{shape}: a repeat differs"
