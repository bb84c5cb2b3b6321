"""GPU: the bf16 fused backward step (csrc/bwd_fused_bf16.h) and the bf16 backward chain entry (psf_chord_chain_bwd_bf16).

The fused kernel computes dV and dW with the arithmetic of the two bf16 window kernels, so the route must be invisible:
  * dV equals bf16_rne(f32 oracle dV) bit for bit,
  * dW is within one bf16 ulp plus 1e-5 max|dW| of bf16_rne(oracle dW) (the bound of tests/test_gpu_bf16.py, restated here),
  * dV AND dW are bit-identical to the same call with the knob bwd_fused = 0 (the two-kernel route).
Inputs are bf16-representable standard normals: every product lies in f32's normal range, where the bit-exact contract of
include/psf_chord.h ("bfloat16") applies. psf_describe_bwd says which kernel ran — without it a silent fallback to the two
kernels would pass every parity check here. No time is asserted anywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import chord_oracle as oc
from sparsefactorization_amd._lib import tuning

pytestmark = pytest.mark.gpu

DW_BAR = 1e-5  # the f32 dW bar of the parity suite, relative to max |dW|


def _mk(shape, seed, scale=1.0):
    """A bf16-representable f32 array (so the oracle sees exactly the kernel's inputs)."""
    a = np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * scale
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def _bt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev)


def _rne(a_f32):
    return torch.from_numpy(np.ascontiguousarray(a_f32, dtype=np.float32)).to(torch.bfloat16)


def _same_bits(a, b, what=""):
    """Two bf16 tensors: NaN in the same places, every other element bit-identical."""
    a, b = a.detach().cpu(), b.detach().cpu()
    an, bn = torch.isnan(a), torch.isnan(b)
    assert torch.equal(an, bn), f"{what}: NaN positions differ ({int(an.sum())} vs {int(bn.sum())})"
    bad = int((a.view(torch.int16)[~an] != b.view(torch.int16)[~bn]).sum())
    assert bad == 0, f"{what}: {bad} of {a.numel()} elements differ"


def _assert_dw(got, want_f32):
    got = got.detach().cpu().float().numpy()
    want = _rne(want_f32).float().numpy()
    mag = np.abs(want)
    ulp = np.where(mag > 0, np.exp2(np.floor(np.log2(np.where(mag > 0, mag, 1.0))) - 7), 0.0)
    err = np.abs(got - want)
    bound = ulp + DW_BAR * np.abs(want_f32).max()
    assert (err <= bound).all(), f"dW off by up to {(err / np.maximum(bound, 1e-30)).max():.2f} x the bound"


def _step(dZ, W, V, B, N, L, C, stride, offsets=None, dW=None, dV=None):
    """One backward step on device tensors (both gradients), outputs pre-filled with NaN."""
    from sparsefactorization_amd.chord import _launch_bwd
    dW = torch.empty_like(W) if dW is None else dW
    dV = torch.empty((B, N, C), dtype=W.dtype, device=W.device) if dV is None else dV
    dW.fill_(float("nan"))
    dV.fill_(float("nan"))
    _launch_bwd(dZ, W, V, dW, dV, B, N, L, C, stride, offsets)
    return dW, dV


def _check_three(gpu, B, N, L, C, seed, fused_knob, offsets=None, broadcast=False, shift=0, knobs=None):
    """The three assertions of the module docstring for one shape; returns the route's (dW, dV)."""
    W, dZ = _mk((B, N, L), seed), _mk((B, N, C), seed + 2)
    V = _mk((N, C) if broadcast else (B, N, C), seed + 1)
    Wt, Vt, dZt = _bt(W, gpu), _bt(V, gpu), _bt(dZ, gpu)
    dWbuf = None
    if shift:  # W and dW off their 16-byte boundary by `shift` elements
        Wt = torch.empty(B * N * L + shift, dtype=torch.bfloat16, device=gpu)[shift:].view(B, N, L).copy_(Wt)
        dWbuf = torch.empty(B * N * L + shift, dtype=torch.bfloat16, device=gpu)[shift:].view(B, N, L)
        assert Wt.data_ptr() % 16 != 0 and dWbuf.data_ptr() % 16 != 0
    stride = 0 if broadcast else N * C
    with tuning(bwd_fused=fused_knob, **(knobs or {})):
        dW1, dV1 = _step(dZt, Wt, Vt, B, N, L, C, stride, offsets, dW=dWbuf)
        dW1, dV1 = dW1.clone(), dV1.clone()
    with tuning(bwd_fused=0):
        dW0, dV0 = _step(dZt, Wt, Vt, B, N, L, C, stride, offsets, dW=dWbuf)
    dF, dVo = oc.spmul_bwd(dZ, W, np.ascontiguousarray(np.broadcast_to(V, (B, N, C))), offsets)
    _same_bits(dV1, _rne(dVo), "dV against the oracle")
    _assert_dw(dW1, dF)
    _same_bits(dV1, dV0, "dV against the two-kernel route")
    _same_bits(dW1, dW0, "dW against the two-kernel route")
    return dW1, dV1


ALIGNED = [
    (2, 512, 10, 8),     # two tiles, no far link
    (2, 1024, 11, 8),    # one far link
    (2, 1024, 12, 8),    # the duplicate link: 2^10 = 0 mod N
    (2, 256, 9, 32),
    (2, 128, 8, 64),
    (3, 64, 7, 128),
    (4, 16384, 15, 8),   # two fronts, five far links
    (2, 2048, 20, 16),   # the most links, W tile of more than one pass
]


@pytest.mark.parametrize("B,N,L,C", ALIGNED)
def test_aligned_instance(gpu, B, N, L, C):
    import sparsefactorization_amd as sfa
    with tuning(bwd_fused=2):
        name = sfa._lib.describe_bwd(B, N, L, C, elem_bytes=2)
    assert name.startswith(f"chord_bwd_fused_k<bf16,L={L},TG={C // 8},NT=256> TR={2048 // C} "), name
    _check_three(gpu, B, N, L, C, 100, 2)


def test_aligned_instance_far_offsets_that_are_no_powers_of_two(gpu):
    B, N, L, C = 2, 2048, 12, 8  # tiles of 256 rows: ten near links, two far ones at multiples of 256
    off = [0] + [1 << k for k in range(9)] + [768, 1280]
    _check_three(gpu, B, N, L, C, 110, 2, offsets=off)
    off[-1] = -512  # reduced mod N by the library: 1536
    _check_three(gpu, B, N, L, C, 113, 2, offsets=off)


def test_aligned_instance_broadcast_v(gpu):
    _check_three(gpu, 3, 1024, 11, 8, 120, 2, broadcast=True)
    _check_three(gpu, 2, 256, 9, 32, 123, 2, broadcast=True)


@pytest.mark.parametrize("knob,values", [("bwd_fronts", (1, 2, 4)), ("bwd_fused_wg_limit", (0, 2, 5))])
def test_knobs_do_not_change_bits(gpu, knob, values):
    import sparsefactorization_amd as sfa
    B, N, L, C = 4, 16384, 15, 8
    outs = []
    for v in values:
        with tuning(bwd_fused=2, **{knob: v}):
            assert "chord_bwd_fused_k<bf16" in sfa._lib.describe_bwd(B, N, L, C, elem_bytes=2)
        outs.append(_check_three(gpu, B, N, L, C, 130, 2, knobs={knob: v}))
    for dW, dV in outs[1:]:
        _same_bits(dW, outs[0][0], knob)
        _same_bits(dV, outs[0][1], knob)


@pytest.mark.parametrize("B,N,L,C,shift", [(2, 513, 10, 8, 0), (1, 4097, 13, 32, 0), (3, 2000, 12, 64, 0), (2, 1024, 11, 8, 1),
                                           (2, 1024, 11, 8, 3)])
def test_ragged_and_misaligned_on_the_automatic_route(gpu, B, N, L, C, shift):
    """Whichever kernel the automatic route takes (there is no bf16 edge instance: the two window kernels)."""
    _check_three(gpu, B, N, L, C, 140, 1, shift=shift)


def test_automatic_route_at_aligned_shapes(gpu):
    """bwd_fused = 1 is the measured gate: whatever it picks, the bits are those of the two kernels."""
    for B, N, L, C in ((2, 1024, 11, 8), (4, 16384, 15, 8), (2, 2048, 12, 64)):
        _check_three(gpu, B, N, L, C, 150, 1)


def test_nan_and_inf(gpu):
    B, N, L, C = 2, 1024, 11, 8
    W, V, dZ = _mk((B, N, L), 160), _mk((B, N, C), 161), _mk((B, N, C), 162)
    rng = np.random.default_rng(163)
    for arr, vals in ((dZ, [np.nan, np.inf, -np.inf]), (W, [np.nan, np.inf, 0.0]), (V, [np.inf, np.nan, -np.inf])):
        flat = arr.reshape(-1)
        flat[rng.choice(flat.size, 6, replace=False)] = np.resize(np.array(vals, dtype=np.float32), 6)
    Wt, Vt, dZt = _bt(W, gpu), _bt(V, gpu), _bt(dZ, gpu)
    with tuning(bwd_fused=2):
        dW1, dV1 = [t.clone() for t in _step(dZt, Wt, Vt, B, N, L, C, N * C)]
    with tuning(bwd_fused=0):
        dW0, dV0 = _step(dZt, Wt, Vt, B, N, L, C, N * C)
    assert bool(torch.isnan(dV0).any()) and bool(torch.isnan(dW0).any())
    _same_bits(dV1, dV0, "dV")
    _same_bits(dW1, dW0, "dW")
    _same_bits(dV1, _rne(oc.spmul_bwd(dZ, W, V)[1]), "dV against the oracle")


@pytest.mark.parametrize("B,N,L,C", [(2, 1024, 11, 8), (2, 256, 9, 32), (3, 64, 7, 128), (2, 2048, 20, 16)])
def test_after_nan_in_every_lds(gpu, B, N, L, C):
    """Right after launches that leave NaN patterns in the LDS of every CU (tests/test_gpu_stale_lds.py): the surplus lanes of
    the W tiles' partial pass land in a pad nobody reads, and nothing else is read unstaged."""
    from test_gpu_stale_lds import _poison
    W, V, dZ = _mk((B, N, L), 170), _mk((B, N, C), 171), _mk((B, N, C), 172)
    Wt, Vt, dZt = _bt(W, gpu), _bt(V, gpu), _bt(dZ, gpu)
    with tuning(bwd_fused=0):
        dW0, dV0 = _step(dZt, Wt, Vt, B, N, L, C, N * C)
    with tuning(bwd_fused=2):
        dWb, dVb = torch.empty_like(Wt), torch.empty_like(Vt)
        _poison(gpu)
        dW1, dV1 = _step(dZt, Wt, Vt, B, N, L, C, N * C, dW=dWb, dV=dVb)
    _same_bits(dV1, dV0, "dV")
    _same_bits(dW1, dW0, "dW")
    _same_bits(dV1, _rne(oc.spmul_bwd(dZ, W, V)[1]), "dV against the oracle")


# ----------------------------------------------------------------------------------------------------
# the chain entry
# ----------------------------------------------------------------------------------------------------
def _chain_operands(gpu, B, N, L, C, M, seed):
    Ws = [_bt(_mk((B, N, L), seed + m, 0.3), gpu) for m in range(M)]
    return Ws, _bt(_mk((B, N, C), seed + 50), gpu), _bt(_mk((B, N, C), seed + 51), gpu)


def _autograd_chain(Ws, V0, dOut, residual):
    import sparsefactorization_amd as sfa
    ws = [w.detach().clone().requires_grad_(True) for w in Ws]
    v0 = V0.detach().clone().requires_grad_(True)
    sfa.chord_chain(ws, v0, residual).backward(dOut)
    return [v0.grad, *[w.grad for w in ws]]


def _entry_chain(gpu, Ws, V0, dOut, residual, B, N, L, C):
    """psf_chord_chain_bwd_bf16 called directly; returns (rc, [dV0, dW_0 .. dW_{M-1}])."""
    from sparsefactorization_amd import _lib, chord
    M = len(Ws)
    _, Wc, outs, _ = chord._chain_forward_raw(V0, residual, None, Ws, True)
    tab = lambda ts: (ctypes.c_void_p * M)(*[t.data_ptr() for t in ts])  # noqa: E731
    dWs = [torch.full_like(w, float("nan")) for w in Wc]
    dXs = [torch.full_like(V0, float("nan")) for _ in range(M)]
    dV0 = torch.full_like(V0, float("nan"))
    with torch.cuda.device(gpu):
        rc = _lib.load().psf_chord_chain_bwd_bf16(dOut.data_ptr(), tab(Wc), V0.data_ptr(), tab([V0, *outs[:-1]]), tab(dWs), dV0.data_ptr(),
                                                  tab(dXs), M, 1 if residual else 0, B, N, L, C, None, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    return rc, [dV0, *dWs]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("M", [3, 14])
@pytest.mark.parametrize("B,N,L,C", [(2, 1024, 11, 8), (2, 513, 10, 16), (40, 128, 8, 8)])
def test_chain_entry_matches_the_per_step_loop(gpu, B, N, L, C, M, residual):
    from sparsefactorization_amd import _lib
    Ws, V0, dOut = _chain_operands(gpu, B, N, L, C, M, 200)
    with tuning(chain_bwd_fused=0):  # the entry returns PSF_E_UNSUPPORTED: chord.py's own loop
        rc, _ = _entry_chain(gpu, Ws, V0, dOut, residual, B, N, L, C)
        assert rc == _lib.PSF_E_UNSUPPORTED
        loop = _autograd_chain(Ws, V0, dOut, residual)
    rc, direct = _entry_chain(gpu, Ws, V0, dOut, residual, B, N, L, C)
    assert rc == 0, _lib.last_error()
    through = _autograd_chain(Ws, V0, dOut, residual)  # chord_chain(...).backward through the entry
    assert not any(bool(torch.isnan(t).any()) for t in loop)
    for i, (a, b, c) in enumerate(zip(loop, direct, through)):
        _same_bits(b, a, f"entry, tensor {i}")
        _same_bits(c, a, f"autograd, tensor {i}")


def test_chain_backward_takes_the_entry(gpu, monkeypatch):
    """chord_chain(...).backward in bf16 calls the entry once and not the per-step entry."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    calls = {"chain": 0}
    real = lib.psf_chord_chain_bwd_bf16

    def spy(*a):
        calls["chain"] += 1
        return real(*a)

    Ws, V0, dOut = _chain_operands(gpu, 2, 1024, 11, 8, 4, 230)
    monkeypatch.setattr(lib, "psf_chord_chain_bwd_bf16", spy)
    monkeypatch.setattr(lib, "psf_chord_spmm_bwd_bf16", lambda *a: pytest.fail("the per-step loop ran"))
    grads = _autograd_chain(Ws, V0, dOut, True)
    assert calls["chain"] == 1 and all(g is not None and g.dtype == torch.bfloat16 for g in grads)


def test_chain_falls_back_when_the_residual_sum_is_outside_its_limits(gpu):
    """B N C % 8 != 0 with the residual: the entry declines, the loop and its f32 sum run — same gradients as float64 to bf16's bar."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib
    B, N, L, C, M = 1, 101, 7, 3, 4
    Ws, V0, dOut = _chain_operands(gpu, B, N, L, C, M, 240)
    rc, _ = _entry_chain(gpu, Ws, V0, dOut, True, B, N, L, C)
    assert rc == _lib.PSF_E_UNSUPPORTED
    got = _autograd_chain(Ws, V0, dOut, True)
    wd = [w.double().requires_grad_(True) for w in Ws]
    vd = V0.double().requires_grad_(True)
    sfa.chord_chain(wd, vd, True).backward(dOut.double())
    for g, r in zip(got, [vd.grad, *[w.grad for w in wd]]):
        assert g.dtype == torch.bfloat16
        assert float((g.double() - r).abs().max()) <= 5e-2 * float(r.abs().max())  # CHAIN_GRAD_BOUND of tests/test_gpu_bf16.py
    # without the residual there is no sum: the entry takes odd sizes too
    rc, direct = _entry_chain(gpu, Ws, V0, dOut, False, B, N, L, C)
    assert rc == 0
    with tuning(chain_bwd_fused=0):
        loop = _autograd_chain(Ws, V0, dOut, False)
    for a, b in zip(loop, direct):
        _same_bits(b, a)
