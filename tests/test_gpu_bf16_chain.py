"""The one-launch LDS-resident forward chain in bf16 (csrc/fwd_chain_lds_bf16.h): chord_chain_lds_k<bf16> and
chord_chain_rows_k<bf16> against the iterated per-step reference, bit for bit.

Expected values as in test_gpu_bf16.py: every step is bf16_rne(oracle f32 step on the upcast inputs [+ V0]); results are
compared as int16 bits. Every case first asserts, through describe_chain_fwd(..., elem_bytes=2) under the knobs it sets, that
the kernel it means to test is the one that runs, asserts that the expected values are finite (no case passes as NaN == NaN;
NaN and Inf have a case of their own), and also runs the per-step route (chain_fused = 0) and asserts equal bits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import chord_oracle as oc
from sparsefactorization_amd._lib import tuning

pytestmark = pytest.mark.gpu


def _mk(shape, seed, scale=1.0):
    """A bf16-representable f32 array (so the oracle sees exactly the kernel's inputs)."""
    a = np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * scale
    return torch.from_numpy(a).to(torch.bfloat16).float().numpy()


def _bt(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(dev)


def _rne(a_f32):
    return torch.from_numpy(np.ascontiguousarray(a_f32, dtype=np.float32)).to(torch.bfloat16)


def _chain_ref_steps(Ws, V0, residual, offsets=None):
    """Every step of the iterated per-step reference, as bf16 tensors: X_{m+1} = bf16_rne(oracle_f32(W_m, X_m) [+ V0])."""
    X, steps = V0, []
    for W in Ws:
        out = oc.spmul_fwd(W, X, offsets)
        if residual:
            out = out + V0  # f32 add; rounded once below
        steps.append(_rne(out))
        X = steps[-1].float().numpy()
    return steps


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _assert_finite(steps):
    for m, s in enumerate(steps):
        assert bool(torch.isfinite(s.float()).all()), f"expected step {m} is not finite: the case would prove nothing"


def _assert_same(got, want, what):
    """Equal bits; where NaN is expected, NaN (any payload) in the same places."""
    got, want = got.detach().cpu(), want.cpu()
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(wn.sum())})"
    bad = int((_bits(got)[~gn] != _bits(want)[~wn]).sum())
    assert bad == 0, f"{what}: {bad} elements differ"


def _run_both_modes(Wt, V0t, residual, want, what, offsets=None):
    """Ping-pong storage (no_grad) and every step kept; each stored step is checked, not only the last."""
    import sparsefactorization_amd as sfa
    M = len(Wt)
    with torch.no_grad():
        last = sfa.chord_chain(Wt, V0t, residual, offsets)
    assert last.dtype == torch.bfloat16
    _assert_same(last, want[-1], f"{what}, last kept")
    Wg = [w.detach().requires_grad_(True) for w in Wt]
    out = sfa.chord_chain(Wg, V0t, residual, offsets)
    saved = list(out.grad_fn.saved_tensors)[1 + M:2 * M]
    assert len(saved) == M - 1
    for m, t in enumerate(saved):
        _assert_same(t, want[m], f"{what}, stored step {m}")
    _assert_same(out, want[-1], f"{what}, every step kept")
    return last, [*saved, out.detach()]


def _check_case(gpu, B, N, M, L, C, residual, cc, kernel, seed=200):
    from sparsefactorization_amd import _lib
    Ws = [_mk((B, N, L), seed + 1 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), seed)
    want = _chain_ref_steps(Ws, V0, residual)
    _assert_finite(want)
    Wt, V0t = [_bt(w, gpu) for w in Ws], _bt(V0, gpu)
    with tuning(chain_fused=2, chain_cc=cc):
        desc = _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2)
        assert desc.startswith(kernel), desc
        one = _run_both_modes(Wt, V0t, residual, want, kernel)
    with tuning(chain_fused=0):
        assert "chain" not in _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2)
        steps = _run_both_modes(Wt, V0t, residual, want, "per-step route")
    assert torch.equal(_bits(one[0]), _bits(steps[0]))
    for a, b in zip(one[1], steps[1]):
        assert torch.equal(_bits(a), _bits(b))


LDS_CASES = [  # (B, N, M, L, C, residual, chain_cc, CC, R): chord_chain_lds_k<bf16>, every (CC, R) instance family
    (3, 200, 4, 9, 8, True, 0, 1, 1), (2, 128, 7, 8, 16, False, 0, 2, 1), (40, 128, 3, 8, 8, True, 0, 1, 1),
    (2, 1101, 7, 11, 8, True, 0, 1, 2), (2, 1000, 5, 12, 32, False, 0, 2, 2), (2, 2048, 3, 12, 8, True, 0, 1, 2),
    (2, 1024, 10, 11, 32, True, 0, 2, 2), (2, 300, 3, 2, 24, False, 0, 2, 2), (2, 1500, 3, 20, 8, True, 0, 1, 2),
    (2, 777, 4, 9, 24, True, 1, 1, 2), (2, 513, 3, 15, 136, False, 0, 2, 2),
    (2, 1025, 4, 12, 32, True, 0, 2, 3), (2, 2049, 3, 15, 8, True, 0, 1, 3), (1, 1056, 2, 18, 16, False, 0, 2, 3),
    (2, 2112, 3, 9, 8, False, 0, 1, 3), (3, 1025, 2, 11, 8, True, 0, 1, 2),
]


@pytest.mark.parametrize("B,N,M,L,C,residual,cc,CC,R", LDS_CASES)
def test_lds_kernel_bit_exact(gpu, B, N, M, L, C, residual, cc, CC, R):
    _check_case(gpu, B, N, M, L, C, residual, cc, f"chord_chain_lds_k<bf16,L={L},CC={CC},R={R}>")


ROWS2_CASES = [  # (B, N, M, L, C, residual): chord_chain_rows_k<bf16, G = 2>, 1057 <= N <= 2048; C = 24, 40: odd group counts
    (2, 2000, 11, 12, 128, True), (2, 1057, 4, 11, 16, False), (2, 2001, 3, 12, 24, True), (1, 1500, 4, 20, 24, True),
    (2, 1999, 3, 15, 40, True), (2, 2048, 3, 9, 16, False), (2, 2047, 3, 2, 16, False),
]


@pytest.mark.parametrize("B,N,M,L,C,residual", ROWS2_CASES)
def test_rows_kernel_two_groups_bit_exact(gpu, B, N, M, L, C, residual):
    _check_case(gpu, B, N, M, L, C, residual, 2, f"chord_chain_rows_k<bf16,L={L},G=2,R=2>", seed=300)


LONG_CASES = [  # (B, N, M, L, C, residual): chord_chain_rows_k<bf16, G = 1>, 2113 <= N <= 4160
    (2, 4097, 12, 14, 32, True), (2, 4160, 3, 13, 8, True), (1, 2113, 3, 12, 24, True), (2, 3000, 3, 20, 8, False),
    (1, 4097, 2, 15, 16, False), (2, 2500, 3, 2, 8, True), (1, 2200, 3, 9, 8, False),
]


@pytest.mark.parametrize("B,N,M,L,C,residual", LONG_CASES)
def test_rows_kernel_long_rows_bit_exact(gpu, B, N, M, L, C, residual):
    _check_case(gpu, B, N, M, L, C, residual, 2, f"chord_chain_rows_k<bf16,L={L},G=1,R=5>", seed=400)


@pytest.mark.parametrize("B,N,M,L,C,cc,kernel", [
    (2, 1101, 5, 11, 8, 0, "chord_chain_lds_k<bf16"), (2, 2000, 4, 12, 32, 2, "chord_chain_rows_k<bf16,L=12,G=2"),
    (1, 4097, 3, 13, 8, 2, "chord_chain_rows_k<bf16,L=13,G=1")])
@pytest.mark.parametrize("residual", [False, True])
def test_nan_and_inf_propagate_like_the_per_step_route(gpu, B, N, M, L, C, cc, kernel, residual):
    from sparsefactorization_amd import _lib
    Ws = [_mk((B, N, L), 501 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 500)
    rng = np.random.default_rng(510)
    for arr, vals in ((V0, [np.nan, np.inf, -np.inf]), (Ws[1], [np.nan, np.inf, 0.0, -np.inf])):
        flat = arr.reshape(-1)
        flat[rng.choice(flat.size, 8, replace=False)] = np.resize(np.array(vals, dtype=np.float32), 8)
    want = _chain_ref_steps(Ws, V0, residual)
    assert bool(torch.isnan(want[-1]).any()) and not bool(torch.isnan(want[-1]).all())
    Wt, V0t = [_bt(w, gpu) for w in Ws], _bt(V0, gpu)
    with tuning(chain_fused=2, chain_cc=cc):
        assert _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2).startswith(kernel)
        _run_both_modes(Wt, V0t, residual, want, kernel)
    with tuning(chain_fused=0):
        _run_both_modes(Wt, V0t, residual, want, "per-step route")


@pytest.mark.parametrize("B,N,M,L,C,cc,kernel", [
    (3, 256, 4, 9, 8, 0, "chord_chain_lds_k<bf16"), (2, 1024, 4, 11, 1024, 0, "chord_chain_lds_k<bf16,L=11,CC=2,R=2>"),
    (2, 1500, 3, 12, 48, 2, "chord_chain_rows_k<bf16,L=12,G=2"), (2, 2500, 3, 13, 16, 2, "chord_chain_rows_k<bf16,L=13,G=1")])
def test_broadcast_v0(gpu, B, N, M, L, C, cc, kernel):
    """The attention map's start: V0 = eye(N, C) as [N, C], shared by the batch."""
    from sparsefactorization_amd import _lib
    Ws = [_mk((B, N, L), 601 + m, 0.3) for m in range(M)]
    E = np.eye(N, C, dtype=np.float32)
    want = _chain_ref_steps(Ws, E, False)
    _assert_finite(want)
    Wt, Et = [_bt(w, gpu) for w in Ws], _bt(E, gpu)
    with tuning(chain_fused=2, chain_cc=cc):
        assert _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2).startswith(kernel)
        one = _run_both_modes(Wt, Et, False, want, kernel)
    with tuning(chain_fused=0):
        steps = _run_both_modes(Wt, Et, False, want, "per-step route")
    assert torch.equal(_bits(one[0]), _bits(steps[0]))


@pytest.mark.parametrize("B,N,M,C,cc,off,kernel", [
    (2, 500, 4, 8, 0, [3, 0, 499, 1000, -7, 250], "chord_chain_lds_k<bf16,L=6"),
    (2, 2000, 3, 16, 2, [0, 1, -1, 1999, 4000, -2500, 77], "chord_chain_rows_k<bf16,L=7,G=2"),
    (1, 3001, 3, 8, 2, [-3000, 5, 0, 1500, 1 << 20], "chord_chain_rows_k<bf16,L=5,G=1")])
def test_explicit_and_negative_offsets(gpu, B, N, M, C, cc, off, kernel):
    from sparsefactorization_amd import _lib
    L = len(off)
    Ws = [_mk((B, N, L), 701 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 700)
    want = _chain_ref_steps(Ws, V0, True, off)
    _assert_finite(want)
    Wt, V0t = [_bt(w, gpu) for w in Ws], _bt(V0, gpu)
    with tuning(chain_fused=2, chain_cc=cc):
        assert _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2).startswith(kernel)
        one = _run_both_modes(Wt, V0t, True, want, kernel, off)
    with tuning(chain_fused=0):
        steps = _run_both_modes(Wt, V0t, True, want, "per-step route", off)
    assert torch.equal(_bits(one[0]), _bits(steps[0]))


def _shifted(t, shift):
    """A copy of t that starts `shift` elements behind an allocation's (>= 256-byte aligned) start."""
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=t.device)
    v = buf[shift:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("B,N,M,L,C,cc", [(2, 1101, 4, 11, 8, 0), (2, 1101, 4, 12, 8, 0), (2, 2000, 3, 15, 32, 2),
                                          (2, 2000, 3, 12, 32, 2), (1, 4097, 3, 13, 8, 2)])
@pytest.mark.parametrize("shift", [1, 3])
def test_w_at_an_odd_two_byte_offset(gpu, B, N, M, L, C, cc, shift):
    """W_m two bytes off a dword boundary: odd L stays on the one launch (the row parity flips), even L takes the per-step
    kernels. Either route; the bits are the reference's."""
    Ws = [_mk((B, N, L), 801 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 800)
    want = _chain_ref_steps(Ws, V0, True)
    _assert_finite(want)
    Wt = [_shifted(_bt(w, gpu), shift) for w in Ws]
    assert all(w.data_ptr() % 4 == 2 for w in Wt)
    Wt[1] = _bt(Ws[1], gpu)  # (one step's W aligned: the parity is per step)
    with tuning(chain_fused=2, chain_cc=cc):
        _run_both_modes(Wt, _bt(V0, gpu), True, want, f"W shifted by {shift}")


@pytest.mark.parametrize("B,N,M,L,C,cc", [(2, 1101, 4, 11, 8, 0), (2, 2000, 3, 12, 32, 2)])
def test_v0_off_its_16_byte_boundary_takes_the_per_step_route(gpu, B, N, M, L, C, cc):
    Ws = [_mk((B, N, L), 851 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 850)
    want = _chain_ref_steps(Ws, V0, True)
    _assert_finite(want)
    V0t = _shifted(_bt(V0, gpu), 1)
    assert V0t.data_ptr() % 16 == 2
    with tuning(chain_fused=2, chain_cc=cc):
        _run_both_modes([_bt(w, gpu) for w in Ws], V0t, True, want, "V0 shifted")


@pytest.mark.parametrize("scale", [2.0 ** 60, 2.0 ** -60])
@pytest.mark.parametrize("B,N,L,C,cc,kernel", [(2, 2048, 12, 8, 0, "chord_chain_lds_k<bf16"),
                                               (2, 2048, 12, 16, 2, "chord_chain_rows_k<bf16")])
def test_edges_of_the_product_range(gpu, scale, B, N, L, C, cc, kernel):
    """Products near 2^120 and 2^-120 (normal f32 numbers): the fused multiply-add gives the bits of the separately rounded
    product and sum. Step 0 multiplies scale x scale; step 1 multiplies back by 1 / scale, so everything stays finite."""
    from sparsefactorization_amd import _lib
    pos = lambda s, shape, sc: _rne(sc * (1.0 + np.random.default_rng(s).random(shape, dtype=np.float32))).float().numpy()  # noqa: E731
    Ws = [pos(901, (B, N, L), scale), pos(902, (B, N, L), 1.0 / scale)]
    V0 = pos(900, (B, N, C), scale)
    want = _chain_ref_steps(Ws, V0, False)
    _assert_finite(want)
    with tuning(chain_fused=2, chain_cc=cc):
        assert _lib.describe_chain_fwd(B, N, L, C, 2, elem_bytes=2).startswith(kernel)
        _run_both_modes([_bt(w, gpu) for w in Ws], _bt(V0, gpu), False, want, f"scale={scale}")


def test_two_identical_runs_give_identical_bits(gpu):
    import sparsefactorization_amd as sfa
    for (B, N, M, L, C, cc) in [(4, 1024, 10, 11, 32, 0), (4, 2000, 6, 12, 64, 2), (2, 4097, 5, 14, 16, 2)]:
        Wt = [_bt(_mk((B, N, L), 951 + m, 0.3), gpu) for m in range(M)]
        V0t = _bt(_mk((B, N, C), 950), gpu)
        with tuning(chain_fused=2, chain_cc=cc), torch.no_grad():
            a = sfa.chord_chain(Wt, V0t, True).clone()
            b = sfa.chord_chain(Wt, V0t, True).clone()
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("B,N,M,L,C", [(32, 2000, 3, 12, 128), (32, 2048, 3, 12, 64), (32, 1024, 3, 11, 32), (32, 4097, 3, 14, 32),
                                       (16, 4097, 2, 14, 32), (40, 1024, 3, 11, 8)])
def test_default_route_on_the_lra_shapes(gpu, B, N, M, L, C):
    """chain_fused = 1 at the LRA launch sizes: whatever the measured gate decides, the bits are the reference's."""
    Ws = [_mk((B, N, L), 1001 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 1000)
    want = _chain_ref_steps(Ws, V0, True)
    _assert_finite(want)
    with tuning(chain_fused=1, chain_cc=0):
        _run_both_modes([_bt(w, gpu) for w in Ws], _bt(V0, gpu), True, want, "default route")


@pytest.mark.parametrize("B,N,M,L,C,cc,kernel", [
    (2, 1101, 3, 11, 8, 0, "chord_chain_lds_k<bf16,L=11,CC=1,R=2>"), (2, 1025, 3, 12, 16, 0, "chord_chain_lds_k<bf16,L=12,CC=2,R=3>"),
    (2, 2001, 3, 12, 24, 2, "chord_chain_rows_k<bf16,L=12,G=2,R=2>"), (1, 4097, 3, 13, 8, 2, "chord_chain_rows_k<bf16,L=13,G=1,R=5>")])
def test_nothing_outside_the_results_is_written(gpu, B, N, M, L, C, cc, kernel):
    """Every step's result sits inside a larger buffer filled with a sentinel: N is not a multiple of the rows-per-thread
    tiling, and the rows / channel groups a workgroup clamps must not be stored."""
    from sparsefactorization_amd import _lib
    from sparsefactorization_amd.chord import _stream_ptr
    Ws = [_mk((B, N, L), 1101 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 1100)
    want = _chain_ref_steps(Ws, V0, True)
    _assert_finite(want)
    Wt, V0t = [_bt(w, gpu) for w in Ws], _bt(V0, gpu)
    GUARD, n = 4096, B * N * C  # elements; both multiples of 8, so every result stays 16-byte aligned
    SENTINEL = 0x7B7B  # as int16 bits
    arena = torch.full((M * (n + GUARD) + GUARD,), SENTINEL, dtype=torch.int16, device=gpu)
    outs = [arena[GUARD + m * (n + GUARD):GUARD + m * (n + GUARD) + n] for m in range(M)]
    assert all(o.data_ptr() % 16 == 0 for o in outs)
    lib = _lib.load()
    w_tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Wt])
    o_tab = (ctypes.c_void_p * M)(*[o.data_ptr() for o in outs])
    with tuning(chain_fused=2, chain_cc=cc):
        assert _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2).startswith(kernel)
        with torch.cuda.device(gpu):
            rc = lib.psf_chord_chain_fwd_bf16(w_tab, V0t.data_ptr(), o_tab, M, 1, B, N, L, C, N * C, None, _stream_ptr(gpu))
        _lib.check(rc, "psf_chord_chain_fwd_bf16")
        torch.cuda.synchronize()
    host = arena.cpu()
    inside = torch.zeros(host.numel(), dtype=torch.bool)
    for m in range(M):
        lo = GUARD + m * (n + GUARD)
        inside[lo:lo + n] = True
        assert torch.equal(host[lo:lo + n].view(B, N, C), _bits(want[m])), f"step {m}"
    assert bool((host[~inside] == SENTINEL).all()), "a write outside [B, N, C]"
