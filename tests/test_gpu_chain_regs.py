"""GPU: psf_chord_chain_last_f32 (csrc/fwd_chain_regs.h: the last result of a long f32 chain in one launch, X in registers, W
streamed through LDS) against the per-step route (knob chain_fused = 0) and the CPU oracle, bit for bit.

N = 16384, L = 15: the one compiled shape. The grids are B * C / 2 <= 54 workgroups, so a case takes a second or two, most of it
the oracle. What a case can catch: C = 4 / 8 / 12 are one, two and an odd number of 16-byte channel groups (two to six channel
pairs, each a workgroup); B = 9 puts two sequences on one XCD under the XCD-aware map; M = 1, 2, 3, 14 are both parities of the
X_m / X_{m+1} register swap and a chain whose W ring runs across many step boundaries. One-hot V0 rows at 0, T - 1, T and N - 1
(T = 512 rows per block) move under a wrong link, a wrong block carry of the exchange ring or a wrong wrap mod N; a W that is
zero except for one link isolates that link. The output sits between canary rows; W, V0 and the canaries must be what they
were."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import chord_oracle as oc

pytestmark = pytest.mark.gpu

N, L, T = 16384, 15, 512
CANARY_ROWS = 8
CANARY = -12345.5


@pytest.fixture(scope="module")
def index():
    rows, cols = oc.chord_indices(N, L)
    return np.stack([rows, cols])


def _rand(shape, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)).astype(np.float32)


def _stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _guarded_out(B, C, gpu):
    """[B, N, C] as a view between CANARY_ROWS canary rows on either side (the view stays 16-byte aligned: C % 4 == 0)."""
    buf = torch.full(((B * N + 2 * CANARY_ROWS) * C,), CANARY, device=gpu)
    lo = CANARY_ROWS * C
    return buf, buf[lo:lo + B * N * C].view(B, N, C)


def _canaries_intact(buf, B, C):
    lo = CANARY_ROWS * C
    return bool((buf[:lo] == CANARY).all()) and bool((buf[lo + B * N * C:] == CANARY).all())


def _last(lib, Wts, V0t, out, res, B, C, gpu):
    """The new entry on device tensors; V0t [B, N, C] or [N, C] (broadcast)."""
    M = len(Wts)
    tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Wts])
    stride = 0 if V0t.dim() == 2 else N * C
    return lib.psf_chord_chain_last_f32(tab, V0t.data_ptr(), out.data_ptr(), M, 1 if res else 0, B, N, L, C, stride, None, _stream(gpu))


def _per_step(lib, Wts, V0t, res, B, C, gpu):
    """The parent's route: psf_chord_chain_fwd_f32 under chain_fused = 0, two buffers taking turns; returns X_M."""
    from sparsefactorization_amd import _lib
    M = len(Wts)
    bufs = [torch.empty((B, N, C), device=gpu) for _ in range(min(M, 2))]
    outs = [bufs[m % len(bufs)] for m in range(M)]
    vp = ctypes.c_void_p
    stride = 0 if V0t.dim() == 2 else N * C
    with _lib.tuning(chain_fused=0):
        rc = lib.psf_chord_chain_fwd_f32((vp * M)(*[w.data_ptr() for w in Wts]), V0t.data_ptr(), (vp * M)(*[o.data_ptr() for o in outs]),
                                         M, 1 if res else 0, B, N, L, C, stride, None, _stream(gpu))
    _lib.check(rc, "psf_chord_chain_fwd_f32")
    return outs[-1]


def _check(gpu, index, W, V0, res, broadcast=False):
    """W [M, B, N, L], V0 [B, N, C] ([N, C] with broadcast): the entry's X_M == the per-step route's == the oracle's, bit for
    bit; operands and canaries untouched. Returns the entry's result (a CPU array)."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    M, B = W.shape[:2]
    C = V0.shape[-1]
    Wts = [torch.from_numpy(W[m]).to(gpu) for m in range(M)]
    V0t = torch.from_numpy(V0).to(gpu)
    keep = [w.clone() for w in Wts], V0t.clone()
    buf, out = _guarded_out(B, C, gpu)
    _lib.check(_last(lib, Wts, V0t, out, res, B, C, gpu), "psf_chord_chain_last_f32")
    torch.cuda.synchronize(gpu)
    assert _canaries_intact(buf, B, C)
    assert all(torch.equal(a, b) for a, b in zip(Wts, keep[0])) and torch.equal(V0t, keep[1])
    assert torch.equal(out, _per_step(lib, Wts, V0t, res, B, C, gpu))
    full = np.ascontiguousarray(np.broadcast_to(V0, (B, N, C))) if broadcast else V0
    got = out.cpu().numpy()
    assert np.array_equal(got, oc.chain(index, W, full, res)[-1])
    return got


# every value of C, B, M and the residual; every pair (C, B); both parities of M with and without the residual
CASES = [(4, 1, 1, True), (4, 3, 2, False), (4, 9, 3, True), (8, 1, 14, True), (8, 3, 3, False), (8, 9, 2, True),
         (12, 1, 2, False), (12, 3, 14, True), (12, 9, 1, False), (8, 3, 1, True), (4, 3, 14, False), (12, 9, 3, True)]


@pytest.mark.parametrize("C,B,M,res", CASES)
def test_last_result_equals_per_step_route_and_oracle(gpu, index, C, B, M, res):
    _check(gpu, index, _rand((M, B, N, L), 100 + 7 * M + B, 0.3), _rand((B, N, C), 200 + C), res)


@pytest.mark.parametrize("M", [1, 2])
def test_broadcast_v0_without_residual(gpu, index, M):
    _check(gpu, index, _rand((M, 3, N, L), 31 + M, 0.3), _rand((N, 8), 32), False, broadcast=True)


@pytest.mark.parametrize("res", [False, True])
def test_one_hot_rows_at_block_and_sequence_edges(gpu, index, res):
    """V0 is zero but for rows 0, T - 1, T and N - 1 (distinct values per row and channel): three steps spread them over
    8^3 positions at most, so a wrong link, block carry or wrap puts a value where the oracle has none."""
    B, C, M = 3, 4, 3
    V0 = np.zeros((B, N, C), dtype=np.float32)
    for i, p in enumerate((0, T - 1, T, N - 1)):
        V0[:, p, :] = 1.0 + i + 0.25 * np.arange(C, dtype=np.float32)[None, :] + 0.125 * np.arange(B, dtype=np.float32)[:, None]
    got = _check(gpu, index, _rand((M, B, N, L), 41, 0.5), V0, res)
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("k", range(L))
def test_one_link_at_a_time(gpu, index, k):
    """W is zero except link k (offset 0 for k = 0, else 2^(k-1)): X_2[p] = w1[p] w0[p + off] V0[p + 2 off]."""
    B, C, M = 1, 4, 2
    W = np.zeros((M, B, N, L), dtype=np.float32)
    W[..., k] = _rand((M, B, N), 50 + k, 0.7)
    _check(gpu, index, W, _rand((B, N, C), 51), False)


def test_repeat_gives_equal_bits(gpu):
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    B, C, M = 9, 8, 3
    Wts = [torch.from_numpy(_rand((B, N, L), 60 + m, 0.3)).to(gpu) for m in range(M)]
    V0t = torch.from_numpy(_rand((B, N, C), 61)).to(gpu)
    outs = [torch.empty((B, N, C), device=gpu) for _ in range(2)]
    for o in outs:
        _lib.check(_last(lib, Wts, V0t, o, True, B, C, gpu), "psf_chord_chain_last_f32")
    assert torch.equal(outs[0], outs[1])


def test_chord_chain_no_grad_equals_the_differentiable_call(gpu, monkeypatch):
    """Python level, chain_fused = 2 (the route on request): under no_grad chord_chain takes the new entry — counted — and returns
    the bits of the same call with inputs that require gradients (every step kept: psf_chord_chain_fwd_f32)."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    calls = []
    real = lib.psf_chord_chain_last_f32
    monkeypatch.setattr(lib, "psf_chord_chain_last_f32", lambda *a: calls.append(1) or real(*a), raising=False)
    B, C, M = 3, 8, 3
    Ws = [torch.from_numpy(_rand((B, N, L), 70 + m, 0.3)).to(gpu) for m in range(M)]
    V0 = torch.from_numpy(_rand((B, N, C), 71)).to(gpu)
    with _lib.tuning(chain_fused=2):
        with torch.no_grad():
            a = sfa.chord_chain(Ws, V0, True)
        assert len(calls) == 1
        b = sfa.chord_chain([w.clone().requires_grad_(True) for w in Ws], V0.clone().requires_grad_(True), True)
        assert len(calls) == 1
    assert torch.equal(a, b.detach())
