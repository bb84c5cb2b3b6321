"""GPU: the fused bf16 producer forward (psf_mlp_fwd_bf16, csrc/mlp_fwd_bf16.hip) against the float64 reference of its
three-rounding contract (tests/mlp_bf16_ref.py): known answers bit for bit, random inputs inside the envelope with at most
1 % of the elements differing, guard bands, token locality, stale state, graph capture and the Python route.

(Sorted behind tests/test_gpu_coresidence.py, as the suite's other graph tests are: see tests/test_gpu_graph_bf16_bwd.py.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mlp_bf16_ref as R
from conftest import rel_inf

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B  # a bf16 pattern no case produces wholesale (2.4e+16)
IDS = [f"{T}x{E}x{len(layers)}" for T, E, layers in R.SHAPES]


# ---------------------------------------------------------------- plumbing
def dev_bf16(v, gpu):
    """bf16-valued float64 array -> bf16 device tensor (exact)."""
    R.to_bits(v)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).to(gpu)


def bits(t) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def values(t) -> np.ndarray:
    return t.float().cpu().numpy().astype(np.float64)


def dev_params(params, gpu):
    return [dev_bf16(p, gpu) for ps in params for p in ps]


def workspace_bytes(E, flat):
    from sparsefactorization_amd import _lib
    K = len(flat) // 4
    h = (ctypes.c_int32 * K)(*[A.shape[0] for A in flat[0::4]])
    O = (ctypes.c_int32 * K)(*[B.shape[0] for B in flat[2::4]])
    n = _lib.load().psf_mlp_fwd_bf16_workspace(E, K, h, O)
    assert n > 0
    return n, h, O


def raw(x2, flat, ys=None, ws=None):
    """One call of the raw entry on [T, E] bf16 ``x2`` and the flat parameter list (A0, a0, B0, b0, A1, ...)."""
    from sparsefactorization_amd import _lib
    from sparsefactorization_amd.fused_mlp import _ptrs
    lib = _lib.load()
    T, E = x2.shape
    K = len(flat) // 4
    n, h, O = workspace_bytes(E, flat)
    if ys is None:
        ys = [torch.empty((T, B.shape[0]), dtype=torch.bfloat16, device=x2.device) for B in flat[2::4]]
    if ws is None:
        ws = torch.zeros(n, dtype=torch.uint8, device=x2.device)
    assert ws.numel() >= n
    rc = lib.psf_mlp_fwd_bf16(x2.data_ptr(), T, E, K, _ptrs(flat[0::4]), _ptrs(flat[1::4]), _ptrs(flat[2::4]), _ptrs(flat[3::4]),
                              h, O, _ptrs(ys), ws.data_ptr(), ws.numel(), _lib.stream_ptr(x2.device))
    _lib.check(rc, "psf_mlp_fwd_bf16")
    return ys


@functools.lru_cache(maxsize=None)
def known(kind, idx):
    """The construction of shape ``idx`` and its answers' bits (computed once, shared, never modified)."""
    T, E, layers = R.SHAPES[idx]
    X, params, answers = R.KINDS[kind][0](T, E, layers, R.seed_of(T, E))
    return X, params, [R.plus_zero(R.to_bits(y)) for y in answers]


@functools.lru_cache(maxsize=None)
def random_case(T, E, layers, scale=1.0):
    """Random inputs and their reference (y, envelope) per MLP, computed once on the CPU from the bf16 values."""
    X = R.random_x(T, E, R.seed_of(T, E))
    params = R.random_params(E, list(layers), seed=T + 7 * E, scale=scale)
    refs = [R.ref(X, *ps)[2:] for ps in params]
    return X, params, refs


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("kind", sorted(R.KINDS))
@pytest.mark.parametrize("idx", range(len(R.SHAPES)), ids=IDS)
def test_known_answers_bit_for_bit(gpu, kind, idx):
    X, params, want = known(kind, idx)
    ys = raw(dev_bf16(X, gpu), dev_params(params, gpu))
    torch.cuda.synchronize()
    for k, (y, w) in enumerate(zip(ys, want)):
        got = R.plus_zero(bits(y))
        bad = np.argwhere(got != w)
        assert bad.size == 0, f"{kind} MLP {k}: {len(bad)} of {w.size} elements differ, first at (t, o) = {bad[0]}"


# ---------------------------------------------------------------- random inputs
RANDOM = [(T, E, tuple(layers), 1.0) for T, E, layers in R.SHAPES] + [(64 * 1024 + 7, 32, tuple(R.ADDING), 1.0),
                                                                     (257, 32, tuple(R.ADDING), 8.0)]


@pytest.mark.parametrize("T,E,layers,scale", RANDOM, ids=[f"{T}x{E}x{len(l)}x{s:g}" for T, E, l, s in RANDOM])
def test_random_inputs_inside_the_envelope(gpu, T, E, layers, scale):
    X, params, refs = random_case(T, E, layers, scale)
    ys = raw(dev_bf16(X, gpu), dev_params(params, gpu))
    torch.cuda.synchronize()
    for k, (y, (want, env)) in enumerate(zip(ys, refs)):
        R.assert_close(values(y), want, env, f"fused {T}x{E} MLP {k}")


class _Block(torch.nn.Module):
    def __init__(self, ps, gpu):
        super().__init__()
        A, a, B, b = ps
        l1, l2 = torch.nn.Linear(A.shape[1], A.shape[0]), torch.nn.Linear(B.shape[1], B.shape[0])
        self.network = torch.nn.Sequential(l1, torch.nn.GELU(), l2)
        with torch.no_grad():
            for p, v in zip((l1.weight, l1.bias, l2.weight, l2.bias), ps):
                p.copy_(torch.from_numpy(v))
        self.to(torch.bfloat16).to(gpu)


@pytest.mark.parametrize("idx", [2, 3], ids=[IDS[2], IDS[3]])
def test_the_cap_holds_for_the_stacked_route_too(gpu, idx):
    """The same assertion on ``stacked_apply``, the route these models took before: the cap is not tuned to the new kernel."""
    from sparsefactorization_amd import fused_mlp
    T, E, layers = R.SHAPES[idx]
    X, params, refs = random_case(T, E, tuple(layers), 1.0)
    blocks = [_Block(ps, gpu) for ps in params]
    with torch.no_grad():
        x = dev_bf16(X, gpu)
        assert fused_mlp.stackable(x, blocks)
        ys = fused_mlp.stacked_apply(x, blocks)
    for k, (y, (want, env)) in enumerate(zip(ys, refs)):
        R.assert_close(values(y), want, env, f"stacked {T}x{E} MLP {k}")


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("idx", [0, 1, 2], ids=IDS[:3])
def test_guard_bands(gpu, idx):
    """Every Y[k] a 16-byte-aligned slice of a sentinel-filled buffer: the 64 bytes before and after it stay untouched."""
    T, E, layers = R.SHAPES[idx]
    X, params, want = known("linear", idx)
    starts, pos = [], 64
    for _, O in layers:
        starts.append(pos)
        pos = (pos + T * O + 64 + 7) // 8 * 8  # the next Y starts 16-byte aligned, at least 128 bytes behind this one
    buf = torch.full((pos + 64,), SENTINEL, dtype=torch.int16, device=gpu)
    ys = [buf[s:s + T * O].view(torch.bfloat16).view(T, O) for s, (_, O) in zip(starts, layers)]
    assert all(y.data_ptr() % 16 == 0 for y in ys)
    raw(dev_bf16(X, gpu), dev_params(params, gpu), ys=ys)
    torch.cuda.synchronize()
    flat = buf.cpu().numpy().view(np.uint16)
    inside = np.zeros(flat.size, bool)
    for k, (s, (_, O), w) in enumerate(zip(starts, layers, want)):
        inside[s:s + T * O] = True
        assert np.all(flat[s - 32:s] == SENTINEL), f"MLP {k}: the 64 bytes before Y were written"
        assert np.all(flat[s + T * O:s + T * O + 32] == SENTINEL), f"MLP {k}: the 64 bytes after Y were written"
        assert np.array_equal(R.plus_zero(flat[s:s + T * O].reshape(T, O)), w), f"MLP {k}"
    assert np.all(flat[~inside] == SENTINEL)


# ---------------------------------------------------------------- token locality
def test_a_nan_token_stays_in_its_row(gpu):
    T, E, layers = R.SHAPES[1]
    X, params, _ = random_case(T, E, tuple(layers), 1.0)
    flat = dev_params(params, gpu)
    x = dev_bf16(X, gpu)
    base = [bits(y) for y in raw(x, flat)]
    for t in (32, T - 1, 3 * 32 + 5):  # first token of a tile, last token of the ragged tile, a token of wave 3
        xn = x.clone()
        xn[t, 7] = float("nan")
        for k, (y, b0) in enumerate(zip(raw(xn, flat), base)):
            got = values(y)
            assert np.all(np.isnan(got[t])), f"token {t}, MLP {k}: the row is not all NaN"
            others = np.arange(T) != t
            assert np.array_equal(bits(y)[others], b0[others]), f"token {t}, MLP {k}: another row changed"


def test_an_inf_weight_stays_in_its_mlp(gpu):
    T, E, layers = R.SHAPES[1]
    X, params, _ = random_case(T, E, tuple(layers), 1.0)
    flat = dev_params(params, gpu)
    x = dev_bf16(X, gpu)
    base = [bits(y) for y in raw(x, flat)]
    for k, which, idx in ((0, 0, (31, 31)), (14, 2, (14, 0)), (7, 0, (0, 5))):  # A of g, B of the last MLP, A of a middle one
        hit = [p.clone() for p in flat]
        hit[4 * k + which][idx] = float("inf")
        ys = raw(x, hit)
        for kk, (y, b0) in enumerate(zip(ys, base)):
            if kk == k:
                assert not np.all(np.isfinite(values(y))), f"MLP {k}: the Inf left no trace"
            else:
                assert np.array_equal(bits(y), b0), f"Inf in MLP {k} changed MLP {kk}"


# ---------------------------------------------------------------- stale state, graph capture
def test_no_stale_state_between_calls(gpu):
    """(257, 32) after (1000, 64) in one workspace, and twice in a row: the bits of a first call on a fresh workspace."""
    Xa, pa, want_a = known("linear", 1)
    Xb, pb, want_b = known("select", 3)
    xa, fa, xb, fb = dev_bf16(Xa, gpu), dev_params(pa, gpu), dev_bf16(Xb, gpu), dev_params(pb, gpu)
    first = [bits(y) for y in raw(xa, fa)]
    ws = torch.zeros(max(workspace_bytes(32, fa)[0], workspace_bytes(64, fb)[0]), dtype=torch.uint8, device=gpu)
    for y, w in zip(raw(xb, fb, ws=ws), want_b):
        assert np.array_equal(R.plus_zero(bits(y)), w)
    for rep in range(2):
        again = [bits(y) for y in raw(xa, fa, ws=ws)]
        for k, (g, f, w) in enumerate(zip(again, first, want_a)):
            assert np.array_equal(g, f), f"run {rep}, MLP {k}: differs from the first call"
            assert np.array_equal(R.plus_zero(g), w)
    Xr, pr, _ = random_case(R.SHAPES[3][0], 64, tuple(R.SHAPES[3][2]), 1.0)
    xr, fr = dev_bf16(Xr, gpu), dev_params(pr, gpu)
    r1, r2 = [bits(y) for y in raw(xr, fr, ws=ws)], [bits(y) for y in raw(xr, fr, ws=ws)]
    assert all(np.array_equal(p, q) for p, q in zip(r1, r2))  # run to run


def test_replays_from_a_graph(gpu):
    T, E, layers = R.SHAPES[1]
    X, params, _ = random_case(T, E, tuple(layers), 1.0)
    x, flat = dev_bf16(X, gpu), dev_params(params, gpu)
    eager = [bits(y) for y in raw(x, flat)]
    ys = [torch.empty((T, O), dtype=torch.bfloat16, device=gpu) for _, O in layers]
    ws = torch.zeros(workspace_bytes(E, flat)[0], dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw(x, flat, ys=ys, ws=ws)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw(x, flat, ys=ys, ws=ws)  # pack + kernel on the capture stream
    for rep in range(2):
        for y in ys:
            y.fill_(float("nan"))
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, (y, e) in enumerate(zip(ys, eager)):
            assert np.array_equal(bits(y), e), f"replay {rep}, MLP {k}"


# ---------------------------------------------------------------- the Python route
def test_forward_keeps_leading_dims_and_equals_the_raw_entry(gpu):
    from sparsefactorization_amd import fused_mlp
    layers = [(32, 8), (33, 15), (128, 1)]
    params = R.random_params(32, layers, seed=5)
    blocks = [_Block(ps, gpu) for ps in params]
    x = dev_bf16(R.random_x(1500, 32, 9), gpu).view(3, 500, 32)
    with torch.no_grad():
        assert fused_mlp.bf16_eligible(x, blocks)
        outs = fused_mlp.fused_mlp_forward_bf16(x, blocks)
    want = raw(x.view(1500, 32), dev_params(params, gpu))
    for y, w, (_, O) in zip(outs, want, layers):
        assert y.shape == (3, 500, O) and y.dtype == torch.bfloat16
        assert np.array_equal(bits(y).reshape(1500, O), bits(w))


def _psfnet(gpu):
    from sparsefactorization_amd.synthetic_psf import PSFNet
    torch.manual_seed(42)
    cfg = dict(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=128, n_W=7, Ws=[32, 'GELU'],
               V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
               use_cuda=True, use_residuals=True, use_pos_embedding=False, problem="adding")
    return PSFNet(**cfg).to(gpu), torch.rand(8, 128, 2, device=gpu)


def test_psfnet_in_bf16_takes_the_route_under_no_grad(gpu, monkeypatch):
    from sparsefactorization_amd import fused_mlp
    net, x = _psfnet(gpu)
    with torch.no_grad():
        ref32 = net(x).cpu().numpy()
    net = net.to(torch.bfloat16)
    xb = x.to(torch.bfloat16)
    calls = []
    real = fused_mlp.fused_mlp_forward_bf16
    monkeypatch.setattr(fused_mlp, "fused_mlp_forward_bf16", lambda *a: calls.append(1) or real(*a))
    with torch.no_grad():
        data = net.init_linear(xb)
        blocks = [net.g] + list(net.fs)
        assert fused_mlp.bf16_eligible(data, blocks)
        V, links = net.produce(data)
        assert len(calls) == 1
        want = real(data, blocks)
        assert len(links) == len(want) - 1 == 7
        for got, w in zip([V] + list(links), want):
            assert got.dtype == torch.bfloat16 and got.shape == w.shape and np.array_equal(bits(got), bits(w))
        out = net(xb)
        assert len(calls) == 2 and out.dtype == torch.bfloat16
        assert rel_inf(out.float().cpu().numpy(), ref32) <= 3e-2
        monkeypatch.setattr(fused_mlp, "bf16_enabled", False)
        stacked = net(xb)
        assert len(calls) == 2
        assert rel_inf(out.float().cpu().numpy(), stacked.float().cpu().numpy()) <= 3e-2


def test_psfnet_in_bf16_trains_on_the_route_it_had(gpu, monkeypatch):
    from sparsefactorization_amd import fused_mlp
    net, x = _psfnet(gpu)
    net(x).sum().backward()
    trained = {n for n, p in net.named_parameters() if p.grad is not None}
    assert any(n.startswith("fs.") for n in trained) and any(n.startswith("g.") for n in trained)
    net = net.to(torch.bfloat16)
    net.zero_grad(set_to_none=True)

    def refuse(*a):
        raise AssertionError("the inference route was taken with gradients enabled")
    monkeypatch.setattr(fused_mlp, "fused_mlp_forward_bf16", refuse)
    xb = x.to(torch.bfloat16)
    assert not fused_mlp.bf16_eligible(net.init_linear(xb), [net.g] + list(net.fs))
    out = net(xb)
    assert out.dtype == torch.bfloat16
    out.float().sum().backward()
    assert {n for n, p in net.named_parameters() if p.grad is not None} == trained
    for name in trained:
        p = net.get_parameter(name)
        assert p.grad.dtype == torch.bfloat16 and torch.isfinite(p.grad).all(), name
