"""GPU: the fused bf16 producer backward (psf_mlp_bwd_bf16, csrc/mlp_bwd_bf16.hip) against the float64 reference of its
contract (tests/mlp_bf16_bwd_ref.py): known answers bit for bit, random inputs inside the envelope and no further from the true
gradient than the stacked route, guard bands, token locality, stale state, graph capture and the opt-in Python route.

(Sorted behind tests/test_gpu_coresidence.py, as the suite's other graph tests are: see tests/test_gpu_graph_bf16_bwd.py.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mlp_bf16_bwd_ref as BR
import mlp_bf16_ref as R

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0  # a bf16 NaN
IDS = [f"{T}x{E}x{len(layers)}" for T, E, layers in BR.SHAPES]


# ---------------------------------------------------------------- plumbing
def dev_bf16(v, gpu):
    """bf16-valued float64 array -> bf16 device tensor (exact)."""
    R.to_bits(v)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.bfloat16).to(gpu)


def bits(t) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def values(t) -> np.ndarray:
    return t.detach().float().cpu().numpy().astype(np.float64)


def sizes(flat):
    """flat = (A0, a0, B0, A1, ...): (K, h table, O table)."""
    K = len(flat) // 3
    return K, (ctypes.c_int32 * K)(*[A.shape[0] for A in flat[0::3]]), (ctypes.c_int32 * K)(*[B.shape[0] for B in flat[2::3]])


def workspace_bytes(T, E, flat):
    from sparsefactorization_amd import _lib
    K, h, O = sizes(flat)
    n = _lib.load().psf_mlp_bwd_bf16_workspace(T, E, K, h, O)
    assert n > 0
    return n


def raw(x, flat, dys, need_dx=True, ws=None, out=None):
    """One call of the raw entry. ``out``: (dX or None, [dA0, da0, dB0, db0, dA1, ...]) to write into (allocated when None).
    Returns that pair."""
    from sparsefactorization_amd import _lib
    from sparsefactorization_amd.fused_mlp import _ptrs
    lib = _lib.load()
    T, E = x.shape
    K, h, O = sizes(flat)
    if out is None:
        grads = []
        for A, a, B in zip(flat[0::3], flat[1::3], flat[2::3]):
            grads += [torch.empty_like(A), torch.empty_like(a), torch.empty_like(B), torch.empty(B.shape[0], dtype=A.dtype, device=A.device)]
        out = (torch.empty_like(x) if need_dx else None, grads)
    dX, grads = out
    if ws is None:
        ws = torch.zeros(workspace_bytes(T, E, flat), dtype=torch.uint8, device=x.device)
    rc = lib.psf_mlp_bwd_bf16(x.data_ptr(), T, E, K, _ptrs(flat[0::3]), _ptrs(flat[1::3]), _ptrs(flat[2::3]), h, O, _ptrs(dys),
                              dX.data_ptr() if dX is not None else None, _ptrs(grads[0::4]), _ptrs(grads[1::4]),
                              _ptrs(grads[2::4]), _ptrs(grads[3::4]), ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device))
    _lib.check(rc, "psf_mlp_bwd_bf16")
    return out


def result_bits(out):
    """[(name, bits with -0 -> +0)] of a raw() result, in BR.tensors' order; a missing dX is left out."""
    dX, grads = out
    names = [f"{n}[{k}]" for k in range(len(grads) // 4) for n in BR.NAMES]
    return ([("dX", R.plus_zero(bits(dX)))] if dX is not None else []) + [(n, R.plus_zero(bits(g))) for n, g in zip(names, grads)]


def result_values(out):
    dX, grads = out
    return {"dX": values(dX), "grads": [tuple(values(g) for g in grads[4 * k:4 * k + 4]) for k in range(len(grads) // 4)]}


def on_device(case, gpu):
    flat = [dev_bf16(p, gpu) for ps in case.params for p in ps[:3]]
    return dev_bf16(case.X, gpu), flat, [dev_bf16(dy, gpu) for dy in case.dYs]


@functools.lru_cache(maxsize=None)
def known(kind, idx):
    """The construction of shape ``idx`` and its answers' bits (computed once, shared, never modified)."""
    if kind == "round_once":
        case = BR.make_round_once(63)
    else:
        T, E, layers = BR.SHAPES[idx]
        case = BR.KINDS[kind][0](T, E, layers, BR.seed_of(T, E))
    return case, BR.bits_of(case.answers)


@functools.lru_cache(maxsize=None)
def random_case(T, E, layers):
    """Random inputs with their reference, envelope and true gradient, computed once on the CPU from the bf16 values."""
    layers = list(layers)
    X = R.random_x(T, E, R.seed_of(T, E))
    params = R.random_params(E, layers, seed=T + 7 * E)
    dYs = BR.random_dys(T, layers, seed=T + 11 * E)
    want, env = BR.ref_bwd(X, params, dYs)
    return BR.Case("random", X, params, dYs), want, env, BR.true_grad(X, params, dYs)


def assert_same_bits(got, want, what=""):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {name}: {len(bad)} of {w.size} elements differ, first at {bad[0]}: {g[tuple(bad[0])]:#06x} for {w[tuple(bad[0])]:#06x}"


# ---------------------------------------------------------------- known answers
@pytest.mark.parametrize("kind", sorted(BR.KINDS))
@pytest.mark.parametrize("idx", range(len(BR.SHAPES)), ids=IDS)
def test_known_answers_bit_for_bit(gpu, kind, idx):
    case, want = known(kind, idx)
    out = raw(*on_device(case, gpu))
    torch.cuda.synchronize()
    assert_same_bits(result_bits(out), want, kind)


def test_dx_is_rounded_once_over_all_mlps(gpu):
    case, want = known("round_once", 0)
    out = raw(*on_device(case, gpu))
    torch.cuda.synchronize()
    assert values(out[0])[61, 0] == 256.0  # 257 - 1; rounded per MLP it would be 255
    assert_same_bits(result_bits(out), want, "round_once")


@pytest.mark.parametrize("kind", sorted(BR.KINDS))
def test_dx_may_be_null(gpu, kind):
    case, want = known(kind, 1)
    out = raw(*on_device(case, gpu), need_dx=False)
    torch.cuda.synchronize()
    assert out[0] is None
    assert_same_bits(result_bits(out), want[1:], kind)


# ---------------------------------------------------------------- random inputs
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


def module_grads(x, blocks, dys, fused_mlp):
    """dX and the parameters' gradients of ``fused_mlp.apply(x, blocks)`` under autograd, as a result dict."""
    x = x.detach().clone().requires_grad_(True)
    for b in blocks:
        b.zero_grad(set_to_none=True)
    ys = fused_mlp.apply(x, blocks)
    torch.autograd.backward(ys, dys)
    return {"dX": values(x.grad), "grads": [tuple(values(p.grad) for p in fused_mlp._params_of([b])) for b in blocks]}


@pytest.mark.parametrize("T,E,layers", BR.RANDOM, ids=[f"{T}x{E}x{len(l)}" for T, E, l in BR.RANDOM])
def test_random_inputs_inside_the_envelope_and_as_close_to_the_truth_as_the_stacked_route(gpu, T, E, layers, monkeypatch):
    """Both routes make the same roundings and differ only in f32 summation order and flipped ties, so the fused kernel's RMS
    error against the unrounded float64 gradient may exceed the stacked route's by that noise only: 1.25 x, a margin and not a
    measurement. The ratios are printed; profiles/bf16_mlp_bwd_ab.md records them."""
    from sparsefactorization_amd import fused_mlp
    case, want, env, true = random_case(T, E, tuple(layers))
    x, flat, dys = on_device(case, gpu)
    got = result_values(raw(x, flat, dys))
    worst, where = BR.worst_in_envelope(got, want, env)
    print(f"fused {T}x{E}: worst |err| / envelope = {worst:.4f} in {where}")
    assert worst <= 1.0, f"outside the envelope in {where} ({worst:.3f} of it)"

    blocks = [_Block(ps, gpu) for ps in case.params]
    monkeypatch.setattr(fused_mlp, "bf16_train_route", "never")
    probe = x.detach().clone().requires_grad_(True)
    assert fused_mlp.route(probe, blocks) == ("stacked" if len(blocks) > 1 else None)
    if len(blocks) > 1:
        stacked = module_grads(x, blocks, dys, fused_mlp)
    else:  # a single MLP is not stacked: the modules themselves are the route it has
        xs = x.detach().clone().requires_grad_(True)
        torch.autograd.backward([blocks[0].network(xs)], dys)
        stacked = {"dX": values(xs.grad), "grads": [tuple(values(p.grad) for p in fused_mlp._params_of(blocks))]}
    assert BR.worst_in_envelope(stacked, want, env)[0] <= 1.0  # the envelope is not tuned to the new kernel
    ours, theirs = BR.rms_errors(got, true), BR.rms_errors(stacked, true)
    ratios = {n: (ours[n] / theirs[n] if theirs[n] > 0 else (1.0 if ours[n] == 0 else float("inf"))) for n in ours}
    for kind in ("dX",) + BR.NAMES:
        rs = [r for n, r in ratios.items() if n.split("[")[0] == kind]
        print(f"rms ratio fused / stacked {T}x{E} {kind}: max {max(rs):.4f} mean {sum(rs) / len(rs):.4f} ({len(rs)} tensors)")
    over = {n: round(r, 4) for n, r in ratios.items() if not r <= 1.25}
    assert not over, f"RMS error against the true gradient above 1.25 x the stacked route's: {over}"


# ---------------------------------------------------------------- guard bands
def _banded(shapes, gpu, align):
    """Tensors of ``shapes`` as slices of one NaN-filled bf16 buffer, each start a multiple of ``align`` elements and at least
    32 elements of NaN on either side. Returns (buffer, tensors, starts)."""
    starts, pos = [], 32
    for s in shapes:
        pos = (pos + align - 1) // align * align
        starts.append(pos)
        pos += int(np.prod(s)) + 32
    buf = torch.full((pos + 32,), NAN16, dtype=torch.int16, device=gpu)
    assert buf.data_ptr() % 16 == 0
    views = [buf[st:st + int(np.prod(s))].view(torch.bfloat16).view(*s) for st, s in zip(starts, shapes)]
    return buf, views, starts


@pytest.mark.parametrize("idx", [0, 1, 2], ids=IDS[:3])
def test_guard_bands_around_every_gradient_and_the_workspace(gpu, idx):
    T, E, layers = BR.SHAPES[idx]
    case, want = known("linear", idx)
    x, flat, dys = on_device(case, gpu)
    shapes = [(T, E)] + [s for h, O in layers for s in ((h, E), (h,), (O, h), (O,))]
    buf, views, starts = _banded(shapes, gpu, 8)  # dX needs 16 bytes; the others start on odd multiples of 2 bytes too:
    odd_buf, odd_views, odd_starts = _banded(shapes[1:], gpu, 1)
    n = workspace_bytes(T, E, flat)
    ws_buf = torch.full((n + 512,), 0xFF, dtype=torch.uint8, device=gpu)  # f32 NaNs
    off = 256 + (-(ws_buf.data_ptr() + 256)) % 16
    for grads, b, st, shp in ((views[1:], buf, starts, shapes), (odd_views, odd_buf, odd_starts, shapes[1:])):
        ws_buf.fill_(0xFF)
        raw(x, flat, dys, ws=ws_buf[off:off + n], out=(views[0], grads))
        torch.cuda.synchronize()
        assert_same_bits(result_bits((views[0], grads)), want, "banded")
        flat_bits = b.cpu().numpy().view(np.uint16)
        inside = np.zeros(flat_bits.size, bool)
        for s0, s in zip(st, shp):
            inside[s0:s0 + int(np.prod(s))] = True
        assert np.all(flat_bits[~inside] == NAN16), "a gradient was written outside its tensor"
        w = ws_buf.cpu().numpy()
        assert np.all(w[:off] == 0xFF) and np.all(w[off + n:] == 0xFF), "the workspace was overrun"


def test_nothing_behind_x_or_dy_is_read(gpu):
    """Odd O and ragged T (257 tokens, O = 15): NaNs directly behind X and behind every dY[k] reach no gradient."""
    T, E, layers = BR.SHAPES[1]
    for kind in sorted(BR.KINDS):
        case, want = known(kind, 1)
        x, flat, dys = on_device(case, gpu)
        buf, views, _ = _banded([(T, E)] + [(T, O) for _, O in layers], gpu, 8)
        for v, src in zip(views, [x] + dys):
            v.copy_(src)
        assert all(v.data_ptr() % 16 == 0 for v in views)
        out = raw(views[0], flat, views[1:])
        torch.cuda.synchronize()
        for name, t in [("dX", out[0])] + list(zip("g" * len(out[1]), out[1])):
            assert torch.isfinite(t.float()).all(), f"{kind}: a NaN reached a gradient ({name})"
        assert_same_bits(result_bits(out), want, kind)


# ---------------------------------------------------------------- token locality
def test_a_nan_token_stays_in_its_row_of_dx(gpu):
    T, E, layers = BR.SHAPES[1]
    case, _, _, _ = random_case(4097, 32, tuple(BR.ADDING))
    x, flat, dys = on_device(case, gpu)
    x, dys = x[:T].contiguous(), [d[:T].contiguous() for d in dys]
    base = bits(raw(x, flat, dys)[0])
    for t in (32, T - 1, 3 * 32 + 5):  # first token of a tile, the one token of the ragged tile, a token of wave 3
        xn = x.clone()
        xn[t, 7] = float("nan")
        dX = raw(xn, flat, dys)[0]
        got = values(dX)
        assert np.all(np.isnan(got[t])), f"token {t}: its row of dX is not all NaN"
        others = np.arange(T) != t
        assert np.all(np.isfinite(got[others])) and np.array_equal(bits(dX)[others], base[others]), f"token {t}: another row changed"


def test_element_indices_past_2_31(gpu):
    """Not a smallest-shape test, and the one test here that is large on purpose: an index past 2^31 can only go wrong at that
    size. T = 2^26 + 33 tokens with O = 32, so dY holds more than 2^31 elements (4.3 GB); with X, dX (1.1 GB each at E = 8) and
    the workspace (131 073 partial-sum slots of one unit, 1.1 GB) about 7.6 GB for about a second. One hidden row (h = 1), and
    dY's float64 sums are taken in chunks, to keep everything else small. It is also the only random-data comparison of the
    two-tiles-per-wave instance (the whole call) with the one-tile instance (the calls on the windows).
    dX[t] depends on token t's rows only, so the rows of two windows — the head, and the tokens around dY's element 2^31 up to the
    ragged tail — must be the bits of a call on those tokens alone; and the bias gradient of the second layer, a plain sum of dY
    over all tokens, must be the float64 sum of dY to f32 summation accuracy."""
    T, E, h, O, win = (1 << 26) + 33, 8, 1, 32, 2048
    g = torch.Generator(device=gpu).manual_seed(1)
    x = torch.randn(T, E, device=gpu, dtype=torch.bfloat16, generator=g)
    dy = torch.randn(T, O, device=gpu, dtype=torch.bfloat16, generator=g)
    assert dy.numel() > 1 << 31
    flat = [dev_bf16(p, gpu) for p in R.random_params(E, [(h, O)], seed=3)[0][:3]]
    dX, grads = raw(x, flat, [dy])
    torch.cuda.synchronize()
    for lo in (0, (1 << 26) - win):  # the second window runs from 2048 tokens before dY's element 2^31 to the ragged end
        hi = min(lo + 2 * win, T)
        part = raw(x[lo:hi], flat, [dy[lo:hi]])[0]
        assert torch.equal(dX[lo:hi].view(torch.int16), part.view(torch.int16)), f"dX rows {lo}..{hi} differ from a call on them alone"
    want, mag = np.zeros(O), np.zeros(O)
    for chunk in dy.split(1 << 22):  # 4 M tokens at a time: 1 GB of float64 in flight instead of 17
        c64 = chunk.double()
        want += c64.sum(0).cpu().numpy()
        mag += c64.abs().sum(0).cpu().numpy()
    assert np.all(np.abs(values(grads[3]) - want) <= R.ulp_bf16(want) + T * 2.0 ** -24 * mag)
    assert all(torch.isfinite(t.float()).all() for t in grads)


# ---------------------------------------------------------------- stale state, graph capture
def test_two_calls_give_equal_bits_and_a_workspace_carries_nothing_over(gpu):
    case_a, want_a = known("linear", 1)
    case_b, want_b = known("select", 2)
    a, b = on_device(case_a, gpu), on_device(case_b, gpu)
    n = max(workspace_bytes(case_a.T, case_a.E, a[1]), workspace_bytes(case_b.T, case_b.E, b[1]))
    ws = torch.zeros(n, dtype=torch.uint8, device=gpu)
    assert_same_bits(result_bits(raw(*b, ws=ws)), want_b, "first call")
    for rep in range(2):
        assert_same_bits(result_bits(raw(*a, ws=ws)), want_a, f"call {rep} after other inputs")
    assert_same_bits(result_bits(raw(*b, ws=ws)), want_b, "back again")
    case, _, _, _ = random_case(*[(T, E, tuple(l)) for T, E, l in BR.RANDOM][1])
    r = on_device(case, gpu)
    ws.fill_(0xFF)
    first = result_bits(raw(*r, ws=ws))
    assert_same_bits(result_bits(raw(*r, ws=ws)), first, "run to run")
    assert_same_bits(result_bits(raw(*r)), first, "fresh workspace")


def test_replays_from_a_graph(gpu):
    case, _, _, _ = random_case(*[(T, E, tuple(l)) for T, E, l in BR.RANDOM][1])
    x, flat, dys = on_device(case, gpu)
    eager = result_bits(raw(x, flat, dys))
    out = raw(x, flat, dys)
    ws = torch.zeros(workspace_bytes(case.T, case.E, flat), dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw(x, flat, dys, ws=ws, out=out)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw(x, flat, dys, ws=ws, out=out)  # pack, kernel and the two reduction stages on the capture stream
    for rep in range(3):
        for t in [out[0]] + out[1]:
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert_same_bits(result_bits(out), eager, f"replay {rep}")


# ---------------------------------------------------------------- the module surface
def _psfnet(gpu):
    from sparsefactorization_amd.synthetic_psf import PSFNet
    torch.manual_seed(42)
    cfg = dict(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=128, n_W=7, Ws=[32, 'GELU'],
               V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
               use_cuda=True, use_residuals=True, use_pos_embedding=False, problem="adding")
    return PSFNet(**cfg).to(torch.bfloat16).to(gpu), torch.rand(8, 128, 2, device=gpu).to(torch.bfloat16)


def test_psfnet_in_bf16_trains_on_the_new_route_only_when_asked(gpu, monkeypatch):
    from sparsefactorization_amd import fused_mlp
    net, xb = _psfnet(gpu)
    blocks = [net.g] + list(net.fs)
    seen = {}
    real_stacked, real_fused = fused_mlp.stacked_apply, fused_mlp.fused_mlp_apply_bf16

    def stacked(x, bl):
        ys = real_stacked(x, bl)
        for y in ys:
            y.retain_grad()
        seen["never"] = (x.detach(), ys)
        return ys

    def fused(x, bl):
        seen["always"] = seen.get("always", 0) + 1
        return real_fused(x, bl)

    monkeypatch.setattr(fused_mlp, "stacked_apply", stacked)
    monkeypatch.setattr(fused_mlp, "fused_mlp_apply_bf16", fused)
    assert fused_mlp.bf16_train_route == "never"
    assert fused_mlp.route(net.init_linear(xb), blocks) == "stacked"
    net(xb).float().sum().backward()
    assert "never" in seen and "always" not in seen, "with \"never\" the model takes the route it had"
    data, ys = seen["never"]
    T = data.numel() // 32
    params = [tuple(values(p) for p in fused_mlp._params_of([b])) for b in blocks]
    want, env = BR.ref_bwd(values(data).reshape(T, 32), params, [values(y.grad).reshape(T, -1) for y in ys])
    never = {"dX": want["dX"], "grads": [tuple(values(p.grad) for p in fused_mlp._params_of([b])) for b in blocks]}
    assert BR.worst_in_envelope(never, want, env)[0] <= 1.0

    net.zero_grad(set_to_none=True)
    monkeypatch.setattr(fused_mlp, "bf16_train_route", "always")
    assert fused_mlp.route(net.init_linear(xb), blocks) == "bf16_train"
    out = net(xb)
    assert out.dtype == torch.bfloat16 and seen.get("always") == 1
    out.float().sum().backward()
    always = {"dX": want["dX"], "grads": [tuple(values(p.grad) for p in fused_mlp._params_of([b])) for b in blocks]}
    for b in blocks:
        assert all(p.grad.dtype == torch.bfloat16 for p in fused_mlp._params_of([b]))
    worst, where = BR.worst_in_envelope(always, want, env)
    print(f"PSFNet Adding N = 128, \"always\": worst |err| / envelope = {worst:.4f} in {where}")
    assert worst <= 1.0


def _watch_alignment(fused_mlp, monkeypatch):
    """Counts the tensors that reach ``fused_mlp._aligned16`` off a 16-byte boundary."""
    seen = {"misaligned": 0, "calls": 0}
    real = fused_mlp._aligned16

    def aligned16(t):
        seen["calls"] += 1
        seen["misaligned"] += int(t.data_ptr() % 16 != 0)
        out = real(t)
        assert out.data_ptr() % 16 == 0 and (out is t or torch.equal(out, t))
        return out

    monkeypatch.setattr(fused_mlp, "_aligned16", aligned16)
    return seen


def test_output_gradients_that_are_views_off_their_16_byte_boundary(gpu, monkeypatch):
    """The gradients of the W_m reach the producers as the M slices of ONE [M, B, N, L] tensor (chord.py's backward chain); with
    B N L = 100 x 15 every other slice starts 8 bytes off a 16-byte boundary, and so does an x that is a slice of a larger
    buffer. The route copies what is misaligned; the gradients are the bits of a call on freshly allocated copies."""
    from sparsefactorization_amd import fused_mlp
    T, E, layers = 100, 32, [(32, 15)] * 6
    params = R.random_params(E, layers, seed=11)
    blocks = [_Block(ps, gpu) for ps in params]
    xbuf = dev_bf16(R.random_x(T + 1, E, 5), gpu).reshape(-1)
    x_view = xbuf[4:4 + T * E].view(T, E)  # 8 bytes off
    gbuf = dev_bf16(np.stack(BR.random_dys(T, layers, seed=13)), gpu)  # [6, 100, 15]
    views = list(gbuf.unbind(0))
    assert x_view.data_ptr() % 16 == 8 and [v.data_ptr() % 16 for v in views] == [0, 8] * 3
    monkeypatch.setattr(fused_mlp, "bf16_train_route", "always")
    seen = _watch_alignment(fused_mlp, monkeypatch)
    probe = x_view.detach().requires_grad_(True)
    assert fused_mlp.route(probe, blocks) == "bf16_train"
    got = module_grads_of(probe, blocks, views, fused_mlp)
    assert seen["misaligned"] == 4  # x and three of the six dY
    fresh = module_grads_of(x_view.detach().clone().requires_grad_(True), blocks, [v.clone() for v in views], fused_mlp)
    for (name, a), (_, b) in zip(BR.tensors(got), BR.tensors(fresh)):
        assert np.array_equal(a, b), name
    want, env = BR.ref_bwd(values(x_view), params, [values(v) for v in views])
    assert BR.worst_in_envelope(got, want, env)[0] <= 1.0


def module_grads_of(x, blocks, dys, fused_mlp):
    """As module_grads, on the very tensor ``x`` (a leaf that requires a gradient) instead of a fresh copy of it."""
    for b in blocks:
        b.zero_grad(set_to_none=True)
    x.grad = None
    torch.autograd.backward(fused_mlp.apply(x, blocks), dys)
    return {"dX": values(x.grad), "grads": [tuple(values(p.grad) for p in fused_mlp._params_of([b])) for b in blocks]}


def test_psfnet_whose_link_gradients_are_misaligned_views_trains_on_the_new_route(gpu, monkeypatch):
    """A bf16 PSFNet with N = 100, L = 15, B = 3: B N L = 4 500 is no multiple of 8, so the backward chain hands every other
    fs[m] an output gradient 8 bytes off a 16-byte boundary. With "always" the model takes "bf16_train", trains, and the
    producers' parameter gradients lie inside the envelope of the float64 reference on the inputs the route was given."""
    from sparsefactorization_amd import fused_mlp
    from sparsefactorization_amd.synthetic_psf import PSFNet
    torch.manual_seed(7)
    cfg = dict(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=100, n_W=14, Ws=[32, 'GELU'],
               V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
               use_cuda=True, use_residuals=True, use_pos_embedding=False, problem="adding")
    net = PSFNet(**cfg).to(torch.bfloat16).to(gpu)
    xb = torch.rand(3, 100, 2, device=gpu).to(torch.bfloat16)
    blocks = [net.g] + list(net.fs)
    monkeypatch.setattr(fused_mlp, "bf16_train_route", "always")
    seen = _watch_alignment(fused_mlp, monkeypatch)
    taken = {}
    real = fused_mlp.fused_mlp_apply_bf16

    def fused(x, bl):
        ys = real(x, bl)
        for y in ys:
            y.retain_grad()
        taken["io"] = (x.detach(), ys)
        return ys

    monkeypatch.setattr(fused_mlp, "fused_mlp_apply_bf16", fused)
    assert fused_mlp.route(net.init_linear(xb), blocks) == "bf16_train"
    out = net(xb)
    out.float().sum().backward()
    assert "io" in taken and seen["misaligned"] >= 7, f"the case did not produce misaligned gradients: {seen}"
    data, ys = taken["io"]
    T = data.numel() // 32
    params = [tuple(values(p) for p in fused_mlp._params_of([b])) for b in blocks]
    want, env = BR.ref_bwd(values(data).reshape(T, 32), params, [values(y.grad).reshape(T, -1) for y in ys])
    got = {"dX": want["dX"], "grads": [tuple(values(p.grad) for p in fused_mlp._params_of([b])) for b in blocks]}
    worst, where = BR.worst_in_envelope(got, want, env)
    print(f"PSFNet N = 100, L = 15, B = 3, \"always\": worst |err| / envelope = {worst:.4f} in {where}; {seen}")
    assert worst <= 1.0

