"""GPU: the whole bf16 mixer of a short sequence in one launch (psf_mixer_fwd_bf16, csrc/mixer_lds_bf16.h).

Its contract is "the bits of psf_mlp_fwd_bf16 followed by psf_chord_chain_fwd_bf16", so the first reference is exactly that:
the two entries run on the same operands, V0 and every stored step compared as bits (NaN positions equal). The second
reference depends on no GPU code of the project: the known-answer constructions of tests/mlp_bf16_ref.py fix V0 and every
W_m to the bit, and the iterated oracle step (test_gpu_bf16_chain._chain_ref_steps) gives every X_m. Then guard bands, NaN /
Inf containment, stale state, graph capture and the Python route.

(Sorted behind tests/test_gpu_coresidence.py, as the suite's other graph tests are: see tests/test_gpu_graph_bf16_bwd.py.)"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mlp_bf16_ref as R
from test_gpu_bf16_chain import _assert_finite, _assert_same, _chain_ref_steps
from test_gpu_mlp_bf16 import _psfnet, bits, dev_bf16, dev_params, raw

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5B  # a bf16 pattern no case produces wholesale (2.4e+16)
E_UNSUPPORTED = -7


# ---------------------------------------------------------------- plumbing
def _tables(flat):
    from sparsefactorization_amd.fused_mlp import _ptrs
    K = len(flat) // 4
    h = (ctypes.c_int32 * K)(*[A.shape[0] for A in flat[0::4]])
    return h, [_ptrs(flat[i::4]) for i in range(4)]


def mixer_rc(x3, flat, residual, outs, V0=None, ws=None):
    """One call of the raw entry on [B, N, E] bf16 ``x3`` and the flat parameter list (A0, a0, B0, b0, A1, ...) of g, fs[0..M):
    the return code (nothing is checked)."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    B, N, E = x3.shape
    M = len(flat) // 4 - 1
    C, L = flat[2].shape[0], flat[6].shape[0]
    h, (A, a, Bw, b) = _tables(flat)
    if ws is None:
        n = lib.psf_mixer_fwd_bf16_workspace(N, E, M, h, C, L)
        ws = torch.zeros(max(n, 16), dtype=torch.uint8, device=x3.device)
    o_tab = (ctypes.c_void_p * M)(*[o.data_ptr() for o in outs])
    return lib.psf_mixer_fwd_bf16(x3.data_ptr(), B, N, E, M, A, a, Bw, b, h, C, L, 1 if residual else 0,
                                  V0.data_ptr() if V0 is not None else None, o_tab, ws.data_ptr(), ws.numel(), _lib.stream_ptr(x3.device))


def mixer(x3, flat, residual, keep_all=True, ws=None, want_v0=True):
    """(V0 or None, [step m or None]) of one call: every step kept, or two alternating buffers (then only the last two steps
    reach memory)."""
    from sparsefactorization_amd import _lib
    B, N, _ = x3.shape
    M, C = len(flat) // 4 - 1, flat[2].shape[0]
    bufs = [torch.full((B, N, C), float("nan"), dtype=torch.bfloat16, device=x3.device) for _ in range(M if keep_all else min(M, 2))]
    outs = [bufs[m % len(bufs)] for m in range(M)]
    V0 = torch.full((B, N, C), float("nan"), dtype=torch.bfloat16, device=x3.device) if want_v0 else None
    _lib.check(mixer_rc(x3, flat, residual, outs, V0, ws), "psf_mixer_fwd_bf16")
    torch.cuda.synchronize()
    steps = [outs[m] if (keep_all or m >= M - len(bufs)) else None for m in range(M)]
    return V0, steps


def two_calls(x3, flat, residual):
    """The parent's route: psf_mlp_fwd_bf16, then psf_chord_chain_fwd_bf16 on its outputs, every step kept. (V0, [steps])."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    B, N, E = x3.shape
    M = len(flat) // 4 - 1
    ys = raw(x3.reshape(B * N, E), flat)
    C, L = ys[0].shape[1], ys[1].shape[1]
    V0 = ys[0].view(B, N, C)
    outs = [torch.empty_like(V0) for _ in range(M)]
    vp = ctypes.c_void_p
    rc = lib.psf_chord_chain_fwd_bf16((vp * M)(*[y.data_ptr() for y in ys[1:]]), V0.data_ptr(), (vp * M)(*[o.data_ptr() for o in outs]),
                                      M, 1 if residual else 0, B, N, L, C, N * C, None, _lib.stream_ptr(x3.device))
    _lib.check(rc, "psf_chord_chain_fwd_bf16")
    torch.cuda.synchronize()
    return V0, outs


def _layers(C, L, M, hg, hf):
    """g of width hg; the link MLPs alternate hf and hg, so one call holds MLPs of different unit counts."""
    return [(hg, C)] + [(hf if m % 2 == 0 else hg, L) for m in range(M)]


def _random_case(gpu, B, N, C, E, hg, hf, L, M, seed=0):
    layers = _layers(C, L, M, hg, hf)
    x3 = dev_bf16(R.random_x(B * N, E, 1000 + seed + N + 3 * E), gpu).view(B, N, E)
    flat = dev_params(R.random_params(E, layers, seed=seed + N + 7 * E + L), gpu)
    return x3, flat


def _check_against_two_calls(x3, flat, residual, what):
    want_v0, want = two_calls(x3, flat, residual)
    M = len(want)
    v0, steps = mixer(x3, flat, residual, keep_all=True)
    _assert_same(v0, want_v0, f"{what}: V0")
    for m in range(M):
        _assert_same(steps[m], want[m], f"{what}: step {m}, every step kept")
    v0, steps = mixer(x3, flat, residual, keep_all=False)
    _assert_same(v0, want_v0, f"{what}: V0, two buffers")
    for m in range(M):
        if steps[m] is not None:
            _assert_same(steps[m], want[m], f"{what}: step {m}, two alternating buffers")
    assert steps[M - 1] is not None
    return want_v0, want


# ---------------------------------------------------------------- bit identity with the two-call route
# (B, N, C, E, h of g, h of the even link MLPs, L, M, residual). N: one tile; three tiles on three waves; Adding's 128; two
# tiles per wave (512) and one-or-two (288). h: a ragged unit, one, two, four. L: both W-tile strides (<= 12, > 12); at
# N = 32 the offsets of L = 20 wrap to 0 and repeat. B = 300: more sequences than CUs.
GRID = [
    (1, 32, 8, 8, 7, 7, 4, 1, True), (3, 32, 16, 24, 32, 33, 20, 3, False), (300, 32, 8, 32, 32, 32, 12, 2, True),
    (1, 32, 16, 64, 33, 128, 13, 14, False), (3, 32, 8, 24, 128, 128, 12, 14, True), (300, 32, 16, 32, 7, 33, 15, 3, True),
    (3, 96, 8, 32, 33, 128, 13, 3, True), (1, 96, 16, 64, 128, 7, 15, 2, False), (3, 96, 16, 8, 32, 32, 4, 1, True),
    (3, 96, 8, 24, 7, 7, 20, 14, False), (1, 96, 8, 64, 32, 33, 12, 1, True),
    (8, 128, 8, 32, 32, 32, 8, 7, True), (8, 128, 8, 32, 32, 32, 15, 14, True), (1, 128, 16, 8, 128, 128, 20, 1, False),
    (3, 128, 16, 24, 7, 33, 4, 14, True), (1, 128, 8, 64, 33, 33, 12, 3, False), (1, 128, 16, 32, 128, 32, 13, 2, True),
    (3, 128, 8, 8, 33, 7, 15, 3, False),
    (1, 288, 16, 32, 32, 32, 12, 2, True),
    (1, 512, 8, 32, 32, 32, 12, 2, True), (3, 512, 16, 64, 128, 128, 20, 3, False), (1, 512, 16, 8, 33, 7, 13, 14, True),
    (3, 512, 8, 24, 128, 32, 15, 1, False), (3, 512, 8, 64, 7, 128, 4, 2, True), (1, 512, 16, 32, 32, 33, 15, 14, False),
]


@pytest.mark.parametrize("B,N,C,E,hg,hf,L,M,residual", GRID, ids=["-".join(str(int(v)) for v in c) for c in GRID])
def test_bits_of_the_two_call_route(gpu, B, N, C, E, hg, hf, L, M, residual):
    from sparsefactorization_amd import _lib
    x3, flat = _random_case(gpu, B, N, C, E, hg, hf, L, M)
    h, _ = _tables(flat)
    assert _lib.load().psf_mixer_fwd_bf16_plan(N, E, M, h, C, L) == 2
    want_v0, want = _check_against_two_calls(x3, flat, residual, f"N={N} C={C} E={E} L={L} M={M}")
    assert bool(torch.isfinite(want[-1].float()).all()) and float(want[-1].float().abs().max()) > 0  # (no case passes as NaN == NaN)


@pytest.mark.parametrize("N", [544, 1024])
def test_beyond_512_is_either_covered_and_right_or_refused(gpu, N):
    """plan_mixer_lds_bf16 decides; whichever way, the entry keeps its word."""
    from sparsefactorization_amd import _lib
    B, C, E, L, M = 2, 16, 32, 12, 2
    x3, flat = _random_case(gpu, B, N, C, E, 32, 33, L, M)
    h, _ = _tables(flat)
    if _lib.load().psf_mixer_fwd_bf16_plan(N, E, M, h, C, L) == 2:
        _check_against_two_calls(x3, flat, True, f"N={N}")
    else:
        outs = [torch.full((B, N, C), float("nan"), dtype=torch.bfloat16, device=gpu) for _ in range(M)]
        assert mixer_rc(x3, flat, True, outs, ws=torch.zeros(1 << 16, dtype=torch.uint8, device=gpu)) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)  # nothing ran


# ---------------------------------------------------------------- known answers from the CPU alone
# (B, N, E, C, L, M, h): M <= 3; layers [(h, C)] + [(h, L)] * M. known_case asserts, on the CPU, that every expected step is
# finite and every nonzero product of a step lies inside [2^-126, FLT_MAX].
KNOWN = [(2, 32, 8, 8, 4, 1, 9), (3, 96, 24, 16, 13, 3, 33), (2, 128, 32, 8, 8, 3, 32), (1, 512, 64, 16, 20, 2, 128)]


@functools.lru_cache(maxsize=None)
def known_case(kind, idx):
    """The construction, V0 and every X_m of the iterated oracle reference as bf16 tensors (computed once, never modified)."""
    B, N, E, C, L, M, h = KNOWN[idx]
    layers = [(h, C)] + [(h, L)] * M
    X, params, answers = R.KINDS[kind][0](B * N, E, layers, R.seed_of(B * N, E))
    R.KINDS[kind][1](X, params, answers)
    V0 = np.ascontiguousarray(answers[0], np.float32).reshape(B, N, C)
    Ws = [np.ascontiguousarray(y, np.float32).reshape(B, N, L) for y in answers[1:]]
    out = {}
    for residual in (False, True):
        out[residual] = _chain_ref_steps(Ws, V0, residual)
        _assert_finite(out[residual])
        # the kernels fuse the (exact) product into the sum; that equals the oracle's rounded product only while every
        # nonzero product is a normal f32: smallest and largest |w x| of every step
        for W, Xm in zip(Ws, [V0] + [s.float().numpy() for s in out[residual][:-1]]):
            w, x = np.abs(W[W != 0]).astype(np.float64), np.abs(Xm[Xm != 0]).astype(np.float64)
            assert w.size and x.size and w.min() * x.min() >= 2.0 ** -126 and w.max() * x.max() < 3.4e38
    return X, params, V0, out


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("kind", sorted(R.KINDS))
@pytest.mark.parametrize("idx", range(len(KNOWN)), ids=["x".join(map(str, k)) for k in KNOWN])
def test_known_answers_from_the_cpu_alone(gpu, kind, idx, residual):
    B, N, E, C, L, M, h = KNOWN[idx]
    X, params, V0, steps = known_case(kind, idx)
    want = steps[residual]
    _assert_finite(want)
    x3, flat = dev_bf16(X, gpu).view(B, N, E), dev_params(params, gpu)
    for keep_all in (True, False):
        v0, got = mixer(x3, flat, residual, keep_all=keep_all)
        assert np.array_equal(R.plus_zero(bits(v0)), R.plus_zero(R.to_bits(V0))), f"{kind}: V0"
        for m in range(M):
            if got[m] is not None:
                bad = int((R.plus_zero(bits(got[m])) != R.plus_zero(bits(want[m]))).sum())
                assert bad == 0, f"{kind}, step {m}, keep_all={keep_all}: {bad} elements differ"


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("B,N,C,E,hg,hf,L,M", [(3, 32, 8, 8, 7, 33, 13, 4), (2, 128, 16, 32, 32, 32, 8, 5), (1, 512, 16, 64, 128, 33, 20, 3)])
def test_guard_bands_and_skipped_steps(gpu, B, N, C, E, hg, hf, L, M):
    """V0 and the step buffers carved from ONE sentinel-filled allocation, 64 bytes untouched on either side of each. Two
    alternating buffers plus one of its own for step 0: the mask skips every step a later one overwrites — step 0's buffer
    holds step 0, the others the last two — and V0 = NULL writes nothing at all."""
    from sparsefactorization_amd import _lib
    x3, flat = _random_case(gpu, B, N, C, E, hg, hf, L, M, seed=5)
    want_v0, want = two_calls(x3, flat, True)
    n = B * N * C
    stride = (n + 64 + 7) // 8 * 8  # elements: every region 16-byte aligned, >= 128 bytes of sentinel between two
    starts = [64 + i * stride for i in range(4)]  # V0, own buffer of step 0, ping, pong
    for use_v0 in (True, False):
        buf = torch.full((starts[-1] + stride,), SENTINEL, dtype=torch.int16, device=gpu)
        reg = [buf[s:s + n].view(torch.bfloat16).view(B, N, C) for s in starts]
        assert all(r.data_ptr() % 16 == 0 for r in reg)
        outs = [reg[1]] + [reg[2 + (m % 2)] for m in range(1, M)]
        _lib.check(mixer_rc(x3, flat, True, outs, V0=reg[0] if use_v0 else None), "psf_mixer_fwd_bf16")
        torch.cuda.synchronize()
        flat_bits = buf.cpu().numpy().view(np.uint16)
        inside = np.zeros(flat_bits.size, bool)
        last = {id(outs[m]): m for m in range(M)}  # the step a buffer ends up holding
        for r, s in zip(reg[1:], starts[1:]):
            m = last[id(r)]
            inside[s:s + n] = True
            _assert_same(r, want[m], f"buffer of step {m}")
        if use_v0:
            inside[starts[0]:starts[0] + n] = True
            _assert_same(reg[0], want_v0, "V0")
        assert np.all(flat_bits[~inside] == SENTINEL), "written outside the results (V0 = NULL: V0's region included)"
    # a step the mask skips is not stored anywhere: steps 0 and 2 share a buffer, step 1 has its own; V0 = NULL
    buf = torch.full((starts[-1] + stride,), SENTINEL, dtype=torch.int16, device=gpu)
    reg = [buf[s:s + n].view(torch.bfloat16).view(B, N, C) for s in starts]
    flat3 = flat[:4 * 4]  # g and three link MLPs
    _, want3 = two_calls(x3, flat3, True)
    _lib.check(mixer_rc(x3, flat3, True, [reg[1], reg[2], reg[1]], V0=None), "psf_mixer_fwd_bf16")
    torch.cuda.synchronize()
    _assert_same(reg[1], want3[2], "the shared buffer holds step 2")
    _assert_same(reg[2], want3[1], "step 1")
    keep = np.zeros(buf.numel(), bool)
    keep[starts[1]:starts[1] + n] = keep[starts[2]:starts[2] + n] = True
    assert np.all(buf.cpu().numpy().view(np.uint16)[~keep] == SENTINEL)


# ---------------------------------------------------------------- NaN / Inf containment
@pytest.mark.parametrize("residual", [False, True])
def test_nan_row_and_inf_weight_land_where_the_two_call_route_puts_them(gpu, residual):
    B, N, C, E, L, M = 3, 128, 8, 32, 12, 4
    x3, flat = _random_case(gpu, B, N, C, E, 32, 33, L, M, seed=9)
    x3 = x3.clone()
    x3[1, 37, 5] = float("nan")         # one token row of sequence 1
    flat = [p.clone() for p in flat]
    flat[4 * 2 + 2][3, 1] = float("inf")  # second-layer weight of fs[1]: link 3 of every row of step 1
    want_v0, want = _check_against_two_calls(x3, flat, residual, "NaN row + Inf weight")
    nan0 = torch.isnan(want_v0.float())
    assert bool(nan0[1, 37].all()) and int(nan0.sum()) == C  # V0: that row only
    assert not bool(torch.isfinite(want[1].float()).all())   # the Inf weight shows from step 1 on
    assert bool(torch.isfinite(want[0][0].float()).all())    # sequence 0, step 0: untouched by either


# ---------------------------------------------------------------- stale state, repeatability
def test_no_stale_state_between_calls_and_ten_identical_launches(gpu):
    big = _random_case(gpu, 2, 512, 16, 64, 128, 128, 20, 3, seed=1)
    small = _random_case(gpu, 5, 96, 8, 8, 7, 33, 4, 2, seed=2)
    fresh_big, fresh_small = mixer(*big, True), mixer(*small, False)
    ws = torch.zeros(1 << 18, dtype=torch.uint8, device=gpu)
    for rep in range(2):
        for case, fresh, res, name in ((big, fresh_big, True, "big"), (small, fresh_small, False, "small")):
            v0, steps = mixer(*case, res, ws=ws)
            _assert_same(v0, fresh[0], f"{name} after the other shape, round {rep}: V0")
            for m, (s, f) in enumerate(zip(steps, fresh[1])):
                _assert_same(s, f, f"{name} after the other shape, round {rep}: step {m}")
    x3, flat = _random_case(gpu, 8, 128, 8, 32, 32, 32, 15, 14, seed=3)
    first = mixer(x3, flat, True, keep_all=False, ws=ws)
    for rep in range(9):
        again = mixer(x3, flat, True, keep_all=False, ws=ws)
        assert torch.equal(bits_t(again[0]), bits_t(first[0])), f"launch {rep + 2}: V0"
        assert torch.equal(bits_t(again[1][-1]), bits_t(first[1][-1])), f"launch {rep + 2}: V_M"


def bits_t(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- graph capture
def test_replays_from_a_graph_with_changed_input(gpu):
    from sparsefactorization_amd import _lib
    B, N, C, E, L, M = 8, 128, 8, 32, 15, 7
    x3, flat = _random_case(gpu, B, N, C, E, 32, 32, L, M, seed=4)
    inputs = [x3] + [dev_bf16(R.random_x(B * N, E, 50 + i), gpu).view(B, N, E) for i in range(2)]
    eager = [mixer(x, flat, True, keep_all=False) for x in inputs]
    xin = x3.clone()
    bufs = [torch.empty((B, N, C), dtype=torch.bfloat16, device=gpu) for _ in range(2)]
    outs = [bufs[m % 2] for m in range(M)]
    V0 = torch.empty((B, N, C), dtype=torch.bfloat16, device=gpu)
    h, _ = _tables(flat)
    ws = torch.zeros(_lib.load().psf_mixer_fwd_bf16_workspace(N, E, M, h, C, L), dtype=torch.uint8, device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.check(mixer_rc(xin, flat, True, outs, V0, ws), "warm-up")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(mixer_rc(xin, flat, True, outs, V0, ws), "capture")  # pack + mixer on the capture stream
    for rep, (x, (e_v0, e_steps)) in enumerate(zip(inputs, eager)):
        xin.copy_(x)
        for t in (*bufs, V0):
            t.fill_(float("nan"))
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits_t(V0), bits_t(e_v0)), f"replay {rep}: V0"
        assert torch.equal(bits_t(outs[M - 1]), bits_t(e_steps[M - 1])), f"replay {rep}: V_M"
        assert torch.equal(bits_t(outs[M - 2]), bits_t(e_steps[M - 2])), f"replay {rep}: V_(M-1)"


# ---------------------------------------------------------------- the Python route
def test_python_forward_equals_the_raw_entry(gpu):
    from sparsefactorization_amd import fused_mixer
    from test_gpu_mlp_bf16 import _Block
    B, N, C, E, L, M = 3, 96, 16, 32, 13, 3
    layers = _layers(C, L, M, 33, 128)
    params = R.random_params(E, layers, seed=11)
    blocks = [_Block(ps, gpu) for ps in params]
    x3 = dev_bf16(R.random_x(B * N, E, 12), gpu).view(B, N, E)
    with torch.no_grad():
        assert fused_mixer.covered_bf16(x3, blocks[0], blocks[1:])
        assert not fused_mixer.covered_bf16(x3.float(), blocks[0], blocks[1:])
        out = fused_mixer.mixer_forward_bf16(x3, blocks[0], blocks[1:], True)
    _, want = two_calls(x3, dev_params(params, gpu), True)
    assert out.dtype == torch.bfloat16 and out.shape == (B, N, C)
    _assert_same(out, want[-1], "mixer_forward_bf16")


def test_psfnet_route_gives_the_same_bits_and_is_not_taken_under_grad(gpu, monkeypatch):
    from sparsefactorization_amd import fused_mixer
    net, x = _psfnet(gpu)
    net = net.to(torch.bfloat16)
    xb = x.to(torch.bfloat16)
    calls = []
    real = fused_mixer.mixer_forward_bf16
    monkeypatch.setattr(fused_mixer, "mixer_forward_bf16", lambda *a, **k: calls.append(1) or real(*a, **k))
    assert fused_mixer.bf16_route == "never"
    with torch.no_grad():
        never = net(xb)
        assert not calls
        monkeypatch.setattr(fused_mixer, "bf16_route", "always")
        data = net.init_linear(xb)
        assert fused_mixer.covered_bf16(data, net.g, list(net.fs))
        always = net(xb)
        assert len(calls) == 1
    assert never.dtype == always.dtype == torch.bfloat16 and bool(torch.isfinite(never.float()).all())
    assert torch.equal(bits_t(always), bits_t(never))
    out = net(xb)  # gradients enabled: the parameters want them, the inference route is not taken
    assert len(calls) == 1 and out.requires_grad
    out.float().sum().backward()
    assert net.g.network[0].weight.grad is not None
