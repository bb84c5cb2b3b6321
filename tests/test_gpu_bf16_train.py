"""GPU: the kernels and routes of graph-captured bf16 training, called directly and through the Python layer.

  psf_adam_step_master        exact known answers; master, exp_avg, exp_avg_sq bit-equal to psf_adam_step_f32 on the widened
                              gradient and inside the float64 envelope; sizes around the 4096-element chunk, the scalar path by
                              an odd bf16 offset, 41 tensors (two launches), count = 0, the device step counter
  psf_embed_tokens_bwd_bf16   every exact case of helper_cases.EMB_GRAD (an answer independent of the summation order: a
                              kernel that rounds a partial sum fails at the large T), clamped ids, random gradients against
                              the f32 entry rounded once
  psf_embed_tokens_bf16       exact integer tables, random tables against the stock bf16 expression, the grid-stride loop,
                              clamped ids, misaligned tables
  routes                      token_linear.bf16_route and make_adam(master_weights=...) — which entries a bf16 model calls
  ChunkedAdam                 step, state_dict, torch.save, load, load_state_dict, step == two uninterrupted steps, bit for bit

Every array the Adam entry touches sits between sentinel bands that must come back unchanged; the embedding outputs and
workspaces sit between NaN bands and are pre-filled with NaN (tests/test_gpu_helpers_exact.py's form). The graph tests are in
tests/test_gpu_graph_bf16_train.py.
"""
import ctypes
import io

import numpy as np
import pytest
import torch

import adam_cases as ac
import helper_cases as hc
import test_gpu_guard_bands as gb

pytestmark = pytest.mark.gpu

BAND = 128  # elements on either side: 512 bytes of f32, 256 of bf16 (the view stays 16-byte aligned)
SENTINEL = -1234.5
E_ALIGN = -4
BF16 = torch.bfloat16


def _libs(gpu):
    from sparsefactorization_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream(gpu).cuda_stream


def _bits(t):
    """The raw bits of an f32 or bf16 tensor as a numpy integer array."""
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, what
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"


class Banded:
    """``values`` (numpy f32 or a torch tensor) as a device view of ``dtype`` between sentinel bands, ``shift`` elements off
    the aligned position."""

    def __init__(self, values, dtype, gpu, shift=0):
        src = torch.from_numpy(np.ascontiguousarray(values)) if isinstance(values, np.ndarray) else values
        n = src.numel()
        self.buf = torch.full((n + 2 * BAND + 8,), SENTINEL, dtype=dtype, device=gpu)
        self.lo, self.hi = BAND + shift, BAND + shift + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(src.reshape(-1).to(gpu))
        assert self.buf.data_ptr() % 16 == 0
        self.before = self.buf.clone()

    def ptr(self):
        return self.buf.data_ptr() + self.lo * self.buf.element_size()  # (an empty view has no data_ptr)

    def bands_untouched(self):
        a, b = _bits(self.buf), _bits(self.before)
        return np.array_equal(a[:self.lo], b[:self.lo]) and np.array_equal(a[self.hi:], b[self.hi:])

    def unchanged(self):
        return np.array_equal(_bits(self.buf), _bits(self.before))


# ================================================================================================ Adam
def _hyper_args(h):
    return h["lr"], h["beta1"], h["beta2"], h["eps"]


def _tab(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _master_step(gpu, tensors, h, step, step_dev=None):
    """tensors: a list of (master, param, grad, m, v) Banded. One psf_adam_step_master call over the list."""
    _lib, lib, s = _libs(gpu)
    n = len(tensors)
    tabs = [_tab([t[j].ptr() for t in tensors]) for j in range(5)]
    sizes = (ctypes.c_int64 * max(n, 1))(*[t[0].hi - t[0].lo for t in tensors])
    rc = lib.psf_adam_step_master(*tabs, sizes, n, *_hyper_args(h), float(step), None if step_dev is None else step_dev.data_ptr(), s)
    _lib.check(rc, "psf_adam_step_master")


def _f32_step(gpu, tensors, h, step, step_dev=None):
    """tensors: a list of (p, g, m, v) device tensors. One psf_adam_step_f32 call."""
    _lib, lib, s = _libs(gpu)
    n = len(tensors)
    tabs = [_tab([t[j].data_ptr() if t[j].numel() else 256 for t in tensors]) for j in range(4)]
    sizes = (ctypes.c_int64 * max(n, 1))(*[t[0].numel() for t in tensors])
    rc = lib.psf_adam_step_f32(*tabs, sizes, n, *_hyper_args(h), float(step), None if step_dev is None else step_dev.data_ptr(), s)
    _lib.check(rc, "psf_adam_step_f32")


def _master_operands(gpu, p, g_bf16, m, v, shifts=(0, 0, 0, 0, 0), seed=0):
    """(master, param, grad, m, v) Banded; the parameter starts as noise (the entry overwrites it, never reads it)."""
    noise = torch.from_numpy(np.random.default_rng(seed).standard_normal(p.size).astype(np.float32)).to(BF16)
    return (Banded(p, torch.float32, gpu, shifts[0]), Banded(noise, BF16, gpu, shifts[1]), Banded(g_bf16, BF16, gpu, shifts[2]),
            Banded(m, torch.float32, gpu, shifts[3]), Banded(v, torch.float32, gpu, shifts[4]))


def _check_bands_and_param(ops, what):
    master, param, grad, m, v = ops
    for name, b in zip(("master", "param", "grad", "exp_avg", "exp_avg_sq"), ops):
        assert b.bands_untouched(), f"{what}: the bands around {name} were written"
    assert grad.unchanged(), f"{what}: the gradient was written"
    _same(param.view, master.view.to(BF16), f"{what}: param == rne_bf16(master')")  # torch's cast: nearest even, NaN kept


def _rne_bf16_bits(x):
    """float32 array -> int16 bits of its bfloat16 rounding (nearest, ties to even), independent of torch's cast."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


@pytest.mark.parametrize("path", ["vector", "scalar_grad_offset", "scalar_size"])
@pytest.mark.parametrize("zero_gradient", [False, True], ids=["first_step_rule", "zero_gradient"])
def test_master_step_known_answers_bit_for_bit(gpu, zero_gradient, path):
    """adam_cases.known_answer restricted to the gradients +-2k that bf16 holds exactly (2k with at most 8 significant bits):
    master' = p - 2^-7 sign(g), m' = g / 2, v' = g^2 / 4 bit for bit, and the parameter is rne_bf16(master')."""
    p, g, m, v, h, wp, wm, wv = ac.known_answer(zero_gradient)
    g_bf16 = torch.from_numpy(g).to(BF16)
    keep = (g_bf16.float().numpy() == g)
    assert 600 < int(keep.sum()) < g.size or zero_gradient  # a real restriction: most of k <= 1024 is not a bf16 value
    p, g, m, v, wp, wm, wv = (a[keep] for a in (p, g, m, v, wp, wm, wv))
    n = p.size // 4 * 4 - (1 if path == "scalar_size" else 0)
    p, g, m, v, wp, wm, wv = (a[:n] for a in (p, g, m, v, wp, wm, wv))
    g_bf16 = torch.from_numpy(g).to(BF16)
    assert np.array_equal(g_bf16.float().numpy(), g), "the gradients must pass through bf16 unchanged"
    shifts = (0, 0, 1, 0, 0) if path == "scalar_grad_offset" else (0, 0, 0, 0, 0)
    ops = _master_operands(gpu, p, g_bf16, m, v, shifts)
    _master_step(gpu, [ops], ac.hyper(**h), 1)
    for name, got, want in zip(("master", "exp_avg", "exp_avg_sq"), (ops[0], ops[3], ops[4]), (wp, wm, wv)):
        bad = int((_bits(got.view) != want.view(np.int32)).sum())
        assert bad == 0, f"{name}': {bad} of {n} elements differ"
    assert np.array_equal(_bits(ops[1].view), _rne_bf16_bits(wp)), "param != rne_bf16(master')"
    _check_bands_and_param(ops, path)


@pytest.mark.parametrize("t", ac.STEPS)
def test_master_step_has_the_bits_of_the_f32_step_and_sits_inside_the_envelope(gpu, t):
    """The operands of the f32 envelope test with g rounded to bf16 first: psf_adam_step_master on (master, g_bf16) and
    psf_adam_step_f32 on (master.clone(), g_bf16.float()) — one template body — give the same bits, inside adam_cases.bounds
    (factor 1, as tests/test_gpu_adam.py)."""
    h = ac.hyper()
    p, g, m, v = ac.operands(t)
    g_bf16 = torch.from_numpy(g).to(BF16)
    g_wide = g_bf16.float().numpy()
    ops = _master_operands(gpu, p, g_bf16, m, v)
    _master_step(gpu, [ops], h, t)
    ref = [torch.from_numpy(a.copy()).to(gpu) for a in (p, g_wide, m, v)]
    _f32_step(gpu, [ref], h, t)
    for name, got, want in zip(("master", "exp_avg", "exp_avg_sq"), (ops[0], ops[3], ops[4]), (ref[0], ref[2], ref[3])):
        _same(got.view, want, f"{name} against psf_adam_step_f32 at t = {t}")
    _check_bands_and_param(ops, f"t = {t}")
    want, E = ac.bounds(p, g_wide, m, v, h, t)
    got = tuple(b.view.cpu().numpy() for b in (ops[0], ops[3], ops[4]))
    assert all(np.isfinite(a).all() for a in got)
    wp, wm, wv = ac.worst(got, want, E)
    print(f"ADAM_MASTER_ENVELOPE t={t}: of the bound p {wp:.3f} m {wm:.3f} v {wv:.3f}")
    assert wm <= 1.0 and wv <= 1.0 and wp <= 1.0, (wp, wm, wv)


def _random_ops(n, seed):
    rng = np.random.default_rng([11, seed, n])
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    return (rng.standard_normal(n).astype(np.float32), torch.from_numpy(g).to(BF16), (0.1 * rng.standard_normal(n)).astype(np.float32),
            (rng.standard_normal(n) ** 2 + 1e-6).astype(np.float32))


def _against_f32(gpu, tensors, raw, h, step, what):
    """Every tensor of a master call against psf_adam_step_f32 on the same operands with the gradient widened."""
    ref = [[torch.from_numpy(p.copy()).to(gpu), g.float().to(gpu), torch.from_numpy(m.copy()).to(gpu), torch.from_numpy(v.copy()).to(gpu)]
           for p, g, m, v in raw]
    for r in ref:
        if r[0].numel():
            _f32_step(gpu, [r], h, step)
    for k, (ops, r) in enumerate(zip(tensors, ref)):
        for name, got, want in zip(("master", "exp_avg", "exp_avg_sq"), (ops[0], ops[3], ops[4]), (r[0], r[2], r[3])):
            _same(got.view, want, f"{what}: {name} of tensor {k} (n = {r[0].numel()})")
        _check_bands_and_param(ops, f"{what}, tensor {k}")
        if r[0].numel():
            assert not np.array_equal(_bits(ops[0].view), _bits(ops[0].before[ops[0].lo:ops[0].hi])), f"{what}: tensor {k} was not updated"


@pytest.mark.parametrize("shifts", [(0, 0, 0, 0, 0), (0, 1, 1, 0, 0), (0, 0, 1, 0, 0), (1, 2, 2, 1, 1), (0, 4, 0, 0, 0)],
                         ids=["aligned", "bf16_odd_offset", "grad_odd_offset", "f32_one_float_off", "param_8_byte_aligned"])
@pytest.mark.parametrize("n", [1, 3, 4, 4095, 4096, 4097, 8200])
def test_master_step_sizes_and_alignments(gpu, n, shifts):
    """Sizes around the 4096-element chunk on the vector path (f32 arrays 16-byte, bf16 arrays 8-byte aligned, n % 4 == 0: the
    bf16 parameter 4 elements off still qualifies) and on the scalar path (a bf16 view at an odd element offset, an f32 view one
    float off, n % 4 != 0): the f32 entry's bits, the rounded parameter, nothing outside the arrays."""
    raw = _random_ops(n, 1)
    ops = _master_operands(gpu, *raw, shifts=shifts)
    assert ops[1].ptr() % 16 == 2 * shifts[1] and ops[0].ptr() % 16 == 4 * shifts[0]
    _master_step(gpu, [ops], ac.hyper(), 3)
    _against_f32(gpu, [ops], [raw], ac.hyper(), 3, f"n = {n}")


def test_master_step_over_41_tensors_is_two_launches(gpu):
    """40 tensors go into a launch: the 41st is a launch of its own. Sizes around the chunk, empty tensors among them, aligned
    and not, in one call; every tensor gets the bits it gets from the f32 entry alone."""
    sizes = [(1, 3, 4, 4095, 4096, 4097, 8200, 0, 12, 100)[(3 * k + 1) % 10] for k in range(41)]
    sizes[0], sizes[39], sizes[40] = 4097, 0, 8200
    all_shifts = ((0, 0, 0, 0, 0), (0, 1, 1, 0, 0), (1, 0, 0, 1, 1), (0, 4, 4, 0, 0))
    raw = [_random_ops(n, 100 + k) for k, n in enumerate(sizes)]
    tensors = [_master_operands(gpu, *r, shifts=all_shifts[k % 4], seed=k) for k, r in enumerate(raw)]
    _master_step(gpu, tensors, ac.hyper(), 5)
    _against_f32(gpu, tensors, raw, ac.hyper(), 5, "41 tensors")


def test_master_step_with_count_zero_does_nothing(gpu):
    _lib, lib, s = _libs(gpu)
    raw = _random_ops(100, 2)
    ops = _master_operands(gpu, *raw)
    tabs = [_tab([b.ptr()]) for b in ops]
    assert lib.psf_adam_step_master(*tabs, (ctypes.c_int64 * 1)(100), 0, *_hyper_args(ac.hyper()), 1.0, None, s) == 0
    assert lib.psf_adam_step_master(None, None, None, None, None, None, 0, *_hyper_args(ac.hyper()), 0.0, None, s) == 0
    torch.cuda.synchronize(gpu)
    assert all(b.unchanged() for b in ops)


def test_master_step_device_counter_gives_the_bits_of_the_host_counter(gpu):
    """Three steps with the count read from a device scalar (advanced between the calls, as ChunkedAdam(capturable=True) does;
    the host argument, 99, must be ignored) against three steps with the host count."""
    h = ac.hyper()
    raws = [_random_ops(n, 7 + n) for n in (4096, 77)]
    grads = [[torch.from_numpy(np.random.default_rng([5, k, t]).standard_normal(r[0].size).astype(np.float32)).to(BF16) for t in range(3)]
             for k, r in enumerate(raws)]
    runs = []
    for device_counter in (False, True):
        tensors = [_master_operands(gpu, *r) for r in raws]
        step_dev = torch.zeros((), device=gpu)
        for t in range(3):
            for ops, gs in zip(tensors, grads):
                ops[2].view.copy_(gs[t].to(gpu))
            if device_counter:
                step_dev.add_(1.0)
                _master_step(gpu, tensors, h, 99, step_dev=step_dev)
            else:
                _master_step(gpu, tensors, h, t + 1)
        runs.append(tensors)
    for k, (a, b) in enumerate(zip(*runs)):
        for j, name in ((0, "master"), (1, "param"), (3, "exp_avg"), (4, "exp_avg_sq")):
            _same(b[j].view, a[j].view, f"{name} of tensor {k}: device counter against host counter")
            assert b[j].bands_untouched()


# ================================================================================================ embedding gradient
def _nan_banded(shape, dtype, gpu):
    """(buffer, view, span): ``shape`` of ``dtype`` pre-filled with NaN between NaN bands, the view 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND,), float("nan"), dtype=dtype, device=gpu)
    return buf, buf[BAND:BAND + n].view(*shape), (BAND, BAND + n)


def _bf16_input(a, gpu):
    """A numpy f32 array as a bf16 device tensor between NaN bands (a read past its ends that is USED shows as NaN)."""
    _, view, _ = _nan_banded(a.shape, BF16, gpu)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(BF16))
    return view


def _embed_bwd_bf16(gpu, T, V, E, idx, dout, want_bits_of, what):
    """Two runs of psf_embed_tokens_bwd_bf16 into NaN-filled, banded dTable and workspace: the expected bits, twice."""
    _lib, lib, s = _libs(gpu)
    nbytes = lib.psf_embed_tokens_bwd_workspace(T, V, E)
    assert nbytes > 0
    for run in range(2):
        table = _nan_banded((V, E), BF16, gpu)
        ws = gb._banded((nbytes // 4,), gpu)
        _lib.check(lib.psf_embed_tokens_bwd_bf16(idx.data_ptr(), dout.data_ptr(), T, V, E, table[1].data_ptr(), ws[1].data_ptr(), nbytes, s),
                   "psf_embed_tokens_bwd_bf16")
        assert gb._bands_intact(table[0].float(), table[2]), f"{what}: a NaN band of dTable was written, or dTable holds NaN"
        lo, hi = ws[2]
        assert bool(torch.isnan(ws[0][:lo]).all()) and bool(torch.isnan(ws[0][hi:]).all()), f"{what}: written outside the workspace"
        _same(table[1], want_bits_of, f"{what} (run {run})")
    return table[1]


def _exact_grad_case(gpu, case, idx_np, want_i64):
    dout_np = case.dout()
    assert np.abs(dout_np).max() <= 4  # exact in bf16
    dout = _bf16_input(dout_np, gpu)
    assert np.array_equal(dout.float().cpu().numpy(), dout_np)
    want = torch.from_numpy(hc.as_f32(want_i64)).to(BF16)  # the exact sum, rounded once: independent of the summation order
    return _embed_bwd_bf16(gpu, case.T, case.V, case.E, torch.from_numpy(idx_np).to(gpu), dout, want, case.id)


@pytest.mark.parametrize("case", hc.EMB_GRAD, ids=[c.id for c in hc.EMB_GRAD])
def test_bf16_embedding_gradient_is_the_exact_sum_rounded_once(gpu, case):
    idx = case.idx()
    got = _exact_grad_case(gpu, case, idx, case.expected(idx=idx))
    named = np.zeros(case.V, dtype=bool)
    named[idx] = True
    if not named.all():  # rows no token names: +0.0 out of a workspace and an output full of NaN
        assert not got[torch.from_numpy(~named).to(gpu)].view(torch.int16).any()


@pytest.mark.parametrize("case", hc.EMB_GRAD_CLAMPED, ids=[c.id for c in hc.EMB_GRAD_CLAMPED])
def test_bf16_embedding_gradient_clamps_ids_outside_the_table(gpu, case):
    """Ids -2, -1, V, V + 1 (first and last token among them): rows 0 and V - 1 receive those tokens, nothing lands in the NaN
    bands beside dTable."""
    bad = hc.with_out_of_range_ids(case.idx(), case.V, seed=3)
    assert bad.min() == -2 and bad.max() == case.V + 1
    _exact_grad_case(gpu, case, bad, case.expected(idx=np.clip(bad, 0, case.V - 1)))


@pytest.mark.parametrize("T,V,E", [(999, 193, 5), (4096, 512, 64), (300, 4, 4096)])
def test_bf16_embedding_gradient_is_the_f32_entry_rounded_once(gpu, T, V, E):
    _lib, lib, s = _libs(gpu)
    gen = torch.Generator().manual_seed(T + V + E)
    idx = torch.randint(0, V, (T,), generator=gen).to(gpu)
    dout = _bf16_input(torch.randn(T, E, generator=gen).numpy(), gpu)
    wide = dout.float().contiguous()
    nbytes = lib.psf_embed_tokens_bwd_workspace(T, V, E)
    ws = torch.empty(nbytes // 4, device=gpu)
    ref = torch.full((V, E), float("nan"), device=gpu)
    _lib.check(lib.psf_embed_tokens_bwd_f32(idx.data_ptr(), wide.data_ptr(), T, V, E, ref.data_ptr(), ws.data_ptr(), nbytes, s),
               "psf_embed_tokens_bwd_f32")
    _embed_bwd_bf16(gpu, T, V, E, idx, dout, ref.to(BF16), f"T{T}-V{V}-E{E}")


# ================================================================================================ embedding forward
FWD_SHAPES = [(1, 1, 1, 8, False), (3, 7, 6, 8, True), (7, 10000, 6, 256, True), (2, 2049, 512, 32, False)]  # (B, N, V, E, pos)
FWD_IDS = ["B1-N1-V1-E8-nopos", "B3-N7-V6-E8-pos", "B7-N10000-V6-E256-pos", "B2-N2049-V512-E32-nopos"]


def _ints(seed, bound, shape):
    return np.random.default_rng(seed).integers(-bound, bound + 1, size=shape).astype(np.float32)


def _embed_fwd_bf16(gpu, idx, table, pos, B, N, V, E):
    _lib, lib, s = _libs(gpu)
    out = _nan_banded((B * N, E), BF16, gpu)
    _lib.check(lib.psf_embed_tokens_bf16(idx.data_ptr(), table.data_ptr(), None if pos is None else pos.data_ptr(), out[1].data_ptr(),
                                         B * N, N, V, E, s), "psf_embed_tokens_bf16")
    assert gb._bands_intact(out[0].float(), out[2]), "a NaN band of out was written, or out holds NaN"
    return out[1]


@pytest.mark.parametrize("B,N,V,E,with_pos", FWD_SHAPES, ids=FWD_IDS)
def test_bf16_embedding_forward(gpu, B, N, V, E, with_pos):
    """Integer tables |.| <= 127: every sum is an integer of at most 254, exact in bf16 — the int64 answer, bit for bit.
    Random tables: the bits of the stock ``F.embedding(idx, w) + pos`` on bf16 tensors."""
    if (B, N) == (7, 10000):
        assert B * N * E // 8 > hc.STRIDE_GRID * hc.STRIDE_THREADS  # more vectors than threads: the grid-stride loop runs
    idx_np = np.random.default_rng([3, B, N, V]).integers(0, V, B * N, dtype=np.int64)
    idx = torch.from_numpy(idx_np).to(gpu)
    tab_np, pos_np = _ints([4, V, E], 127, (V, E)), _ints([5, N, E], 127, (N, E)) if with_pos else None
    want = tab_np.astype(np.int64)[idx_np]
    if with_pos:
        want = want + pos_np.astype(np.int64)[np.arange(B * N) % N]
    assert np.abs(want).max() <= 256
    got = _embed_fwd_bf16(gpu, idx, _bf16_input(tab_np, gpu), _bf16_input(pos_np, gpu) if with_pos else None, B, N, V, E)
    _same(got, torch.from_numpy(want.astype(np.float32)).to(BF16), "integer tables")

    gen = torch.Generator().manual_seed(B + N + V + E)
    table = _bf16_input(torch.randn(V, E, generator=gen).numpy(), gpu)
    pos = _bf16_input(torch.randn(N, E, generator=gen).numpy(), gpu) if with_pos else None
    stock = torch.nn.functional.embedding(idx.view(B, N), table)
    if with_pos:
        stock = stock + pos.unsqueeze(0)
    assert stock.dtype == BF16
    _same(_embed_fwd_bf16(gpu, idx, table, pos, B, N, V, E), stock.reshape(B * N, E), "random tables against the stock expression")


def _between_nan_rows(a, gpu):
    """``a`` [rows, E] as a bf16 view with CLAMP_BAND_ROWS rows of NaN on either side, inside one allocation."""
    rows, E = a.shape
    buf = torch.full((rows + 2 * hc.CLAMP_BAND_ROWS, E), float("nan"), dtype=BF16, device=gpu)
    view = buf[hc.CLAMP_BAND_ROWS:hc.CLAMP_BAND_ROWS + rows]
    view.copy_(torch.from_numpy(a).to(BF16))
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("case", hc.EMB_FWD_CLAMPED, ids=[c.id for c in hc.EMB_FWD_CLAMPED])
def test_bf16_embedding_forward_clamps_ids_outside_the_table(gpu, case):
    """Ids -2, -1, V, V + 1 read row 0 / row V - 1; the table and the positional rows sit between NaN rows of their own
    allocation, so a missing clamp shows as NaN, never as a read of foreign memory."""
    B, N, V, E = case.B, case.N, case.V, case.E
    assert E % 8 == 0
    bad = hc.with_out_of_range_ids(case.idx(), V, seed=2)
    assert bad.min() == -2 and bad.max() == V + 1
    tab_np, pos_np = _ints([6, V, E], 127, (V, E)), _ints([7, N, E], 127, (N, E)) if case.pos else None
    want = tab_np.astype(np.int64)[np.clip(bad, 0, V - 1)]
    if case.pos:
        want = want + pos_np.astype(np.int64)[np.arange(case.T) % N]
    got = _embed_fwd_bf16(gpu, torch.from_numpy(bad).to(gpu), _between_nan_rows(tab_np, gpu),
                          _between_nan_rows(pos_np, gpu) if case.pos else None, B, N, V, E)
    _same(got, torch.from_numpy(want.astype(np.float32)).to(BF16), "clamped ids")


def _misaligned_table(V, E, gpu, seed):
    """A contiguous [V, E] bf16 view two bytes off a 16-byte boundary."""
    buf = torch.zeros(V * E + 8, dtype=BF16, device=gpu)
    view = buf[1:1 + V * E].view(V, E)
    view.copy_(torch.randn(V, E, generator=torch.Generator().manual_seed(seed)).to(BF16))
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    return view


def test_bf16_embedding_forward_refuses_a_misaligned_table_and_embed_tokens_routes_around_it(gpu, monkeypatch):
    from sparsefactorization_amd import token_linear
    from test_gpu_model_twin import Spy
    _lib, lib, s = _libs(gpu)
    B, N, V, E = 2, 5, 6, 16
    idx = torch.randint(0, V, (B, N), generator=torch.Generator().manual_seed(1)).to(gpu)
    table = _misaligned_table(V, E, gpu, 2)
    out = torch.zeros(B * N, E, dtype=BF16, device=gpu)
    assert lib.psf_embed_tokens_bf16(idx.data_ptr(), table.data_ptr(), None, out.data_ptr(), B * N, N, V, E, s) == E_ALIGN
    torch.cuda.synchronize(gpu)
    assert not out.view(torch.int16).any()

    monkeypatch.setattr(token_linear, "bf16_route", "always")
    pos = torch.randn(N, E, generator=torch.Generator().manual_seed(3)).to(BF16).to(gpu)
    emb = token_linear.TokenEmbedding(V, E).to(gpu).to(BF16)
    spy = Spy(monkeypatch)
    for weight, calls in ((table, 0), (table.clone(), 1)):  # the misaligned view: the stock path; an aligned copy: the kernel
        emb.weight = torch.nn.Parameter(weight)
        spy.reset()
        got = token_linear.embed_tokens(idx, emb, pos)
        assert spy.calls["psf_embed_tokens_bf16"] == calls
        _same(got, torch.nn.functional.embedding(idx, weight) + pos.unsqueeze(0), f"embed_tokens with {calls} kernel calls")
    emb.weight = torch.nn.Parameter(table.clone())
    spy.reset()
    token_linear.embed_tokens(idx, emb, _misaligned_table(N, E, gpu, 4))  # a misaligned pos: the stock path too
    assert spy.calls["psf_embed_tokens_bf16"] == 0


# ================================================================================================ routes
def _order_net(gpu, n_vec=128, seed=0):
    from sparsefactorization_amd import psf_training
    torch.manual_seed(seed)
    return psf_training.build_model("order", n_vec, use_cuda=False).to(gpu).to(BF16)


def _order_batch(gpu, B, n_vec, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, 6, (B, n_vec, 1), generator=gen).to(gpu), torch.randint(0, 4, (B,), generator=gen).to(gpu)


@pytest.mark.parametrize("route", ["never", "always"])
def test_which_entries_a_bf16_model_calls(gpu, monkeypatch, route):
    """At the defaults a bf16 Temporal-Order model calls none of the three entries (stock lookup, the aten table gradient,
    torch's Adam): nothing changed for it. With bf16_route = "always" and master_weights=True each is called once per step,
    and the f32 entries they stand in for are not."""
    from sparsefactorization_amd import token_linear
    from sparsefactorization_amd.train import ChunkedAdam, make_adam
    from test_gpu_model_twin import Spy
    assert token_linear.bf16_route == "never"
    monkeypatch.setattr(token_linear, "bf16_route", route)
    net = _order_net(gpu)
    opt = make_adam(net.parameters(), 1e-3, master_weights=route == "always")
    assert isinstance(opt, ChunkedAdam) == (route == "always")
    X, Y = _order_batch(gpu, 8, 128)
    loss = torch.nn.CrossEntropyLoss()
    spy = Spy(monkeypatch)
    for step in range(2):
        spy.reset()
        opt.zero_grad()
        loss(net(X).squeeze(), Y).backward()
        opt.step()
        want = 1 if route == "always" else 0
        for entry in ("psf_embed_tokens_bf16", "psf_embed_tokens_bwd_bf16", "psf_adam_step_master"):
            assert spy.calls[entry] == want, (step, entry, spy.calls[entry])
        for entry in ("psf_embed_tokens_f32", "psf_embed_tokens_bwd_f32", "psf_adam_step_f32"):
            assert spy.calls[entry] == 0, (step, entry)
    assert net.embedding.weight.grad.dtype == BF16 and net.pos_embedding.weight.grad.dtype == BF16


def _ulp_bf16(x):
    """The spacing of bf16 values at |x| (float64 array): 2^(floor(log2 |x|) - 7), from the smallest normal up."""
    ax = np.maximum(np.abs(x), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


def test_embedding_and_positional_gradients_on_the_bf16_route(gpu, monkeypatch):
    """embed_tokens at "always": d(embedding.weight) and d(pos) against a float64 recomputation from the same bf16 d(out),
    each within one bf16 ulp of the float64 value (the kernel's f32 sum rounded once is within half an ulp plus the f32 sum's
    own error; pos's is torch's bf16 batch sum)."""
    from sparsefactorization_amd import token_linear
    monkeypatch.setattr(token_linear, "bf16_route", "always")
    B, N, V, E = 5, 24, 6, 16
    gen = torch.Generator().manual_seed(9)
    emb = token_linear.TokenEmbedding(V, E).to(gpu).to(BF16)
    pos = torch.randn(N, E, generator=gen).to(BF16).to(gpu).requires_grad_(True)
    idx = torch.randint(0, V, (B, N), generator=gen).to(gpu)
    dout = torch.randn(B, N, E, generator=gen).to(BF16).to(gpu)
    out = token_linear.embed_tokens(idx, emb, pos)
    assert out.dtype == BF16 and out.grad_fn is not None and "EmbedTokensFn" in type(out.grad_fn).__name__
    out.backward(dout)
    d64 = dout.double().cpu().numpy()
    want_w = np.zeros((V, E))
    np.add.at(want_w, idx.cpu().numpy().reshape(-1), d64.reshape(-1, E))
    want_pos = d64.sum(0)
    for name, got, want in (("embedding.weight", emb.weight.grad, want_w), ("pos", pos.grad, want_pos)):
        assert got.dtype == BF16 and tuple(got.shape) == want.shape
        err = np.abs(got.double().cpu().numpy() - want) / _ulp_bf16(want)
        print(f"BF16_ROUTE_GRAD {name}: worst error {err.max():.3f} bf16 ulp")
        assert err.max() <= 1.0, name


def test_padding_row_gradient_is_zero_on_the_bf16_route(gpu, monkeypatch):
    from sparsefactorization_amd import token_linear
    from test_gpu_model_twin import Spy
    monkeypatch.setattr(token_linear, "bf16_route", "always")
    V, E, pad = 7, 12, 2
    emb = token_linear.TokenEmbedding(V, E, padding_idx=pad).to(gpu).to(BF16)
    gen = torch.Generator().manual_seed(4)
    idx = torch.randint(0, V, (3, 50), generator=gen).to(gpu)
    assert int((idx == pad).sum()) > 0
    spy = Spy(monkeypatch)
    out = emb(idx)
    dout = torch.randn(3, 50, E, generator=gen).to(BF16).to(gpu)
    out.backward(dout)
    assert spy.calls["psf_embed_tokens_bwd_bf16"] == 1
    g = emb.weight.grad
    assert g.dtype == BF16 and not g[pad].view(torch.int16).any()
    want = torch.zeros(V, E, dtype=torch.float64, device=gpu).index_add_(0, idx.reshape(-1), dout.double().reshape(-1, E))
    want[pad] = 0
    err = np.abs((g.double() - want).cpu().numpy()) / _ulp_bf16(want.cpu().numpy())
    assert err.max() <= 1.0


# ================================================================================================ state round trip
@pytest.mark.parametrize("capturable", [False, True])
def test_state_round_trip_continues_bit_for_bit(gpu, capturable):
    """step, state_dict, torch.save, load, load_state_dict, step on a mixed f32 + bf16 list == two uninterrupted steps."""
    from sparsefactorization_amd.train import ChunkedAdam
    gen = torch.Generator().manual_seed(12)
    shapes = [((33, 7), BF16), ((4096,), torch.float32), ((5,), BF16), ((8, 16), torch.float32), ((4100,), BF16)]
    start = [torch.randn(*shape, generator=gen).to(dt).to(gpu) for shape, dt in shapes]
    grads = [[torch.randn(*shape, generator=gen).to(dt).to(gpu) for shape, dt in shapes] for _ in range(2)]

    def fresh():
        params = [torch.nn.Parameter(t.clone()) for t in start]
        return params, ChunkedAdam(params, lr=1e-2, capturable=capturable)

    def step(params, opt, t):
        for p, g in zip(params, grads[t]):
            p.grad = g.clone()
        opt.step()

    pa, oa = fresh()
    step(pa, oa, 0)
    step(pa, oa, 1)

    pb, ob = fresh()
    step(pb, ob, 0)
    blob = io.BytesIO()
    torch.save({"opt": ob.state_dict(), "params": [p.detach() for p in pb]}, blob)
    blob.seek(0)
    saved = torch.load(blob)
    pc = [torch.nn.Parameter(t.clone()) for t in saved["params"]]
    oc = ChunkedAdam(pc, lr=1e-2, capturable=capturable)
    oc.load_state_dict(saved["opt"])
    for p in pc:
        if p.dtype == BF16:
            assert all(oc.state[p][k].dtype == torch.float32 and oc.state[p][k].is_cuda for k in ChunkedAdam.MASTER_STATE)
    step(pc, oc, 1)
    for k, (a, c) in enumerate(zip(pa, pc)):
        _same(c, a, f"parameter {k}")
        assert not np.array_equal(_bits(a), _bits(start[k])), f"parameter {k} did not move"
        names = ChunkedAdam.MASTER_STATE if a.dtype == BF16 else ChunkedAdam.MASTER_STATE[1:]
        assert set(oa.state[a]) == set(names) | {"step"}
        for name in names:
            _same(oc.state[c][name], oa.state[a][name], f"{name} of parameter {k}")
        assert float(oc.state[c]["step"]) == float(oa.state[a]["step"]) == 2.0
        if a.dtype == BF16:
            _same(a, oa.state[a]["master"].to(BF16), f"parameter {k} is its master, rounded")
