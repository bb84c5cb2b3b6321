"""CPU: the host side of graph-captured bf16 training — nothing here launches a kernel.

  a. psf_adam_step_master, psf_embed_tokens_bf16 and psf_embed_tokens_bwd_bf16 are exported and bound, and refuse NULL, shape
     and alignment errors with the documented codes before any launch (every pointer here is fake: a call that got past its
     checks would launch on it, so only refused calls and the documented no-ops — count = 0, T = 0 — are made)
  b. ChunkedAdam.load_state_dict puts the f32 master and moments of a bf16 parameter back as f32 with their saved bits
     (torch's own casts them to the parameter's dtype), and ``step`` follows the capturable rule
  c. make_adam's routing (default against master_weights=True; double, CPU and mixed parameter lists) and, on a stub library,
     which entry a mixed f32 / bf16 list reaches with which tables; f16 is a TypeError
  d. the reason for master weights, as arithmetic: torch's Adam on a bf16 parameter at 1.0 never moves it, the master rule does;
     and the exact embedding-gradient cases the GPU test uses do leave bf16's precision
  e. train.check_capturable admits a bf16 TokenEmbedding only at token_linear.bf16_route = "always"
"""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as ac

NEW_ENTRIES = ("psf_adam_step_master", "psf_embed_tokens_bf16", "psf_embed_tokens_bwd_bf16")
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---------------------------------------------------------------------------------------------- a. boundary
def test_the_three_entries_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), f"libpsf_chord.so does not export {name}"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    # the bf16 instances take the arguments of their f32 neighbours; the master step has one pointer table more
    for a, b, more in (("psf_embed_tokens_bf16", "psf_embed_tokens_f32", 0), ("psf_embed_tokens_bwd_bf16", "psf_embed_tokens_bwd_f32", 0),
                       ("psf_adam_step_master", "psf_adam_step_f32", 1)):
        assert len(_lib.SIGNATURES[a][0]) == len(_lib.SIGNATURES[b][0]) + more and _lib.SIGNATURES[a][1] is ctypes.c_int
    # positions whose element type is not the one the name ends in (int64 ids, the f32 workspace; everything of the entry that
    # ends in no type) are bound as DeviceAddr / DeviceAddrTable, never as a plain c_void_p
    assert _lib.SIGNATURES["psf_embed_tokens_bf16"][0][0] is _lib.DeviceAddr
    assert [i for i, t in enumerate(_lib.SIGNATURES["psf_embed_tokens_bwd_bf16"][0]) if t is _lib.DeviceAddr] == [0, 6]
    master = _lib.SIGNATURES["psf_adam_step_master"][0]
    assert master[:5] == [_lib.DeviceAddrTable] * 5 and master[-2:] == [_lib.DeviceAddr] * 2
    assert not any(t in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)) for t in master)
    assert lib.psf_version() == 2


def test_master_step_is_validated_in_full_before_the_first_launch(lib):
    """The form of test_adam_step_is_validated_in_full_before_the_first_launch (test_abi_host.py): a fault behind the first 40
    (or 80) tensors comes back as its code with nothing launched. Tables: master, params_bf16, grads_bf16, exp_avg, exp_avg_sq."""
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    f = lib.psf_adam_step_master
    hyper = (1e-3, 0.9, 0.999, 1e-8)

    def tables(count, fault=None, at=None):
        tabs = [[4096 + 64 * (5 * k + j) for k in range(count)] for j in range(5)]
        sizes = [16] * count
        if fault is not None and fault.startswith("null"):
            tabs[int(fault[-1])][at] = None
        elif fault == "align_f32":    # an f32 array two bytes off
            tabs[3][at] += 2
        elif fault == "align_master":
            tabs[0][at] += 2
        elif fault == "align_param":  # a bf16 array one byte off
            tabs[1][at] += 1
        elif fault == "align_grad":
            tabs[2][at] += 1
        elif fault == "negative":
            sizes[at] = -1
        elif fault == "blocks":  # 2^31 - 1 workgroups of 4096 elements, and one more, inside one launch
            sizes[at - 1], sizes[at] = 4096 * (2 ** 31 - 1), 1
        return [(vp * max(count, 1))(*t) for t in tabs] + [(i64 * max(count, 1))(*sizes)]

    faults = [(f"null{j}", E_NULL) for j in range(5)] + [("negative", E_NULL), ("align_f32", E_ALIGN), ("align_master", E_ALIGN),
                                                         ("align_param", E_ALIGN), ("align_grad", E_ALIGN), ("blocks", E_SHAPE)]
    for fault, code in faults:
        for at in (0, 40, 79, 80):
            if fault == "blocks" and at in (0, 40, 80):
                continue  # (the count is per launch: index at - 1 would sit in the launch before)
            assert f(*tables(81, fault, at), 81, *hyper, 1.0, None, None) == code, (fault, at)
            assert b"psf_adam_step_master" in lib.psf_last_error()
    t81 = tables(81)
    for step in (0.5, 0.0, -1.0, float("nan")):
        assert f(*t81, 81, *hyper, step, None, None) == E_SHAPE and b"step" in lib.psf_last_error()
    assert f(*t81, -1, *hyper, 1.0, None, None) == E_SHAPE                                        # count < 0
    assert f(*t81, 0, *hyper, 1.0, None, None) == 0                                               # count = 0: nothing is looked at
    assert f(None, None, None, None, None, None, 0, *hyper, 0.5, None, None) == 0
    for j in range(6):                                                                            # a NULL table
        t = list(t81)
        t[j] = None
        assert f(*t, 81, *hyper, 1.0, None, None) == E_NULL


def test_bf16_embedding_entries_validate_before_touching_the_gpu(lib):
    vp = ctypes.c_void_p
    one, two, three = vp(16), vp(32), vp(48)
    f = lib.psf_embed_tokens_bf16   # (idx, table, pos, out, T, N, V, E, stream)
    assert f(None, one, None, two, 100, 10, 6, 32, None) == E_NULL
    assert f(one, None, None, two, 100, 10, 6, 32, None) == E_NULL
    assert f(one, one, None, None, 100, 10, 6, 32, None) == E_NULL and b"psf_embed_tokens_bf16" in lib.psf_last_error()
    for E in (0, 4, 12, 30, -8):                                                   # 8 channels per 16-byte vector
        assert f(one, one, None, two, 100, 10, 6, E, None) == E_SHAPE, E
    assert b"multiple of 8" in lib.psf_last_error()
    assert f(one, one, None, two, -1, 10, 6, 32, None) == E_SHAPE
    assert f(one, one, None, two, 100, 0, 6, 32, None) == E_SHAPE
    assert f(one, one, None, two, 100, 10, 0, 32, None) == E_SHAPE
    assert f(one, vp(18), None, two, 100, 10, 6, 32, None) == E_ALIGN              # table + 2 bytes
    assert f(one, vp(24), None, two, 100, 10, 6, 32, None) == E_ALIGN              # table 8-byte aligned only
    assert f(one, one, vp(40), two, 100, 10, 6, 32, None) == E_ALIGN               # pos
    assert f(one, one, three, vp(34), 100, 10, 6, 32, None) == E_ALIGN             # out
    assert f(vp(20), one, three, two, 100, 10, 6, 32, None) == E_ALIGN             # idx: 8 bytes
    assert f(one, one, three, two, 0, 10, 6, 32, None) == 0                         # no tokens: nothing to do

    g = lib.psf_embed_tokens_bwd_bf16   # (idx, dOut, T, V, E, dTable, workspace, workspace_bytes, stream)
    need = lib.psf_embed_tokens_bwd_workspace(65536, 225, 32)
    assert need > 0
    for hole in range(4):
        args = [one, one, 65536, 225, 32, two, three, need, None]
        args[(0, 1, 5, 6)[hole]] = None
        assert g(*args) == E_NULL, hole
    assert g(one, one, 65536, 513, 32, two, three, 1 << 30, None) == E_SHAPE       # vocabulary beyond the LDS table
    assert g(one, one, 65536, 225, 4097, two, three, 1 << 30, None) == E_SHAPE
    assert g(one, one, 0, 225, 32, two, three, 1 << 30, None) == E_SHAPE
    assert g(one, one, 65536, 225, 32, two, three, need - 4, None) == E_SHAPE and b"workspace" in lib.psf_last_error()
    assert g(one, vp(17), 65536, 225, 32, two, three, need, None) == E_ALIGN       # dOut one byte off
    assert g(one, one, 65536, 225, 32, vp(33), three, need, None) == E_ALIGN and b"2-byte" in lib.psf_last_error()


# ---------------------------------------------------------------------------------------------- b. load_state_dict
def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().copy()


@pytest.mark.parametrize("capturable", [False, True])
def test_load_state_dict_restores_the_f32_state_of_a_bf16_parameter(capturable):
    """torch.optim.Optimizer.load_state_dict casts floating state to the parameter's dtype: every value below would lose its
    low 16 bits. ChunkedAdam puts master, exp_avg and exp_avg_sq back as f32 with the saved bits; the f32 parameter beside
    it is loaded as always."""
    from sparsefactorization_amd.train import ChunkedAdam
    gen = torch.Generator().manual_seed(5)
    pb = torch.nn.Parameter(torch.randn(7, 3, generator=gen).to(torch.bfloat16))
    pf = torch.nn.Parameter(torch.randn(5, generator=gen))
    src = ChunkedAdam([pb, pf], lr=1e-3, capturable=capturable)
    fine = lambda *shape: torch.randn(*shape, generator=gen) * (1 + 2.0 ** -20)  # noqa: E731
    step = torch.tensor(3.0) if capturable else 3.0
    src.state[pb] = dict(step=step, master=fine(7, 3), exp_avg=fine(7, 3) * 1e-3, exp_avg_sq=fine(7, 3) ** 2)
    src.state[pf] = dict(step=step, exp_avg=fine(5), exp_avg_sq=fine(5) ** 2)
    for name in ChunkedAdam.MASTER_STATE:  # the test is about bits a bf16 tensor cannot hold
        v = src.state[pb][name]
        assert not torch.equal(v.to(torch.bfloat16).float(), v), name
    sd = src.state_dict()

    plain = torch.optim.Adam([pb, pf], lr=1e-3)  # what the base class does on its own
    plain.load_state_dict(sd)
    assert plain.state[pb]["exp_avg"].dtype == torch.bfloat16

    dst = ChunkedAdam([pb, pf], lr=1e-3, capturable=capturable)
    dst.load_state_dict(sd)
    for name in ChunkedAdam.MASTER_STATE:
        got, want = dst.state[pb][name], src.state[pb][name]
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        assert np.array_equal(_bits(got), _bits(want)), name
        assert got.data_ptr() != want.data_ptr(), f"{name} must be a copy"
    for name in ("exp_avg", "exp_avg_sq"):
        assert np.array_equal(_bits(dst.state[pf][name]), _bits(src.state[pf][name]))
    if capturable:  # ONE device scalar shared by the group
        s = dst.state[pb]["step"]
        assert torch.is_tensor(s) and s.dtype == torch.float32 and float(s) == 3.0
        assert dst.state[pf]["step"] is s
    else:           # a host count
        assert dst.state[pb]["step"] == 3.0 and isinstance(dst.state[pb]["step"], float)
        assert isinstance(dst.state[pf]["step"], float)


def test_load_state_dict_survives_torch_save(tmp_path):
    from sparsefactorization_amd.train import ChunkedAdam
    pb = torch.nn.Parameter(torch.ones(4, dtype=torch.bfloat16))
    src = ChunkedAdam([pb], lr=1e-3)
    master = torch.tensor([1.0 - 2.0 ** -20, 1.0 + 2.0 ** -18, 0.3, -7.000001])
    src.state[pb] = dict(step=2.0, master=master.clone(), exp_avg=master * 1e-3, exp_avg_sq=master ** 2)
    torch.save(src.state_dict(), tmp_path / "opt.pt")
    dst = ChunkedAdam([pb], lr=1e-3)
    dst.load_state_dict(torch.load(tmp_path / "opt.pt"))
    assert dst.state[pb]["master"].dtype == torch.float32
    assert np.array_equal(_bits(dst.state[pb]["master"]), _bits(master))
    assert np.array_equal(_bits(dst.state[pb]["exp_avg_sq"]), _bits(master ** 2))


# ---------------------------------------------------------------------------------------------- c. make_adam routing
class _StubLib:
    """Records (entry, count, [tables as lists of addresses]) instead of launching."""

    def __init__(self):
        self.calls = []

    def _record(self, name, n_tables, *args):
        count = args[n_tables + 1]
        self.calls.append((name, count, [[tab[i] for i in range(count)] for tab in args[:n_tables]], list(args[n_tables][:count]),
                           args[n_tables + 2:]))
        return 0

    def psf_adam_step_f32(self, *args):
        return self._record("psf_adam_step_f32", 4, *args)

    def psf_adam_step_master(self, *args):
        return self._record("psf_adam_step_master", 5, *args)


@pytest.fixture
def on_a_pretend_gpu(monkeypatch):
    """CPU tensors that answer is_cuda = True, and a library that records: make_adam's choice and ChunkedAdam.step's tables
    can then be looked at without a device."""
    import contextlib
    from sparsefactorization_amd import _lib
    stub = _StubLib()
    real_is_cuda = torch.Tensor.is_cuda
    pretend = []
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: any(self is t for t in pretend) or real_is_cuda.__get__(self)))
    monkeypatch.setattr(_lib, "load", lambda: stub)
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return stub, pretend


def test_make_adam_routing(on_a_pretend_gpu):
    from sparsefactorization_amd.train import ChunkedAdam, make_adam
    _stub, pretend = on_a_pretend_gpu
    mk = lambda dtype, gpu=True: torch.nn.Parameter(torch.zeros(6, dtype=dtype))  # noqa: E731
    f32, bf16, f64, other_bf16 = mk(torch.float32), mk(torch.bfloat16), mk(torch.float64), mk(torch.bfloat16)
    pretend.extend([f32, bf16, f64, other_bf16])
    on_cpu = mk(torch.bfloat16)
    # default: exactly as before — ChunkedAdam for f32 alone, torch's Adam as soon as a bf16 parameter is in the list
    assert type(make_adam([f32], 1e-3)) is ChunkedAdam
    assert type(make_adam([bf16], 1e-3)) is torch.optim.Adam
    assert type(make_adam([f32, bf16], 1e-3, capturable=True)) is torch.optim.Adam
    # master_weights=True: f32 and bf16, alone or mixed
    for params in ([f32], [bf16], [f32, bf16, other_bf16]):
        opt = make_adam(params, 1e-3, capturable=True, master_weights=True)
        assert type(opt) is ChunkedAdam and opt.defaults["capturable"] is True
    assert make_adam([bf16], 2e-3, master_weights=True).defaults["lr"] == 2e-3
    # a double parameter, a CPU parameter, a non-contiguous one: torch's Adam, with or without the keyword
    for master_weights in (False, True):
        assert type(make_adam([f32, f64], 1e-3, master_weights=master_weights)) is torch.optim.Adam
        assert type(make_adam([bf16, on_cpu], 1e-3, master_weights=master_weights)) is torch.optim.Adam
    strided = torch.nn.Parameter(torch.zeros(4, 6, dtype=torch.bfloat16).t())
    pretend.append(strided)
    assert type(make_adam([strided], 1e-3, master_weights=True)) is torch.optim.Adam


def test_chunked_adam_refuses_other_dtypes_at_construction():
    from sparsefactorization_amd.train import ChunkedAdam
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 parameters and bfloat16 parameters"):
            ChunkedAdam([torch.nn.Parameter(torch.zeros(3, dtype=dtype))])
    with pytest.raises(TypeError):
        ChunkedAdam([{"params": [torch.nn.Parameter(torch.zeros(3))]}, {"params": [torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))]}])


@pytest.mark.parametrize("capturable", [False, True])
def test_a_mixed_list_reaches_each_entry_with_its_own_tables(on_a_pretend_gpu, capturable):
    """f32 parameters go to psf_adam_step_f32 and bf16 ones to psf_adam_step_master — (master, parameter, gradient, exp_avg,
    exp_avg_sq), the moments and the master f32 — under one step count; a parameter without a gradient is in neither."""
    from sparsefactorization_amd.train import make_adam
    stub, pretend = on_a_pretend_gpu
    a, b, c, d, idle = (torch.nn.Parameter(torch.full((n,), 1.0, dtype=dt))
                        for n, dt in ((5, torch.float32), (8, torch.bfloat16), (3, torch.bfloat16), (4, torch.float32), (2, torch.bfloat16)))
    pretend.extend([a, b, c, d, idle])
    opt = make_adam([a, b, c, d, idle], 1e-3, capturable=capturable, master_weights=True)
    for p in (a, b, c, d):
        p.grad = torch.ones_like(p)
    for step in (1, 2):
        del stub.calls[:]
        opt.step()
        assert [c_[0] for c_ in stub.calls] == ["psf_adam_step_f32", "psf_adam_step_master"]
        (_, n32, t32, sizes32, rest32), (_, n16, t16, sizes16, rest16) = stub.calls
        assert (n32, sizes32, n16, sizes16) == (2, [5, 4], 2, [8, 3])
        st = opt.state
        assert t32 == [[a.data_ptr(), d.data_ptr()], [a.grad.data_ptr(), d.grad.data_ptr()],
                       [st[a]["exp_avg"].data_ptr(), st[d]["exp_avg"].data_ptr()], [st[a]["exp_avg_sq"].data_ptr(), st[d]["exp_avg_sq"].data_ptr()]]
        assert t16 == [[st[b]["master"].data_ptr(), st[c]["master"].data_ptr()], [b.data_ptr(), c.data_ptr()],
                       [b.grad.data_ptr(), c.grad.data_ptr()], [st[b]["exp_avg"].data_ptr(), st[c]["exp_avg"].data_ptr()],
                       [st[b]["exp_avg_sq"].data_ptr(), st[c]["exp_avg_sq"].data_ptr()]]
        assert rest32 == rest16  # lr, betas, eps, step, step_dev, stream: one counter for the group
        if capturable:
            assert rest32[5] == st[a]["step"].data_ptr() and st[a]["step"] is st[b]["step"] and float(st[b]["step"]) == step
        else:
            assert rest32[4] == float(step) and rest32[5] is None and st[b]["step"] == float(step)
    for p in (b, c):
        assert set(opt.state[p]) == {"step", "master", "exp_avg", "exp_avg_sq"}
        assert all(opt.state[p][k].dtype == torch.float32 and opt.state[p][k].shape == p.shape for k in ("master", "exp_avg", "exp_avg_sq"))
        assert torch.equal(opt.state[p]["master"], p.detach().float())  # p.float() at the first step (the stub moves nothing)
    assert set(opt.state[a]) == {"step", "exp_avg", "exp_avg_sq"} and not opt.state[idle]
    # one parameter's state dropped between steps: fresh moments and a fresh master for it alone, its own count -> per-tensor calls
    if not capturable:
        old_master = opt.state[b]["master"]
        opt.state[c].clear()
        del stub.calls[:]
        opt.step()
        assert [(c_[0], c_[1]) for c_ in stub.calls] == [("psf_adam_step_f32", 1)] * 2 + [("psf_adam_step_master", 1)] * 2
        assert [c_[4][4] for c_ in stub.calls] == [3.0, 3.0, 3.0, 1.0]
        assert opt.state[b]["master"] is old_master and opt.state[c]["master"].dtype == torch.float32


# ---------------------------------------------------------------------------------------------- d. why master weights
def _rne_bf16(x):
    """float32 -> the float32 value of its bfloat16 rounding (nearest, ties to even), by bits."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32)


def test_a_pure_bf16_adam_never_moves_the_weight_and_the_master_rule_does():
    """p = 1, g = 1, lr = 1e-3: every update is ~1e-3, half a bf16 ulp below 1 is 2^-9 = 1.95e-3 (3.9e-3 above), so the bf16
    parameter of torch's Adam is exactly 1.0 after 16 steps. With an f32 master (adam_cases.emulate) the 16 updates add up to
    0.016, and the bf16 parameter — the master rounded to nearest even — is 252 / 256."""
    p = torch.nn.Parameter(torch.ones(1, dtype=torch.bfloat16))
    opt = torch.optim.Adam([p], lr=1e-3)
    for _ in range(16):
        p.grad = torch.ones_like(p)
        opt.step()
    assert p.dtype == torch.bfloat16 and float(p.detach()) == 1.0

    h = ac.hyper(lr=1e-3)
    master, g = np.ones(1, np.float32), np.ones(1, np.float32)
    m, v = np.zeros(1, np.float32), np.zeros(1, np.float32)
    param = None
    for t in range(1, 17):
        master, m, v = ac.emulate(master, g, m, v, h, t)
        param = _rne_bf16(master)
    assert abs(float(master[0]) - 0.984) < 1e-5
    assert float(param[0]) == 0.984375 == 252 / 256
    assert float(torch.from_numpy(master).to(torch.bfloat16)) == 0.984375  # torch's cast is the same rounding
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(_rne_bf16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


def test_the_large_exact_gradient_cases_do_round():
    """What the GPU test of psf_embed_tokens_bwd_bf16 relies on (tests/test_gpu_bf16_train.py): at the large T of
    helper_cases.EMB_GRAD the exact sums leave bf16's 8 bits, so the single rounding is exercised, and partial sums rounded to
    bf16 on the way — two halves of the tokens here — give another answer."""
    import helper_cases as hc
    for case in (c for c in hc.EMB_GRAD if c.T >= 262144):
        want = hc.as_f32(case.expected())
        rounded = torch.from_numpy(want).to(torch.bfloat16).float().numpy()
        assert (rounded != want).any(), case.id
        first = np.arange(case.T) < case.T // 2
        halves = [torch.from_numpy(hc.as_f32(case.expected(keep=k))).to(torch.bfloat16).float() for k in (first, ~first)]
        assert ((halves[0] + halves[1]).to(torch.bfloat16).float().numpy() != rounded).any(), case.id


# ---------------------------------------------------------------------------------------------- e. check_capturable
class _Net(torch.nn.Module):
    def __init__(self, vocab, width, dtype):
        super().__init__()
        from sparsefactorization_amd.token_linear import TokenEmbedding
        self.embedding = TokenEmbedding(vocab, width).to(dtype)


def test_check_capturable_admits_bf16_tables_only_on_the_bf16_route(monkeypatch):
    from sparsefactorization_amd import token_linear
    from sparsefactorization_amd.train import check_capturable
    assert token_linear.bf16_route == "never"
    check_capturable(_Net(6, 32, torch.float32))
    with pytest.raises(RuntimeError, match=r"torch\.bfloat16.*token_linear\.bf16_route = \"always\""):
        check_capturable(_Net(6, 32, torch.bfloat16))
    with pytest.raises(RuntimeError, match="513 x 32"):
        check_capturable(_Net(513, 32, torch.bfloat16))
    with pytest.raises(RuntimeError, match="float16"):
        check_capturable(_Net(6, 32, torch.float16))
    monkeypatch.setattr(token_linear, "bf16_route", "always")
    check_capturable(_Net(6, 32, torch.bfloat16))
    check_capturable(_Net(512, 4096, torch.bfloat16))
    check_capturable(_Net(6, 32, torch.float32))
    for vocab, width in ((513, 32), (6, 4097)):
        with pytest.raises(RuntimeError, match=f"{vocab} x {width}"):
            check_capturable(_Net(vocab, width, torch.bfloat16))
    with pytest.raises(RuntimeError, match="float16"):  # the switch is about bfloat16 alone
        check_capturable(_Net(6, 32, torch.float16))
    frozen = _Net(513, 32, torch.bfloat16)
    frozen.embedding.weight.requires_grad_(False)
    check_capturable(frozen)


def test_bf16_route_defaults_to_never_and_keeps_cpu_tensors_on_the_stock_path(monkeypatch):
    from sparsefactorization_amd import token_linear
    from sparsefactorization_amd.token_linear import TokenEmbedding, embed_tokens
    emb = TokenEmbedding(6, 8).to(torch.bfloat16)
    pos = torch.randn(5, 8).to(torch.bfloat16)
    idx = torch.tensor([[0, 5, 2, 2, 1]])
    want = torch.nn.functional.embedding(idx, emb.weight) + pos.unsqueeze(0)
    for route in ("never", "always"):
        monkeypatch.setattr(token_linear, "bf16_route", route)
        assert torch.equal(embed_tokens(idx, emb, pos), want)   # CPU: never a kernel
        assert torch.equal(emb(idx), torch.nn.functional.embedding(idx, emb.weight))
