"""GPU: rows and columns of the attention map without the dense map — psf_chord_chain_tr_f32 / _bf16 through the raw ABI
(bits against the CPU oracle's dV applied M times, guard bands, Q untouched, stale LDS, the same bits as M direct calls of
psf_chord_spmm_bwd_*), and attention_map.py / ChangedPSF.attention on top of them (the reference's own map, float64 bounds,
the Python boundary). Cases and references: tests/attention_cases.py. The graph replay is in test_gpu_graph_attention.py."""
import ctypes

import numpy as np
import pytest
import torch

import attention_cases as ac
from conftest import golden_state_dict, load_golden, rel_inf

pytestmark = pytest.mark.gpu

CANARY = {torch.float32: -7.25, torch.bfloat16: -7.25}
PAD = 64  # elements on each side of out and scratch


def _dev(a, gpu, dtype):
    return torch.from_numpy(np.array(a)).to(gpu).to(dtype)  # (bf16 operands are bf16-representable: exact)


def _odd(t):
    """the same values at an odd element offset (bf16: an odd 2-byte address)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % (2 * t.element_size()) == t.element_size()
    return v


def run_entry(gpu, Ws, Q, offsets=None, with_scratch=True, odd_w=False):
    """The entry on device operands, out and scratch inside one canary-filled buffer. Returns (out as f32 numpy, one_launch);
    asserts that nothing around out and scratch was written, that Q is unchanged and that the one launch leaves scratch alone."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    dtype = Q.dtype
    B, N, R = Q.shape
    M, L = len(Ws), Ws[0].shape[2]
    if odd_w:
        Ws = [_odd(w) for w in Ws]
    n = B * N * R
    buf = torch.full((3 * PAD + 2 * n,), CANARY[dtype], dtype=dtype, device=gpu)
    out, scratch = buf[PAD:PAD + n], buf[2 * PAD + n:2 * PAD + 2 * n]
    assert out.data_ptr() % 16 == 0 and scratch.data_ptr() % 16 == 0 and Q.data_ptr() % 16 == 0
    q_before = Q.clone()
    one_launch = bool(lib.psf_chord_chain_tr_supported(N, L, R, M, Q.element_size()))
    fn = lib.psf_chord_chain_tr_bf16 if dtype == torch.bfloat16 else lib.psf_chord_chain_tr_f32
    w_tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Ws])
    rc = fn(w_tab, Q.data_ptr(), out.data_ptr(), scratch.data_ptr() if with_scratch else None, M, B, N, L, R,
            _lib.offsets_array(offsets), _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    canary = torch.tensor(CANARY[dtype], dtype=dtype, device=gpu)
    for lo, hi in ((0, PAD), (PAD + n, 2 * PAD + n), (2 * PAD + 2 * n, 3 * PAD + 2 * n)):
        assert bool((buf[lo:hi] == canary).all()), f"guard band [{lo}, {hi}) was written"
    if one_launch or M == 1 or not with_scratch:
        assert bool((scratch == canary).all()), "scratch was written where the entry does not need it"
    assert torch.equal(Q.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       q_before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), "Q was written"
    return out.view(B, N, R).float().cpu().numpy(), one_launch


def _operands(gpu, case, dtype):
    Ws, Q, rows = ac.operands(case, dtype == torch.bfloat16)
    return [_dev(W, gpu, dtype) for W in Ws], _dev(Q, gpu, dtype), rows


# ---- bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.F32_CASES, ids=[c[0] for c in ac.F32_CASES])
def test_f32_entry_returns_the_oracle_bits(gpu, case):
    Ws, Q, _ = _operands(gpu, case, torch.float32)
    got, one_launch = run_entry(gpu, Ws, Q, case[6])
    assert one_launch == (case[2] <= 1024)
    assert ac.same_bits(got, ac.expected(case)) == 0
    if case[7] in ("nan", "inf"):
        assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("case", ac.BF16_CASES + [ac.BF16_ODD_W], ids=[c[0] for c in ac.BF16_CASES + [ac.BF16_ODD_W]])
def test_bf16_entry_returns_the_rounded_oracle_bits(gpu, case):
    Ws, Q, _ = _operands(gpu, case, torch.bfloat16)
    got, one_launch = run_entry(gpu, Ws, Q, case[6], odd_w=case is ac.BF16_ODD_W)
    assert one_launch == (case[2] <= 1024)
    assert ac.same_bits(got, ac.expected(case, True)) == 0
    if case[7] in ("nan", "inf"):
        assert np.isnan(got).any() and np.isfinite(got).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["n63", "pathfinder", "ragged_r20", "n1025", "explicit"])
def test_entry_has_the_bits_of_m_direct_dv_calls(gpu, name, dtype):
    """One launch (N <= 1024) and the per-step route (N = 1025) against M calls of psf_chord_spmm_bwd_* with dW = NULL."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    cases = ac.BF16_CASES if dtype == torch.bfloat16 else ac.F32_CASES
    case = next(c for c in cases if c[0] == name)
    Ws, Q, _ = _operands(gpu, case, dtype)
    B, N, R = Q.shape
    L = Ws[0].shape[2]
    got, _ = run_entry(gpu, Ws, Q, case[6])
    got_m1, _ = run_entry(gpu, Ws[-1:], Q, case[6], with_scratch=False)  # M = 1 needs no scratch on either route
    step = lib.psf_chord_spmm_bwd_bf16 if dtype == torch.bfloat16 else lib.psf_chord_spmm_bwd_f32
    y, first = Q, None
    for W in reversed(Ws):
        nxt = torch.empty_like(Q)
        rc = step(y.data_ptr(), W.data_ptr(), None, None, nxt.data_ptr(), B, N, L, R, N * R, _lib.offsets_array(case[6]),
                  _lib.stream_ptr(gpu))
        assert rc == 0, _lib.last_error()
        y = nxt
        first = y if first is None else first
    torch.cuda.synchronize()
    assert ac.same_bits(got, y.float().cpu().numpy()) == 0
    assert ac.same_bits(got_m1, first.float().cpu().numpy()) == 0


def test_one_launch_needs_no_scratch_and_the_per_step_route_says_so(gpu):
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    case = next(c for c in ac.F32_CASES if c[0] == "n63")
    Ws, Q, _ = _operands(gpu, case, torch.float32)
    got, one_launch = run_entry(gpu, Ws, Q, with_scratch=False)
    assert one_launch and ac.same_bits(got, ac.expected(case)) == 0
    case = next(c for c in ac.F32_CASES if c[0] == "n1025")
    Ws, Q, _ = _operands(gpu, case, torch.float32)
    out = torch.full_like(Q, -7.25)
    w_tab = (ctypes.c_void_p * len(Ws))(*[w.data_ptr() for w in Ws])
    rc = lib.psf_chord_chain_tr_f32(w_tab, Q.data_ptr(), out.data_ptr(), None, len(Ws), *Q.shape[:2], Ws[0].shape[2], Q.shape[2],
                                    None, _lib.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == _lib.PSF_E_UNSUPPORTED and bool((out == -7.25).all())


# ---- stale LDS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_second_call_with_other_data_after_nan_in_every_lds(gpu, dtype):
    """N = 63 and 65 leave lanes of the last wave without a row, R = 20 / 40 (five column groups: workgroups of 3 + 2) leaves the
    last workgroup a slot group that it fills with a repeat and must not store, and the later calls' shapes are smaller than
    the first's: nothing of what an earlier call or the NaN-filling kernels left in LDS may reach a sum."""
    from test_gpu_stale_lds import _poison
    bf = dtype == torch.bfloat16
    cases = ac.BF16_CASES if bf else ac.F32_CASES
    for name in ("pathfinder", "ragged_r52", "n65_m64", "ragged_r20", "n63", "n3_l20"):
        case = next(c for c in cases if c[0] == name)
        Ws, Q, _ = _operands(gpu, case, dtype)
        _poison(gpu)
        got, _ = run_entry(gpu, Ws, Q, case[6])
        assert ac.same_bits(got, ac.expected(case, bf)) == 0, name


# ---- the reference's own map ---------------------------------------------------------------------------------------------
def test_rows_and_columns_of_the_reference_pathfinder_map(gpu):
    import sparsefactorization_amd as sfa
    g = load_golden("lra_pathfinder_ckpt.npz")
    W = g["W"]  # [M, 1, N, L]
    M, B, N, L = W.shape
    assert (B, N) == (1, 1024)
    Ws = [torch.from_numpy(W[m].copy()).to(gpu) for m in range(M)]
    rows = sfa.attention_rows(Ws, range(0, N, 16))
    assert rows.shape == (1, N // 16, N) and not rows.requires_grad
    assert rel_inf(rows[0].cpu().numpy(), g["Wfinal_rows"]) <= 1e-4
    cols = [0, 1, 31, 32, 33, 100, 255, 256, 257, 511, 512, 640, 777, 800, 901, 1000, 1022, 1023]
    assert len(cols) == 18
    got = sfa.attention_cols(Ws, cols)
    with torch.no_grad():
        dense = sfa.chord_chain(Ws, torch.eye(N, N, device=gpu), False)
    assert got.shape == (1, N, 18) and torch.equal(got, dense[..., cols])
    # the same rows read off the dense map: two summation orders of the same products
    assert rel_inf(rows[0].cpu().numpy(), dense[0, ::16, :].cpu().numpy()) <= 1e-5


# ---- against float64 -------------------------------------------------------------------------------------------------------
BOUND_CASES = [("b64", 2, 64, 7, 6, 8, None, None), next(c for c in ac.F32_CASES if c[0] == "pathfinder"),
               next(c for c in ac.F32_CASES if c[0] == "imdb")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", BOUND_CASES, ids=[c[0] for c in BOUND_CASES])
def test_rows_against_the_float64_transposed_chain(gpu, case, dtype):
    import sparsefactorization_amd as sfa
    bf = dtype == torch.bfloat16
    _name, B, N, L, M, R, _off, _sp = case
    Wn, Qn, rows = ac.operands(case, bf)
    got = sfa.attention_rows([_dev(W, gpu, dtype) for W in Wn], rows).float().cpu().numpy()  # [B, R, N]
    assert got.shape == (B, R, N)
    exact = ac.tr_chain_f64(Wn, Qn).transpose(0, 2, 1)
    absprod = ac.tr_chain_f64([np.abs(W) for W in Wn], Qn).transpose(0, 2, 1)
    err, bound = np.abs(got - exact), ac.gamma(M, L, 2 if bf else 4) * absprod
    print(f"{_name} {dtype}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}, max |exact| = {np.abs(exact).max():.3g}")
    assert np.abs(exact).max() > 0 and np.all(err <= bound)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_changed_psf_attention_on_the_pathfinder_checkpoint(gpu):
    from sparsefactorization_amd.lra_psf import ChangedPSF
    from test_gpu_models import PATHFINDER
    g = load_golden("lra_pathfinder_ckpt.npz")
    net = ChangedPSF(**PATHFINDER)
    net.load_state_dict(golden_state_dict(g), strict=True)
    net = net.to(gpu).eval()
    x = torch.from_numpy(g["x"]).to(gpu)
    with torch.no_grad():
        logits, att = net(x)
        logits_q, rows, cols = net.attention(x, rows=[0, 5], cols=[7])
        links = []
        net.features(x, links)
    assert torch.equal(logits_q, logits)
    assert cols.shape == (1, 1024, 1) and torch.equal(cols, att[:, :, [7]])
    assert rows.shape == (1, 2, 1024)
    Wn = [w.cpu().numpy() for w in links]
    M, L = len(Wn), Wn[0].shape[2]
    Q = ac.one_hot(np.array([[0, 5]]), 1024, np.float64)
    absprod = ac.tr_chain_f64([np.abs(W) for W in Wn], Q).transpose(0, 2, 1)
    assert np.all(np.abs(rows.cpu().numpy().astype(np.float64) - att[:, [0, 5], :].cpu().numpy()) <= ac.gamma(M, L) * absprod)
    only_logits = net.attention(x)
    assert only_logits[1] is None and only_logits[2] is None


def test_changed_psf_attention_rows_at_the_text_length(gpu):
    """An IMDb-shaped net (N = 4097, CLS pooling, residual on V but never on the map), random weights, one row per sample as
    psf_utils_attn_IMDb.py reads it. Judged against the float64 transposed chain of the net's own links: no dense map here."""
    from sparsefactorization_amd.lra_psf import ChangedPSF
    from test_gpu_models import IMDB4097
    torch.manual_seed(11)
    net = ChangedPSF(**IMDB4097).to(gpu).eval()
    x = torch.randint(0, IMDB4097["vocab_size"] - 2, (2, 4097), device=gpu)
    with torch.no_grad():
        logits, rows, cols = net.attention(x, rows=[0])
        links = []
        net.features(x, links)
    assert logits.shape == (2, 2) and cols is None and rows.shape == (2, 1, 4097)
    Wn = [w.cpu().numpy() for w in links]
    M, L = len(Wn), Wn[0].shape[2]
    assert (M, L) == (12, 13)
    Q = ac.one_hot(np.zeros((2, 1), dtype=np.int64), 4097, np.float64)
    exact = ac.tr_chain_f64(Wn, Q).transpose(0, 2, 1)
    absprod = ac.tr_chain_f64([np.abs(W) for W in Wn], Q).transpose(0, 2, 1)
    assert np.abs(exact).max() > 0
    assert np.all(np.abs(rows.cpu().numpy() - exact) <= ac.gamma(M, L) * absprod)


# ---- the Python boundary -------------------------------------------------------------------------------------------------------
def test_python_boundary(gpu):
    import sparsefactorization_amd as sfa
    case = next(c for c in ac.F32_CASES if c[0] == "n63")
    Wn, _, _ = ac.operands(case)
    B, N, L = Wn[0].shape
    Ws = [_dev(W, gpu, torch.float32) for W in Wn]
    rng = np.random.default_rng(3)
    # R = 1 and R = 5: padded to the entry's multiple and cut off again; a requires_grad W gives a detached result
    for R in (1, 5):
        Y = rng.standard_normal((B, N, R)).astype(np.float32)
        Ws[0].requires_grad_(True)
        got = sfa.chain_transposed(Ws, _dev(Y, gpu, torch.float32))
        Ws[0].requires_grad_(False)
        assert got.shape == (B, N, R) and not got.requires_grad
        assert ac.same_bits(got.cpu().numpy(), ac.oracle_f32(Wn, Y)) == 0
        Yb = ac.rne_bf16(Y)
        Wb = [ac.rne_bf16(W) for W in Wn]
        got = sfa.chain_transposed([_dev(W, gpu, torch.bfloat16) for W in Wb], _dev(Yb, gpu, torch.bfloat16))
        assert got.dtype == torch.bfloat16 and ac.same_bits(got.float().cpu().numpy(), ac.oracle_bf16(Wb, Yb)) == 0
    # [R] and [B, R] index forms, lists and tensors
    per_sample = np.array([[0, 62, 7, 7, 30]] * B)
    per_sample[1] = [5, 4, 3, 2, 1]
    a = sfa.attention_rows(Ws, [0, 62, 7, 7, 30])
    b = sfa.attention_rows(Ws, torch.tensor(per_sample, device=gpu))
    assert a.shape == b.shape == (B, 5, N) and torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    assert ac.same_bits(b.transpose(1, 2).cpu().numpy(), ac.oracle_f32(Wn, ac.one_hot(per_sample, N))) == 0
    c = sfa.attention_cols(Ws, torch.tensor(per_sample, dtype=torch.int32))
    with torch.no_grad():
        dense = sfa.chord_chain(Ws, torch.eye(N, device=gpu), False)
    assert c.shape == (B, N, 5)
    for bb in range(B):
        assert torch.equal(c[bb], dense[bb][:, per_sample[bb]])
        assert rel_inf(b[bb].cpu().numpy(), dense[bb][per_sample[bb], :].cpu().numpy()) <= 1e-5
    # explicit offsets reach the kernels
    off = (0, 3, 7, 50, 99, -1, 200)
    Y = ac.one_hot(np.array([[1, 2, 3, 4]] * B), N)
    got = sfa.chain_transposed(Ws, _dev(Y, gpu, torch.float32), offsets=off)
    assert ac.same_bits(got.cpu().numpy(), ac.oracle_f32(Wn, Y, off)) == 0
    # faults
    for bad in ([N], [-1], [0, N + 5], torch.tensor([[0], [1], [N]])):
        with pytest.raises(ValueError):
            sfa.attention_rows(Ws, bad)
        with pytest.raises(ValueError):
            sfa.attention_cols(Ws, bad)
    with pytest.raises(ValueError):
        sfa.attention_rows(Ws, [])
    with pytest.raises(ValueError):
        sfa.attention_rows(Ws, [0.5])
    with pytest.raises(ValueError):
        sfa.attention_rows(Ws, torch.zeros(B + 1, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.attention_rows([w.cpu() for w in Ws], [0])
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.chain_transposed(Ws, torch.zeros(B, N, 4))
    with pytest.raises(TypeError, match="dtype"):
        sfa.chain_transposed(Ws, torch.zeros(B, N, 4, device=gpu, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="dtype"):
        sfa.attention_rows([Ws[0], Ws[1].double()], [0])
    with pytest.raises(TypeError):
        sfa.attention_rows([w.half() for w in Ws], [0])


def test_float64_takes_the_per_step_loop(gpu, monkeypatch):
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    calls = {"f64": 0, "tr": 0}
    real64, real_tr = lib.psf_chord_spmm_bwd_f64, lib.psf_chord_chain_tr_f32

    def count64(*a):
        calls["f64"] += 1
        return real64(*a)

    def count_tr(*a):
        calls["tr"] += 1
        return real_tr(*a)
    monkeypatch.setattr(lib, "psf_chord_spmm_bwd_f64", count64)
    monkeypatch.setattr(lib, "psf_chord_chain_tr_f32", count_tr)
    case = next(c for c in ac.F32_CASES if c[0] == "n63")
    Wn, _, _ = ac.operands(case)
    Wn = [W.astype(np.float64) for W in Wn]
    B, N, L = Wn[0].shape
    rows = np.array([[0, 1, 62]] * B)
    got = sfa.attention_rows([_dev(W, gpu, torch.float64) for W in Wn], rows)
    assert calls == {"f64": len(Wn), "tr": 0} and got.dtype == torch.float64 and got.shape == (B, 3, N)
    exact = ac.tr_chain_f64(Wn, ac.one_hot(rows, N, np.float64)).transpose(0, 2, 1)
    absprod = ac.tr_chain_f64([np.abs(W) for W in Wn], ac.one_hot(rows, N, np.float64)).transpose(0, 2, 1)
    n = len(Wn) * (L + 1) * 2.0 ** -53
    assert np.all(np.abs(got.cpu().numpy() - exact) <= n / (1 - n) * absprod)
    sfa.attention_rows([_dev(W, gpu, torch.float32) for W in Wn], rows)
    assert calls == {"f64": len(Wn), "tr": 1}
