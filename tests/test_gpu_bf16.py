"""bf16 on the chord path: bf16 storage, f32 accumulation, one rounding per element (include/psf_chord.h, "bfloat16").

Expected values come from the CPU oracle in f32 on the upcast inputs: out and dV must equal bf16_rne(oracle_f32 [+ res])
bit for bit (NaN in the same places); dW must be within one bf16 ulp of bf16_rne(oracle_f32 dW) plus the f32 dW bar.
"""
import numpy as np
import pytest
import torch

from conftest import rel_inf
from oracle import chord_oracle as oc

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


def _assert_bits(got, want_f32, what=""):
    """got: a bf16 tensor; want_f32: the f32 reference before its one rounding."""
    got = got.detach().cpu()
    want = _rne(want_f32)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ ({int(gn.sum())} vs {int(wn.sum())})"
    gb, wb = got.view(torch.int16)[~gn], want.view(torch.int16)[~wn]
    bad = int((gb != wb).sum())
    assert bad == 0, f"{what}: {bad} elements differ, rel={rel_inf(got.float().numpy(), want.float().numpy()):.3e}"


def _assert_dw(got, want_f32):
    got = got.detach().cpu().float().numpy()
    want = _rne(want_f32).float().numpy()
    mag = np.abs(want)
    ulp = np.where(mag > 0, np.exp2(np.floor(np.log2(np.where(mag > 0, mag, 1.0))) - 7), 0.0)
    err = np.abs(got - want)
    bound = ulp + DW_BAR * np.abs(want_f32).max()
    assert (err <= bound).all(), f"dW off by up to {(err / np.maximum(bound, 1e-30)).max():.2f} x the bound"


def _fwd_ref(W, V, res=None, offsets=None):
    out = oc.spmul_fwd(W, V, offsets)
    return out if res is None else out + res  # f32 add, rounded once to bf16 by the caller


FWD_SHAPES = [
    # (B, N, L, C): headline; narrow / wide rows (TG 1..16, 128-channel chunks at C = 256); ragged N; N shorter than a
    # tile; C % 8 != 0 (one element per lane); channel groups not a multiple of TG; L beyond the window kernels
    (64, 16384, 15, 8), (40, 128, 8, 8), (3, 2000, 12, 16), (2, 1024, 12, 32), (2, 2048, 12, 64), (2, 513, 10, 128),
    (2, 1100, 11, 256), (1, 4097, 13, 8), (2, 100, 9, 8), (2, 300, 9, 6), (2, 777, 11, 24), (2, 777, 22, 8), (1, 1, 1, 8),
]


@pytest.mark.parametrize("variant", [0, 1])  # automatic (window where it applies) / generic forced
@pytest.mark.parametrize("B,N,L,C", FWD_SHAPES)
def test_forward_step_bit_exact(gpu, B, N, L, C, variant):
    import sparsefactorization_amd as sfa
    W, V, R = _mk((B, N, L), 1), _mk((B, N, C), 2), _mk((B, N, C), 3)
    sfa.set_tuning("fwd_variant", variant)
    try:
        for res in (None, R):
            got = sfa.chord_spmm(_bt(W, gpu), _bt(V, gpu), None if res is None else _bt(res, gpu))
            assert got.dtype == torch.bfloat16
            _assert_bits(got, _fwd_ref(W, V, res), f"variant={variant} res={res is not None}")
    finally:
        sfa.set_tuning("fwd_variant", 0)


@pytest.mark.parametrize("B,N,L,C", [(3, 1101, 11, 8), (2, 2000, 12, 16), (64, 16384, 15, 8)])
def test_forward_window_and_generic_agree(gpu, B, N, L, C):
    import sparsefactorization_amd as sfa
    W, V, R = _bt(_mk((B, N, L), 4), gpu), _bt(_mk((B, N, C), 5), gpu), _bt(_mk((B, N, C), 6), gpu)
    outs = []
    for variant in (2, 1):  # window forced, generic forced
        sfa.set_tuning("fwd_variant", variant)
        try:
            outs.append(sfa.chord_spmm(W, V, R).view(torch.int16))
        finally:
            sfa.set_tuning("fwd_variant", 0)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shift", [1, 3, 5])
@pytest.mark.parametrize("B,N,L,C", [(3, 1101, 11, 8), (2, 2048, 12, 32)])
def test_forward_misaligned_W_and_V(gpu, B, N, L, C, shift):
    """W at any 2-byte offset takes the window kernel's misaligned W tile; V off its 16-byte boundary the generic VEC = 1 kernel."""
    import sparsefactorization_amd as sfa
    W, V, R = _mk((B, N, L), 7), _mk((B, N, C), 8), _mk((B, N, C), 9)
    Wb = torch.empty(B * N * L + shift, dtype=torch.bfloat16, device=gpu)[shift:].view(B, N, L)
    Wb.copy_(_bt(W, gpu))
    assert Wb.data_ptr() % 16 != 0
    _assert_bits(sfa.chord_spmm(Wb, _bt(V, gpu), _bt(R, gpu)), _fwd_ref(W, V, R), "misaligned W")
    Vb = torch.empty(B * N * C + shift, dtype=torch.bfloat16, device=gpu)[shift:].view(B, N, C)
    Vb.copy_(_bt(V, gpu))
    _assert_bits(sfa.chord_spmm(_bt(W, gpu), Vb), _fwd_ref(W, V), "misaligned V")


def test_forward_explicit_negative_offsets_and_broadcast(gpu):
    import sparsefactorization_amd as sfa
    B, N, L, C = 2, 500, 6, 8
    W, V = _mk((B, N, L), 10), _mk((B, N, C), 11)
    off = [3, 0, 499, 1000, -7, 250]
    _assert_bits(sfa.chord_spmm(_bt(W, gpu), _bt(V, gpu), offsets=off), _fwd_ref(W, V, None, off), "explicit offsets")
    # chord near links (window kernel) with arbitrary far ones
    B, N, L, C = 2, 4096, 12, 8
    W, V = _mk((B, N, L), 12), _mk((B, N, C), 13)
    off = [0] + [1 << k for k in range(9)] + [777, -3001]
    _assert_bits(sfa.chord_spmm(_bt(W, gpu), _bt(V, gpu), offsets=off), _fwd_ref(W, V, None, off), "far offsets")
    # a broadcast V ([N, C] shared by the batch)
    W, E = _mk((3, 256, 9), 14), np.eye(256, 8, dtype=np.float32)
    _assert_bits(sfa.chord_spmm(_bt(W, gpu), _bt(E, gpu)), _fwd_ref(W, E), "broadcast V")


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,N,L,C", [(2, 2048, 12, 8), (2, 1101, 11, 16), (2, 300, 9, 6)])
def test_forward_nan_and_inf(gpu, B, N, L, C, variant):
    import sparsefactorization_amd as sfa
    W, V, R = _mk((B, N, L), 20), _mk((B, N, C), 21), _mk((B, N, C), 22)
    rng = np.random.default_rng(23)
    for arr, vals in ((V, [np.nan, np.inf, -np.inf]), (W, [np.nan, np.inf, 0.0]), (R, [np.inf, np.nan])):
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, 6, replace=False)
        flat[idx] = np.resize(np.array(vals, dtype=np.float32), 6)
    sfa.set_tuning("fwd_variant", variant)
    try:
        for res in (None, R):
            got = sfa.chord_spmm(_bt(W, gpu), _bt(V, gpu), None if res is None else _bt(res, gpu))
            _assert_bits(got, _fwd_ref(W, V, res), f"variant={variant} res={res is not None}")
    finally:
        sfa.set_tuning("fwd_variant", 0)


BWD_SHAPES = [(3, 16384, 15, 8), (2, 2000, 12, 16), (2, 1024, 12, 32), (2, 513, 10, 128), (2, 300, 9, 6), (1, 4097, 13, 8),
              (2, 777, 22, 8), (2, 640, 10, 5)]


@pytest.mark.parametrize("bwd_variant", [0, 1])  # automatic (LDS-window dV / dW where they apply) / generic forced
@pytest.mark.parametrize("B,N,L,C", BWD_SHAPES)
def test_backward_step(gpu, B, N, L, C, bwd_variant):
    import sparsefactorization_amd as sfa
    W, V, dZ = _mk((B, N, L), 15), _mk((B, N, C), 16), _mk((B, N, C), 17)
    Wt = _bt(W, gpu).requires_grad_(True)
    Vt = _bt(V, gpu).requires_grad_(True)
    Rt = _bt(np.zeros_like(V), gpu).requires_grad_(True)
    sfa.set_tuning("bwd_variant", bwd_variant)
    try:
        sfa.chord_spmm(Wt, Vt, Rt).backward(_bt(dZ, gpu))
    finally:
        sfa.set_tuning("bwd_variant", 0)
    dF, dV = oc.spmul_bwd(dZ, W, V)
    assert Wt.grad.dtype == Vt.grad.dtype == torch.bfloat16
    _assert_bits(Vt.grad, dV, "dV")
    _assert_dw(Wt.grad, dF)
    assert torch.equal(Rt.grad.cpu().view(torch.int16), _rne(dZ).view(torch.int16))


@pytest.mark.parametrize("B,N,L,C", [(3, 16384, 15, 8), (2, 2000, 12, 16), (2, 1101, 11, 24), (2, 4096, 20, 64),
                                     (1, 4097, 13, 8), (2, 1100, 11, 256)])
def test_backward_window_and_generic_routes_agree(gpu, B, N, L, C):
    """The bf16 LDS-window dV (links ascending, f32 accumulator) gives the generic kernel's bits; dW both to the bar."""
    import sparsefactorization_amd as sfa
    W, V, dZ = _mk((B, N, L), 33), _mk((B, N, C), 34), _mk((B, N, C), 35)
    dF, dV = oc.spmul_bwd(dZ, W, V)
    grads = []
    for variant in (0, 1):
        Wt, Vt = _bt(W, gpu).requires_grad_(True), _bt(V, gpu).requires_grad_(True)
        sfa.set_tuning("bwd_variant", variant)
        try:
            sfa.chord_spmm(Wt, Vt).backward(_bt(dZ, gpu))
        finally:
            sfa.set_tuning("bwd_variant", 0)
        _assert_bits(Vt.grad, dV, f"dV bwd_variant={variant}")
        _assert_dw(Wt.grad, dF)
        grads.append(Vt.grad.view(torch.int16))
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("scale", [2.0 ** 60, 2.0 ** -60])
def test_forward_and_dv_bit_exact_at_the_edges_of_the_product_range(gpu, scale):
    """Products near FLT_MAX (2^120) and near FLT_MIN (2^-120) are still normal f32 numbers: the fused multiply-add of the
    bf16 kernels gives the bits of the separately rounded product and sum there too (include/psf_chord.h, "bfloat16")."""
    import sparsefactorization_amd as sfa
    B, N, L, C = 2, 2048, 12, 8
    # positive magnitudes in [1, 2) x scale: every product and every partial sum stays a normal f32 number (no cancellation)
    W, V, dZ = [_rne(scale * (1.0 + np.random.default_rng(s).random(shape, dtype=np.float32))).float().numpy()
                for s, shape in ((36, (B, N, L)), (37, (B, N, C)), (38, (B, N, C)))]
    for variant in (0, 1):
        sfa.set_tuning("fwd_variant", variant)
        try:
            _assert_bits(sfa.chord_spmm(_bt(W, gpu), _bt(V, gpu)), _fwd_ref(W, V), f"fwd scale={scale}")
        finally:
            sfa.set_tuning("fwd_variant", 0)
    Wt, Vt = _bt(W, gpu).requires_grad_(True), _bt(V, gpu).requires_grad_(True)
    sfa.chord_spmm(Wt, Vt).backward(_bt(dZ, gpu))
    _assert_bits(Vt.grad, oc.spmul_bwd(dZ, W, V)[1], f"dV scale={scale}")


def test_backward_misaligned_and_broadcast(gpu):
    import sparsefactorization_amd as sfa
    B, N, L, C = 2, 1101, 11, 8
    W, V, dZ = _mk((B, N, L), 30), _mk((B, N, C), 31), _mk((B, N, C), 32)
    g = torch.empty(B * N * C + 1, dtype=torch.bfloat16, device=gpu)[1:].view(B, N, C)
    g.copy_(_bt(dZ, gpu))
    Wt, Vt = _bt(W, gpu).requires_grad_(True), _bt(V, gpu).requires_grad_(True)
    sfa.chord_spmm(Wt, Vt).backward(g)
    dF, dV = oc.spmul_bwd(dZ, W, V)
    _assert_bits(Vt.grad, dV, "dV, misaligned dZ")
    _assert_dw(Wt.grad, dF)
    E = np.eye(N, C, dtype=np.float32)
    Wt = _bt(W, gpu).requires_grad_(True)
    sfa.chord_spmm(Wt, _bt(E, gpu)).backward(_bt(dZ, gpu))
    _assert_dw(Wt.grad, oc.spmul_bwd(dZ, W, E)[0])


def _chain_ref(Ws, V0, residual):
    """The iterated per-step reference: every step is bf16_rne(oracle_f32(W_m, X_m) [+ V0])."""
    X = V0
    for W in Ws:
        X = _rne(_fwd_ref(W, X, V0 if residual else None)).float().numpy()
    return X


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("B,N,M,L,C", [(64, 16384, 14, 15, 8), (2, 1101, 7, 11, 8)])
def test_chain_forward_bit_exact(gpu, B, N, M, L, C, residual):
    import sparsefactorization_amd as sfa
    Ws = [_mk((B, N, L), 40 + m, 0.3) for m in range(M)]
    V0 = _mk((B, N, C), 39)
    got = sfa.chord_chain([_bt(w, gpu) for w in Ws], _bt(V0, gpu), residual)
    assert got.dtype == torch.bfloat16
    want = _rne(_chain_ref(Ws, V0, residual))
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


CHAIN_GRAD_BOUND = 5e-2  # rel. to max |grad| of the float64 chain: bf16 keeps 8 significant bits at every step


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("B,N,M,L,C", [(2, 1101, 7, 11, 8), (2, 2048, 5, 12, 16), (1, 300, 4, 9, 6)])
def test_chain_backward_against_float64(gpu, B, N, M, L, C, residual):
    import sparsefactorization_amd as sfa
    Ws = [_mk((B, N, L), 60 + m, 0.3) for m in range(M)]
    V0, dOut = _mk((B, N, C), 59), _mk((B, N, C), 58)
    wb = [_bt(w, gpu).requires_grad_(True) for w in Ws]
    vb = _bt(V0, gpu).requires_grad_(True)
    sfa.chord_chain(wb, vb, residual).backward(_bt(dOut, gpu))
    wd = [torch.from_numpy(w).double().to(gpu).requires_grad_(True) for w in Ws]
    vd = torch.from_numpy(V0).double().to(gpu).requires_grad_(True)
    sfa.chord_chain(wd, vd, residual).backward(torch.from_numpy(dOut).double().to(gpu))
    assert vb.grad.dtype == torch.bfloat16
    assert rel_inf(vb.grad.float().cpu().numpy(), vd.grad.cpu().numpy()) <= CHAIN_GRAD_BOUND
    for m in range(M):
        assert rel_inf(wb[m].grad.float().cpu().numpy(), wd[m].grad.cpu().numpy()) <= CHAIN_GRAD_BOUND, m


@pytest.mark.parametrize("K,shape", [(15, (4, 1000, 8)), (2, (3, 64, 8)), (32, (1, 8, 8)), (5, (3, 7, 3))])
def test_sum_tensors_bf16_is_one_f32_sum_rounded_once(gpu, K, shape):
    from sparsefactorization_amd import chord
    terms = [_mk(shape, 80 + k) for k in range(K)]
    acc = terms[0].copy()
    for t in terms[1:]:
        acc = (acc + t).astype(np.float32)  # numpy f32, left to right
    got = chord._sum_tensors([_bt(t, gpu) for t in terms])
    assert got.dtype == torch.bfloat16
    _assert_bits(got, acc, f"K={K}")


def test_chain_is_deterministic(gpu):
    import sparsefactorization_amd as sfa
    B, N, M, L, C = 8, 16384, 14, 15, 8
    Ws = [_bt(_mk((B, N, L), 100 + m, 0.3), gpu).requires_grad_(True) for m in range(M)]
    V0 = _bt(_mk((B, N, C), 99), gpu).requires_grad_(True)
    dOut = _bt(_mk((B, N, C), 98), gpu)
    runs = []
    for _ in range(2):
        for w in Ws:
            w.grad = None
        V0.grad = None
        out = sfa.chord_chain(Ws, V0, True)
        out.backward(dOut)
        runs.append([out.detach().clone(), V0.grad.clone(), *[w.grad.clone() for w in Ws]])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


class _RefStyleNet(torch.nn.Module):
    """The reference's loop shape: Linear producers, one spmm plus a residual add per factor."""

    def __init__(self, spmm, n_vec=256, width=32, channels=8, n_W=8):
        super().__init__()
        from sparsefactorization_amd import get_chord_indices_assym
        self.spmm, self.n_vec, self.n_W = spmm, n_vec, n_W
        self.lift = torch.nn.Linear(2, width)
        mlp = lambda out: torch.nn.Sequential(torch.nn.Linear(width, width), torch.nn.GELU(), torch.nn.Linear(width, out))  # noqa: E731
        self.fs = torch.nn.ModuleList([mlp(n_W + 1) for _ in range(n_W)])
        self.g = mlp(channels)
        self.final = torch.nn.Linear(n_vec * channels, 1)
        self.register_buffer("idx", torch.tensor(get_chord_indices_assym(n_vec, n_W + 1)))

    def forward(self, x):
        data = self.lift(x)
        V = self.g(data)
        res = V
        for m in range(self.n_W):
            W = self.fs[m](data)
            V = self.spmm(self.idx, W.reshape(W.size(0), -1), self.n_vec, self.n_vec, V)
            V = V + res
        return self.final(V.reshape(V.size(0), -1)).squeeze(-1)


@pytest.mark.parametrize("lazy", [True, False])  # the torch_sparse shim's operator / the eager drop-in
def test_reference_style_model_under_autocast(gpu, lazy):
    from sparsefactorization_amd import chord
    from sparsefactorization_amd import lazy as lazy_mod
    spmm = lazy_mod.spmm if lazy else chord.spmm
    torch.manual_seed(7)
    net = _RefStyleNet(spmm).to(gpu)
    x = (torch.rand(16, 256, 2, device=gpu) * 2 - 1)
    y = x[..., 0].mean(dim=1)
    with torch.no_grad():
        ref = net(x).float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x)
    assert out.dtype == torch.bfloat16
    assert rel_inf(out.float().cpu().numpy(), ref.cpu().numpy()) <= 3e-2
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = torch.nn.functional.mse_loss(net(x).float(), y)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses


def test_psfnet_in_bf16(gpu):
    from sparsefactorization_amd.synthetic_psf import PSFNet
    torch.manual_seed(42)
    cfg = dict(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=128, n_W=7, Ws=[32, 'GELU'],
               V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
               use_cuda=True, use_residuals=True, use_pos_embedding=False, problem="adding")
    net = PSFNet(**cfg).to(gpu)
    x = torch.rand(8, 128, 2, device=gpu)
    ref = net(x)
    ref.sum().backward()
    trained = {n for n, p in net.named_parameters() if p.grad is not None}  # (the adding task leaves the embedding unused)
    assert any(n.startswith("fs.") for n in trained) and any(n.startswith("g.") for n in trained)
    ref = ref.detach().cpu().numpy()
    net = net.to(torch.bfloat16)
    net.zero_grad(set_to_none=True)
    out = net(x.to(torch.bfloat16))
    assert out.dtype == torch.bfloat16
    assert rel_inf(out.detach().float().cpu().numpy(), ref) <= 3e-2
    out.float().sum().backward()
    assert {n for n, p in net.named_parameters() if p.grad is not None} == trained
    for name in trained:
        p = net.get_parameter(name)
        assert p.grad.dtype == torch.bfloat16 and torch.isfinite(p.grad).all(), name


def test_float16_and_mixed_dtypes_still_raise(gpu):
    import sparsefactorization_amd as sfa
    W, V = torch.zeros(1, 64, 4, device=gpu), torch.zeros(1, 64, 8, device=gpu)
    with pytest.raises(TypeError):
        sfa.chord_spmm(W.half(), V.half())
    with pytest.raises(TypeError):
        sfa.chord_spmm(W.bfloat16(), V)
