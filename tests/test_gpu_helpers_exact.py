"""GPU: known-answer tests of the token-wise helper kernels — every result bit-equal to the exact answer.

The cases (tests/helper_cases.py) are small integers with sum |terms| < 2^24 per output, so the exact answer is the kernels'
answer whatever order they sum in (test_helper_cases_cpu.py shows the cases exact, the lists reaching the paths named below,
and emulated defects changing the answers). Kernels, through their C entries:

  psf_embed_tokens_bwd_f32   1 .. 64 sub-tables, idle columns, a partial 64-column chunk, 64 chunks, V = 192 | 193 (the 48 KB
                             dynamic-LDS boundary), V = 512, T < 128, T > 262 144 (capped, longer slices; empty trailing ones),
                             rows no token names (exactly +0.0), one row named by every token
  psf_embed_tokens_f32       a second trip through the grid-stride loop
  psf_affine_rows_f32        K = 1, 2, 3, with and without bias, one position per workgroup (E = 516, 1024), second trips
  psf_flat_head_f32          both chunk lengths with ragged tails, K < 4096, J = 1, 3, 8, a last row group of one row; the same
                             rows on both sides of the chunk rule
  psf_flat_head_bwd_f32      dX only, dW only, both; B = 1024 x J = 16: 64 KB of dynamic LDS
  psf_linear_wgrad_f32 / psf_linear_wgrad_strided_f32   m, n = 1 and 128, T = 1, odd T below one unrolled pass, db = NULL,
                             column slices of wider arrays whose other columns are NaN
  ids outside [0, V)         psf_embed_tokens_f32, psf_embed_tokens_bwd_f32 and the single-launch mixer's TOKENS recipe clamp

Every output and every workspace (sized to exactly what its _workspace function returns) sits between 256-byte NaN bands and
is pre-filled with NaN; the operands sit between NaN bands too. No tolerance anywhere: equality of bits, or a NaN check.
"""
import numpy as np
import pytest
import torch

import helper_cases as hc
import test_gpu_guard_bands as gb

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _lib_and_stream(gpu):
    from sparsefactorization_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream(gpu).cuda_stream


def _eq(got, want, what):
    """Equal bits (so +0.0 is not -0.0); count, first index and max |diff| of what differs."""
    got = got.detach().cpu().contiguous().numpy()
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}, "
                           f"max |diff| {np.abs(got.astype(np.float64) - want).max():.3e}")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _written_inside(band, what):
    buf, _, span = band
    assert gb._bands_intact(buf, span), f"{what}: a NaN band was written, or the output holds NaN"


def _workspace(nbytes, gpu):
    """Exactly ``nbytes`` between NaN bands (a kernel may leave part of it unused: only the bands are checked)."""
    assert nbytes > 0 and nbytes % 4 == 0, nbytes
    return gb._banded((nbytes // 4,), gpu)


def _bands_untouched(band, what):
    buf, _, (lo, hi) = band
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all()), f"{what}: written outside"


def _in(a, gpu):
    return None if a is None else gb._banded_input(np.ascontiguousarray(a), gpu)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- embedding gradient
def _embed_bwd(gpu, case, idx_np, want):
    _lib, lib, s = _lib_and_stream(gpu)
    T, V, E = case.T, case.V, case.E
    idx = torch.from_numpy(idx_np).to(gpu)
    dout = _in(case.dout(), gpu)
    nbytes = lib.psf_embed_tokens_bwd_workspace(T, V, E)
    assert nbytes > 0, "inside the header's limits (1 <= V <= 512, 1 <= E <= 4096)"
    runs = []
    for run in range(2):
        table, ws = gb._banded((V, E), gpu), _workspace(nbytes, gpu)
        _lib.check(lib.psf_embed_tokens_bwd_f32(idx.data_ptr(), dout.data_ptr(), T, V, E, table[1].data_ptr(), ws[1].data_ptr(),
                                                nbytes, s), "psf_embed_tokens_bwd_f32")
        _written_inside(table, "dTable")
        _bands_untouched(ws, "workspace")
        _eq(table[1], want, f"dTable (run {run})")
        runs.append(table[1])
    assert _same_bits(*runs)
    return runs[0]


@pytest.mark.parametrize("case", hc.EMB_GRAD, ids=_ids(hc.EMB_GRAD))
def test_embedding_gradient_is_exact(gpu, case):
    idx = case.idx()
    got = _embed_bwd(gpu, case, idx, hc.as_f32(case.expected(idx=idx)))
    named = np.zeros(case.V, dtype=bool)
    named[idx] = True
    if not named.all():  # rows no token names: +0.0 out of a workspace and an output full of NaN
        assert not got[torch.from_numpy(~named).to(gpu)].view(torch.int32).any()


# ---------------------------------------------------------------------------------------------- embedding forward
def _table_between_nan_rows(a, gpu):
    """``a`` [rows, E] as a view into a buffer with CLAMP_BAND_ROWS rows of NaN on either side: an index up to that many rows
    outside the table reads NaN inside the same allocation."""
    rows, E = a.shape
    buf = torch.full((rows + 2 * hc.CLAMP_BAND_ROWS, E), float("nan"), device=gpu)
    view = buf[hc.CLAMP_BAND_ROWS:hc.CLAMP_BAND_ROWS + rows]
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


def _embed_fwd(gpu, case, idx_np, want, table=None, pos=None):
    _lib, lib, s = _lib_and_stream(gpu)
    idx = torch.from_numpy(idx_np).to(gpu)
    table = _in(case.table(), gpu) if table is None else table
    pos = (_in(case.pos_rows(), gpu) if pos is None else pos) if case.pos else None
    out = gb._banded((case.T, case.E), gpu)
    _lib.check(lib.psf_embed_tokens_f32(idx.data_ptr(), table.data_ptr(), _ptr(pos), out[1].data_ptr(), case.T, case.N, case.V,
                                        case.E, s), "psf_embed_tokens_f32")
    _written_inside(out, "out")
    _eq(out[1], want, "out")


@pytest.mark.parametrize("case", hc.EMB_FWD, ids=_ids(hc.EMB_FWD))
def test_embedding_forward_is_exact(gpu, case):
    _embed_fwd(gpu, case, case.idx(), hc.as_f32(case.expected()))


# ---------------------------------------------------------------------------------------------- affine rows
@pytest.mark.parametrize("case", hc.AFFINE, ids=_ids(hc.AFFINE))
def test_affine_rows_are_exact(gpu, case):
    _lib, lib, s = _lib_and_stream(gpu)
    x, w, b = _in(case.x(), gpu), _in(case.w(), gpu), _in(case.b(), gpu)
    out = gb._banded((case.T, case.E), gpu)
    _lib.check(lib.psf_affine_rows_f32(x.data_ptr(), w.data_ptr(), _ptr(b), out[1].data_ptr(), case.T, case.K, case.E, s),
               "psf_affine_rows_f32")
    _written_inside(out, "out")
    _eq(out[1], hc.as_f32(case.expected()), "out")


# ---------------------------------------------------------------------------------------------- head forward
def _exact_on_gpu(t64):
    """An answer computed in float64 on the GPU (the large heads): integral, below 2^24, as f32 on the host."""
    assert bool((t64 == t64.round()).all()) and float(t64.abs().max()) < hc.LIMIT
    return t64.float().cpu().numpy()


def _head_fwd(gpu, case):
    _lib, lib, s = _lib_and_stream(gpu)
    B, K, J = case.B, case.K, case.J
    x, w, b = _in(case.x(), gpu), _in(case.w(), gpu), _in(case.b(), gpu)
    if B * K > (1 << 20):
        ref = x.double() @ w.double().t()
        want = _exact_on_gpu(ref + b.double() if b is not None else ref)
        del ref
    else:
        want = hc.as_f32(case.expected())
    nbytes = lib.psf_flat_head_workspace(B, K, J)
    assert nbytes > 0
    runs = []
    for run in range(2):
        out, ws = gb._banded((B, J), gpu), _workspace(nbytes, gpu)
        _lib.check(lib.psf_flat_head_f32(x.data_ptr(), w.data_ptr(), _ptr(b), out[1].data_ptr(), B, K, J, ws[1].data_ptr(), nbytes, s),
                   "psf_flat_head_f32")
        _written_inside(out, "out")
        _bands_untouched(ws, "workspace")
        _eq(out[1], want, f"out (run {run})")
        runs.append(out[1])
    assert _same_bits(*runs)
    return runs[0]


@pytest.mark.parametrize("case", hc.HEAD_FWD, ids=_ids(hc.HEAD_FWD))
def test_head_forward_is_exact(gpu, case):
    # the side of the chunk rule this case is here for (>= 1024 workgroups of 4096 floats x 8 rows: 4096-float chunks)
    wgs = -(-case.K // 4096) * -(-case.B // 8)
    assert (wgs >= 1024) == ((case.B, case.K, case.J) in hc.HEAD_FWD_LARGE_CHUNK)
    _head_fwd(gpu, case)


def test_head_forward_gives_the_same_bits_on_both_sides_of_the_chunk_rule(gpu):
    """128 rows run in 4096-float chunks, their first 120 alone in 1024-float chunks: with exact data, the same logits."""
    big, small = (next(c for c in hc.HEAD_FWD if (c.B, c.K, c.J) == k) for k in hc.HEAD_FWD_ACROSS)
    assert big.chunk() == 4096 and small.chunk() == 1024
    assert _same_bits(_head_fwd(gpu, big)[:small.B], _head_fwd(gpu, small))


# ---------------------------------------------------------------------------------------------- head backward
def _head_bwd(gpu, case):
    _lib, lib, s = _lib_and_stream(gpu)
    B, K, J = case.B, case.K, case.J
    dy = _in(case.dy(), gpu)
    x = _in(case.x(), gpu) if case.want_dw else None  # (dW needs X, dX needs W: the other one is NULL)
    w = _in(case.w(), gpu) if case.want_dx else None
    want_dx, want_dw = (hc.as_f32(a) for a in case.expected())
    runs = []
    for run in range(2):
        dX = gb._banded((B, K), gpu) if case.want_dx else None
        dW = gb._banded((J, K), gpu) if case.want_dw else None
        rc = lib.psf_flat_head_bwd_f32(dy.data_ptr(), _ptr(x), _ptr(w), dX[1].data_ptr() if dX else None,
                                       dW[1].data_ptr() if dW else None, B, K, J, s)
        _lib.check(rc, f"psf_flat_head_bwd_f32 with {B * J * 4} bytes of dY in LDS")
        for band, want, name in ((dX, want_dx, "dX"), (dW, want_dw, "dW")):
            if band is not None:
                _written_inside(band, name)
                _eq(band[1], want, f"{name} (run {run})")
        runs.append([band[1] for band in (dX, dW) if band is not None])
    assert all(_same_bits(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("case", hc.HEAD_BWD, ids=_ids(hc.HEAD_BWD))
def test_head_backward_is_exact(gpu, case):
    _head_bwd(gpu, case)


def test_head_backward_runs_at_its_documented_limits(gpu):
    """B = 1024, J = 16: dY fills exactly 64 KB of dynamic LDS. The entry must launch there (return 0) and be exact."""
    case = next(c for c in hc.HEAD_BWD if (c.B, c.J) == (hc.HEAD_BWD_MAX_B, hc.HEAD_BWD_MAX_J) and c.want_dx and c.want_dw)
    assert case.B * case.J * 4 == 64 * 1024 and case.K == 4096
    _head_bwd(gpu, case)
    torch.cuda.synchronize(gpu)


# ---------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("case", hc.WGRAD, ids=_ids(hc.WGRAD))
def test_weight_gradient_is_exact(gpu, case):
    from sparsefactorization_amd.token_linear import linear_wgrad
    _lib, lib, s = _lib_and_stream(gpu)
    T, m, n = case.T, case.m, case.n
    want_w, want_b = (hc.as_f32(a) for a in case.expected())
    if case.strided:  # column slices of wider arrays, every other column NaN
        xw, yw = (_in(a, gpu) for a in case.wide())
        x, dy = xw[:, case.X_OFF:case.X_OFF + m], yw[:, case.DY_OFF:case.DY_OFF + n]
        assert (x.stride(0), dy.stride(0)) == (case.ldx, case.ldy) == (m + 3, n + 5)
        dW, db = linear_wgrad(x, dy, need_bias=case.need_bias)  # passes the strides on
        _eq(dW, want_w, "dWeight (token_linear.linear_wgrad)")
        assert (db is None) == (not case.need_bias)
        if db is not None:
            _eq(db, want_b, "dBias (token_linear.linear_wgrad)")
    else:
        x, dy = _in(case.x(), gpu), _in(case.dy(), gpu)
    nbytes = lib.psf_linear_wgrad_workspace(T, m, n)
    assert nbytes > 0
    dWt, ws = gb._banded((n, m), gpu), _workspace(nbytes, gpu)
    db = gb._banded((n,), gpu) if case.need_bias else None
    if case.strided:
        rc = lib.psf_linear_wgrad_strided_f32(x.data_ptr(), case.ldx, dy.data_ptr(), case.ldy, T, m, n, dWt[1].data_ptr(),
                                              db[1].data_ptr() if db else None, ws[1].data_ptr(), nbytes, s)
    else:
        rc = lib.psf_linear_wgrad_f32(x.data_ptr(), dy.data_ptr(), T, m, n, dWt[1].data_ptr(), db[1].data_ptr() if db else None,
                                      ws[1].data_ptr(), nbytes, s)
    _lib.check(rc, "psf_linear_wgrad")
    _written_inside(dWt, "dWt")
    _bands_untouched(ws, "workspace")
    _eq(dWt[1], want_w, "dWt")
    if db is not None:
        _written_inside(db, "db")
        _eq(db[1], want_b, "db")


# ---------------------------------------------------------------------------------------------- ids outside [0, V)
@pytest.mark.parametrize("case", hc.EMB_FWD_CLAMPED, ids=_ids(hc.EMB_FWD_CLAMPED))
def test_embedding_forward_clamps_ids_outside_the_table(gpu, case):
    """Ids -2, -1, V, V + 1 (first and last token among them) read row 0 / row V - 1: the table and the positional rows sit
    between NaN rows of their own allocation, so a missing clamp shows as NaN, never as a read of foreign memory."""
    bad = hc.with_out_of_range_ids(case.idx(), case.V, seed=2)
    assert bad.min() == -2 and bad.max() == case.V + 1
    want = hc.as_f32(case.expected(idx=np.clip(bad, 0, case.V - 1)))
    _embed_fwd(gpu, case, bad, want, table=_table_between_nan_rows(case.table(), gpu),
               pos=_table_between_nan_rows(case.pos_rows(), gpu) if case.pos else None)


@pytest.mark.parametrize("case", hc.EMB_GRAD_CLAMPED, ids=_ids(hc.EMB_GRAD_CLAMPED))
def test_embedding_gradient_clamps_ids_outside_the_table(gpu, case):
    """The same ids in the gradient: rows 0 and V - 1 receive those tokens, nothing lands outside dTable."""
    bad = hc.with_out_of_range_ids(case.idx(), case.V, seed=3)
    assert bad.min() == -2 and bad.max() == case.V + 1
    _embed_bwd(gpu, case, bad, hc.as_f32(case.expected(idx=np.clip(bad, 0, case.V - 1))))


def test_single_launch_mixer_clamps_ids_outside_the_table(gpu, monkeypatch):
    """PSF_MIXER_IN_TOKENS evaluated inside the single-launch kernel (BASELINE configs[0] with tokens and positional rows):
    the result on ids outside [0, K) has the bits of the same call on the clamped ids, and no NaN from the rows around the table."""
    import test_gpu_mixer as tm
    from sparsefactorization_amd import _lib, fused_mixer
    name, kind, B, N, E, h, C, L, M, residual, with_pos, K = next(c for c in tm.RECIPE_CASES if c[0] == "cfg1_order_tokens_lds")
    assert kind == "tokens" and with_pos
    g, fs = tm._blocks(E, h, C, L, M, seed=21)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    rng = np.random.default_rng(8)
    table = _table_between_nan_rows(rng.standard_normal((K, E)).astype(np.float32), gpu)
    pos = _table_between_nan_rows((0.5 * rng.standard_normal((N, E))).astype(np.float32), gpu)
    bad_np = hc.with_out_of_range_ids(rng.integers(0, K, (B, N), dtype=np.int64), K, seed=4)
    assert bad_np.min() == -2 and bad_np.max() == K + 1 and bad_np[0, 0] < 0 and bad_np[-1, -1] >= K
    bad = torch.from_numpy(bad_np).to(gpu)
    monkeypatch.setattr(fused_mixer, "recipe_in_kernel", True)
    assert _lib.load().psf_mixer_fwd_plan(N, E, *fused_mixer._block_sizes(E, g, fs)) == 2, "the single launch must take this shape"
    with torch.no_grad():
        outs = []
        for idx in (bad, bad.clamp(0, K - 1)):
            r = fused_mixer.Recipe.tokens(idx, table, pos)
            assert r.ok()
            outs.append(fused_mixer.mixer_forward_in(r, g, fs, residual).clone())
    assert not bool(torch.isnan(outs[0]).any()) and bool(torch.isfinite(outs[1]).all())
    assert _same_bits(*outs)
