"""GPU: psf_mlp_wide_fwd_f32 / psf_mlp_wide_bwd_f32 through the raw entry points, at the edges of their contract.

Every other wide test goes through fused_mlp.wide_apply, which hands the kernels torch allocations: 256-byte aligned, padded
and often larger than asked for. Here one harness places everything itself (tests/wide_cases.py; its CPU self-tests are
test_wide_cases_cpu.py):

* every operand sits inside canary bands (a NaN of fixed bits), every output — each Y[k], dX, every dA, da, dB, db — is a view
  in a canary-filled buffer with bands on both sides;
* `saved` and both workspaces are 256-byte-aligned views of EXACTLY the byte counts the three psf_mlp_wide_* size functions
  advertise, pre-filled with 0xFF bytes (NaN as f32 and as bf16), inside a larger allocation with 64 KB of 0xFF on each side:
  a scratch overrun lands in a band, never in unmapped memory. Inference (saved = NULL) gets fwd_workspace + saved_bytes.

After every call: bands intact, outputs fully written, values against the case's reference — equal bits where the case is a
known-answer construction of tests/x3_exact.py, else forward <= 1e-5 and gradients <= 2e-5 of max|reference| per tensor
against float64 copies of the same MLPBlocks (the bounds of test_gpu_wide_mlp.py). Everything else here is bit equality, band
integrity or a return code.

Alignment: include/psf_chord.h asks 16 bytes of X and the forward's A[k] only. The kernels were read for it: wide_pack_fwd_k
and x3_split_planes_k load A[k] and X as float4; a, B, b, the backward's A and the partial-tile dY are scalar loads; wide_out_k
and the GEMM's fused epilogue store Y as float4 only when O % 4 == 0 and Y[k] is 16-byte aligned (vec_ok), wide_mid_k reads
dY rows as float4 under the same test (row4); the dX epilogue, the three reduce kernels (dA, da, dB, db) store scalars. So
every placement below is one the contract allows and the code handles.
"""
import ctypes

import numpy as np
import pytest
import torch

import wide_cases as wc
from conftest import rel_inf

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("dA", "da", "dB", "db")


def _tables(layers):
    K = len(layers)
    return K, (ctypes.c_int32 * K)(*[h for h, _ in layers]), (ctypes.c_int32 * K)(*[o for _, o in layers])


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _advertised(lib, name):
    """The three byte counts the library advertises for the case (the mirror's, as test_wide_cases_cpu.py shows)."""
    T, E, layers = wc.CASES[name]
    K, h, O = _tables(layers)
    sizes = tuple(f(T, E, K, h, O) for f in (lib.psf_mlp_wide_saved_bytes, lib.psf_mlp_wide_fwd_workspace, lib.psf_mlp_wide_bwd_workspace))
    p = wc.plan(T, E, layers)
    assert sizes == (p["saved"], p["fwd_ws"], p["bwd_ws"]) and min(sizes) > 0, name
    assert not [r for r in wc.split_ranges(p["chunks"], p["splits"]) if r[1] <= r[0]], name  # every split has a K range
    return sizes


def _outputs_ok(outs, what):
    for label, (buf, _view, span) in outs:
        assert wc.band_damage(buf, span) == 0, f"{what}: wrote outside {label}"
        assert wc.unwritten(buf, span) == 0, f"{what}: {wc.unwritten(buf, span)} elements of {label} never written"


def forward(gpu, name, X=None, keep=True, shift=0, kind=None):
    """One raw psf_mlp_wide_fwd_f32 call on the case. ``shift``: floats off the 16-byte boundary for everything the contract
    lets sit there (a, B, b, Y; X and A stay aligned). Returns {"Y": [arrays], "saved": the record (a GPU byte view)}."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    T, E, layers = wc.CASES[name]
    X0, params, _dYs, _ref, _exact = wc.problem(name, kind)
    K, h, O = _tables(layers)
    n_saved, n_fwd, _ = _advertised(lib, name)
    x = wc.banded_input(X0 if X is None else X, gpu)
    As = [wc.banded_input(A, gpu) for A, _, _, _ in params]
    rest = [[wc.banded_input(ps[i], gpu, shift) for ps in params] for i in (1, 2, 3)]
    ys = [wc.banded((T, o), gpu, shift) for _, o in layers]
    sbuf, saved = wc.scratch(n_saved if keep else 0, gpu)
    n_ws = n_fwd + (0 if keep else n_saved)
    wbuf, ws = wc.scratch(n_ws, gpu)
    assert x.data_ptr() % 16 == 0 and all(A.data_ptr() % 16 == 0 for A in As)
    assert all(t.data_ptr() % 16 == 4 * shift for ts in rest for t in ts) and all(y[1].data_ptr() % 16 == 4 * shift for y in ys)
    assert ws.data_ptr() % 256 == 0 and saved.data_ptr() % 256 == 0 and ws.numel() == n_ws
    rc = lib.psf_mlp_wide_fwd_f32(x.data_ptr(), T, E, K, _ptrs(As), _ptrs(rest[0]), _ptrs(rest[1]), _ptrs(rest[2]), h, O,
                                  _ptrs([y[1] for y in ys]), saved.data_ptr() if keep else None, n_saved if keep else 0,
                                  ws.data_ptr(), n_ws, torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(rc, "psf_mlp_wide_fwd_f32")
    torch.cuda.synchronize(gpu)
    what = f"{name} forward (keep={keep}, shift={shift})"
    _outputs_ok([(f"Y[{k}]", y) for k, y in enumerate(ys)], what)
    assert wc.scratch_damage(wbuf, n_ws) == 0, f"{what}: wrote outside the workspace"
    assert wc.scratch_damage(sbuf, n_saved if keep else 0) == 0, f"{what}: wrote outside saved"
    return {"Y": [y[1].cpu().numpy() for y in ys], "saved": saved if keep else None, "_keep": sbuf}


def backward(gpu, name, saved, dYs=None, need_dx=True, shift=0, kind=None):
    """One raw psf_mlp_wide_bwd_f32 call from a forward's record. ``shift`` moves A, B, dY, dX and all gradients off their
    16-byte boundary. Returns {"dX": array or None, "grads": [(dA, da, dB, db)]}."""
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    T, E, layers = wc.CASES[name]
    _X, params, dY0, _ref, _exact = wc.problem(name, kind)
    K, h, O = _tables(layers)
    n_saved, _, n_bwd = _advertised(lib, name)
    As = [wc.banded_input(ps[0], gpu, shift) for ps in params]
    Bs = [wc.banded_input(ps[2], gpu, shift) for ps in params]
    gys = [wc.banded_input(d, gpu, shift) for d in (dY0 if dYs is None else dYs)]
    grads = [[wc.banded(ps[i].shape, gpu, shift) for ps in params] for i in range(4)]
    dx = wc.banded((T, E), gpu, shift)   # with need_dx False: a bystander that must stay untouched
    wbuf, ws = wc.scratch(n_bwd, gpu)
    assert saved.numel() == n_saved and saved.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0 and ws.numel() == n_bwd
    assert all(t.data_ptr() % 16 == 4 * shift for t in As + Bs + gys + [dx[1]] + [g[1] for gs in grads for g in gs])
    rc = lib.psf_mlp_wide_bwd_f32(saved.data_ptr(), n_saved, T, E, K, _ptrs(As), _ptrs(Bs), h, O, _ptrs(gys),
                                  dx[1].data_ptr() if need_dx else None, *[_ptrs([g[1] for g in gs]) for gs in grads],
                                  ws.data_ptr(), n_bwd, torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(rc, "psf_mlp_wide_bwd_f32")
    torch.cuda.synchronize(gpu)
    what = f"{name} backward (dX={need_dx}, shift={shift})"
    _outputs_ok([(f"{GRAD_NAMES[i]}[{k}]", g) for i, gs in enumerate(grads) for k, g in enumerate(gs)], what)
    if need_dx:
        _outputs_ok([("dX", dx)], what)
    else:
        assert wc.band_damage(dx[0], dx[2]) == 0 and wc.unwritten(dx[0], dx[2]) == T * E, f"{what}: touched a buffer it was not given"
    assert wc.scratch_damage(wbuf, n_bwd) == 0, f"{what}: wrote outside the workspace"
    return {"dX": dx[1].cpu().numpy() if need_dx else None,
            "grads": [tuple(grads[i][k][1].cpu().numpy() for i in range(4)) for k in range(K)]}


def _value(name, label, got, want, exact, tol):
    if exact:
        want = np.asarray(want).astype(np.float32)
        bad = got != want
        assert got.shape == want.shape and not bad.any(), (f"{name} {label}: {int(bad.sum())} of {bad.size} values differ from the exact answer, "
                                                           f"first at {np.argwhere(bad)[0].tolist()}")
    else:
        err = rel_inf(got, want)
        print(f"{name} {label}: {err:.3e} of max|reference| (bound {tol:.0e})")
        assert err <= tol, (name, label, err)


def check_forward(name, fwd, kind=None):
    _X, _p, _d, ref, exact = wc.problem(name, kind)
    for k, (y, want) in enumerate(zip(fwd["Y"], ref["Y"])):
        _value(name, f"Y[{k}]", y, want, exact, wc.TOL_FWD)


def check_backward(name, bwd, kind=None):
    _X, _p, _d, ref, exact = wc.problem(name, kind)
    if bwd["dX"] is not None:
        _value(name, "dX", bwd["dX"], ref["dX"], exact, wc.TOL_BWD)
    for k, (got, want) in enumerate(zip(bwd["grads"], ref["grads"])):
        for label, g, w in zip(GRAD_NAMES, got, want):
            _value(name, f"{label}[{k}]", g, w, exact, wc.TOL_BWD)


def _same(a, b, what):
    assert wc.same_bits(a, b), f"{what}: bits differ"


def _same_run(f1, b1, f2, b2, what, dx=True):
    for k, (u, v) in enumerate(zip(f1["Y"], f2["Y"])):
        _same(u, v, f"{what}: Y[{k}]")
    if b1 is None:
        return
    if dx:
        _same(b1["dX"], b2["dX"], f"{what}: dX")
    for k, (gu, gv) in enumerate(zip(b1["grads"], b2["grads"])):
        for label, u, v in zip(GRAD_NAMES, gu, gv):
            _same(u, v, f"{what}: {label}[{k}]")


_clean_cache = {}


def _clean(gpu, name):
    """The aligned, unpoisoned training run of a small case, checked against its reference once and shared."""
    if name not in _clean_cache:
        fwd = forward(gpu, name)
        bwd = backward(gpu, name, fwd["saved"])
        check_forward(name, fwd)
        check_backward(name, bwd)
        _clean_cache[name] = (fwd, bwd)
    return _clean_cache[name]


@pytest.mark.parametrize("name,kind", wc.TABLE_RUNS, ids=[f"{n}-{k or 'float64'}" for n, k in wc.TABLE_RUNS])
def test_raw_calls_stay_inside_exact_scratch_and_banded_outputs(gpu, name, kind):
    """The table of tests/wide_cases.py: one token, ragged everything, kMaxWideUnits and the kSlotClass slots of class 2, more
    work items than waves, the widest stacked GEMMs, and the split-K shapes (uneven, empty before the fix, the 64-split cap).
    On seeded dense operands against float64, and on a known-answer construction (equal bits) where the table names one."""
    fwd = forward(gpu, name, kind=kind)
    bwd = backward(gpu, name, fwd["saved"], kind=kind)
    check_forward(name, fwd, kind)
    check_backward(name, bwd, kind)


@pytest.mark.parametrize("name", wc.ALIGN)
def test_contract_only_alignment_gives_the_same_bits(gpu, name):
    """Every Y[k], dY[k], dX, a, B, b, dA, da, dB, db (and the backward's A) one float off its 16-byte boundary: the same
    arithmetic with another store width."""
    f0, b0 = _clean(gpu, name)
    f1 = forward(gpu, name, shift=1)
    b1 = backward(gpu, name, f1["saved"], shift=1)
    _same_run(f0, b0, f1, b1, f"{name} one float off")
    check_forward(name, f1)
    check_backward(name, b1)


@pytest.mark.parametrize("name", wc.NULL_DX)
def test_null_dx_changes_no_other_gradient(gpu, name):
    f0, b0 = _clean(gpu, name)
    b1 = backward(gpu, name, f0["saved"], need_dx=False)
    assert b1["dX"] is None
    _same_run(f0, b0, f0, b1, f"{name} dX = NULL", dx=False)


@pytest.mark.parametrize("name,fuse", [(n, f) for n in wc.FUSE for f in (1, 0)] + [("odd", 1)])
def test_inference_equals_training_forward(gpu, name, fuse):
    """saved = NULL with a workspace of exactly fwd_workspace + saved_bytes: the same Y as the call that keeps its record, with
    the second layers in the GEMM epilogue (wide_fuse 1) and in wide_out_k (0) — which again agree bit for bit."""
    import sparsefactorization_amd as sfa
    f0, _ = _clean(gpu, name)
    sfa.set_tuning("wide_fuse", fuse)
    try:
        inf = forward(gpu, name, keep=False)
        tr = forward(gpu, name)
        bwd = backward(gpu, name, tr["saved"])
    finally:
        sfa.set_tuning("wide_fuse", 1)
    _same_run(tr, None, inf, None, f"{name} inference (wide_fuse={fuse})")
    _same_run(f0, _clean(gpu, name)[1], tr, bwd, f"{name} wide_fuse={fuse} against the default")


def _with_row(a, t0, value):
    out = np.array(a, copy=True)
    out[t0, :] = value
    return out


def _rows_but(a, t0):
    return np.delete(a, t0, axis=0)


@pytest.mark.parametrize("t0", wc.LOCAL_TOKENS)
def test_nan_in_one_token_of_x_stays_in_that_token(gpu, t0):
    """Padded hidden rows (100 -> 128, 33 -> 64, J -> J_pad) and padded token rows carry zeros: 0 x NaN must not reach another
    token through them."""
    name = wc.LOCAL
    f0, _ = _clean(gpu, name)
    f1 = forward(gpu, name, X=_with_row(wc.problem(name)[0], t0, np.nan))
    for k, (y0, y1) in enumerate(zip(f0["Y"], f1["Y"])):
        assert np.isnan(y1[t0]).all(), (k, t0)
        _same(_rows_but(y0, t0), _rows_but(y1, t0), f"Y[{k}] away from token {t0}")


@pytest.mark.parametrize("t0", wc.LOCAL_TOKENS)
def test_nan_in_one_token_of_dy_stays_in_that_token_and_that_mlp(gpu, t0):
    name = wc.LOCAL
    f0, b0 = _clean(gpu, name)
    dYs = list(wc.problem(name)[2])
    k_bad = wc.LOCAL_TOKENS.index(t0) % len(dYs)
    dYs[k_bad] = _with_row(dYs[k_bad], t0, np.nan)
    b1 = backward(gpu, name, f0["saved"], dYs=dYs)
    assert np.isnan(b1["dX"][t0]).all()
    _same(_rows_but(b0["dX"], t0), _rows_but(b1["dX"], t0), f"dX away from token {t0}")
    for k, (g0, g1) in enumerate(zip(b0["grads"], b1["grads"])):
        for label, u, v in zip(GRAD_NAMES, g0, g1):
            if k == k_bad:
                assert np.isnan(v).all(), (label, k, t0)
            else:
                _same(u, v, f"{label}[{k}] with NaN in dY[{k_bad}]")


@pytest.mark.parametrize("t0", [31, 299])
def test_inf_in_one_token_stays_in_that_token(gpu, t0):
    """Locality only: the split of Inf into bf16 terms gives NaN terms (Inf - Inf), so the row's own content is not the
    float64 reference's (DESIGN.md records what it holds)."""
    name = wc.LOCAL
    f0, b0 = _clean(gpu, name)
    f1 = forward(gpu, name, X=_with_row(wc.problem(name)[0], t0, np.inf))
    for k, (y0, y1) in enumerate(zip(f0["Y"], f1["Y"])):
        _same(_rows_but(y0, t0), _rows_but(y1, t0), f"Y[{k}] away from the Inf token {t0}")
    print(f"Inf in X row {t0}: Y rows hold", [("nan" if np.isnan(y[t0]).all() else y[t0][:4].tolist()) for y in f1["Y"]])
    dYs = list(wc.problem(name)[2])
    dYs[1] = _with_row(dYs[1], t0, np.inf)
    b1 = backward(gpu, name, f0["saved"], dYs=dYs)
    _same(_rows_but(b0["dX"], t0), _rows_but(b1["dX"], t0), f"dX away from the Inf token {t0}")
    for label, u, v in zip(GRAD_NAMES, b0["grads"][0], b1["grads"][0]):
        _same(u, v, f"{label}[0] with Inf in dY[1]")
    print(f"Inf in dY[1] row {t0}: dX row", "nan" if np.isnan(b1["dX"][t0]).all() else b1["dX"][t0][:4].tolist(),
          "; gradients of MLP 1 all NaN:", [bool(np.isnan(v).all()) for v in b1["grads"][1]])


@pytest.mark.parametrize("name", wc.STALE)
def test_after_nan_in_every_lds(gpu, name):
    """x3_gemm_k keeps a 48 KB ring per stage set in LDS, wide_mid_k transposes through two LDS planes per wave: after launches
    that leave NaN in the LDS of every CU the bits are those of the unpoisoned run."""
    from test_gpu_stale_lds import _poison
    f0, b0 = _clean(gpu, name)
    _poison(gpu)
    f1 = forward(gpu, name)
    _poison(gpu)
    b1 = backward(gpu, name, f1["saved"])
    _same_run(f0, b0, f1, b1, f"{name} after NaN in LDS")


@pytest.mark.parametrize("name", wc.REPEAT)
def test_two_identical_raw_calls_give_identical_bits(gpu, name):
    f0, b0 = _clean(gpu, name)
    f1 = forward(gpu, name)
    b1 = backward(gpu, name, f1["saved"])
    _same_run(f0, b0, f1, b1, f"{name} repeated")
