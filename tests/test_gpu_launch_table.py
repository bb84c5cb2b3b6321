"""GPU: every link count of every launcher of the *_inst.hip units reaches its own instance, and the dynamic-LDS limit of a
kernel is raised whenever a launch needs more than every launch before it.

The launchers turn a run-time L into a template instance (csrc/psf_common.h: with_int) and allow a kernel more than 48 KB of
dynamic LDS before the first launch that asks for it (allow_dynamic_lds). A wrong (L -> instance) mapping is wrong at any
size, so every L of a family's compiled range runs once at the smallest N for which psf_describe_* names the family (walked
upward on the host, at most to 8192), plus Lmin - 1 and Lmax + 1 through whatever route the planner picks for them.

Only bit equality with the CPU oracle is asserted. f32: the oracle's bits. bf16: bf16_rne of the oracle's f32 result on the
upcast operands (tests/test_gpu_bf16.py). dW sums run in another order than the oracle's, so the backward cases use the
integer operands of tests/bf16_edges.py (int_case: every partial sum is an exact f32 integer in any order), which leaves one
correct dW: the oracle's bits in f32, rne_bits(exact) in bf16 — the verdict of test_dw_known_answers_bit_for_bit.

The one exception is the step kernel that computes its own W tile (fwd_mlp_step_inst.hip): its W comes from split-bf16 GEMMs
and meets the oracle to 1e-5, not bit for bit, so that family keeps the verdict of tests/test_gpu_mixer.py unchanged
(rel_inf <= 1e-5 against the oracle's chain fed with the MLPs in float64). A wrong instance reads another link count and
misses by O(1).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_edges as be
from oracle import chord_oracle as oc
from sparsefactorization_amd._lib import tuning

pytestmark = pytest.mark.gpu

N_MAX = 8192
WIN_L = range(4, 21)    # kWinLmin..kWinLmax, also the fused steps' and the chunk dW's
CHAIN_L = range(2, 21)  # kChainLdsLmin..kChainLdsLmax

# family: (describe entry, element bytes, C, knobs, what the string must show for L)
FAMILIES = {
    "fwd_f32": ("fwd", 4, 8, {}, ["chord_fwd_win_k<f32,L={L},"]),
    "fwd_bf16": ("fwd", 2, 8, {}, ["chord_fwd_win_k<bf16,L={L},"]),
    "win_f32": ("bwd", 4, 8, {"bwd_fused": 0}, ["chord_dw_win_k<f32,L={L},", "chord_dv_win_k<f32,L={L},"]),
    "win_bf16": ("bwd", 2, 8, {"bwd_fused": 0}, ["chord_dw_win_k<bf16,L={L},", "chord_dv_win_k<bf16,L={L},"]),
    "chunk_f32": ("bwd", 4, 32, {"bwd_fused": 0}, ["chord_dw_chunk_k<f32,L={L},"]),
    "fused_f32": ("bwd", 4, 8, {"bwd_fused": 2}, ["chord_bwd_fused_k<f32,L={L},"]),
    "fused_edge_f32": ("bwd", 4, 8, {"bwd_fused": 1}, ["chord_bwd_fused_edge_k<f32,L={L},"]),
    "fused_bf16": ("bwd", 2, 8, {"bwd_fused": 2}, ["chord_bwd_fused_k<bf16,L={L},"]),
    "chain_f32": ("chain", 4, 8, {"chain_fused": 2}, ["chord_chain_lds_k<f32,L={L},"]),
    "chain_bf16": ("chain", 2, 8, {"chain_fused": 2}, ["chord_chain_lds_k<bf16,L={L},"]),
    "rows_f32": ("chain", 4, 8, {"chain_fused": 2, "chain_cc": 2}, ["chord_chain_rows_k<f32,L={L},"]),
    "rows_bf16": ("chain", 2, 8, {"chain_fused": 2, "chain_cc": 2}, ["chord_chain_rows_k<bf16,L={L},"]),
}
B, M = 2, 2  # batch elements; steps of a chain


def _describe(family, N, L, batch=B, C=None):
    from sparsefactorization_amd import _lib
    entry, eb, C0, _knobs, _subs = FAMILIES[family]
    C = C0 if C is None else C
    if entry == "fwd":
        return _lib.describe_fwd(batch, N, L, C, elem_bytes=eb)
    if entry == "bwd":
        return _lib.describe_bwd(batch, N, L, C, elem_bytes=eb)
    return _lib.describe_chain_fwd(batch, N, L, C, M, elem_bytes=eb)


def _names(family, s, L, also=()):
    return all(x.format(L=L) in s for x in FAMILIES[family][4]) and all(x in s for x in also)


# the knobs that decide a route stand at their defaults while N is walked, whatever the caller has set (the answer is cached)
ROUTE_DEFAULTS = {"fwd_variant": 0, "bwd_variant": 0, "fwd_split": 1, "fwd_wide": 0, "dw_variant": 0, "dv_threads": 0, "bwd_fused": 1,
                  "dw_tgs": 0, "fwd_rows": 0, "chain_fused": 1, "chain_cc": 0}


@functools.lru_cache(maxsize=None)
def _smallest_n(family, L, also=(), batch=B, C=None):
    """The smallest N at which describe names the family's kernel for L (and every string of `also`), or None. Host only."""
    with tuning(**{**ROUTE_DEFAULTS, **FAMILIES[family][3]}):
        for N in range(1, N_MAX + 1):
            if _names(family, _describe(family, N, L, batch, C), L, also):
                return N
    return None


def _confirm(family, N, L, also=(), batch=B, C=None):
    """Under the family's knobs (set by the caller): the case takes the kernel it was written for."""
    assert N is not None, f"{family}: no N <= {N_MAX} takes the kernel for L = {L}"
    s = _describe(family, N, L, batch, C)
    assert _names(family, s, L, also), f"{family} N={N} L={L}: {s}"
    return s


# ---------------------------------------------------------------- operands and verdicts
def _dtype(eb):
    return torch.float32 if eb == 4 else torch.bfloat16


def _dev(a, eb, gpu):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(_dtype(eb)).to(gpu)


def _bits(t):
    """The raw bits of a result as a numpy integer array."""
    t = t.detach().contiguous().cpu()
    return t.view(torch.int32).numpy().view(np.uint32) if t.dtype == torch.float32 else t.view(torch.int16).numpy().view(np.uint16)


def _want_bits(a_f32, eb):
    a = np.ascontiguousarray(a_f32, dtype=np.float32)
    return a.view(np.uint32) if eb == 4 else be.rne_bits(a)


def _assert_bits(got, want_f32, eb, what):
    got, want = _bits(got).ravel(), _want_bits(want_f32, eb).ravel()
    bad = int((got != want).sum()) if eb == 4 else be.same_bits(got, want)
    assert bad == 0, f"{what}: {bad} of {want.size} elements differ from the oracle's bits"


def _fwd_case(gpu, eb, N, L, C, offsets, what):
    import sparsefactorization_amd as sfa
    W, V, R = be.normal_case((B, N, L), 1, 0.5), be.normal_case((B, N, C), 2), be.normal_case((B, N, C), 3)
    ref = oc.spmul_fwd(W, V, offsets)
    for res in (None, R):
        got = sfa.chord_spmm(_dev(W, eb, gpu), _dev(V, eb, gpu), None if res is None else _dev(res, eb, gpu), offsets=offsets)
        _assert_bits(got, ref if res is None else ref + res, eb, f"{what} residual={res is not None}")


def _bwd_case(gpu, eb, batch, N, L, C, what):
    from sparsefactorization_amd.chord import _launch_bwd
    dZ, V, W = be.int_case((batch, N, C), 50 + L), be.int_case((batch, N, C), 51 + L), be.normal_case((batch, N, L), 52, 0.5)
    dF, dV = oc.spmul_bwd(dZ, W, V)
    exact, _ = be.dw_sums(dZ, V, L)
    assert np.abs(exact).max() < 2.0 ** 24 and np.array_equal(exact.astype(np.float32), dF)  # (one correct dW, the oracle's)
    gW = torch.full((batch, N, L), float("nan"), device=gpu, dtype=_dtype(eb))
    gV = torch.full((batch, N, C), float("nan"), device=gpu, dtype=_dtype(eb))
    _launch_bwd(_dev(dZ, eb, gpu), _dev(W, eb, gpu), _dev(V, eb, gpu), gW, gV, batch, N, L, C, N * C, None)
    _assert_bits(gW, dF, eb, f"{what} dW")
    _assert_bits(gV, dV, eb, f"{what} dV")


def _chain_case(gpu, eb, N, L, C, what):
    import sparsefactorization_amd as sfa
    Ws = [be.normal_case((B, N, L), 60 + m, 0.4) for m in range(M)]
    V0 = be.normal_case((B, N, C), 59)
    for residual in (False, True):
        X = V0
        for W in Ws:  # every step: the oracle in f32 (+ V0), stored once (bf16: rounded once)
            X = oc.spmul_fwd(W, X)
            X = (X + V0).astype(np.float32) if residual else X
            X = X if eb == 4 else be.as_bf16(X)
        with torch.no_grad():
            got = sfa.chord_chain([_dev(W, eb, gpu) for W in Ws], _dev(V0, eb, gpu), residual)
        _assert_bits(got, X, eb, f"{what} residual={residual}")


# ---------------------------------------------------------------- 1. every link count of every launcher
def _far(s):
    return int(re.search(r"far=(\d+)", s).group(1))


@pytest.mark.parametrize("L", WIN_L)
@pytest.mark.parametrize("family", ["fwd_f32", "fwd_bf16"])
def test_forward_window_every_link_count(gpu, family, L):
    """Aligned tiles (MODE 2), a ragged N (MODE 1), and full tiles with a far offset off the tile grid (MODE 0: no scalar block
    addresses). MODE 0 needs a far link: while every link is near, N % TR == 0 alone makes the launch aligned. At C = 8 the
    tiles hold 256 (f32) or 512 (bf16) rows, which leaves far links from L = 11 / 12 on, so MODE 0 runs at the narrowest of
    C = 8 .. 256 whose tile is short enough for L to have one (f32, shortest tile 8 rows: every L >= 6; bf16, shortest tile 32
    rows: every L >= 8), and below that no shape reaches the instance. describe knows chord offsets only: it confirms the aligned
    launch of the same shape, not the offset that turns it into MODE 0."""
    from sparsefactorization_amd import _lib
    _e, eb, C, knobs, _s = FAMILIES[family]
    aligned = ("tiles=full, aligned",)
    N = _smallest_n(family, L, aligned)
    with tuning(**knobs):
        _confirm(family, N, L, aligned)
        _fwd_case(gpu, eb, N, L, C, None, f"{family} L={L} N={N} aligned")
        s = _confirm(family, N + 1, L)
        assert s.endswith("tiles=edge") or s.endswith("tiles=full+ragged"), s
        _fwd_case(gpu, eb, N + 1, L, C, None, f"{family} L={L} N={N + 1} ragged")
        shape = _full_mode_shape(family, L)
        assert (shape is not None) == (L >= (6 if eb == 4 else 8)), shape
        if shape is not None:
            Cf, Nf = shape
            assert _far(_confirm(family, Nf, L, aligned, C=Cf)) > 0
            off = _lib.chord_offsets(Nf, L)
            off[-1] = (off[-1] + 1) % Nf
            _fwd_case(gpu, eb, Nf, L, Cf, off, f"{family} L={L} N={Nf} C={Cf} full")


@functools.lru_cache(maxsize=None)
def _full_mode_shape(family, L):
    """(C, N): the narrowest rows, then the shortest sequence, whose aligned launch has a far link; None where there is none
    (two tiles are at most 1024 rows, so N is walked to 2048)."""
    with tuning(**{**ROUTE_DEFAULTS, **FAMILIES[family][3]}):
        for C in (8, 16, 32, 64, 128, 256):
            for N in range(1, 2049):
                s = _describe(family, N, L, B, C)
                if _names(family, s, L, ("tiles=full, aligned",)) and _far(s) > 0:
                    return C, N
    return None


@pytest.mark.parametrize("L", WIN_L)
@pytest.mark.parametrize("family,batch", [("win_f32", 2), ("win_bf16", 2), ("chunk_f32", 2), ("fused_f32", 2), ("fused_edge_f32", 2),
                                          ("fused_bf16", 2), ("fused_bf16", 1)])
def test_backward_steps_every_link_count(gpu, family, batch, L):
    _e, eb, C, knobs, _s = FAMILIES[family]
    N = _smallest_n(family, L, (), batch)
    with tuning(**knobs):
        _confirm(family, N, L, (), batch)
        _bwd_case(gpu, eb, batch, N, L, C, f"{family} B={batch} L={L} N={N}")


@pytest.mark.parametrize("L", CHAIN_L)
@pytest.mark.parametrize("family", ["chain_f32", "chain_bf16", "rows_f32", "rows_bf16"])
def test_forward_chain_every_link_count(gpu, family, L):
    _e, eb, C, knobs, _s = FAMILIES[family]
    N = _smallest_n(family, L)
    with tuning(**knobs):
        _confirm(family, N, L)
        _chain_case(gpu, eb, N, L, C, f"{family} L={L} N={N}")


def _bwd_chain_case(gpu, N, L, C, residual, integers=False):
    """psf_chord_chain_bwd_f32's one launch: dV0 and every dW_m are the oracle's per-step backward, the residual terms summed
    left to right (tests/test_gpu_parity.py: test_backward_chain_in_one_launch). `integers`: for the per-step kernels, whose dW
    sums run in another order: W in [-2, 2], V0 and dOut in [-15, 15] keep every value of the two steps an integer below 2^24,
    exact in any order."""
    import sparsefactorization_amd as sfa
    if integers:
        W = [np.random.default_rng(81 + m).integers(-2, 3, size=(B, N, L)).astype(np.float32) for m in range(M)]
        V0, gout = be.int_case((B, N, C), 80), be.int_case((B, N, C), 79)
    else:
        W = [be.normal_case((B, N, L), 81 + m, 0.4) for m in range(M)]
        V0, gout = be.normal_case((B, N, C), 80), be.normal_case((B, N, C), 79)
    X = [V0]
    for m in range(M):
        nxt = oc.spmul_fwd(W[m], X[-1])
        X.append((nxt + V0).astype(np.float32) if residual else nxt)
    g, want_dW, terms = gout, [None] * M, []
    for m in range(M - 1, -1, -1):
        terms.append(g)
        want_dW[m], g = oc.spmul_bwd(g, W[m], X[m])
    if residual:
        acc = terms[0]
        for t in terms[1:] + [g]:
            acc = (acc + t).astype(np.float32)
        g = acc
    Wg = [_dev(w, 4, gpu).requires_grad_(True) for w in W]
    Vg = _dev(V0, 4, gpu).requires_grad_(True)
    sfa.chord_chain(Wg, Vg, residual).backward(_dev(gout, 4, gpu))
    _assert_bits(Vg.grad, g, 4, f"bwd chain L={L} dV0")
    for m in range(M):
        _assert_bits(Wg[m].grad, want_dW[m], 4, f"bwd chain L={L} dW_{m}")


@pytest.mark.parametrize("L", CHAIN_L)
def test_backward_chain_every_link_count(gpu, L):
    """No describe entry names this kernel: psf_chord_chain_bwd_supported says whether the one launch takes the shape."""
    from sparsefactorization_amd import _lib
    N, C = 100, 8
    assert _lib.load().psf_chord_chain_bwd_supported(N, L, C, M) == 1
    for residual in (False, True):
        _bwd_chain_case(gpu, N, L, C, residual)


@pytest.mark.parametrize("L", range(3, 22))  # kMlpStepLmin - 1 .. kMlpStepLmax + 1
def test_mixer_step_kernel_every_link_count(gpu, L):
    """chord_fwd_mlp_k (knob mixer_lds = 0 keeps short sequences off the single-launch mixer) at the smallest N that
    psf_mixer_fwd_plan gives to the step kernels. L = 3 and 21 are outside the fused path: the MLPs, then the chain."""
    import ctypes
    import sparsefactorization_amd as sfa
    from conftest import rel_inf
    from sparsefactorization_amd import _lib, fused_mixer
    from test_gpu_mixer import TOL, _blocks, _reference
    E, h, C = 32, 32, 8
    hs = (ctypes.c_int32 * (M + 1))(*[h] * (M + 1))
    plan = lambda n, l: _lib.load().psf_mixer_fwd_plan(n, E, M, hs, C, l)  # noqa: E731
    with tuning(mixer_lds=0):
        N = next(n for n in range(1, N_MAX + 1) if plan(n, min(max(L, 4), 20)) == 1)
        assert plan(N, L) == (1 if 4 <= L <= 20 else 0)
        g, fs = _blocks(E, h, C, L, M, seed=11)
        x = torch.randn(B, N, E, generator=torch.Generator().manual_seed(5))
        want = {res: _reference(x, g, fs, res)[0] for res in (False, True)}
        for blk in (g, *fs):
            blk.to(gpu)
        xd = x.to(gpu)
        for res in (False, True):
            with torch.no_grad():
                if 4 <= L <= 20:
                    assert fused_mixer.covered(xd, g, fs)
                    got = fused_mixer.mixer_forward(xd, g, fs, res)
                else:
                    assert not fused_mixer.covered(xd, g, fs)
                    got = sfa.chord_chain([f(xd) for f in fs], g(xd), res)
            got = got.cpu().numpy()
            assert np.isfinite(got).all()
            assert rel_inf(got, want[res]) <= TOL, f"L={L} N={N} residual={res}: rel {rel_inf(got, want[res]):.3e}"


@pytest.mark.parametrize("family,L", [(f, L) for f in ("fwd_f32", "fwd_bf16", "win_f32", "win_bf16", "chunk_f32", "fused_f32",
                                                       "fused_edge_f32", "fused_bf16") for L in (3, 21)]
                         + [(f, L) for f in ("chain_f32", "chain_bf16", "rows_f32", "rows_bf16", "bwd_chain") for L in (1, 21)])
def test_one_link_count_outside_the_compiled_range(gpu, family, L):
    """Lmin - 1 and Lmax + 1 at the N of Lmin and Lmax, through whatever route the planner picks: the oracle's bits."""
    if family == "bwd_chain":
        from sparsefactorization_amd import _lib
        assert _lib.load().psf_chord_chain_bwd_supported(100, L, 8, M) == 0
        for residual in (False, True):
            _bwd_chain_case(gpu, 100, L, 8, residual, integers=True)
        return
    entry, eb, C, knobs, _s = FAMILIES[family]
    N = _smallest_n(family, L + 1 if L < 4 else L - 1)
    with tuning(**knobs):
        assert not _names(family, _describe(family, N, L), L)
        if entry == "fwd":
            _fwd_case(gpu, eb, N, L, C, None, f"{family} L={L} N={N}")
        elif entry == "bwd":
            _bwd_case(gpu, eb, B, N, L, C, f"{family} L={L} N={N}")
        else:
            _chain_case(gpu, eb, N, L, C, f"{family} L={L} N={N}")


# ---------------------------------------------------------------- 2. first-launch state of the LDS raise
def _child(gpu):
    """In a fresh process (the high-water marks are per process): requests below 48 KB, then above it on instances that have
    already run, then below again; a missed raise is a launch error from the library."""
    from sparsefactorization_amd import _lib
    L, C = 8, 8
    # The library does not report a launch's LDS request, so the crossing is checked on the sizes themselves: the instances' own
    # LDS (FwdWinCfg<float, 8, 1, 2, 256>, BwdFusedCfg<8, 1, 256>, BwdFusedBf16Cfg<8, 0, 256>::lds_bytes: the instances that
    # _confirm names below) and the limiter's rule (psf_common.h: lds_for_wg_limit).
    own = {"fwd_f32": 28672, "fused_f32": 24576, "fused_bf16": 24576}
    want_name = {"fwd_f32": "chord_fwd_win_k<f32,L=8,TG=2,R=2,NT=256>", "fused_f32": "chord_bwd_fused_k<f32,L=8,TG=2,NT=256>",
                 "fused_bf16": "chord_bwd_fused_k<bf16,L=8,TG=1,NT=256>"}
    request = lambda own_bytes, n: max(own_bytes, 160 * 1024 // (n + 1) + 256)  # noqa: E731  (both floors are below 64 KB)
    shapes = {"fwd_f32": _smallest_n("fwd_f32", L, ("tiles=full, aligned",)), "fused_f32": _smallest_n("fused_f32", L),
              "fused_bf16": _smallest_n("fused_bf16", L)}
    for limit in (3, 2, 3):
        with tuning(fwd_wg_limit=limit, bwd_fused_wg_limit=limit, bwd_fused=2):
            assert _lib.get_tuning("fwd_wg_limit") == limit and _lib.get_tuning("bwd_fused_wg_limit") == limit
            for family, N in shapes.items():
                assert _confirm(family, N, L).startswith(want_name[family])
                assert (request(own[family], limit) > 48 * 1024) == (limit == 2), (family, limit)
                if family == "fwd_f32":
                    _fwd_case(gpu, 4, N, L, C, None, f"forward, limit {limit}")
                else:
                    _bwd_case(gpu, FAMILIES[family][1], B, N, L, C, f"{family}, limit {limit}")
    with tuning(chain_fused=2):
        for N, lds in ((600, 38400), (1000, 64000)):  # 2 buffers x 2 N slots x 16 bytes on chord_chain_lds_k<L, 2, 2, RES, 1024>
            s = _confirm("chain_f32", N, L, ("CC=2,R=2",))
            assert int(re.search(r"(\d+) threads", s).group(1)) > 512 and 2 * 2 * N * 16 == lds, s
            _chain_case(gpu, 4, N, L, C, f"chain N={N}")
    print("LDS_RAISE_OK")


def test_lds_limit_is_raised_on_instances_that_have_already_run(gpu):
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]\n"
            "import torch, test_gpu_launch_table as t\nt._child(torch.device('cuda:0'))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "LDS_RAISE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
