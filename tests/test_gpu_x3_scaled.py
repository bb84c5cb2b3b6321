"""GPU: componentwise accuracy and 2^k scaling laws of the split-bf16 producer MLPs on dense operands through the curved
part of GELU (tests/x3_scaled.py; its CPU self-tests are test_x3_scaled_cpu.py).

Accuracy. Every output element's error against the float64 reference (true erf-GELU, torch double on the GPU) is divided by
2^-24 times the element's own first-order scale sum |terms| — not by the tensor's maximum —, on operands whose tokens, columns,
hidden rows or outputs are scaled by powers of two from 2^-12 to 2^12. The worst ratio per output family must stay below a
threshold that is computed, when the test runs, from the documented arithmetic restated with f32 sums in both rounding
modes (x3_scaled.thresholds: never from a kernel). The CPU self-tests show that a dropped term product, zeroed third terms,
G from two bf16 planes and an error proportional to the tensor's maximum each land at least 2 x above it.

Scaling laws. (a) X[:, e] 2^k(e) with A[:, e] 2^-k(e) leaves every Y bit-identical; (b) B[o, :] 2^k, b[o] 2^k, dY[:, o] 2^-k
scales Y[:, o], dB[o, :], db[o] exactly and leaves dX, dA, da bit-identical; (c) dY[t, :] 2^k(t) scales dX[t, :] exactly.
They need no constant at all: a shared exponent, a flush to zero or a value-dependent path breaks them.

Paths: psf_mlp_fwd_f32 (mlp_variant 1, 2, 3), psf_mlp_fwd_f32 + psf_mlp_bwd_f32 under autograd with and without dX,
psf_mlp_wide_fwd_f32 / psf_mlp_wide_bwd_f32 (wide_fuse 0 and 1, inference and training) and psf_mixer_fwd_in_f32 (the
per-step kernels and the single launch; V_0 and every step output).

With X3_SCALED_RECORD set to a file name every measured ratio is appended there as a JSON line
(profiles/x3_componentwise.md).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import x3_scaled as xs

pytestmark = pytest.mark.gpu


def _blocks(gpu, case):
    from sparsefactorization_amd.psfnet import MLPBlock
    E = case.X.shape[1]
    blocks = []
    for A, a, B, b in case.params:
        blk = MLPBlock([A.shape[0], 'GELU'], E, B.shape[0])
        with torch.no_grad():
            for p, v in zip((blk.network[0].weight, blk.network[0].bias, blk.network[2].weight, blk.network[2].bias), (A, a, B, b)):
                p.copy_(torch.from_numpy(v))
        blocks.append(blk.to(gpu))
    return blocks


def _grads(blocks, ys, dx):
    out = {"Y": [y.detach() for y in ys], "dX": dx, "dA": [], "da": [], "dB": [], "db": []}
    for blk in blocks:
        for f, p in (("dA", blk.network[0].weight), ("da", blk.network[0].bias), ("dB", blk.network[2].weight),
                     ("db", blk.network[2].bias)):
            assert p.grad is not None, f
            out[f].append(p.grad.detach().clone())
    return out


# ---------------------------------------------------------------- the paths: case -> outputs in x3_scaled.reference's layout
def narrow_forward(gpu, variant):
    def run(case):
        import sparsefactorization_amd as sfa
        from sparsefactorization_amd import fused_mlp
        blocks = _blocks(gpu, case)
        x = torch.from_numpy(case.X).to(gpu)
        sfa.set_tuning("mlp_variant", variant)
        try:
            with torch.no_grad():
                assert fused_mlp.eligible(x, blocks)
                return {"Y": fused_mlp.fused_mlp_forward(x, blocks)}
        finally:
            sfa.set_tuning("mlp_variant", 0)
    return run


def narrow_apply(gpu, need_dx):
    def run(case):
        from sparsefactorization_amd import fused_mlp
        blocks = _blocks(gpu, case)
        x = torch.from_numpy(case.X).to(gpu).requires_grad_(need_dx)
        assert fused_mlp.trainable(x, blocks)
        ys = fused_mlp.fused_mlp_apply(x, blocks)
        torch.autograd.backward(ys, [torch.from_numpy(d).to(gpu) for d in case.dYs])
        return _grads(blocks, ys, x.grad if need_dx else None)
    return run


def wide(gpu, fuse, train):
    def run(case):
        import sparsefactorization_amd as sfa
        from sparsefactorization_amd import fused_mlp
        blocks = _blocks(gpu, case)
        x = torch.from_numpy(case.X).to(gpu)
        sfa.set_tuning("wide_fuse", fuse)
        try:
            assert fused_mlp.wide_ok(x, blocks)
            if not train:
                with torch.no_grad():
                    return {"Y": fused_mlp.wide_apply(x, blocks)}  # inference: no record kept
            x.requires_grad_(True)
            ys = fused_mlp.wide_apply(x, blocks)
            torch.autograd.backward(ys, [torch.from_numpy(d).to(gpu) for d in case.dYs])
        finally:
            sfa.set_tuning("wide_fuse", 1)
        return _grads(blocks, ys, x.grad)
    return run


def mixer(gpu, spec, lds):
    """psf_mixer_fwd_in_f32 through the raw entry point, as test_gpu_guard_bands.py calls it, but with a buffer of its own
    per step, so that every step output is kept (include/psf_chord.h: a step buffer that no later step overwrites is
    stored): {"V0": g(X) [B, N, C], "steps": [V_1 .. V_M]}."""
    def run(case):
        import sparsefactorization_amd as sfa
        from sparsefactorization_amd import _lib, fused_mixer, fused_mlp
        name, B, N, E, h, C, L, M, residual, _ = spec
        blocks = _blocks(gpu, case)
        g, fs = blocks[0], blocks[1:]
        xd = torch.from_numpy(case.X.reshape(B, N, E)).to(gpu)
        Mh, htab, C2, L2 = fused_mixer._block_sizes(E, g, fs)
        assert (Mh, C2, L2) == (M, C, L)
        lib = _lib.load()
        params = [p.detach().contiguous() for p in fused_mlp._params_of([g, *fs])]
        sfa.set_tuning("mixer_lds", lds)
        try:
            # no silent change of kernel: 2 = the single launch, 1 = the per-step kernels
            assert lib.psf_mixer_fwd_plan(N, E, M, htab, C, L) == (2 if lds else 1), (name, lds)
            ws_bytes = lib.psf_mixer_fwd_workspace(N, E, M, htab, C, L)
            assert ws_bytes >= 0
            ws = torch.empty(ws_bytes // 4 + 4, device=gpu)
            v0 = torch.empty(B, N, C, device=gpu)
            v0.fill_(float("nan"))
            bufs = [torch.full((B, N, C), float("nan"), device=gpu) for _ in range(M)]
            o_tab = (ctypes.c_void_p * M)(*[b.data_ptr() for b in bufs])
            spec_in = _lib.MixerInput(_lib.MIXER_IN_DATA, 0, xd.data_ptr(), None, None, None)
            ptrs = fused_mixer._ptrs
            rc = lib.psf_mixer_fwd_in_f32(ctypes.byref(spec_in), B, N, E, M, ptrs(params[0::4]), ptrs(params[1::4]),
                                          ptrs(params[2::4]), ptrs(params[3::4]), htab, C, L, 1 if residual else 0,
                                          v0.data_ptr(), o_tab, ws.data_ptr(), ws_bytes,
                                          torch.cuda.current_stream(gpu).cuda_stream)
            _lib.check(rc, "psf_mixer_fwd_in_f32")
            torch.cuda.synchronize(gpu)
        finally:
            sfa.set_tuning("mixer_lds", 1)
        return {"V0": v0, "steps": bufs}
    return run


# ---------------------------------------------------------------- accuracy
def _record(what, case, res):
    path = os.environ.get("X3_SCALED_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"run": what, "case": case.name, **{k: v[0] for k, v in res.items()}}) + "\n")


def _hold(what, path, case, res):
    """Every family's worst ratio is at most the path's threshold; the message names family, case, element and ratio."""
    thr = xs.thresholds(path)
    _record(what, case, res)
    bad = [f"{f}: ratio {r:.3g} > {thr[f]:.3g} at {where}" for f, (r, where) in res.items() if not r <= thr[f]]
    assert not bad, f"{what}, case {case.name}: " + "; ".join(bad)


def _accuracy(gpu, what, path, case, run, fams):
    """Runs the case and holds exactly the families ``fams``: one that the run does not return is a failure."""
    got = run(case)
    for f in fams:
        assert got.get(f) is not None and (f == "dX" or len(got[f]) == len(case.params)), f"{what}: no {f} ({case.name})"
    res = xs.ratios(case, got, gpu, fams)
    assert set(res) == set(fams)
    _hold(what, path, case, res)
    return got


ALL, NO_DX, FWD = xs.FAMILIES, tuple(f for f in xs.FAMILIES if f != "dX"), ("Y",)


NARROW_F32 = [(i, k, v) for i, k in xs.cases("narrow_f32") for v in (1, 2) if v == 1 or i in xs.RESIDENT_FITS]


@pytest.mark.parametrize("i,kind", xs.cases("narrow"))
def test_narrow_split_bf16_forward_and_backward_componentwise(gpu, i, kind):
    """mlp_variant 3 (psf_mlp_fwd_f32 on the bf16 pipe) and fused_mlp_apply with and without dX."""
    case = xs.case_of("narrow", i, kind)
    fwd = _accuracy(gpu, "fused_mlp_forward mlp_variant=3", "narrow", case, narrow_forward(gpu, 3), FWD)
    full = _accuracy(gpu, "fused_mlp_apply", "narrow", case, narrow_apply(gpu, True), ALL)
    nodx = _accuracy(gpu, "fused_mlp_apply without dX", "narrow", case, narrow_apply(gpu, False), NO_DX)
    assert nodx["dX"] is None
    for a, b in zip(fwd["Y"], full["Y"]):
        assert torch.equal(a, b)  # the default forward is variant 3 at these widths


@pytest.mark.parametrize("i,kind,variant", NARROW_F32)
def test_narrow_f32_matrix_instruction_forward_componentwise(gpu, i, kind, variant):
    """mlp_variant 1 (streamed weights) and 2 (weights resident in LDS, where the K images fit): erf form of GELU."""
    case = xs.case_of("narrow_f32", i, kind)
    _accuracy(gpu, f"fused_mlp_forward mlp_variant={variant}", "narrow_f32", case, narrow_forward(gpu, variant), FWD)


@pytest.mark.parametrize("i,kind", xs.cases("wide"))
def test_wide_forward_and_backward_componentwise(gpu, i, kind):
    case = xs.case_of("wide", i, kind)
    inf = _accuracy(gpu, "wide_apply inference", "wide", case, wide(gpu, 1, False), FWD)
    tr = _accuracy(gpu, "wide_apply training", "wide", case, wide(gpu, 1, True), ALL)
    assert all(torch.equal(a, b) for a, b in zip(inf["Y"], tr["Y"]))


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("i,kind", xs.cases("wide_fuse"))
def test_wide_second_layer_in_the_epilogue_componentwise(gpu, i, kind, fuse):
    case = xs.case_of("wide_fuse", i, kind)
    _accuracy(gpu, f"wide_apply inference wide_fuse={fuse}", "wide_fuse", case, wide(gpu, fuse, False), FWD)
    _accuracy(gpu, f"wide_apply training wide_fuse={fuse}", "wide_fuse", case, wide(gpu, fuse, True), ALL)


MIXER_RUNS = [(i, k, lds) for i, k in xs.cases("mixer") for lds in xs.MIXER[i][9]]


@pytest.mark.parametrize("i,kind,lds", MIXER_RUNS, ids=[f"{xs.MIXER[i][0]}-{k}-lds{lds}" for i, k, lds in MIXER_RUNS])
def test_mixer_componentwise(gpu, i, kind, lds):
    """V_0 = g(X) and every step output V_1 .. V_M of the W-in-the-step mixer against the float64 chain fed with
    float64-MLP W; a step's scale adds its own sum |w||v| and what W's and V's scales leave in it
    (x3_scaled.mixer_reference). V_0 is an MLP output and is held to the path's Y threshold."""
    case, spec = xs.case_of("mixer", i, kind), xs.MIXER[i]
    got = mixer(gpu, spec, lds)(case)
    assert all(bool(torch.isfinite(v).all()) for v in [got["V0"], *got["steps"]])  # every step written, none left NaN
    ref, S = xs.reference(case, gpu, backward=False)
    r0, i0 = xs.ratio(got["V0"].reshape(ref["Y"][0].shape), ref["Y"][0], S["Y"][0])
    where0 = f"element {np.unravel_index(i0, tuple(ref['Y'][0].shape))}"
    _hold(f"psf_mixer_fwd_in_f32 mixer_lds={lds}", "mixer", case, {"Y": (r0, where0), "V": xs.mixer_ratio(case, spec, got["steps"])})


# ---------------------------------------------------------------- scaling laws (one kind per shape: the first listed)
def _first(path):
    return [(i, xs.PATHS[path]["shapes"][i][3][0]) for i in range(len(xs.PATHS[path]["shapes"]))]


@pytest.mark.parametrize("i,kind", _first("narrow"))
def test_narrow_scaling_laws(gpu, i, kind):
    case = xs.case_of("narrow", i, kind)
    xs.check_laws(case, narrow_apply(gpu, True))
    xs.check_laws(case, narrow_forward(gpu, 3), laws=("a", "b"))
    for variant in (1, 2):  # the f32 matrix instruction: law (a) alone
        if variant == 1 or i in xs.RESIDENT_FITS:
            xs.check_laws(case, narrow_forward(gpu, variant), laws=("a",))


@pytest.mark.parametrize("i,kind", _first("wide"))
def test_wide_scaling_laws(gpu, i, kind):
    case = xs.case_of("wide", i, kind)
    xs.check_laws(case, wide(gpu, 1, True))
    xs.check_laws(case, wide(gpu, 1, False), laws=("a", "b"))


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("i,kind", _first("wide_fuse"))
def test_wide_epilogue_scaling_laws(gpu, i, kind, fuse):
    case = xs.case_of("wide_fuse", i, kind)
    xs.check_laws(case, wide(gpu, fuse, True))
    xs.check_laws(case, wide(gpu, fuse, False), laws=("a", "b"))


@pytest.mark.parametrize("i,lds", [(i, lds) for i in range(len(xs.MIXER)) for lds in xs.MIXER[i][9]],
                         ids=[f"{xs.MIXER[i][0]}-lds{lds}" for i in range(len(xs.MIXER)) for lds in xs.MIXER[i][9]])
def test_mixer_scaling_law_a(gpu, i, lds):
    """X[:, e] 2^k(e) with A[:, e] 2^-k(e): the same W bit for bit, so the same V_1 .. V_M."""
    case, spec = xs.case_of("mixer", i, "flat"), xs.MIXER[i]
    run = mixer(gpu, spec, lds)
    base = [v.clone() for v in run(case)["steps"]]
    scaled = xs.law_a(case, np.random.default_rng(5))
    xs.check_normal(scaled)
    for m, (v, v0) in enumerate(zip(run(scaled)["steps"], base)):
        assert torch.equal(v, v0), f"law a: V_{m + 1} changes under X 2^k, A 2^-k ({case.name}, mixer_lds={lds})"
