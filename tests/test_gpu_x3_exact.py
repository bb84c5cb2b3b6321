"""GPU: known-answer tests of the split-bf16 producer kernels — every result bit-equal to the exact answer.

The inputs (tests/x3_exact.py) put every pre-activation in the linear GELU regime, every value on a grid where all partial
sums are exact in f32, and every product where the three term products the kernels drop are zero — while operands of
every GEMM carry nonzero third bf16 terms. The exact result is then the kernels' result whatever their summation order, so
a dropped split term, a wrong fragment, a lost plane or a mishandled tail shows as a wrong bit (the CPU self-tests in
test_x3_exact_cpu.py show that emulations of such defects change these answers).

Paths: psf_mlp_fwd_f32 (mlp_variant 1, 2, 3), psf_mlp_bwd_f32 (with and without dX), psf_mlp_wide_fwd_f32 /
psf_mlp_wide_bwd_f32 (wide_fuse 0 and 1) and psf_mixer_fwd_f32 (the per-step kernels and the single-launch mixer_lds).

Not covered here: dense operands through the curved part of GELU. The max-normalised bounds of test_gpu_producer.py and
test_gpu_wide_mlp.py hold them per tensor; test_gpu_x3_scaled.py (tests/x3_scaled.py, self-tests in test_x3_scaled_cpu.py)
holds every element against its own scale on 2^k-scaled tokens, columns, hidden rows and outputs, and the 2^k scaling laws.
"""
import numpy as np
import pytest
import torch

import x3_exact as xe
from oracle import chord_oracle as oc

pytestmark = pytest.mark.gpu

KINDS = ("x", "w", "dy")

NARROW, RESIDENT, WIDE, WIDE_FUSE, MIXER = xe.NARROW, xe.RESIDENT, xe.WIDE, xe.WIDE_FUSE, xe.MIXER


def _case(kind, path, T, E, layers):
    """The case whose exactness test_x3_exact_cpu.py::test_constructions_are_exact asserts (same seed)."""
    return xe.make_case(kind, T, E, layers, seed=xe.seed(path, T, E))


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


def _eq(got, want, what):
    got = got.detach().cpu().numpy()
    want = np.asarray(want).astype(np.float32)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}, "
                           f"max |diff| {np.abs(got.astype(np.float64) - want).max():.3e}")


def _check_forward(case, ys):
    for k, (y, want) in enumerate(zip(ys, case.reference()["Y"])):
        _eq(y, want, f"Y[{k}]")


def _check_backward(case, blocks, dx):
    ref = case.reference()
    if dx is not None:
        _eq(dx, ref["dX"], "dX")
    for k, (blk, (dA, da, dB, db)) in enumerate(zip(blocks, ref["grads"])):
        for name, p, want in (("dA", blk.network[0].weight, dA), ("da", blk.network[0].bias, da),
                              ("dB", blk.network[2].weight, dB), ("db", blk.network[2].bias, db)):
            assert p.grad is not None, (k, name)
            _eq(p.grad, want, f"{name}[{k}]")


@pytest.mark.parametrize("variant", [1, 3])
@pytest.mark.parametrize("kind", KINDS[:2])
@pytest.mark.parametrize("T,E,layers", NARROW)
def test_narrow_forward_is_exact(gpu, T, E, layers, kind, variant):
    """psf_mlp_fwd_f32: the split-bf16 kernel (variant 3) and the f32-MFMA kernel with streamed weights (variant 1)."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mlp
    case = _case(kind, "narrow", T, E, layers)
    blocks = _blocks(gpu, case)
    x = torch.from_numpy(case.X).to(gpu)
    sfa.set_tuning("mlp_variant", variant)
    try:
        with torch.no_grad():
            assert fused_mlp.eligible(x, blocks)
            ys = fused_mlp.fused_mlp_forward(x, blocks)
    finally:
        sfa.set_tuning("mlp_variant", 0)
    _check_forward(case, ys)


@pytest.mark.parametrize("kind", KINDS[:2])
@pytest.mark.parametrize("T,E,layers", RESIDENT)
def test_narrow_forward_resident_weights_is_exact(gpu, T, E, layers, kind):
    """psf_mlp_fwd_f32, mlp_variant 2 (f32 MFMA, weights resident in LDS)."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mlp
    case = _case(kind, "resident", T, E, layers)
    blocks = _blocks(gpu, case)
    x = torch.from_numpy(case.X).to(gpu)
    sfa.set_tuning("mlp_variant", 2)
    try:
        with torch.no_grad():
            ys = fused_mlp.fused_mlp_forward(x, blocks)
    finally:
        sfa.set_tuning("mlp_variant", 0)
    _check_forward(case, ys)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,E,layers", NARROW)
def test_narrow_backward_is_exact(gpu, T, E, layers, kind):
    """psf_mlp_fwd_f32 + psf_mlp_bwd_f32 under autograd (fused_mlp_apply): every output, dX and all four weight
    gradients bit-exact; and again with an input that needs no gradient (dX = NULL)."""
    from sparsefactorization_amd import fused_mlp
    case = _case(kind, "narrow", T, E, layers)
    blocks = _blocks(gpu, case)
    dys = [torch.from_numpy(d).to(gpu) for d in case.dYs]
    for need_dx in (True, False):
        for b in blocks:
            b.zero_grad(set_to_none=True)
        x = torch.from_numpy(case.X).to(gpu).requires_grad_(need_dx)
        assert fused_mlp.trainable(x, blocks)
        ys = fused_mlp.fused_mlp_apply(x, blocks)
        _check_forward(case, ys)
        torch.autograd.backward(ys, dys)
        _check_backward(case, blocks, x.grad if need_dx else None)


def _wide_run(gpu, case, fuse):
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mlp
    blocks = _blocks(gpu, case)
    dys = [torch.from_numpy(d).to(gpu) for d in case.dYs]
    sfa.set_tuning("wide_fuse", fuse)
    try:
        x0 = torch.from_numpy(case.X).to(gpu)
        with torch.no_grad():
            assert fused_mlp.wide_ok(x0, blocks)
            _check_forward(case, fused_mlp.wide_apply(x0, blocks))  # inference: no record kept
        x = x0.clone().requires_grad_(True)
        ys = fused_mlp.wide_apply(x, blocks)
        _check_forward(case, ys)
        torch.autograd.backward(ys, dys)
    finally:
        sfa.set_tuning("wide_fuse", 1)
    _check_backward(case, blocks, x.grad)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,E,layers", WIDE)
def test_wide_forward_backward_is_exact(gpu, T, E, layers, kind):
    """psf_mlp_wide_fwd_f32 / psf_mlp_wide_bwd_f32 through wide_apply: outputs, dX and the weight gradients bit-exact."""
    _wide_run(gpu, _case(kind, "wide", T, E, layers), 1)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,E,layers", WIDE_FUSE)
def test_wide_epilogue_second_layer_is_exact(gpu, T, E, layers, kind, fuse):
    """97..128 hidden rows everywhere: the second layer in the GEMM epilogue (wide_fuse 1) and in wide_out_k (0)."""
    _wide_run(gpu, _case(kind, "wide_fuse", T, E, layers), fuse)


@pytest.mark.parametrize("kind", KINDS[:2])
@pytest.mark.parametrize("name,B,N,E,h,C,L,M,residual,forms", MIXER, ids=[m[0] for m in MIXER])
def test_mixer_equals_exact_w_through_the_chain_and_the_oracle(gpu, name, B, N, E, h, C, L, M, residual, forms, kind):
    """psf_mixer_fwd_f32 computes W_m inside the chain step. With exact W_m, V0 it must equal, bit for bit, the chain
    (chord_chain) and the CPU oracle fed with those exact W_m and V0: the step sums the links in the oracle's order with
    uncontracted multiply and add (csrc/fwd_mlp_step.h). mixer_lds 1: the one-launch mixer, 0: the per-step kernels."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib, fused_mixer
    case = xe.mixer_case(kind, B, N, E, h, C, L, M, seed=N + E + h)  # exact: test_the_mixer_cases_are_exact
    blocks = _blocks(gpu, case)
    g, fs = blocks[0], blocks[1:]
    ys = [y.astype(np.float32).reshape(B, N, -1) for y in case.reference()["Y"]]
    V0, Ws = ys[0], ys[1:]
    rows, cols = oc.chord_indices(N, L)
    want = oc.chain(np.stack([rows, cols]), np.stack(Ws), V0, residual)[-1]
    x = torch.from_numpy(case.X.reshape(B, N, E)).to(gpu)
    with torch.no_grad():
        chain = sfa.chord_chain([torch.from_numpy(w).to(gpu) for w in Ws], torch.from_numpy(V0).to(gpu), residual)
        _eq(chain, want, "chord_chain(exact W) vs oracle")
        assert fused_mixer.covered(x, g, fs)
        sizes = fused_mixer._block_sizes(E, g, fs)  # (M, h table, C, L)
        for lds in forms:
            sfa.set_tuning("mixer_lds", lds)
            try:
                # no silent change of kernel: 2 = the single launch, 1 = the per-step kernels
                assert _lib.load().psf_mixer_fwd_plan(N, E, *sizes) == (2 if lds else 1), (name, lds)
                got = fused_mixer.mixer_forward(x, g, fs, residual)
            finally:
                sfa.set_tuning("mixer_lds", 1)
            _eq(got, want, f"mixer (mixer_lds={lds}) vs oracle")
