"""GPU: the mixer whose steps compute their own W tile (psf_mixer_fwd_f32, csrc/fwd_mlp_step.h)
against the CPU oracle's chain fed with W_m = fs[m](data) evaluated in float64.

What is compared: V_M of ``V = g(data); for m: V = spmm(idx, fs[m](data), V) (+ V0)`` (SyntheticExperiments/psf.py:165-188).
Reference: the MLPs in float64 torch on the CPU, their outputs rounded to f32, then the oracle's f32 chain (links ascending).
Tolerance: max|a - b| <= 1e-5 max|ref| (BASELINE.json) — the fused path's W carries the split-bf16 GEMMs' ~1e-7 relative
error instead of the f32 rounding of a float64 result, everything after it is the oracle's arithmetic in the oracle's order.
"""

import numpy as np
import pytest
import torch
from torch import nn

from conftest import rel_inf
from oracle import chord_oracle as oc

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _blocks(E, h, C, L, M, seed):
    from sparsefactorization_amd.psfnet import MLPBlock
    torch.manual_seed(seed)
    g = MLPBlock([h, 'GELU'], E, C)
    fs = [MLPBlock([h, 'GELU'], E, L) for _ in range(M)]
    return g, fs


def _reference(x, g, fs, residual):
    """float64 MLPs on the CPU -> f32 operands -> the oracle's chain."""
    B, N, _ = x.shape
    with torch.no_grad():
        x64 = x.double()
        V0 = g.double()(x64).float().numpy()
        Ws = [f.double()(x64).float().numpy() for f in fs]
        g.float()
        for f in fs:
            f.float()
    L = Ws[0].shape[-1]
    rows, cols = oc.chord_indices(N, L)
    index = np.stack([rows, cols])
    return oc.chain(index, np.stack(Ws), V0, residual)[-1], V0


# (name, B, N, E, h, C, L, M, residual) — BASELINE configs[1] / [4] (Adding, Temporal Order), the Pathfinder, CIFAR-10, IMDb
# (ragged N, residual) and genome networks, plus shapes that exercise partial feature groups, channel groups that are
# not a power of two, a hidden layer that is not a multiple of 32 and the smallest legal N (two tiles)
CASES = [
    ("cfg2", 3, 16384, 32, 32, 8, 15, 14, True),
    ("pathfinder", 3, 1024, 32, 128, 32, 12, 11, False),
    ("cifar10", 3, 1024, 16, 16, 16, 11, 10, False),
    ("imdb", 2, 4097, 32, 128, 32, 13, 12, True),
    ("genome", 1, 16384, 32, 32, 32, 15, 14, False),
    ("odd", 2, 600, 12, 40, 12, 9, 5, True),
    ("c4", 2, 1000, 8, 24, 4, 10, 4, False),
    ("two_tiles", 2, 512, 32, 32, 8, 10, 9, True),
    ("h96", 2, 2048, 32, 96, 32, 12, 3, True),
    # the ends of the compiled ranges: L = 20 (N = 2^19: two steps keep the float64 reference cheap), L = 4, E = 4, C = 16 at
    # the smallest N with 16-channel rows (two 128-row tiles)
    ("l20_n512k", 1, 1 << 19, 32, 32, 8, 20, 2, True),
    ("l4_e4", 3, 512, 4, 8, 4, 4, 3, False),
    ("c16_two_tiles", 2, 256, 32, 32, 16, 9, 8, True),
    # the single-launch LDS-resident mixer (csrc/mixer_lds.h): BASELINE configs[0] and the other shapes of its plan
    ("cfg1", 40, 128, 32, 32, 8, 8, 7, True),
    ("lds_n512", 3, 512, 32, 32, 8, 10, 9, True),
    ("lds_n256_nores", 5, 256, 32, 32, 8, 9, 8, False),
    ("lds_c4_h128", 3, 256, 16, 128, 4, 9, 8, True),
    ("lds_n64", 7, 64, 32, 32, 8, 7, 6, True),
]


@pytest.mark.parametrize("name,B,N,E,h,C,L,M,residual", CASES, ids=[c[0] for c in CASES])
def test_mixer_matches_the_oracle_chain_fed_with_float64_mlp_w(gpu, name, B, N, E, h, C, L, M, residual):
    from sparsefactorization_amd import fused_mixer
    g, fs = _blocks(E, h, C, L, M, seed=11)
    x = torch.randn(B, N, E, generator=torch.Generator().manual_seed(5))
    want, _ = _reference(x, g, fs, residual)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    xd = x.to(gpu)
    with torch.no_grad():
        assert fused_mixer.covered(xd, g, fs), "the fused path must cover this shape"
        got = fused_mixer.mixer_forward(xd, g, fs, residual).cpu().numpy()
    assert np.isfinite(got).all()
    assert rel_inf(got, want) <= TOL, f"{name}: rel {rel_inf(got, want):.3e}"


def test_short_sequences_run_as_one_launch_and_agree_with_the_per_step_kernels(gpu):
    """N = 512, C = 8 is covered by both forms of the fused mixer: the LDS-resident single launch (default) and the per-step
    kernels (knob mixer_lds = 0) compute the same W and accumulate in the same order: equal bits."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mixer
    g, fs = _blocks(32, 32, 8, 10, 9, seed=2)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    x = torch.randn(6, 512, 32, device=gpu)
    with torch.no_grad():
        one = fused_mixer.mixer_forward(x, g, fs, True).clone()
        sfa.set_tuning("mixer_lds", 0)
        try:
            steps = fused_mixer.mixer_forward(x, g, fs, True).clone()
        finally:
            sfa.set_tuning("mixer_lds", 1)
    assert torch.equal(one, steps)


RECIPE_CASES = [
    # name, kind, B, N, E, h, C, L, M, residual, with positional rows, K (inputs per position / vocabulary)
    ("adding_affine", "affine", 3, 16384, 32, 32, 8, 15, 14, True, False, 2),
    ("order_tokens_pos", "tokens", 3, 16384, 32, 32, 8, 15, 14, True, True, 6),
    ("pathfinder_tokens_pos", "tokens", 3, 1024, 32, 128, 32, 12, 11, False, True, 225),
    ("imdb_tokens_ragged", "tokens", 2, 4097, 32, 128, 32, 13, 12, True, True, 95),
    ("cifar_tokens_e16", "tokens", 3, 1024, 16, 16, 16, 11, 10, False, True, 256),
    ("affine_k3_pos_e12", "affine", 2, 600, 12, 40, 12, 9, 5, True, True, 3),
    ("tokens_nopos_c4", "tokens", 2, 1000, 8, 24, 4, 10, 4, False, False, 11),
    ("cfg1_adding_affine_lds", "affine", 40, 128, 32, 32, 8, 8, 7, True, False, 2),
    ("cfg1_order_tokens_lds", "tokens", 40, 128, 32, 32, 8, 8, 7, True, True, 6),
]


@pytest.mark.parametrize("name,kind,B,N,E,h,C,L,M,residual,with_pos,K", RECIPE_CASES, ids=[c[0] for c in RECIPE_CASES])
def test_mixer_from_the_recipe_of_data_matches_the_float64_reference(gpu, name, kind, B, N, E, h, C, L, M, residual, with_pos, K):
    """The mixer from the RECIPE of `data` — the affine input layer (init_linear, psf.py:153-154) or the embedding lookup
    (+ positional rows, psf.py:151-162): rows written once for the per-step kernels, evaluated in place by the single-launch
    kernel (psf_mixer_fwd_in_f32; the two cfg1 cases). Reference: data in float64 from the same raw inputs, the MLPs in
    float64, the oracle's f32 chain."""
    from sparsefactorization_amd import fused_mixer
    g, fs = _blocks(E, h, C, L, M, seed=21)
    gen = torch.Generator().manual_seed(8)
    pos = 0.5 * torch.randn(N, E, generator=gen) if with_pos else None
    if kind == "affine":
        lin = nn.Linear(K, E)
        inp = torch.rand(B, N, K, generator=gen) * 2 - 1
        data64 = torch.nn.functional.linear(inp.double(), lin.weight.double(), lin.bias.double())
    else:
        table = torch.randn(K, E, generator=gen)
        inp = torch.randint(0, K, (B, N), generator=gen)
        data64 = table.double()[inp]
    if pos is not None:
        data64 = data64 + pos.double()
    want, _ = _reference(data64.float(), g, fs, residual)  # (the reference rounds data to f32 once, as the network does)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    posd = pos.to(gpu) if pos is not None else None
    if kind == "affine":
        r = fused_mixer.Recipe.affine(inp.to(gpu), lin.to(gpu), posd)
    else:
        r = fused_mixer.Recipe.tokens(inp.to(gpu), table.to(gpu), posd)
    with torch.no_grad():
        assert r.ok()
        got = fused_mixer.mixer_forward_in(r, g, fs, residual).cpu().numpy()  # rows written once, then the mixer
        fused_mixer.recipe_in_kernel = True  # short sequences: the single-launch kernel evaluates the recipe itself
        try:
            got_k = fused_mixer.mixer_forward_in(r, g, fs, residual).cpu().numpy()
        finally:
            fused_mixer.recipe_in_kernel = False
    assert np.isfinite(got).all()
    assert rel_inf(got, want) <= TOL, f"{name}: rel {rel_inf(got, want):.3e}"
    assert rel_inf(got_k, want) <= TOL, f"{name} (recipe in the kernel): rel {rel_inf(got_k, want):.3e}"
    from sparsefactorization_amd import _lib
    single_launch = _lib.load().psf_mixer_fwd_plan(N, E, *fused_mixer._block_sizes(E, g, fs)) == 2
    assert single_launch == name.endswith("_lds")
    if single_launch:
        # the single launch evaluated the recipe itself: the rows psf_affine_rows_f32 / psf_embed_tokens_f32 wrote for `got` and
        # the rows it computed are the same bits (include/psf_chord.h), and so is everything after them
        assert np.array_equal(got, got_k), f"{name}: rows written once and rows from the recipe differ"


@pytest.mark.parametrize("K,E,bias", [(2, 32, True), (1, 8, True), (3, 12, False)])
def test_affine_rows_kernel_matches_float64_and_the_linear_module(gpu, K, E, bias):
    """psf_affine_rows_f32 (init_linear of the synthetic PSFNet as one pass over its output, psf.py:153-154) against the same
    layer in float64, through TokenLinear's no-grad path; under autograd the module's forward gives the same bits."""
    from sparsefactorization_amd.token_linear import TokenLinear
    torch.manual_seed(5)
    lin = TokenLinear(K, E, bias=bias)
    x = torch.rand(3, 1000, K) * 4 - 2
    with torch.no_grad():
        want = torch.nn.functional.linear(x.double(), lin.weight.double(), lin.bias.double() if bias else None).numpy()
    lin.to(gpu)
    xg = x.to(gpu)
    with torch.no_grad():
        got = lin(xg)
    assert got.shape == (3, 1000, E)
    assert rel_inf(got.cpu().numpy(), want) <= 1e-6
    again = lin(xg)  # grad enabled: the autograd function's forward
    assert again.requires_grad and torch.equal(again.detach(), got)
    again.sum().backward()
    assert torch.isfinite(lin.weight.grad).all()


def test_mixer_equals_producer_plus_chain_closely(gpu):
    """The same network through the two routes of this package: W_m written by psf_mlp_fwd_f32 and read by the chain, and W_m
    computed inside the step. Same split-bf16 arithmetic for W, same chain order: they agree far below the parity bar."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mixer, fused_mlp
    g, fs = _blocks(32, 32, 8, 15, 14, seed=3)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    x = torch.randn(2, 16384, 32, device=gpu)
    with torch.no_grad():
        outs = fused_mlp.fused_mlp_forward(x, [g, *fs])
        ref = sfa.chord_chain(outs[1:], outs[0], True)
        got = fused_mixer.mixer_forward(x, g, fs, True)
    assert rel_inf(got.cpu().numpy(), ref.cpu().numpy()) <= 2e-6


@pytest.mark.parametrize("N,C,L,M,h", [(16384, 8, 15, 14, 32), (4096, 32, 13, 12, 32), (128, 8, 8, 7, 32)])
def test_mixer_at_full_size_treats_batch_elements_independently(gpu, N, C, L, M, h):
    """Size-independent properties at BASELINE.json's full sequence length (configs[1]: N = 16384, M = 14), where the CPU
    reference takes minutes: (1) the mixer of a batch equals, bit for bit, the mixer of each of its sequences alone — tiles,
    XCD mapping, zigzag walk and the batch size must not leak into the arithmetic; (2) so does a batch with its sequences
    permuted; (3) the residual route equals the non-residual route plus nothing when V0's producer is zero (g = 0):
    then V_M = sum of the chain applied to 0 = 0 without residual, and with it V_M solves V <- W V, V_0 = 0: also 0."""
    from sparsefactorization_amd import fused_mixer
    g, fs = _blocks(32, h, C, L, M, seed=31)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    x = torch.randn(5, N, 32, device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    with torch.no_grad():
        whole = fused_mixer.mixer_forward(x, g, fs, True).clone()
        for i in (0, 3):
            alone = fused_mixer.mixer_forward(x[i:i + 1].contiguous(), g, fs, True)
            assert torch.equal(alone[0], whole[i]), f"sequence {i} alone differs from its place in the batch"
        perm = torch.tensor([3, 0, 4, 2, 1], device=gpu)
        assert torch.equal(fused_mixer.mixer_forward(x[perm].contiguous(), g, fs, True), whole[perm])
        for p in g.parameters():
            p.zero_()
        for res in (False, True):
            out = fused_mixer.mixer_forward(x, g, fs, res)
            assert float(out.abs().max()) == 0.0


def test_mixer_step_is_bit_stable_under_repetition(gpu):
    """The first build of the step kernel came out wrong in a few lanes of a few launches in a hundred at these shapes
    (profiles/r04b_mixer_lds_wait.md): 200 launches each must be bit-identical, and equal to the W-through-memory route."""
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mixer, fused_mlp
    for B, N, E, h, C, L, res in [(16, 16384, 32, 32, 32, 15, False), (64, 16384, 32, 32, 8, 15, True)]:
        g, fs = _blocks(E, h, C, L, 1, seed=0)
        g.to(gpu)
        fs[0].to(gpu)
        x = torch.randn(B, N, E, device=gpu)
        with torch.no_grad():
            outs = fused_mlp.fused_mlp_forward(x, [g, fs[0]])
            ref = sfa.chord_chain([outs[1]], outs[0], res)
            bad = sum(0 if torch.equal(fused_mixer.mixer_forward(x, g, fs, res), ref) else 1 for _ in range(200))
        assert bad == 0, f"{bad} of 200 launches differ at N={N} C={C} B={B}"


def test_mixer_is_deterministic_and_leaves_v0_intact(gpu):
    from sparsefactorization_amd import fused_mixer
    g, fs = _blocks(32, 128, 32, 12, 11, seed=9)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    x = torch.randn(4, 1024, 32, device=gpu)
    with torch.no_grad():
        a = fused_mixer.mixer_forward(x, g, fs, False).clone()
        b = fused_mixer.mixer_forward(x, g, fs, False).clone()
    assert torch.equal(a, b)


def test_nets_take_the_fused_mixer_in_inference_and_agree_with_the_unfused_route(gpu):
    """SyntheticPSFNet (Adding and Temporal Order, N = 8192) and the LRA network (Pathfinder widths) under no_grad: with the
    fused mixer on ("always": the token recipe too), neither `data` nor any W_m is produced (the chain entry point is never
    called); logits agree with the unfused route to 1e-5."""
    from sparsefactorization_amd import chord, fused_mixer
    from sparsefactorization_amd.psfnet import LRAPSFNet, SyntheticPSFNet
    torch.manual_seed(0)
    nets = [
        (SyntheticPSFNet(1, True, 32, 8192, 13, [32, 'GELU'], [32, 'GELU'], 8, 1, 'FLATTEN', ['linear'], True, True, False,
                         'adding'), torch.rand(4, 8192, 2, device=gpu)),
        (SyntheticPSFNet(6, False, 32, 8192, 13, [32, 'GELU'], [32, 'GELU'], 8, 4, 'FLATTEN', ['linear'], True, True, True,
                         'order'), torch.randint(0, 6, (4, 8192, 1), device=gpu)),
        (LRAPSFNet(225, 32, 1024, 11, [128, 'GELU'], [128, 'GELU'], 32, 2, 'FLATTEN', ['linear'], True, False, 0.1, 0.1, 0.1,
                   False, True, 'pathfinder'), torch.randint(0, 225, (4, 1024), device=gpu)),
    ]
    calls = []
    orig = chord.chord_chain

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    for net, x in nets:
        net = net.to(gpu).eval()
        with torch.no_grad():
            fused_mixer.route = "never"
            want = net(x)
            import sparsefactorization_amd.psfnet as pn
            pn.chord_chain = spy
            fused_mixer.route = "always"  # (the automatic rule keeps the Pathfinder widths on the W-through-memory route)
            try:
                got = net(x)
            finally:
                pn.chord_chain = orig
                fused_mixer.route = "auto"
        assert not calls, "the fused mixer path must not run the W-from-memory chain"
        assert rel_inf(got.cpu().numpy(), want.cpu().numpy()) <= 1e-5
        net.train()  # dropout active / gradients wanted: the fused inference path must step aside
        out = net(x)
        assert out.requires_grad


def test_automatic_route_follows_the_measured_rule(gpu):
    """fused_mixer's automatic route (profiles/infer_route_sweep.py): long sequences with hidden <= 32 and every shape of the
    single-launch kernel always; per-step kernels for short sequences when the forward is eager and either the widths are
    CIFAR-10's (hidden <= 32) or the batch is small enough for the host to be the bound (B N <= 40 000 tokens at hidden 128);
    never under stream capture, where the GPU-time rule stands."""
    from sparsefactorization_amd import fused_mixer

    def auto(B, N, E, h, C, L, M):
        g, fs = _blocks(E, h, C, L, M, seed=1)
        g.to(gpu)
        for f in fs:
            f.to(gpu)
        with torch.no_grad():
            return fused_mixer.eligible(torch.randn(B, N, E, device=gpu), g, fs)

    assert fused_mixer.route == "auto"
    assert auto(64, 16384, 32, 32, 8, 15, 14)      # Adding / Order
    assert auto(40, 128, 32, 32, 8, 8, 7)          # cfg1: the single launch
    assert auto(32, 1024, 16, 16, 16, 11, 10)      # CIFAR-10, the reference's batch
    assert auto(512, 1024, 16, 16, 16, 11, 10)     # ... and a large one
    assert auto(16, 1024, 32, 128, 32, 12, 11)     # Pathfinder widths, 16 k tokens
    assert not auto(64, 1024, 32, 128, 32, 12, 11)  # ... at the reference's batch (65 k tokens): W through memory
    assert auto(8, 4097, 32, 128, 32, 13, 12)      # IMDb widths, 32 k tokens
    assert not auto(32, 4097, 32, 128, 32, 13, 12)  # ... at the reference's batch
    side = torch.cuda.Stream(gpu)
    graph = torch.cuda.CUDAGraph()
    seen = {}
    g, fs = _blocks(16, 16, 16, 11, 10, seed=1)
    g.to(gpu)
    for f in fs:
        f.to(gpu)
    x = torch.randn(32, 1024, 16, device=gpu)
    with torch.cuda.stream(side):
        with torch.no_grad(), torch.cuda.graph(graph, stream=side):
            seen["capturing"] = fused_mixer.eligible(x, g, fs)
    torch.cuda.synchronize()
    assert seen["capturing"] is False


def test_same_samples_on_both_sides_of_the_route_boundary_and_under_capture(gpu):
    """The automatic route picks the kernel family by batch size and by whether a HIP graph is being captured
    (fused_mixer._route_ok: hidden-128 LRA widths take the per-step fused kernels while B N <= 40 000 tokens AND the forward is
    eager; W through memory above that and under capture). The two families evaluate W with different arithmetic (split-bf16
    GEMM inside the step / producer kernel), so the SAME sample gives different bits on the two sides of the boundary and in
    eager vs replayed forwards ("What the route decides"). What is pinned here: every route stays within the
    parity bar of the float64-MLP oracle chain, and therefore within 2e-5 of each other, on the Pathfinder network's shapes
    (LRA/psf_training_config.py:60-88) at 32 k tokens (fused) and 65 k tokens (through memory), eager and captured."""
    from sparsefactorization_amd import fused_mixer
    from sparsefactorization_amd.psfnet import LRAPSFNet
    torch.manual_seed(3)
    net = LRAPSFNet(225, 32, 1024, 11, [128, 'GELU'], [128, 'GELU'], 32, 2, 'FLATTEN', ['linear'], True, False, 0.1, 0.1, 0.1,
                    False, True, 'pathfinder').to(gpu).eval()
    x_small = torch.randint(0, 225, (32, 1024), device=gpu)          # 32 768 tokens: the fused per-step kernels
    x_large = torch.cat([x_small, torch.randint(0, 225, (32, 1024), device=gpu)])  # 65 536 tokens: W through memory
    assert fused_mixer.route == "auto"
    taken = []
    orig = fused_mixer.mixer_forward_in

    def spy(*a, **k):
        taken.append(1)
        return orig(*a, **k)

    fused_mixer.mixer_forward_in = spy
    try:
        with torch.no_grad():
            small = net(x_small)
            n_small = len(taken)
            large = net(x_large)
            n_large = len(taken) - n_small
            # the same 32 samples under stream capture: the GPU-time rule applies, W goes through memory
            static_x = x_small.clone()
            side = torch.cuda.Stream(gpu)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                net(static_x)  # warm-up on the side stream (allocations)
                torch.cuda.synchronize()
                before = len(taken)
                with torch.cuda.graph(graph, stream=side):
                    captured = net(static_x)
                n_capture = len(taken) - before
            graph.replay()
            torch.cuda.synchronize()
    finally:
        fused_mixer.mixer_forward_in = orig
    assert (n_small, n_large, n_capture) == (1, 0, 0), "the routes this test is about were not the ones taken"
    ref = small.double()
    scale = float(ref.abs().max())
    # logits of the same 32 samples: across the batch-size boundary, and eager vs replayed
    assert float((large[:32].double() - ref).abs().max()) <= 2e-5 * scale
    assert float((captured.double() - ref).abs().max()) <= 2e-5 * scale
    assert torch.equal(captured, large[:32])  # both W-through-memory: the same kernels on the same rows, the same bits


def test_an_eager_forward_asks_the_library_once_for_the_plan_and_once_for_the_workspace(gpu, monkeypatch):
    """``find`` / ``find_bf16`` hand the forward everything the library said about the shape: from ``find`` through the launch an
    eager no-grad forward makes at most ONE plan query and ONE workspace query (psf_mixer_fwd_plan / _workspace and their bf16
    twins, counted here on the loaded library), whichever kernels run — the single launch (512 x 8), the per-step kernels on
    ragged tiles (600 x 12), a token recipe evaluated inside the single-launch kernel (128 x 8), the bf16 single launch
    (128 x 8) — and the result has the bits of the same forward called without ``found``."""
    from sparsefactorization_amd import _lib, fused_mixer
    lib, asked = _lib.load(), []
    for name in ("psf_mixer_fwd_plan", "psf_mixer_fwd_workspace", "psf_mixer_fwd_bf16_plan", "psf_mixer_fwd_bf16_workspace"):
        monkeypatch.setattr(lib, name, lambda *a, _real=getattr(lib, name), _name=name: (asked.append(_name), _real(*a))[1])
    monkeypatch.setattr(fused_mixer, "route", "always")
    monkeypatch.setattr(fused_mixer, "bf16_route", "always")
    monkeypatch.setattr(fused_mixer, "recipe_in_kernel", True)
    gen = torch.Generator().manual_seed(13)

    def blocks(E, h, C, L, M, dtype=torch.float32):
        g, fs = _blocks(E, h, C, L, M, seed=4)
        return g.to(gpu, dtype), [f.to(gpu, dtype) for f in fs]
    data = lambda x: (fused_mixer.find, fused_mixer.mixer_forward_in, fused_mixer.Recipe.data(x.to(gpu)))  # noqa: E731
    tokens = fused_mixer.Recipe.tokens(torch.randint(0, 6, (3, 128), generator=gen).to(gpu), torch.randn(6, 32, generator=gen).to(gpu),
                                       torch.randn(128, 32, generator=gen).to(gpu))
    cases = [("data 512 x 8", *data(torch.randn(2, 512, 32, generator=gen)), *blocks(32, 32, 8, 10, 9)),
             ("data 600 x 12", *data(torch.randn(2, 600, 12, generator=gen)), *blocks(12, 40, 12, 9, 5)),
             ("tokens 128 x 8", fused_mixer.find, fused_mixer.mixer_forward_in, tokens, *blocks(32, 32, 8, 8, 7)),
             ("bf16 128 x 8", fused_mixer.find_bf16, fused_mixer.mixer_forward_bf16, torch.randn(3, 128, 32, generator=gen).to(gpu, torch.bfloat16),
              *blocks(32, 32, 8, 8, 7, torch.bfloat16))]
    with torch.no_grad():
        for name, find, forward, x, g, fs in cases:
            del asked[:]
            found = find(x, g, fs)
            assert found is not None, name
            got = forward(x, g, fs, True, found)
            torch.cuda.synchronize()
            print(name, asked)
            assert sum(a.endswith("_plan") for a in asked) <= 1 and sum(a.endswith("_workspace") for a in asked) <= 1, (name, asked)
            assert torch.isfinite(got.float()).all() and torch.equal(got, forward(x, g, fs, True)), name
