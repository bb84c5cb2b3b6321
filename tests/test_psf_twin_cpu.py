"""CPU: the float64 twin of tests/psf_twin.py and its comparator are themselves right.

* The twin, run in float64, reproduces what the reference's own forward / backward recorded in tests/golden (data only).
  The bar is 2e-6 for every tensor, the logits included: the looser 1e-4 the GPU tests use for logits was needed nowhere (the
  largest figure is the shipped Pathfinder checkpoint's logits, 1.9e-6).
* Every case of the GPU suite has 0 < E32 <= 2e-5, so no bar exceeds 8e-5.
* Every defect seeded into the f32 twin lands at least 100 x over the bar of each case it is listed for; the clean f32 twin passes.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import psf_twin as T
from conftest import golden_state_dict, load_golden, rel_inf

F32_BAR = 2e-6     # tensors recorded from the reference's f32 run against the float64 twin

ADDING = T._synthetic("adding", 128, 7)
ORDER = T._synthetic("order", 128, 7)
GENOME = dict(T._GENOME, embedding_size=16, n_vec=320, n_W=9, Ws=[16, "GELU"], V=[16, "GELU"], n_channels_V=16)
LISTOPS2000 = T._lra("listops", 20, 16, 2000, 11, 16, 16, 10, "CLS", ["non-linear", 32], True, True)
IMDB4097 = T._lra("imdb", 97, 8, 4097, 12, 8, 8, 2, "CLS", ["linear"], True, False)
PATHFINDER = T._lra("pathfinder", 225, 32, 1024, 11, 128, 32, 2, "FLATTEN", ["linear"], False, True)
ATT300 = dict(vocab_size=50, embedding_size=32, max_seq_len=300, use_cuda=False, use_residuals=True, dropout1_p=0, dropout2_p=0,
              dropout3_p=0)
ATT64 = dict(vocab_size=11, embedding_size=16, max_seq_len=64, use_cuda=False, use_residuals=False, dropout1_p=0, dropout2_p=0,
             dropout3_p=0)


def _sd64(g, grad=False):
    return {k: v.double().requires_grad_(grad) for k, v in golden_state_dict(g).items()}


@pytest.mark.parametrize("cfg,fixture,loss", [(ADDING, "psfnet_adding_n128.npz", "mse"), (ORDER, "psfnet_order_n128.npz", "ce")])
def test_twin_reproduces_the_synthetic_fixtures(cfg, fixture, loss):
    """logits, loss, dW, dV0 (and W, V0, Vfin) of the reference's f32 run: all at 2e-6."""
    g = load_golden(fixture)
    x = torch.from_numpy(g["x"])
    taps = {}
    out = T.forward("synthetic", cfg, _sd64(g, True), x.double() if x.is_floating_point() else x, taps=taps)
    value = T.loss_of(loss, out, torch.from_numpy(g["y"]))
    value.backward()
    assert rel_inf(out.detach().numpy(), g["logits"]) <= F32_BAR
    assert abs(float(value.detach()) - float(g["loss"])) <= F32_BAR * abs(float(g["loss"]))
    assert rel_inf(torch.stack(taps["W"]).detach().numpy(), g["W"]) <= F32_BAR
    assert rel_inf(taps["V0"].detach().numpy(), g["V0"]) <= F32_BAR
    assert rel_inf(taps["Vfin"].detach().numpy(), g["Vfin"]) <= F32_BAR
    assert rel_inf(torch.stack([w.grad for w in taps["W"]]).numpy(), g["dW"]) <= F32_BAR
    assert rel_inf(taps["V0"].grad.numpy(), g["dV0"]) <= F32_BAR


@pytest.mark.parametrize("kind,cfg,fixture", [("genome", GENOME, "genome_n320.npz"), ("lra", LISTOPS2000, "lra_listops_n2000.npz"),
                                              ("lra", IMDB4097, "lra_imdb_n4097.npz")])
def test_twin_reproduces_the_token_model_fixtures(kind, cfg, fixture):
    """logits, V0, Vfin at non-power-of-two N (320, 2000, 4097), CLS and FLATTEN, both heads: all at 2e-6."""
    g = load_golden(fixture)
    taps = {}
    with torch.no_grad():
        out = T.forward(kind, cfg, _sd64(g), torch.from_numpy(g["x"]), training=False, taps=taps)
    assert rel_inf(taps["V0"].numpy(), g["V0"]) <= F32_BAR
    assert rel_inf(taps["Vfin"].numpy(), g["Vfin"]) <= F32_BAR
    assert rel_inf(out.numpy(), g["logits"]) <= F32_BAR


@pytest.mark.parametrize("cfg,fixture", [(ATT300, "attention_block_n300_e32_res.npz"), (ATT64, "attention_block_n64_e16.npz")])
def test_twin_reproduces_the_attention_block_fixtures(cfg, fixture):
    """out, and dW, dV0 of out.backward(gout): all at 2e-6. n_W = ceil(log2(max_seq_len)) is the fixture's."""
    g = load_golden(fixture)
    taps = {}
    out = T.forward("attention", cfg, _sd64(g, True), torch.from_numpy(g["x"]), taps=taps)
    assert len(taps["W"]) == int(g["n_W"]) and taps["W"][0].shape[-1] == int(g["n_links"])
    (out * torch.from_numpy(g["gout"]).double()).sum().backward()
    assert rel_inf(out.detach().numpy(), g["out"]) <= F32_BAR
    assert rel_inf(torch.stack([w.grad for w in taps["W"]]).numpy(), g["dW"]) <= F32_BAR
    assert rel_inf(taps["V0"].grad.numpy(), g["dV0"]) <= F32_BAR


def test_twin_reproduces_the_pathfinder_checkpoint_and_its_dense_map():
    """The shipped checkpoint: W, V0, Vfin, the recorded rows of the dense map and its row sums at 2e-6 against the product of
    the M dense circulant factors, and the logits (values of 1.3e6) at 2e-6 too."""
    g = load_golden("lra_pathfinder_ckpt.npz")
    taps = {}
    with torch.no_grad():
        out, att = T.forward("lra", PATHFINDER, _sd64(g), torch.from_numpy(g["x"]), training=False, want_map=True, taps=taps)
    assert rel_inf(torch.stack(taps["W"]).numpy(), g["W"]) <= F32_BAR
    assert rel_inf(taps["V0"].numpy(), g["V0"]) <= F32_BAR
    assert rel_inf(taps["Vfin"].numpy(), g["Vfin"]) <= F32_BAR
    assert att.shape == (1, 1024, 1024)
    assert rel_inf(att.numpy()[0, ::16, :], g["Wfinal_rows"]) <= F32_BAR
    assert rel_inf(att.numpy().sum(-1), g["Wfinal_rowsum"]) <= F32_BAR
    err = rel_inf(out.numpy(), g["logits"])
    print(f"pathfinder checkpoint logits: {err:.3e}")
    assert err <= F32_BAR


def test_dense_factor_is_the_chord_step():
    """The dense factor applied to V is the roll-and-sum step, duplicates included (N = 5, L = 5: offsets 0 1 2 4 3)."""
    gen = torch.Generator().manual_seed(0)
    for N, L in ((5, 5), (6, 5), (257, 10), (4, 4)):
        off = T.chord_offsets(N, L)
        W, V = torch.randn(2, N, L, generator=gen, dtype=torch.float64), torch.randn(2, N, 3, generator=gen, dtype=torch.float64)
        assert torch.allclose(T.dense_factor(W, off) @ V, T.chord_step(W, V, off), rtol=1e-13, atol=1e-13)
    assert T.chord_offsets(257, 10) == [0, 1, 2, 4, 8, 16, 32, 64, 128, 256] and T.chord_offsets(4, 4) == [0, 1, 2, 0]


def test_fixed_dropout_is_the_twin_s_mask_and_keeps_p():
    mask = (torch.rand(3, 5, generator=torch.Generator().manual_seed(1)) >= 0.3).float()
    d = T.FixedDropout(0.3, mask)
    x = torch.randn(3, 5, dtype=torch.float64)
    assert isinstance(d, torch.nn.Dropout) and d.p == 0.3 and "mask" not in d.state_dict()
    assert torch.equal(d(x), T._drop(x, {"dropout1": mask}, "dropout1", 0.3, True))
    assert torch.equal(d.eval()(x), x)
    assert torch.equal(T.FixedDropout(0.0, mask)(x), x)


# ------------------------------------------------------------------------------------------------- conditions on the cases
@functools.lru_cache(maxsize=None)
def _runs(name):
    case = T.CASE[name]
    sd32 = T.init_state(case)
    return T.run_twin(case, torch.float64, sd32=sd32), T.run_twin(case, torch.float32, sd32=sd32), sd32


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_case_conditions_and_the_clean_f32_twin(name):
    """E32 inside (0, 2e-5]; every parameter has a gradient in the twin; the clean f32 twin passes the comparator (loss and exact
    zeros included); T = B N just above 4096 tokens; the batch really holds what the case is about."""
    case = T.CASE[name]
    r64, r32, _ = _runs(name)
    e32 = T.e32_of(r32, r64)
    print(f"{name}: E32 {e32:.3e}  loss error {T.loss_error(r32, r64):.3e}")
    assert 0 < e32 <= T.E32_MAX
    assert T.loss_error(r32, r64) >= T.LOSS_FLOOR  # the loss bar is not degenerate either (psf_twin.LOSS_FLOOR)
    unused = {"adding": {"embedding.weight", "pos_embedding.weight"}, "deep_mlp": {"embedding.weight", "pos_embedding.weight"},
              "per_step": {"embedding.weight", "pos_embedding.weight"}, "imdb_like": {"pos_embedding.weight"}}.get(name, set())
    assert {k for k, g in r64["grads"].items() if g is None} == unused  # (tables the class builds and this network never reads)
    verdict = T.compare(r32, r64, e32, T.loss_error(r32, r64))
    assert not verdict.failures, verdict.failures
    B, N, E, C, M = T.shape_of(case)
    assert 4096 <= B * N <= 4300
    x, _, masks = T.make_batch(case)
    if case.kind == "lra" and case.cfg["problem"] in ("imdb", "listops"):
        pad = case.cfg["vocab_size"] - 2
        assert (x == pad).any() and not (x[:, 0] == pad).any()
        assert not r64["grads"]["embedding.weight"][pad].any()  # the padding row's gradient is exactly zero
    if name == "order_cls_len":
        assert not (x == 5).any() and not r64["grads"]["embedding.weight"][5].any()  # an id absent from the batch
    for i in (1, 2, 3):
        p = case.cfg.get(f"dropout{i}_p", 0)
        if p:
            assert 0 < 1 - float(masks[f"dropout{i}"].mean()) < 2 * p


@pytest.mark.parametrize("defect,name", [(d, n) for d, (_, where) in T.DEFECTS.items() for n in where])
def test_seeded_defects_are_far_over_the_bar(defect, name):
    r64, r32, sd32 = _runs(name)
    ratio, param = T.defect_ratio(T.CASE[name], defect, r64, T.e32_of(r32, r64), sd32)
    print(f"{defect} in {name}: {ratio:.0f} x the bar at {param}")
    assert ratio >= T.DEFECT_MARGIN


def test_comparator_catches_a_missing_gradient_a_residue_and_a_nan():
    r64, r32, _ = _runs("imdb_like")
    e32 = T.e32_of(r32, r64)
    pad = T.CASE["imdb_like"].cfg["vocab_size"] - 2

    def damaged(fn):
        grads = {k: (None if v is None else v.copy()) for k, v in r32["grads"].items()}
        fn(grads)
        return T.compare({"loss": r32["loss"], "grads": grads}, r64, e32).failures

    assert any("None" in f for f in damaged(lambda g: g.__setitem__("g.network.0.bias", None)))
    assert any("exact zeros" in f for f in damaged(lambda g: g["embedding.weight"].__setitem__((pad, 0), 1e-30)))
    assert any("not finite" in f for f in damaged(lambda g: g["final.bias"].__setitem__(0, np.nan)))
    assert any("names differ" in f for f in damaged(lambda g: g.pop("final.bias")))
    assert any("loss" in f for f in T.compare({"loss": r32["loss"] * 1.001, "grads": r32["grads"]}, r64, e32, 1e-7).failures)


def test_variants_have_a_positive_e32_too():
    """The frozen, accumulating and out.sum() variants of the GPU suite: E32 inside (0, 2e-5] as well, and the frozen
    parameters are exactly the ones without a gradient."""
    for name in T.VARIANT_CASES:
        case = T.CASE[name]
        sd32 = T.init_state(case)
        for kw in [dict(frozen=f) for f in (*T.FROZEN, "one_fs_loop", "g_loop")] + [dict(batches=T.batches_of(name, "accumulate")), dict(batches=T.batches_of(name, "sum_loss"), loss="sum")]:
            r64, r32 = T.run_twin(case, torch.float64, sd32=sd32, **kw), T.run_twin(case, torch.float32, sd32=sd32, **kw)
            e32 = T.e32_of(r32, r64)
            print(f"{name} {kw}: E32 {e32:.3e}")
            assert 0 < e32 <= T.E32_MAX, (name, kw)
            assert T.loss_error(r32, r64) >= T.LOSS_FLOOR, (name, kw)
            if "frozen" in kw:
                assert {k for k, g in r64["grads"].items() if g is None} >= T.frozen_names(case, kw["frozen"], sd32)


def test_batches_follow_the_loss_floor_rule():
    """The batch numbers are the first that pass the floor: one case checked by hand, batch by batch."""
    case = T.CASE["cifar_like"]
    sd32 = T.init_state(case)
    (main,) = T.batches_of("cifar_like")
    errs = [T.loss_error(T.run_twin(case, torch.float32, batches=(k,), sd32=sd32), T.run_twin(case, torch.float64, batches=(k,), sd32=sd32))
            for k in range(main + 1)]
    assert all(e < T.LOSS_FLOOR for e in errs[:-1]) and errs[-1] >= T.LOSS_FLOOR
    assert T.batches_of("cifar_like", "accumulate")[0] == main < T.batches_of("cifar_like", "accumulate")[1]
    assert T.batches_of("per_step") == T.batches_of("adding") and T.batches_of("changed_n257") == (0,)


def test_changed_psf_twin_map_conditions():
    for case in T.CHANGED:
        (l64, a64), (l32, a32) = T.changed_outputs(case, torch.float64), T.changed_outputs(case, torch.float32)
        N = case.cfg["n_vec"]
        assert a64.shape == (case.B, N, N)
        assert 0 < rel_inf(a32, a64) <= T.E32_MAX and 0 < rel_inf(l32, l64) <= T.E32_MAX


def test_report_renders_every_case_and_defect():
    cpu = {c.name: dict(e32=1e-6, e32_param="g.network.0.bias", n_params=44, loss_e32=1e-7, logits_e32=1e-7,
                        defects={d: (1000.0, "final.weight") for d, (_, where) in T.DEFECTS.items() if c.name in where})
           for c in T.CASES}
    log = ("TWIN adding: E32 1.000e-06 bar 4.000e-06 worst 2.000e-06 (0.50 x bar) at final.weight; loss\n"
           ".TWIN adding/g: E32 2.000e-06 bar 8.000e-06 worst 2.000e-06 (0.25 x bar) at final.bias; loss\n"
           "TWIN-LOSS adding/None batches (3,): 0.5 against 0.5: error 1.000e-07 bar 4.000e-07 (0.25 x)\n"
           "TWIN-EVAL adding route=always: mixer calls 1 error 1.000e-07 bar 4.000e-07 (0.25 x)\n"
           "TWIN-MAP changed_n257: map 6.000e-07 bar 1.200e-06; logits 4.000e-08 bar 1.600e-07\n")
    text = T.report(cpu, log)
    assert all(f"| {c.name} |" in text for c in T.CASES) and all(d[0] in text for d in T.DEFECTS.values())
    assert "| 2.00e-06 | 0.50 | `final.weight` |" in text and "| adding/g | 2.00e-06 | 2.00e-06 | 0.25 | `final.bias` |" in text
    assert "| adding | (3,) | 1.000e-07 | 4.000e-07 | 0.25 |" in text and "| adding | always | 1 | 1.000e-07 | 4.000e-07 | 0.25 |" in text
    assert "| changed_n257 | 6.000e-07 | 1.200e-06 | 4.000e-08 | 1.600e-07 |" in text and "`psf_mlp_bwd_f32`: 2" in text
    # the committed file is prose around exactly these blocks: regenerating replaces the blocks and keeps the prose
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "model_twin_grads.md")
    old = open(path).read()
    new = T.report(cpu, log, old)
    strip = lambda t: re.sub(r"<!-- begin (\w+) -->.*?<!-- end \1 -->", "", t, flags=re.S)  # noqa: E731
    assert strip(new) == strip(old) and "| adding | always | 1 | 1.000e-07 |" in new
