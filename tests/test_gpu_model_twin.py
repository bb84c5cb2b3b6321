"""GPU: every parameter gradient of the library's models against the float64 twin of tests/psf_twin.py, which calls nothing of
this library: the autograd wiring of chord.py, fused_mlp.py, token_linear.py, psfnet.py and fused_mixer.py (route selection, saved
tensors, needs_input_grad branches, residual sums, split launches, padding rows, dropout placement) at the smallest shapes that
select each host route.

One case = identical weights, inputs, dropout masks and loss through (a) the twin in float64 and (b) in float32 on the CPU and
(c) the library's network on the GPU. E32 is the largest per-parameter rel_inf error of (b) against (a); the library passes when
the parameters without a gradient are exactly the twin's, every exact zero of the twin's gradients is an exact zero, every
parameter's error is <= 4 x E32 and (a test of its own) the loss is within 4 x the f32 twin's own loss error. The eval-mode logits are held to
4 x the f32 twin's logit error on each of fused_mixer.route = "auto", "never", "always". Every case asserts the routes it names
(psf_twin.CASES[...].routes) by counting calls on the loaded library's entry points and on fused_mlp.route.

Shapes: the planned table as it stands (T = B N just above 4096 tokens so that TokenLinear's kernel runs, N C >= 4096 where
the FLATTEN head kernel is meant to run); no shape had to be moved. Two routes are not where the plan expected them: freezing
``g`` or one ``fs`` alone changes nothing the chain's autograd node sees, because ``data`` still needs a gradient (and every
output of a fused producer's one node requires one anyway); those variants assert the base route. ``need_v0`` false with every W
needing a gradient is reached by "g_loop", and ``all(need_w)`` failing (the per-step loop with ``dW = None``) by "one_fs_loop":
input layer frozen as well, producer MLPs on their own layers. Both assert what the node was asked for and what it returned.
"""
import collections
import functools

import pytest
import torch

import psf_twin as T
from conftest import rel_inf

pytestmark = pytest.mark.gpu

#: substrings of describe_chain_fwd / describe_bwd at the case's shape (the kernels behind the one chain call)
DESCRIBE = {
    "adding": ("one launch for all 9 steps", "chord_bwd_fused_k"),
    "order_cls_len": ("one launch for all 10 steps", "chord_bwd_fused_edge_k"),      # edge instances: N = 1025
    "pathfinder_like": ("one launch for all 8 steps", "chord_bwd_fused_k<f32,L=9,TG=8"),
    "listops_like": ("one launch for all 9 steps", "chord_bwd_fused_edge_k<f32,L=10,TG=16"),  # C = 64 fused backward step
    "cifar_like": ("one launch for all 8 steps", "chord_bwd_fused_k"),
    "imdb_like": ("one launch for all 10 steps", "chord_bwd_fused_edge_k"),
    "genome": ("one launch for all 9 steps", "chord_bwd_fused_k<f32,L=10,TG=8"),
    "attention_block": ("one launch for all 9 steps", "chord_bwd_fused_edge_k<f32,L=10,TG=8"),
    "stacked": ("one launch for all 9 steps", "chord_dw_win_k"),
    "deep_mlp": ("one launch for all 9 steps", "chord_bwd_fused_k"),
    "per_step": ("one launch for all 9 steps", "chord_bwd_fused_k"),
}
#: the cases whose shape the fused mixer covers (fused_mixer.route = "always" must then call psf_mixer_fwd_in_f32 once); not:
#: listops_like (C = 64), stacked (E = 36), deep_mlp (three-layer blocks), per_step (fused_chain off)
MIXER_COVERS = ("adding", "order_cls_len", "pathfinder_like", "cifar_like", "imdb_like", "genome", "attention_block")
_QUIET = ("psf_version", "psf_last_error", "psf_build_info", "psf_device_info", "psf_set_tuning", "psf_get_tuning")


class Spy:
    """Counts the calls of every entry point of the loaded library and records what ``fused_mlp.route`` answers."""

    def __init__(self, monkeypatch):
        from sparsefactorization_amd import _lib, fused_mlp
        self.calls, self.routes = collections.Counter(), []
        lib = _lib.load()
        for name in _lib.SIGNATURES:
            if name not in _QUIET:
                monkeypatch.setattr(lib, name, functools.partial(self._call, name, getattr(lib, name)))
        real_route = fused_mlp.route

        def route(x, blocks):
            name = real_route(x, blocks)
            self.routes.append(name)
            return name

        monkeypatch.setattr(fused_mlp, "route", route)
        # what the chain's autograd node was asked for and what it returned: (need_v0, [need_w], dV0 is None, [dW_m is None])
        from sparsefactorization_amd import chord
        self.chain_nodes = []
        real_backward = chord._ChordChain.backward

        def backward(ctx, g):
            grads = real_backward(ctx, g)
            self.chain_nodes.append((ctx.needs_input_grad[0], list(ctx.needs_input_grad[3:]), grads[0] is None,
                                     [d is None for d in grads[3:]]))
            return grads

        monkeypatch.setattr(chord._ChordChain, "backward", staticmethod(backward))

    def _call(self, name, real, *args):
        self.calls[name] += 1
        return real(*args)

    def reset(self):
        self.calls.clear()
        del self.routes[:]
        del self.chain_nodes[:]


def _class_of(case):
    from sparsefactorization_amd import psfnet
    if case.name.startswith("changed"):
        return psfnet.ChangedPSF
    return {"synthetic": psfnet.SyntheticPSFNet, "lra": psfnet.LRAPSFNet, "genome": psfnet.GenomePSFNet,
            "attention": psfnet.AttentionBlockPSF}[case.kind]


def _set_masks(net, case, masks, gpu):
    for i in (1, 2, 3):
        if hasattr(net, f"dropout{i}"):
            setattr(net, f"dropout{i}", T.FixedDropout(case.cfg.get(f"dropout{i}_p", 0), masks[f"dropout{i}"].to(gpu)))


def _build(case, gpu, frozen=None):
    net = _class_of(case)(**case.cfg)
    net.load_state_dict(T.init_state(case), strict=True)  # (the twin's keys and shapes are the class's)
    net = net.to(gpu)
    if case.name == "per_step":
        net.fused_chain = False
    if frozen:
        names = [n for n, _ in net.named_parameters()]
        for n, p in net.named_parameters():
            if n in T.frozen_names(case, frozen, names):
                p.requires_grad_(False)
    return net


def _run_library(case, net, gpu, batches=None, loss=None):
    net.train()
    value = None
    for which in batches or T.batches_of(case.name):
        x, y, masks = T.make_batch(case, which)
        _set_masks(net, case, masks, gpu)
        value = T.loss_of(loss or case.loss, net(x.to(gpu)), y.to(gpu))
        value.backward()
    torch.cuda.synchronize()
    return {"loss": float(value.detach()),
            "grads": {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in net.named_parameters()}}


@functools.lru_cache(maxsize=None)
def _twin(name, frozen=None, batches=None, loss=None):
    """(float64 run, E32, loss E32) of the twin on the CPU, computed once per configuration."""
    case = T.CASE[name]
    sd32 = T.init_state(case)
    kw = dict(frozen=frozen, batches=batches, loss=loss, sd32=sd32)
    r64, r32 = T.run_twin(case, torch.float64, **kw), T.run_twin(case, torch.float32, **kw)
    return r64, T.e32_of(r32, r64), T.loss_error(r32, r64)


def _judge(tag, got, r64, e32, loss_e32):
    """Everything but the loss, which test_losses_match_the_float64_twin holds on a run of its own."""
    verdict = T.compare(got, r64, e32)
    print(f"TWIN {tag}: E32 {e32:.3e} bar {verdict.bar:.3e} worst {verdict.worst:.3e} ({verdict.worst / verdict.bar:.2f} x bar) at "
          f"{verdict.worst_name}; loss error {T.loss_error(got, r64):.3e} against {T.FACTOR * loss_e32:.3e}; "
          f"{len(verdict.errors)} parameters compared")
    assert len(verdict.errors) == sum(g is not None for g in r64["grads"].values())  # nothing skipped
    assert not verdict.failures, "\n".join(verdict.failures)


def _assert_chain_bwd(case, spy, want):
    from sparsefactorization_amd import _lib
    _, N, _, C, M = T.shape_of(case)
    supported = bool(_lib.load().psf_chord_chain_bwd_supported(N, M + 1, C, M))
    if want == "one_launch":
        assert supported and spy.calls["psf_chord_chain_bwd_f32"] == 1 and spy.calls["psf_chord_spmm_bwd_f32"] == 0
    elif want == "library_steps":
        assert not supported and spy.calls["psf_chord_chain_bwd_f32"] == 1 and spy.calls["psf_chord_spmm_bwd_f32"] == 0
    elif want == "per_step_nodes":
        assert spy.calls["psf_chord_chain_bwd_f32"] == 0 and spy.calls["psf_chord_spmm_bwd_f32"] == M
    else:
        raise AssertionError(want)


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_every_parameter_gradient_matches_the_float64_twin(gpu, monkeypatch, name):
    from sparsefactorization_amd import _lib
    case = T.CASE[name]
    B, N, E, C, M = T.shape_of(case)
    chain_fwd, bwd = DESCRIBE[name]
    assert chain_fwd in _lib.describe_chain_fwd(B, N, M + 1, C, M) and bwd in _lib.describe_bwd(B, N, M + 1, C)
    net = _build(case, gpu)
    spy = Spy(monkeypatch)
    got = _run_library(case, net, gpu)
    print(f"ROUTES {name}: mlp {spy.routes} calls {dict(spy.calls)}")
    assert spy.routes == case.routes["mlp"]
    for entry, n in case.routes["calls"].items():
        assert spy.calls[entry] == n, (entry, spy.calls[entry], n)
    _assert_chain_bwd(case, spy, case.routes["chain_bwd"])
    _judge(name, got, *_twin(name))


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_eval_logits_match_the_float64_twin_on_every_mixer_route(gpu, monkeypatch, name):
    from sparsefactorization_amd import fused_mixer
    case = T.CASE[name]
    l64, l32 = T.eval_logits(case, torch.float64), T.eval_logits(case, torch.float32)
    bar = T.FACTOR * rel_inf(l32, l64)
    assert bar > 0
    net = _build(case, gpu).eval()
    x, _, masks = T.make_batch(case)
    _set_masks(net, case, masks, gpu)
    net.eval()
    spy = Spy(monkeypatch)
    failures = []
    for route in ("auto", "never", "always"):
        monkeypatch.setattr(fused_mixer, "route", route)
        spy.reset()
        with torch.no_grad():
            out = net(x.to(gpu)).cpu().numpy()
        mixer = spy.calls["psf_mixer_fwd_in_f32"]
        err = rel_inf(out, l64)
        print(f"TWIN-EVAL {name} route={route}: mixer calls {mixer} error {err:.3e} bar {bar:.3e} ({err / bar:.2f} x)")
        if route == "never":
            assert mixer == 0
        elif route == "always":  # the shapes the mixer covers run on it, the others fall back: the routes are told apart
            assert mixer == (1 if name in MIXER_COVERS else 0), (name, mixer)
        if not err <= bar:
            failures.append((route, err, bar))
    assert not failures, failures


VARIANTS = [*T.FROZEN, "one_fs_loop", "g_loop", "accumulate", "sum_loss"]


def _variant(name, variant, monkeypatch) -> dict:
    """The arguments of ``_build`` / ``_run_library`` / ``_twin`` for a variant (None: the case as it is)."""
    from sparsefactorization_amd import fused_mlp
    kw = dict(frozen=None, batches=T.batches_of(name, variant), loss=None)
    if variant in T.FROZEN:
        kw["frozen"] = variant
    elif variant in ("one_fs_loop", "g_loop"):
        kw["frozen"] = variant
        monkeypatch.setattr(fused_mlp, "enabled", False)
    elif variant == "sum_loss":
        kw["loss"] = "sum"
    return kw


@pytest.mark.parametrize("name,variant", [(c.name, None) for c in T.CASES] + [(n, v) for v in VARIANTS for n in T.VARIANT_CASES])
def test_losses_match_the_float64_twin(gpu, monkeypatch, name, variant):
    """The loss of every case and variant within 4 x the f32 twin's own loss error, on batches whose bar is not degenerate: the
    first batch numbers for which the f32 twin's loss is at least one f32 rounding error (2^-24) from float64
    (psf_twin.LOSS_FLOOR, batches_of). On batch 0 of everything the rule held in 30 of 32 runs and missed twice where the f32
    twin had landed 0.09 and 0.3 ulp from float64 by roundings that cancel (bars of 4.1e-08 and 1.5e-07 against library losses
    0.7 and 2.3 ulp off, from logits closer to float64 than the twin's). Measured on an MI355X with the rule: 0.005 - 0.25 x."""
    case = T.CASE[name]
    kw = _variant(name, variant, monkeypatch)
    got = _run_library(case, _build(case, gpu, kw["frozen"]), gpu, kw["batches"], kw["loss"])
    r64, _, loss_e32 = _twin(name, kw["frozen"], kw["batches"], kw["loss"])
    err = T.loss_error(got, r64)
    print(f"TWIN-LOSS {name}/{variant} batches {kw['batches']}: {got['loss']!r} against {r64['loss']!r}: error {err:.3e} bar {T.FACTOR * loss_e32:.3e} ({err / (T.FACTOR * loss_e32):.2f} x)")
    assert loss_e32 > 0 and err <= T.FACTOR * loss_e32


@pytest.mark.parametrize("name", T.VARIANT_CASES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_variants_match_the_float64_twin(gpu, monkeypatch, name, variant):
    """Frozen parts, two backward() calls without zero_grad, and loss = out.sum() (an expanded, non-contiguous gradient into the
    head and the chain), each against the twin doing the same: routes, parameters without a gradient, exact zeros and every
    parameter gradient. The losses: test_losses_match_the_float64_twin."""
    case = T.CASE[name]
    M = T.shape_of(case)[4]
    kw = _variant(name, variant, monkeypatch)
    net = _build(case, gpu, kw["frozen"])
    spy = Spy(monkeypatch)
    got = _run_library(case, net, gpu, kw["batches"], kw["loss"])
    print(f"ROUTES {name}/{variant}: mlp {spy.routes} calls {dict(spy.calls)}")
    calls = spy.calls
    if variant == "all_but_final":   # no autograd node for the chain or the producers: nothing of theirs runs backward
        assert not any(calls[k] for k in ("psf_chord_chain_bwd_f32", "psf_chord_spmm_bwd_f32", "psf_mlp_bwd_f32", "psf_mlp_wide_bwd_f32",
                                          "psf_embed_tokens_bwd_f32"))
        assert calls["psf_chord_chain_fwd_f32"] + calls["psf_mixer_fwd_in_f32"] == 1
    elif variant == "one_fs_loop":   # need_w[3] is false: the Python loop, one psf_chord_spmm_bwd_f32 per step, dW[3] = None
        assert spy.routes == [None, None] and calls["psf_chord_chain_bwd_f32"] == 0 and calls["psf_chord_spmm_bwd_f32"] == M
        need_w = [m != 3 for m in range(M)]
        assert spy.chain_nodes == [(True, need_w, False, [not w for w in need_w])]
    elif variant == "g_loop":        # V0 needs no gradient, every W does: the chain entry runs and the node returns no dV0
        assert spy.routes == [None, None] and calls["psf_chord_chain_bwd_f32"] == 1 and calls["psf_chord_spmm_bwd_f32"] == 0
        assert spy.chain_nodes == [(False, [True] * M, True, [False] * M)]
    elif variant == "accumulate":
        assert calls["psf_chord_chain_bwd_f32"] == 2 and calls["psf_chord_spmm_bwd_f32"] == 0
    else:
        assert calls["psf_chord_chain_bwd_f32"] == 1 and calls["psf_chord_spmm_bwd_f32"] == 0
        assert spy.routes == case.routes["mlp"]
    if variant in ("input_layer", "g", "one_fs", "accumulate", "sum_loss"):
        # these keep the base route: V0 and every W are outputs of producers whose input or parameters need a gradient, so the
        # chain node is asked for everything (freezing g or one fs alone only drops that block's own parameter gradients)
        assert spy.chain_nodes == [(True, [True] * M, False, [False] * M)] * len(kw["batches"])
    if variant == "input_layer":     # need_dx is false: no table / input-layer gradient kernel runs
        assert calls["psf_embed_tokens_bwd_f32"] == 0
    _judge(f"{name}/{variant}", got, *_twin(name, kw["frozen"], kw["batches"], kw["loss"]))


@pytest.mark.parametrize("case", T.CHANGED, ids=[c.name for c in T.CHANGED])
def test_changed_psf_logits_and_dense_map_match_the_twin(gpu, monkeypatch, case):
    """ChangedPSF at N = 257 (the identity padded to 260 columns and cut again) and N = 256: logits and the whole map against the
    twin's product of dense factors; the bar is 4 x the f32 twin's own error on the map (logits: on the logits). The map's chain
    call is asserted to be the one meant: C = 260 columns at N = 257, C = N at 256, an unbatched first operand (stride 0)."""
    from sparsefactorization_amd import _lib
    (l64, a64), (l32, a32) = T.changed_outputs(case, torch.float64), T.changed_outputs(case, torch.float32)
    net = _build(case, gpu).eval()
    x, _, _ = T.make_batch(case)
    lib, chains = _lib.load(), []
    real_chain = lib.psf_chord_chain_fwd_f32

    def chain_fwd(*args):  # (w_tab, V0, o_tab, M, residual, B, N, L, C, stride0, offsets, stream)
        chains.append((args[3], args[4], args[6], args[8], args[9]))
        return real_chain(*args)

    monkeypatch.setattr(lib, "psf_chord_chain_fwd_f32", chain_fwd)
    with torch.no_grad():
        logits, att = net(x.to(gpu))
    N = case.cfg["n_vec"]
    M, C = case.cfg["n_W"], case.cfg["n_channels_V"]
    assert chains == [(M, 0, N, C, N * C), (M, 0, N, (N + 3) // 4 * 4, 0)], chains
    assert att.shape == (case.B, N, N)
    e_map, e_log = rel_inf(att.cpu().numpy(), a64), rel_inf(logits.cpu().numpy(), l64)
    print(f"TWIN-MAP {case.name}: map {e_map:.3e} bar {T.FACTOR * rel_inf(a32, a64):.3e}; logits {e_log:.3e} bar {T.FACTOR * rel_inf(l32, l64):.3e}")
    assert e_map <= T.FACTOR * rel_inf(a32, a64)
    assert e_log <= T.FACTOR * rel_inf(l32, l64)
    zero = a64 == 0
    assert not att.cpu().numpy()[zero].any()  # entries no path of links reaches are exact zeros
