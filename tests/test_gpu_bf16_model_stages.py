"""GPU: a bf16 model stage by stage against the float64 contracts of tests/bf16_stage_twin.py, on every opt-in route.

The eleven networks of psf_twin.CASES, built as test_gpu_model_twin._build builds them and converted with
``.to(torch.bfloat16)``, run one training step (and one eval forward) under three settings of the opt-in switches:

  never   every switch at its default: stock PyTorch plus the bf16 chord kernels (the control)
  driver  token_linear.bf16_route, token_linear.bf16_linear_route, psfnet.bf16_head_route at "always": ``psf_training --bf16 --bf16-linear``
  all     driver + fused_mlp.bf16_train_route + chord.bf16_chain_bwd_route

``Taps`` records, without changing anything the library computes, the tensors that pass between the stages — it wraps the
functions psfnet calls between them (embed_tokens, _ChordMixer.produce / link_weights, chord_chain, chord_spmm, _flat_head,
_ChordChain.backward for the saved X_m) and hooks the Linear, GELU and dropout modules — and retains their gradients. After
``backward()`` every stage has its operands, its result, the gradient that entered it and the gradients it returned, and each
is judged against the contract evaluated ON THE OPERANDS THAT STAGE RECEIVED: inside the envelope always, the share of elements
that differ at all within ``bf16_stage_twin.cap`` (stages made of stock ops only: recorded, asserted where the CPU plain
evaluation met the half-cap condition; sums autograd itself adds in bf16: recorded). Then the wiring (what a stage received is
what the stage before returned; every parameter gradient belongs to exactly one stage), the coarse whole-model net (4 x E16
against the float64 twin) and the routes: ``EXPECT`` states, per case and set, what ``fused_mlp.route`` answers and how often
every bf16 entry point is called, derived from the gates in token_linear.py, fused_mlp.py, chord.py and psfnet.py.
"""
import collections
import functools

import numpy as np
import pytest
import torch
from torch import nn

import bf16_edges as be
import bf16_stage_twin as S
import psf_twin as T
from test_gpu_model_twin import Spy, _build, _set_masks

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SETS = ("never", "driver", "all")
NAMES = [c.name for c in T.CASES]

ENTRIES = ("psf_embed_tokens_bf16", "psf_embed_tokens_bwd_bf16", "psf_affine_rows_bf16", "psf_linear_wgrad_bf16", "psf_mlp_fwd_bf16",
           "psf_mlp_bwd_bf16", "psf_chord_chain_fwd_bf16", "psf_chord_chain_bwd_bf16", "psf_chord_chain_bwd_lds_bf16",
           "psf_chord_spmm_fwd_bf16", "psf_chord_spmm_bwd_bf16", "psf_sum_tensors_bf16", "psf_flat_head_bf16", "psf_flat_head_bwd_bf16",
           "psf_mixer_fwd_bf16")


def _calls(embed=(0, 0), affine=0, wgrad=0, mlp=(0, 0), chain=(1, 1, 0), spmm=(0, 0), sums=0, head=(0, 0)) -> dict:
    """Every bf16 entry a training step can reach -> calls in one forward + backward (the entries not named: zero)."""
    return dict(zip(ENTRIES, (*embed, affine, wgrad, *mlp, *chain, *spmm, sums, *head, 0)))


def _expect(mlp, never, driver, all_) -> dict:
    return {"never": (mlp[0], never), "driver": (mlp[1], driver), "all": (mlp[2], all_)}


ST, TR = ["stacked"], ["bf16_train"]
#: case -> set -> (what fused_mlp.route answers, entry -> calls). Read off the gates:
#:   embed     bf16_route "always" and E % 8 == 0: psf_embed_tokens_bf16 + psf_embed_tokens_bwd_bf16. E = 36 ("stacked"): no bf16
#:             pass — the lookup is TokenEmbedding's own Function, whose table gradient still takes psf_embed_tokens_bwd_bf16
#:   linear    bf16_linear_route "always" and T >= 4096: init_linear on psf_affine_rows_bf16 (K = 2), every TokenLinear weight
#:             gradient on psf_linear_wgrad_bf16 — on the "stacked" producer route the M + 1 second layers, each on a column
#:             slice [T, h] of the [T, sum h] hidden buffer; under "all" fused_mlp's "bf16_train" takes the producers (E <= 32,
#:             E % 8 == 0) and those calls away. E = 64 (listops_like) and E = 36 (stacked) stay stacked; three-layer blocks
#:             (deep_mlp) and fused_chain = False (per_step) run the modules' own layers: 3 x 10 + 1 and 2 x 10 + 1 calls
#:   chain     one psf_chord_chain_fwd_bf16; backward one psf_chord_chain_bwd_bf16, or under "all" one
#:             psf_chord_chain_bwd_lds_bf16 where N <= 1024 and C is 8 or 16 (adding, cifar_like, deep_mlp); N = 1025 and
#:             C = 12 / 32 / 64 fall back. per_step: M psf_chord_spmm_fwd_bf16 / _bwd_bf16
#:   head      bf16_head_route "always", FLATTEN, N C >= 4096: psf_flat_head_bf16 (J <= 8) + psf_flat_head_bwd_bf16 (J <= 16:
#:             cifar_like's J = 16 first layer takes F.linear forward); CLS: no head kernel
#:   psf_sum_tensors_bf16 is issued INSIDE psf_chord_chain_bwd_bf16; the Python entry is reached only by the per-step loop of
#:   _ChordChain.backward (test_the_python_loop_of_the_chain_backward_sums_the_residual_once below)
EXPECT = {
    "adding": _expect((ST, ST, TR), _calls(), _calls(affine=1, wgrad=11, head=(1, 1)),
                      _calls(affine=1, wgrad=1, mlp=(1, 1), chain=(1, 0, 1), head=(1, 1))),
    "order_cls_len": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=11, head=(1, 1)),
                             _calls(embed=(1, 1), mlp=(1, 1), head=(1, 1))),
    "pathfinder_like": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=9, head=(1, 1)),
                               _calls(embed=(1, 1), mlp=(1, 1), head=(1, 1))),
    "listops_like": _expect((ST, ST, ST), _calls(), _calls(embed=(1, 1), wgrad=10), _calls(embed=(1, 1), wgrad=10)),
    "cifar_like": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=9, head=(0, 1)),
                          _calls(embed=(1, 1), mlp=(1, 1), chain=(1, 0, 1), head=(0, 1))),
    "imdb_like": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=11), _calls(embed=(1, 1), mlp=(1, 1))),
    "genome": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=10, head=(1, 1)), _calls(embed=(1, 1), mlp=(1, 1), head=(1, 1))),
    "attention_block": _expect((ST, ST, TR), _calls(), _calls(embed=(1, 1), wgrad=10), _calls(embed=(1, 1), mlp=(1, 1))),
    "stacked": _expect((ST, ST, ST), _calls(), _calls(embed=(0, 1), wgrad=10), _calls(embed=(0, 1), wgrad=10)),
    "deep_mlp": _expect(([None, None],) * 3, _calls(), _calls(affine=1, wgrad=31, head=(1, 1)),
                        _calls(affine=1, wgrad=31, chain=(1, 0, 1), head=(1, 1))),
    "per_step": _expect(([],) * 3, _calls(chain=(0, 0, 0), spmm=(9, 9)), _calls(affine=1, wgrad=21, chain=(0, 0, 0), spmm=(9, 9), head=(1, 1)),
                        _calls(affine=1, wgrad=21, chain=(0, 0, 0), spmm=(9, 9), head=(1, 1))),
}
#: the fallbacks the cases contain, by the case that shows each
FALLBACKS = {"E = 36: no bf16 embedding pass": "stacked", "N = 1025: no one-launch backward": "order_cls_len",
             "C = 32: no one-launch backward": "genome", "C = 64: no one-launch backward": "listops_like",
             "E = 64: producers stay stacked": "listops_like", "three-layer blocks": "deep_mlp", "CLS: no head kernel": "imdb_like"}


def _switch(monkeypatch, which):
    from sparsefactorization_amd import chord, fused_mlp, psfnet, token_linear
    if which in ("driver", "all"):
        monkeypatch.setattr(token_linear, "bf16_route", "always")
        monkeypatch.setattr(token_linear, "bf16_linear_route", "always")
        monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    if which == "all":
        monkeypatch.setattr(fused_mlp, "bf16_train_route", "always")
        monkeypatch.setattr(chord, "bf16_chain_bwd_route", "always")


def test_the_table_reaches_every_entry_and_names_every_fallback():
    """Every bf16 entry a training step can reach is called in some (case, set) — psf_linear_wgrad_bf16 on a contiguous operand
    (init_linear) and on column slices (the stacked second layers, widths 128 and 40), the one-launch backward at C = 8 and C = 16,
    the head with J <= 8 and J = 16 — and every fallback has its case. (psf_sum_tensors_bf16: see EXPECT; psf_mixer_fwd_bf16:
    the eval test.)"""
    hit = collections.Counter()
    for name, sets in EXPECT.items():
        for _mlp, calls in sets.values():
            hit.update({k: v for k, v in calls.items() if v})
    assert set(ENTRIES) - set(hit) == {"psf_sum_tensors_bf16", "psf_mixer_fwd_bf16"}
    shape = {n: T.shape_of(T.CASE[n]) for n in NAMES}
    lds = [n for n in NAMES if EXPECT[n]["all"][1]["psf_chord_chain_bwd_lds_bf16"]]
    assert {shape[n][3] for n in lds} == {8, 16}
    assert EXPECT["listops_like"]["driver"][1]["psf_linear_wgrad_bf16"] and T.CASE["listops_like"].cfg["Ws"][0] == 128
    assert EXPECT["stacked"]["driver"][1]["psf_linear_wgrad_bf16"] and T.CASE["stacked"].cfg["Ws"][0] == 40
    assert EXPECT["cifar_like"]["driver"][1]["psf_flat_head_bwd_bf16"] == 1 and EXPECT["cifar_like"]["driver"][1]["psf_flat_head_bf16"] == 0
    assert set(FALLBACKS.values()) <= set(NAMES)
    assert shape["stacked"][2] == 36 and shape["order_cls_len"][1] == 1025 and shape["genome"][3] == 32 and shape["listops_like"][2:4] == (64, 64)


# ----------------------------------------------------------------------------------------------------------------- the taps
def _np(t):
    return t.detach().float().cpu().double().numpy()


def _keep(t):
    if isinstance(t, torch.Tensor) and t.is_floating_point() and t.requires_grad and not t.is_leaf:
        t.retain_grad()
    return t


Event = collections.namedtuple("Event", "stage name ins outs extra")


class Taps:
    """Records the tensors between the stages of one forward (see the module docstring). ``events`` in forward order."""

    def __init__(self, monkeypatch, net):
        from sparsefactorization_amd import chord, psfnet
        self.events, self.saved, self.depth, self.muted = [], [], 0, set()
        self.names = {id(m): n for n, m in net.named_modules()}
        taps = self

        def record(stage, name, ins, outs, **extra):
            for t in (*ins.values(), *outs.values()):
                for u in (t if isinstance(t, (list, tuple)) else (t,)):
                    _keep(u)
            taps.events.append(Event(stage, name, ins, outs, extra))

        real_embed = psfnet.embed_tokens

        def embed_tokens(idx, embedding, pos=None):
            out = real_embed(idx, embedding, pos)
            record("embed", taps.names.get(id(embedding), "embedding"), dict(idx=idx, table=embedding.weight, pos=pos), dict(data=out),
                   pad=embedding.padding_idx)
            return out

        monkeypatch.setattr(psfnet, "embed_tokens", embed_tokens)

        def producer(real, with_g):
            def wrapped(mixer, data):
                before = len(taps.events)
                taps.depth += 1
                try:
                    result = real(mixer, data)
                finally:
                    taps.depth -= 1
                V, links = result if with_g else (None, result)
                outs = ([V] if with_g else []) + list(links or [])
                blocks = ([mixer.g] if with_g else []) + list(mixer.fs)
                if taps.depth == 0 and len(taps.events) == before and len(outs) == len(blocks):  # no layer of a block ran as a module
                    record("producers", "g+fs" if with_g else "fs", dict(data=data), dict(ys=outs), blocks=blocks)
                return result
            return wrapped

        monkeypatch.setattr(psfnet._ChordMixer, "produce", producer(psfnet._ChordMixer.produce, True))
        monkeypatch.setattr(psfnet._ChordMixer, "link_weights", producer(psfnet._ChordMixer.link_weights, False))
        real_chain, real_spmm, real_head = psfnet.chord_chain, psfnet.chord_spmm, psfnet._flat_head

        def chord_chain(W_list, V0, use_residual=False, offsets=None):
            out = real_chain(W_list, V0, use_residual, offsets)
            record("chain", "chain", dict(V0=V0, Ws=list(W_list)), dict(V=out), residual=bool(use_residual))
            return out

        def chord_spmm(W, V, residual=None, offsets=None):
            out = real_spmm(W, V, residual, offsets)
            record("chain_step", f"step{sum(e.stage == 'chain_step' for e in taps.events)}", dict(W=W, V=V, res=residual), dict(out=out))
            return out

        def flat_head(final, flat):
            if not isinstance(final, nn.Linear):
                return real_head(final, flat)
            taps.muted.add(id(final))
            try:
                out = real_head(final, flat)
            finally:
                taps.muted.discard(id(final))
            record("head", taps.names[id(final)], dict(x=flat), dict(y=out), module=final)
            return out

        monkeypatch.setattr(psfnet, "chord_chain", chord_chain)
        monkeypatch.setattr(psfnet, "chord_spmm", chord_spmm)
        monkeypatch.setattr(psfnet, "_flat_head", flat_head)
        inner_backward = chord._ChordChain.backward  # (Spy's wrapper when a Spy is installed first)

        def backward(ctx, g):
            taps.saved.append([t.detach() for t in ctx.saved_tensors])
            return inner_backward(ctx, g)

        monkeypatch.setattr(chord._ChordChain, "backward", staticmethod(backward))

        def layer_hook(module, inputs, output):
            if id(module) in taps.muted:
                return
            name = taps.names[id(module)]
            if isinstance(module, nn.Linear):
                stage = "head" if name.startswith("final") else ("init_linear" if name == "init_linear" else "layer")
                record(stage, name, dict(x=inputs[0]), dict(y=output), module=module)
            elif isinstance(module, nn.GELU):
                record("gelu", name, dict(z=inputs[0]), dict(h=output))
            elif module.training and module.p > 0:
                record("dropout", name, dict(x=inputs[0]), dict(out=output), module=module)

        self.handles = [m.register_forward_hook(layer_hook) for m in net.modules() if isinstance(m, (nn.Linear, nn.GELU, T.FixedDropout))]

    def close(self):
        for h in self.handles:
            h.remove()


# ---------------------------------------------------------------------------------------------------------------- judging
class Verdicts:
    """One (case, set): the printed lines, the pooled shares, the parameters whose gradient a stage has accounted for."""

    def __init__(self, case, tag, stock_ok):
        self.case, self.tag, self.shares, self.params, self.stock_ok, self.links = case, tag, S.Shares(), {}, stock_ok, []

    def judge(self, stage, tensor, got, want, env, n, exact=False, stock=None, recorded=""):
        """``stock``: the CPU stage name when the tensor comes from stock PyTorch ops only (asserted if the plain evaluation met
        the half-cap condition there); ``recorded``: why the share is not asserted at all."""
        note = "exact" if exact else recorded
        asserted = not recorded
        if stock is not None and not recorded and not self.stock_ok(stock):
            note, asserted = "recorded: stock ops, the CPU plain evaluation missed half the cap", False
        share = S.judge(stage, tensor, got, want, 0.0 if exact else env, self.tag, note, self.shares, n, asserted, stage != "chain")
        if exact:
            assert share == 0.0

    def param(self, name, stage):
        assert name not in self.params, f"{name}: the gradient of {self.params[name]} and of {stage}"
        self.params[name] = stage

    def link(self, what, a, b):
        """``b`` (what a stage received) is ``a`` (what the stage before returned): storage, shape and strides; or an equal copy."""
        if a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride():
            kind = "same tensor"
        else:
            assert a.shape == b.shape and torch.equal(a.detach(), b.detach()), f"{what}: not what the stage before returned"
            kind = "a copy"
        self.links.append((what, kind))

    def print(self):
        """The run's record: ``Shares.lines`` and the count of hand-overs (a copy is named)."""
        copies = [what for what, kind in self.links if kind == "a copy"]
        print("\n".join(self.shares.lines(self.tag)))
        print(f"STAGE-LINKS {self.tag}: {len(self.links) - len(copies)} the same tensor, {len(copies)} copies" + (f" ({'; '.join(copies)})" if copies else ""))


def _consumers(events) -> collections.Counter:
    """How many tapped stages read each tensor (by identity): a tensor read more than once gets its gradient from autograd's
    own bf16 adds."""
    seen = collections.Counter()
    for e in events:
        for t in e.ins.values():
            for u in (t if isinstance(t, (list, tuple)) else (t,)):
                if isinstance(u, torch.Tensor) and u.is_floating_point():
                    seen[id(u)] += 1
    return seen


def _summed(v, stage, tensor, got, terms, envs):
    """A gradient autograd formed by adding K bf16 tensors one after the other: the sum of the contracts' values, the envelope
    widened by (K - 1) ulp of the sum of magnitudes; the share is recorded."""
    want = S.bf16_rne(sum(terms))
    env = sum(envs) + S.ulp_bf16(want) + (len(terms) - 1) * S.ulp_bf16(sum(np.abs(t) for t in terms))
    v.judge(stage, tensor, got, want, env, len(terms), recorded=f"recorded: autograd adds {len(terms)} gradients in bf16")


def judge_run(v: Verdicts, taps: Taps, spy: Spy, net, training: bool):
    case = v.case
    B, N, E, C, M = T.shape_of(case)
    off = T.chord_offsets(N, M + 1)
    uses = _consumers(taps.events)
    pname = {id(p): n for n, p in net.named_parameters()}
    stock_embed = not spy.calls["psf_embed_tokens_bf16"]
    first_layer_dx = collections.defaultdict(list)   # id(x) -> [(want, env)] of the layers that read x, where x is read K times
    by_id = {}

    def grad(t):
        return None if (t is None or not training or t.grad is None) else _np(t.grad)

    for e in taps.events:
        if e.stage == "embed":
            idx, table, pos, data = e.ins["idx"], e.ins["table"], e.ins["pos"], e.outs["data"]
            want, env = S.embed_fwd(_np(table), idx.cpu().numpy(), None if pos is None else _np(pos))
            v.judge("embed", "data", _np(data), want, env, 2, exact=pos is None, stock="embed" if stock_embed else None)
            if training:
                w = S.embed_bwd(grad(data), idx.cpu().numpy(), table.shape[0], e.extra["pad"], pos is not None)
                stock = "embed" if not spy.calls["psf_embed_tokens_bwd_bf16"] else None
                v.judge("embed", "dTable", grad(table), *w["dTable"], w["n"]["dTable"], stock=stock)
                v.param(pname[id(table)], "embed")
                if pos is not None:
                    v.judge("embed", "dpos", grad(pos), *w["dpos"], B, stock="embed")  # (a stock sum over the batch on every route)
                    v.param(pname[id(pos)], "embed")
        elif e.stage in ("init_linear", "layer", "head"):
            mod, x, y = e.extra["module"], e.ins["x"], e.outs["y"]
            K, O = mod.weight.shape[1], mod.weight.shape[0]
            kernel = (spy.calls["psf_affine_rows_bf16"] and e.stage == "init_linear") or (spy.calls["psf_flat_head_bf16"] and e.stage == "head" and K >= 4096)
            stock = None if kernel else ("head" if e.stage == "head" else ("init_linear" if e.stage == "init_linear" else "layer"))
            v.judge(e.stage, f"{e.name}.y", _np(y), *S.linear_fwd(_np(x), _np(mod.weight), _np(mod.bias)), K + 1, stock=stock)
            if training:
                w = S.linear_bwd(_np(x), _np(mod.weight), grad(y))
                rows = w["n"]["dW"]
                wgrad_kernel = (spy.calls["psf_linear_wgrad_bf16"] and e.stage != "head") or (spy.calls["psf_flat_head_bwd_bf16"] and e.stage == "head" and K >= 4096)
                stock = None if wgrad_kernel else stock or e.stage
                v.judge(e.stage, f"{e.name}.dW", grad(mod.weight), *w["dW"], rows, stock=stock)
                # (the head's bias gradient is a stock sum over the batch on every route; TokenLinear's comes with dW)
                v.judge(e.stage, f"{e.name}.db", grad(mod.bias), *w["db"], rows, stock=None if wgrad_kernel and e.stage != "head" else e.stage)
                v.param(e.name + ".weight", e.stage)
                v.param(e.name + ".bias", e.stage)
                if x.requires_grad:
                    if uses[id(x)] == 1:
                        v.judge(e.stage, f"{e.name}.dx", grad(x), *w["dx"], O, stock=stock)
                    else:
                        first_layer_dx[id(x)].append(w["dx"])
                        by_id[id(x)] = x
        elif e.stage == "gelu":
            z, h = e.ins["z"], e.outs["h"]
            v.judge("gelu", f"{e.name}.h", _np(h), *S.gelu_fwd(_np(z)), 1, stock="gelu")
            if training and z.requires_grad:
                v.judge("gelu", f"{e.name}.d", grad(z), *S.gelu_bwd(_np(z), grad(h)), 1, stock="gelu")
        elif e.stage == "dropout":
            mod, x, out = e.extra["module"], e.ins["x"], e.outs["out"]
            mask = mod.mask.cpu().numpy()
            v.judge(e.name, "out", _np(out), S.dropout_fwd(_np(x), mask, mod.p), 0.0, 1, exact=True)
            if training and x.requires_grad:
                v.judge(e.name, "dx", grad(x), S.dropout_bwd(grad(out), mask, mod.p), 0.0, 1, exact=True)
        elif e.stage == "producers":
            data, ys, blocks = e.ins["data"], e.outs["ys"], e.extra["blocks"]
            params = [tuple(_np(p) for p in (b.network[0].weight, b.network[0].bias, b.network[2].weight, b.network[2].bias)) for b in blocks]
            X = _np(data).reshape(-1, E)
            fused = bool(spy.calls["psf_mlp_fwd_bf16"])
            stock = None if fused else "producers"
            for k, ((y, env), got) in enumerate(zip(S.producers_fwd(X, params), ys)):
                v.judge("producers", f"y[{k}]", _np(got).reshape(y.shape), y, env, max(E, params[k][0].shape[0]) + 1, stock=stock)
            if training:
                want, env = S.producers_bwd(X, params, [grad(y).reshape(-1, y.shape[-1]) for y in ys])
                got = {"dX": grad(data).reshape(-1, E) if data.requires_grad else want["dX"],
                       "grads": [tuple(grad(p) for p in (b.network[0].weight, b.network[0].bias, b.network[2].weight, b.network[2].bias)) for b in blocks]}
                terms = {"dX": sum(p[0].shape[0] for p in params), "dA": B * N, "da": B * N, "dB": B * N, "db": B * N}
                second = None if fused or spy.calls["psf_linear_wgrad_bf16"] else "producers"  # the stacked route's second layers
                for (nm, g), (_, w), (_, en) in zip(S.RB.tensors(got), S.RB.tensors(want), S.RB.tensors(env)):
                    kind = nm.split("[")[0]
                    if kind == "dX" and not data.requires_grad:
                        continue
                    v.judge("producers", nm, g, w, en, terms[kind], stock=second if kind in ("dB", "db") else stock)
                for b in blocks:
                    for i in (0, 2):
                        for w_ in ("weight", "bias"):
                            v.param(f"{taps.names[id(b)]}.network.{i}.{w_}", "producers")
        elif e.stage == "chain":
            V0, Ws, out, residual = e.ins["V0"], e.ins["Ws"], e.outs["V"], e.extra["residual"]
            W64, V64 = [_np(w) for w in Ws], _np(V0)
            if training:
                assert len(taps.saved) == 1 and len(taps.saved[0]) == 2 * M, "the chain's node saves V0, the W_m and X_1 .. X_{M-1}"
                saved = taps.saved[0]
                assert torch.equal(saved[0], V0.detach()) and all(torch.equal(s, w.detach()) for s, w in zip(saved[1:1 + M], Ws)), \
                    "the chain's node saved other operands than the ones it was given"
                X = [V64] + [_np(s) for s in saved[1 + M:]] + [_np(out)]
                for m in range(M):
                    v.judge("chain", f"X[{m + 1}]", X[m + 1], *S.chain_step(W64[m], X[m], V64 if residual else None, off), M + 2)
                dOut = grad(out)
                terms = S.chain_terms(M, M + 1, C)
                got_dV0, got_dW = grad(V0), [grad(w) for w in Ws]
                if spy.calls["psf_chord_chain_bwd_lds_bf16"]:  # the documented order of the one-launch route: the bits
                    bits_dV0, bits_dW = S.chain_backward_bits((B, N, M, M + 1, C), residual, W64, X[:M], dOut)
                    v.judge("chain", "dV0", got_dV0, be.bits_f32(bits_dV0).astype(np.float64), 0.0, terms["dV0"], exact=True)
                    for m in range(M):
                        v.judge("chain", f"dW[{m}]", got_dW[m], be.bits_f32(bits_dW[m]).astype(np.float64), 0.0, terms["dW"][m], exact=True)
                else:
                    want = S.chain_backward(W64, X[:M], dOut, residual, off)
                    v.judge("chain", "dV0", got_dV0, *want["dV0"], terms["dV0"])
                    for m in range(M):
                        v.judge("chain", f"dW[{m}]", got_dW[m], *want["dW"][m], terms["dW"][m])
            else:
                w, en = S.chain_forward(W64, V64, residual, off)[-1]
                v.judge("chain", "X_M from V0", _np(out), w, en, S.chain_terms(M, M + 1, C)["X_M"])
        elif e.stage == "chain_step":
            W, V, res, out = e.ins["W"], e.ins["V"], e.ins["res"], e.outs["out"]
            v.judge("chain_step", f"{e.name}.X", _np(out), *S.chain_step(_np(W), _np(V), None if res is None else _np(res), off), M + 2)
            if training:
                w = S.chain_backward([_np(W)], [_np(V)], grad(out), False, off)
                v.judge("chain_step", f"{e.name}.dW", grad(W), *w["dW"][0], C)
                if uses[id(V)] == 1:
                    v.judge("chain_step", f"{e.name}.dV", grad(V), *w["dV0"], M + 1)
                else:  # V0: read by step 0 as V and by every step as the residual
                    steps = [s for s in taps.events if s.stage == "chain_step"]
                    _summed(v, "chain_step", "dV0", grad(V), [w["dV0"][0]] + [grad(s.outs["out"]) for s in steps if s.ins["res"] is V],
                            [w["dV0"][1]])
    for key, parts in first_layer_dx.items():
        _summed(v, "layer", "d(data) summed over the blocks", grad(by_id[key]), [p[0] for p in parts], [p[1] for p in parts])


def judge_wiring(v: Verdicts, taps: Taps, net):
    """What each stage received is what the stage before returned, along data -> (dropout1) -> producers -> (dropout2) -> chain
    -> (dropout3) -> pooling -> head; the CLS slice and the reshape are exact stages of their own."""
    case = v.case
    _B, N, E, C, M = T.shape_of(case)
    ev = taps.events
    one = lambda stage, name=None: next((e for e in ev if e.stage == stage and (name is None or e.name == name)), None)
    src = one("embed") or one("init_linear")
    data = src.outs["data" if src.stage == "embed" else "y"]
    d1 = one("dropout", "dropout1")
    if d1 is not None:
        v.link("dropout1 reads the input layer's rows", data, d1.ins["x"])
        data = d1.outs["out"]
    prod = one("producers")
    steps = [e for e in ev if e.stage == "chain_step"]
    if prod is not None:
        v.link("the producers read data", data, prod.ins["data"])
        V0, Ws = prod.outs["ys"][0], prod.outs["ys"][1:]
    else:
        firsts = [e for e in ev if e.stage == "layer" and e.name.endswith("network.0")]
        assert len(firsts) == M + 1
        for e in firsts:
            v.link(f"{e.name} reads data", data, e.ins["x"])
        last = max(int(e.name.rsplit(".", 1)[1]) for e in ev if e.stage == "layer")
        outs = {e.name.split(".network.")[0]: e.outs["y"] for e in ev if e.stage == "layer" and e.name.endswith(f"network.{last}")}
        V0, Ws = outs["g"], [outs[f"fs.{m}"] for m in range(M)]
    d2 = one("dropout", "dropout2")
    if d2 is not None:
        v.link("dropout2 reads g's rows", V0, d2.ins["x"])
        V0 = d2.outs["out"]
    chain = one("chain")
    if chain is not None:
        v.link("the chain reads V0", V0, chain.ins["V0"])
        for m in range(M):
            v.link(f"the chain reads W_{m}", Ws[m], chain.ins["Ws"][m])
        V = chain.outs["V"]
    else:
        assert len(steps) == M
        V = V0
        for m, e in enumerate(steps):
            v.link(f"step {m} reads X_{m}", V, e.ins["V"])
            v.link(f"step {m} reads W_{m}", Ws[m], e.ins["W"])
            if case.cfg["use_residuals"]:
                v.link(f"step {m} reads the residual", V0, e.ins["res"])
            V = e.outs["out"]
    d3 = one("dropout", "dropout3")
    if d3 is not None:
        v.link("dropout3 reads the chain's result", V, d3.ins["x"])
        V = d3.outs["out"]
    head = one("head")
    if head is None:
        assert case.kind == "attention"
        return V
    flat = head.ins["x"]
    if case.cfg["pooling_type"] == "CLS":
        v.judge("cls", "flat", _np(flat), _np(V)[:, 0, :], 0.0, 1, exact=True)
        assert flat.data_ptr() == V.data_ptr(), "the CLS rows are a view of the chain's result"
        if V.grad is not None:
            v.judge("cls", "dV", _np(V.grad), S.cls_bwd(_np(flat.grad), N), 0.0, 1, exact=True)
    else:
        assert flat.data_ptr() == V.data_ptr() and flat.shape == (V.shape[0], N * C) and flat.is_contiguous(), "FLATTEN is a view"
        if V.grad is not None:
            v.judge("flatten", "dV", _np(V.grad).reshape(flat.shape), _np(flat.grad), 0.0, 1, exact=True)
    return V


@functools.lru_cache(maxsize=None)
def _e16(name):
    return S.e16_of(T.CASE[name])


def _stock_ok(name):
    """Whether the CPU plain evaluation of the case met the half-cap condition in a stage (per_step runs adding's network layer
    by layer: the layer and GELU stages of that shape are deep_mlp's on the CPU side)."""
    import test_bf16_stage_twin_cpu as CPU

    def ok(stage):
        has = any(row[0] == stage for row in CPU.clean_shares(name).rows)
        return CPU.clean_ok(name if has else "deep_mlp", stage)
    return ok


def _batch(case, gpu):
    x, y, masks = T.make_batch(case)
    if x.is_floating_point():
        x = x.to(BF)
    if y.is_floating_point() and case.loss == "dot":
        y = y.to(BF).float()
    return x.to(gpu), y.to(gpu), masks


# ------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name", NAMES)
def test_every_stage_of_a_bf16_training_step(gpu, monkeypatch, name, which):
    case = T.CASE[name]
    net = _build(case, gpu).to(BF)
    x, y, masks = _batch(case, gpu)
    _set_masks(net, case, masks, gpu)
    net.train()
    _switch(monkeypatch, which)
    spy = Spy(monkeypatch)
    taps = Taps(monkeypatch, net)
    try:
        out = net(x)
        loss = T.loss_of(case.loss, out.float(), y)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        taps.close()
    tag = f"{name} {which}"
    mlp, calls = EXPECT[name][which]
    print(f"STAGE-ROUTES {name} {which}: mlp {spy.routes} calls { {k: spy.calls[k] for k in ENTRIES if spy.calls[k]} }")
    assert spy.routes == mlp, (spy.routes, mlp)
    for entry, n in calls.items():
        assert spy.calls[entry] == n, (entry, spy.calls[entry], n)

    v = Verdicts(case, tag, _stock_ok(name))
    judge_run(v, taps, spy, net, True)
    judge_wiring(v, taps, net)

    # every parameter gradient is one stage's, and none is left out
    e16, e16_name, r64 = _e16(name)
    with_grad = {k for k, g in r64["grads"].items() if g is not None}
    assert set(v.params) == with_grad, sorted(set(v.params) ^ with_grad)
    assert len(v.params) == len(with_grad)

    # the coarse net, independent of the taps
    got = {"loss": float(loss.detach()), "grads": {n: (None if p.grad is None else _np(p.grad)) for n, p in net.named_parameters()}}
    assert e16 <= S.E16_MAX, (e16, e16_name)
    verdict = T.compare(got, r64, e16)
    print(f"STAGE-E16 {name} {which}: E16 {e16:.3e} at {e16_name} bar {verdict.bar:.3e} worst {verdict.worst:.3e} at {verdict.worst_name}")
    assert not verdict.failures, "\n".join(verdict.failures)

    v.print()
    assert not v.shares.over(), v.shares.over()


@pytest.mark.parametrize("name", NAMES)
def test_eval_forward_stage_by_stage_and_the_one_launch_mixer(gpu, monkeypatch, name):
    """Eval mode under no_grad: the forward stages on the ``bf16_forward`` producer route and the chain without an autograd node;
    then fused_mixer.bf16_route = "always": one psf_mixer_fwd_bf16 call where ``covered_bf16`` holds, none elsewhere, and the
    bits of "never" either way."""
    from sparsefactorization_amd import fused_mixer
    case = T.CASE[name]
    net = _build(case, gpu).to(BF).eval()
    x, _y, masks = _batch(case, gpu)
    _set_masks(net, case, masks, gpu)
    net.eval()
    spy = Spy(monkeypatch)
    taps = Taps(monkeypatch, net)
    try:
        with torch.no_grad():
            never = net(x)
        routes, calls = list(spy.routes), dict(spy.calls)
        v = Verdicts(case, f"{name} eval", _stock_ok(name))
        judge_run(v, taps, spy, net, False)
        judge_wiring(v, taps, net)
        src = next(e for e in taps.events if e.stage in ("embed", "init_linear"))
        data = src.outs["data" if src.stage == "embed" else "y"]
        covered = bool(fused_mixer.covered_bf16(data, net.g, list(net.fs))) and net.fused_chain
        monkeypatch.setattr(fused_mixer, "bf16_route", "always")
        spy.reset()
        with torch.no_grad():
            always = net(x)
        torch.cuda.synchronize()
    finally:
        taps.close()
    print(f"STAGE-EVAL {name}: producers {routes}, psf_mlp_fwd_bf16 {calls.get('psf_mlp_fwd_bf16', 0)}, mixer covered {covered}, "
          f"psf_mixer_fwd_bf16 calls {spy.calls['psf_mixer_fwd_bf16']}, bits equal {torch.equal(never, always)}")
    assert calls.get("psf_mixer_fwd_bf16", 0) == 0 and calls.get("psf_chord_chain_bwd_bf16", 0) == 0
    assert routes == EVAL_ROUTES[name], routes
    assert calls.get("psf_mlp_fwd_bf16", 0) == (1 if EVAL_ROUTES[name] == ["bf16_forward"] else 0)
    assert covered == (name in MIXER_COVERS), (name, covered)
    assert spy.calls["psf_mixer_fwd_bf16"] == (1 if name in MIXER_COVERS else 0)
    assert torch.equal(never, always)
    v.print()
    assert not v.shares.over(), v.shares.over()


#: what fused_mlp.route answers in eval mode: the fused bf16 forward where E is a multiple of 8 up to 64 and no block has more than
#: 32 outputs, stacked otherwise; three-layer blocks are asked twice (produce, link_weights) and match no route; per_step never asks
EVAL_ROUTES = {n: ["bf16_forward"] for n in NAMES}
EVAL_ROUTES.update(stacked=["stacked"],        # E = 36
                   listops_like=["stacked"],   # g has 64 outputs
                   deep_mlp=[None, None], per_step=[])
#: the cases psf_mixer_fwd_bf16 takes, by its documented limits (N <= 512, C = 8 or 16, two-layer blocks, the fused chain): stated
#: here, not asked of fused_mixer.covered_bf16, which is under test
MIXER_COVERS = ("adding", "cifar_like")


@pytest.mark.parametrize("which", SETS)
def test_the_python_loop_of_the_chain_backward_sums_the_residual_once(gpu, monkeypatch, which):
    """psf_sum_tensors_bf16 through its Python entry: the per-step loop of _ChordChain.backward, which runs when one W_m needs no
    gradient (fs[3] and the input layer frozen, the producers on their own layers: psf_twin's "one_fs_loop"). dV0 — the residual
    terms and dX_0 summed once — and every dW_m against the chain's contract; dW_3 is None."""
    from sparsefactorization_amd import fused_mlp
    case = T.CASE["adding"]
    B, N, E, C, M = T.shape_of(case)
    monkeypatch.setattr(fused_mlp, "enabled", False)
    _switch(monkeypatch, which)
    net = _build(case, gpu, "one_fs_loop").to(BF)
    x, y, masks = _batch(case, gpu)
    net.train()
    spy = Spy(monkeypatch)
    taps = Taps(monkeypatch, net)
    try:
        loss = T.loss_of(case.loss, net(x).float(), y)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        taps.close()
    assert spy.calls["psf_sum_tensors_bf16"] == 1 and spy.calls["psf_chord_spmm_bwd_bf16"] == M and spy.calls["psf_chord_chain_bwd_bf16"] == 0
    e = next(e for e in taps.events if e.stage == "chain")
    saved = taps.saved[0]
    W64, V64 = [_np(w) for w in e.ins["Ws"]], _np(e.ins["V0"])
    X = [V64] + [_np(s) for s in saved[1 + M:]]
    want = S.chain_backward(W64, X, _np(e.outs["V"].grad), True, T.chord_offsets(N, M + 1))
    terms = S.chain_terms(M, M + 1, C)
    v = Verdicts(case, f"adding one_fs_loop/{which}", _stock_ok("adding"))
    v.judge("chain", "dV0", _np(e.ins["V0"].grad), *want["dV0"], terms["dV0"])
    for m in range(M):
        if m == 3:
            assert e.ins["Ws"][m].grad is None
        else:
            v.judge("chain", f"dW[{m}]", _np(e.ins["Ws"][m].grad), *want["dW"][m], terms["dW"][m])
    v.print()
    assert not v.shares.over(), v.shares.over()
