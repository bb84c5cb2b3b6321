"""GPU: ``token_linear.bf16_linear_route`` — which entries the token-wise Linear layers of a bf16 model reach, and what they return.

  per layer     TokenLinear in bf16 at T = 4096, widths (2 -> 32), (32 -> 8), (32 -> 128), route "always": one call of
                psf_linear_wgrad_bf16 (and of psf_affine_rows_bf16 for the two-input layer), inside the refusing pointer audit of
                tests/ptr_audit.py. dW and db against the stock nn.Linear on the same operands: both are single roundings of f32
                sums of the same exact products, each within
                    bound = 2^-8 |ref| + T 2^-24 sum_t |dY[t,j]| |X[t,i]|          (tests/test_gpu_linear_wgrad_bf16.py)
                of the float64 product ``ref``, so they differ by at most twice that. dx and the forward: the stock bits.
  a whole model the bf16 SyntheticPSFNet of the Adding configuration at N = 128, B = 32 (T = 4096), init_linear included.
                "always": exactly 1 + (n_W + 1) calls of psf_linear_wgrad_bf16 — init_linear and the second layer of every
                producer MLP, which fused_mlp.stacked_apply hands over as column slices — counted by the spy of
                tests/test_gpu_model_twin.py; every answer of wgrad_supported is True, no F.linear outside _TokenLinearFn.forward
                sees one of those weights, no TokenLinear reaches nn.Linear.forward; init_linear's rows come from
                psf_affine_rows_bf16. (The stacked FIRST layers of the MLPs are one F.linear at either setting.) "never": neither entry is called and every gradient has the
                bits of the stock formulas, recorded in the same test with TokenLinear.forward replaced by nn.Linear.forward.
  graph         one training step captured with train.GraphedStep and master-weight Adam replays with the eager step's bits;
                ``psf_training --problem adding --bf16 --bf16-linear --graph --json`` runs a short epoch.

This file holds graph captures and sorts in front of tests/test_gpu_coresidence.py, which wants to run before any graph has
been replayed in the process (see tests/test_gpu_graph_bf16_bwd.py). The captures are the LAST tests of this file; that the
co-residence test still observes its two streams behind them is checked by running the whole suite in order.
"""
import copy
import json

import numpy as np
import pytest
import torch
from torch import nn

from test_gpu_autocast import Spy, audited

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
NEW = ("psf_linear_wgrad_bf16", "psf_affine_rows_bf16")


@pytest.fixture
def route_always(monkeypatch):
    from sparsefactorization_amd import token_linear as tl
    assert tl.bf16_linear_route == "never"
    monkeypatch.setattr(tl, "bf16_linear_route", "always")


def _bits(t):
    return t.detach().contiguous().view(torch.int16)


def _layer_run(layer, x, dy):
    x = x.detach().clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    out = layer(x)
    out.backward(dy)
    return {"out": out.detach(), "dx": x.grad, "dW": layer.weight.grad, "db": layer.bias.grad}


@pytest.mark.parametrize("widths", [(2, 32), (32, 8), (32, 128)], ids=lambda w: f"{w[0]}to{w[1]}")
def test_layer_gradients_against_the_stock_module(gpu, monkeypatch, route_always, widths):
    from sparsefactorization_amd import token_linear as tl
    fin, fout = widths
    torch.manual_seed(fin * 1000 + fout)
    mine = tl.TokenLinear(fin, fout).to(gpu).to(BF16)
    stock = nn.Linear(fin, fout).to(gpu).to(BF16)
    stock.load_state_dict(mine.state_dict())
    g = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn(4, 1024, fin, device=gpu, generator=g).to(BF16)
    dy = torch.randn(4, 1024, fout, device=gpu, generator=g).to(BF16)
    T = 4096
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        got = _layer_run(mine, x, dy)
    assert spy.calls["psf_linear_wgrad_bf16"] == 1 and spy.calls["psf_affine_rows_bf16"] == (1 if fin <= 3 else 0), dict(spy.calls)
    assert spy.calls["psf_linear_wgrad_strided_f32"] == 0 and spy.calls["psf_affine_rows_f32"] == 0
    want = _layer_run(stock, x, dy)
    x64, y64 = x.reshape(T, fin).to(F64), dy.reshape(T, fout).to(F64)
    ref_W, abs_W = y64.t() @ x64, y64.abs().t() @ x64.abs()
    ref_b, abs_b = y64.sum(0), y64.abs().sum(0)
    for name, ref, mag in (("dW", ref_W, abs_W), ("db", ref_b, abs_b)):
        bound = 2.0 ** -8 * ref.abs() + T * 2.0 ** -24 * mag
        mine_err, pair = (got[name].to(F64) - ref).abs(), (got[name].to(F64) - want[name].to(F64)).abs()
        print(f"{name} {fin}->{fout}: route vs float64 worst ratio {float((mine_err / bound).max()):.4f}, "
              f"route vs stock worst ratio {float((pair / (2 * bound)).max()):.4f}, {int((pair > 0).sum())} of {pair.numel()} differ")
        assert got[name].dtype == BF16 and bool((mine_err <= bound).all()), f"{name}: beyond the bound of the float64 product"
        assert bool((pair <= 2 * bound).all()), f"{name}: further from the stock module than twice the bound"
    diff_out = int((_bits(got["out"]) != _bits(want["out"])).sum())
    print(f"forward {fin}->{fout}: {diff_out} of {got['out'].numel()} elements differ from the stock module")
    assert torch.equal(_bits(got["dx"]), _bits(want["dx"])), "dx is not the stock module's"
    assert diff_out == 0, "the forward is not the stock module's"


def test_a_slice_that_misses_the_alignment_and_an_ineligible_case(gpu, monkeypatch, route_always):
    """stacked_apply's operands: column slices of a wider array — taken with their row stride where the base is aligned, copied
    where it is not; below MIN_TOKENS the stock formulas, and nothing raises."""
    from sparsefactorization_amd import token_linear as tl
    g = torch.Generator(device=gpu).manual_seed(6)
    wide = torch.randn(4096, 72, device=gpu, generator=g).to(BF16)
    dy = torch.randn(4096, 8, device=gpu, generator=g).to(BF16)
    spy = Spy(monkeypatch)
    results = []
    for lo in (0, 8, 4, 1):  # 16-byte aligned twice, 8-byte, 2-byte: the last two are made contiguous (ld = 72 wants 16 bytes)
        x = wide[:, lo:lo + 32]
        assert tl.wgrad_supported(x, 8)
        dW, db = tl.linear_wgrad(x, dy)
        ref = dy.to(F64).t() @ x.to(F64)
        bound = 2.0 ** -8 * ref.abs() + 4096 * 2.0 ** -24 * (dy.to(F64).abs().t() @ x.to(F64).abs())
        assert bool(((dW.to(F64) - ref).abs() <= bound).all()), lo
        results.append(dW)
        assert torch.equal(_bits(dW), _bits(tl.linear_wgrad(x.contiguous(), dy)[0])), f"slice at column {lo}: not the contiguous operand's bits"
    assert spy.calls["psf_linear_wgrad_bf16"] == 8
    spy.reset()
    layer = tl.TokenLinear(32, 8).to(gpu).to(BF16)
    small = wide[:1000, :32]
    got = _layer_run(layer, small, dy[:1000])
    assert all(spy.calls[e] == 0 for e in NEW), dict(spy.calls)
    assert torch.equal(got["out"], nn.functional.linear(small, layer.weight, layer.bias))


def _adding_model(gpu, seed=0):
    from sparsefactorization_amd import psf_training
    torch.manual_seed(seed)
    net = psf_training.build_model("adding", 128, use_cuda=False).to(gpu).to(BF16)
    X, Y = psf_training.make_split("adding", 32, 128, gpu, 11)
    return net, X.to(BF16), Y


def _model_grads(net, X, Y):
    net.zero_grad(set_to_none=True)
    loss = nn.functional.mse_loss(net(X).squeeze().float(), Y)
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _token_linears(net):
    from sparsefactorization_amd import token_linear as tl
    return {name: m for name, m in net.named_modules() if isinstance(m, tl.TokenLinear)}


def test_whole_model_route_always_and_never(gpu, monkeypatch):
    from sparsefactorization_amd import token_linear as tl
    net, X, Y = _adding_model(gpu)
    assert X.shape[0] * X.shape[1] == 4096 and "init_linear" in _token_linears(net)
    spy = Spy(monkeypatch)
    # "never": the parent's path, and its bits — recorded from the stock formulas (nn.Linear.forward in TokenLinear's place)
    assert tl.bf16_linear_route == "never"
    loss_never, never = _model_grads(net, X, Y)
    assert all(spy.calls[e] == 0 for e in NEW), dict(spy.calls)
    with monkeypatch.context() as mp:
        mp.setattr(tl.TokenLinear, "forward", nn.Linear.forward)
        loss_stock, stock = _model_grads(net, X, Y)
    assert loss_never == loss_stock and never.keys() == stock.keys()
    for k in stock:
        assert torch.equal(_bits(never[k]), _bits(stock[k])), f'"never": {k}.grad is not the stock formulas\' bits'
    # "always": init_linear (through TokenLinear.forward) and the second layer of every producer MLP (through
    # fused_mlp.stacked_apply, which asks wgrad_supported itself and otherwise calls F.linear) take the new kernel. Three traps:
    # every answer of wgrad_supported, every F.linear outside _TokenLinearFn.forward, every nn.Linear.forward.
    n_mlps = int(np.log2(128)) + 1  # n_W link MLPs and g
    layers = _token_linears(net)
    assert len(layers) == 1 + 2 * n_mlps, sorted(layers)
    routed = {id(m.weight): name for name, m in layers.items() if name == "init_linear" or name.endswith(".2")}
    second = [name for name in routed.values() if name != "init_linear"]
    assert len(second) == n_mlps, second  # (the blocks are Sequential(Linear, GELU, Linear): the second layer is module "2")
    asked, stray, stock_linears, inside = [], [], [], []
    real_supported, real_linear, real_fn_forward, real_super_forward = tl.wgrad_supported, nn.functional.linear, tl._TokenLinearFn.forward, nn.Linear.forward

    def supported(x2d, out_features):
        ok = real_supported(x2d, out_features)
        asked.append((tuple(x2d.shape), x2d.stride(0), out_features, ok))
        return ok

    def fn_forward(ctx, x, weight, bias):
        inside.append(1)
        try:
            return real_fn_forward(ctx, x, weight, bias)
        finally:
            inside.pop()

    def linear(x, weight, bias=None):
        if not inside and id(weight) in routed:
            stray.append(routed[id(weight)])
        return real_linear(x, weight, bias)

    with monkeypatch.context() as mp:
        mp.setattr(tl, "bf16_linear_route", "always")
        mp.setattr(tl, "wgrad_supported", supported)
        mp.setattr(tl._TokenLinearFn, "forward", staticmethod(fn_forward))
        mp.setattr(nn.functional, "linear", linear)
        mp.setattr(nn.Linear, "forward", lambda self, x: (stock_linears.append(type(self).__name__), real_super_forward(self, x))[1])
        spy.reset()
        routes_before = len(spy.routes)
        loss_always, always = _model_grads(net, X, Y)
    print(f"wgrad_supported answers: {asked}; entry calls: { {e: spy.calls[e] for e in NEW} }; producer routes: {spy.routes[routes_before:]}; "
          f"stray F.linear: {stray}; nn.Linear forwards: {stock_linears}")
    routes = [r for r in spy.routes[routes_before:] if r is not None]
    assert routes and all(r == "stacked" for r in routes), "the producer MLPs of a bf16 model in training take stacked_apply"
    assert len(asked) == 1 + n_mlps and all(ok for *_, ok in asked), asked
    assert sum(1 for shape, ld, _, _ in asked if ld > shape[1]) == n_mlps, "the second layers' operands are column slices of the stacked hidden layer"
    assert spy.calls["psf_linear_wgrad_bf16"] == 1 + n_mlps and spy.calls["psf_affine_rows_bf16"] == 1, dict(spy.calls)
    assert not stray, f"F.linear (a library GEMM for the weight gradient) ran for {stray}"
    assert "TokenLinear" not in stock_linears, "a TokenLinear layer fell back to nn.Linear.forward (a library GEMM for its weight gradient)"
    assert spy.calls["psf_linear_wgrad_strided_f32"] == 0
    assert abs(loss_always - loss_never) <= 2.0 ** -6 * abs(loss_never) + 1e-6
    assert always.keys() == never.keys() and all(bool(torch.isfinite(v.float()).all()) for v in always.values())
    # the switch is back: the parent's bits again
    _, again = _model_grads(net, X, Y)
    assert all(torch.equal(_bits(again[k]), _bits(never[k])) for k in never)


# ------------------------------------------------------------------------------------------------- graph captures: last
def _eager_step(net, opt, loss, X, Y):
    opt.zero_grad(set_to_none=True)
    out = loss(net(X).squeeze(), Y)
    out.backward()
    opt.step()
    return out.detach()


def _f32_mse(pred, target):
    return nn.functional.mse_loss(pred.float(), target)


def test_a_captured_step_replays_with_the_eager_bits(gpu, monkeypatch, route_always):
    from sparsefactorization_amd import token_linear as tl
    from sparsefactorization_amd.train import ChunkedAdam, GraphedStep, make_adam
    monkeypatch.setattr(tl, "bf16_route", "always")  # the model's (unused) bf16 token table: train.check_capturable asks for it
    net_g, X, Y = _adding_model(gpu, seed=2)
    net_e = copy.deepcopy(net_g)
    opt_g = make_adam(net_g.parameters(), 1e-3, capturable=True, master_weights=True)
    opt_e = make_adam(net_e.parameters(), 1e-3, capturable=True, master_weights=True)
    assert isinstance(opt_g, ChunkedAdam)
    step = GraphedStep(net_g, opt_g, _f32_mse, X, Y, warmup_steps=3)
    for k in range(3):
        loss_g, loss_e = float(step(X, Y)), float(_eager_step(net_e, opt_e, _f32_mse, X, Y))
        assert loss_g == loss_e, (k, loss_g, loss_e)
    torch.cuda.synchronize(gpu)
    for (name, pg), pe in zip(net_g.named_parameters(), net_e.parameters()):
        assert torch.equal(_bits(pg), _bits(pe)), name
        assert opt_g.state[pg].keys() == opt_e.state[pe].keys(), name  # (a parameter no gradient reaches has no state in either)
        for key in ("master", "exp_avg", "exp_avg_sq"):
            if key in opt_g.state[pg]:
                assert torch.equal(opt_g.state[pg][key], opt_e.state[pe][key]), (name, key)


def test_the_adding_problem_trains_in_bf16_from_a_graph(gpu, capsys):
    from sparsefactorization_amd import psf_training, psfnet, token_linear as tl
    saved = (tl.bf16_route, tl.bf16_linear_route, psfnet.bf16_head_route)
    # where the driver starts from: its own seed, model and first training batch, before any step
    psf_training.seed_everything(42)
    net0 = psf_training.build_model("adding", 128).to(gpu).to(BF16)
    X0, Y0 = psf_training.make_split("adding", 640, 128, gpu, 1000)
    with torch.no_grad():
        start = float(_f32_mse(net0(X0[:32].to(BF16)).squeeze(), Y0[:32]))
    try:
        psf_training.main(["--problem", "adding", "--n-vec", "128", "--bf16", "--bf16-linear", "--graph", "--json", "--train-seqs", "640",
                           "--eval-seqs", "40", "--batch-size", "32", "--max-steps", "20"])
        last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    finally:
        tl.bf16_route, tl.bf16_linear_route, psfnet.bf16_head_route = saved
    print(f"adding --bf16 --bf16-linear --graph: loss of the untrained model {start:.5f}, mean loss of the 20 timed steps {last['loss']:.5f}")
    assert last["dtype"] == "bf16" and last["hip_graph"] is True and last["steps"] == 20
    assert np.isfinite(start) and np.isfinite(last["loss"]) and last["loss"] < start
