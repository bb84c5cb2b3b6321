"""GPU: ``psfnet.bf16_head_route`` — which entries a bf16 FLATTEN head reaches, and that what it returns is right.

Calls are counted with the spy of tests/test_gpu_autocast.py (``Spy`` of test_gpu_model_twin.py) inside the refusing pointer audit
of tests/ptr_audit.py. Values: out, dX, dW and db against float64 products of the same bf16 operands, every element within
    |got - ref| <= 2^-8 |ref| + n 2^-24 sum_i |a_i| |b_i|
(half a bf16 ulp for the one rounding plus the worst-case f32 accumulation bound; n = K + 1 for the logits, B for dW and db, J for
dX) — the bound of tests/test_gpu_flat_head_bf16.py.

  route "always", J = 4    one call of psf_flat_head_bf16 and one of psf_flat_head_bwd_bf16, none of the f32 entries
  route "always", J = 16   F.linear forward, one psf_flat_head_bwd_bf16
  route "never"            neither entry; the bits of ``final(flat)``
  a view at a 2-byte storage offset, K = 4092, an f32 head, autocast: neither entry, nothing raises, the bits of ``final(flat)``
                           (the stock module's own accuracy is not this file's to pin)
  the bf16 Temporal-Order PSFNet at N = 512 (K = 4096), B = 4; the head captured in a HIP graph; the ``--bf16 --graph`` driver.

This file holds graph captures: it sorts behind tests/test_gpu_coresidence.py (see tests/test_gpu_graph_bf16_bwd.py).
"""
import math

import pytest
import torch
from torch import nn

from test_gpu_autocast import Spy, audited
from test_gpu_flat_head_bf16 import within_bound

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
NEW = ("psf_flat_head_bf16", "psf_flat_head_bwd_bf16")
OLD = ("psf_flat_head_f32", "psf_flat_head_bwd_f32")


def _head(gpu, K, J, seed=21, dtype=BF16):
    torch.manual_seed(seed)
    return nn.Linear(K, J).to(gpu).to(dtype)


def _operands(gpu, B, K, J, seed=22, dtype=BF16):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(B, K, device=gpu, generator=g).to(dtype), torch.randn(B, J, device=gpu, generator=g).to(dtype)


def _run(final, flat, dy, amp=False):
    from sparsefactorization_amd.psfnet import _flat_head
    flat = flat.detach().requires_grad_(True)  # a leaf on the caller's storage: a view keeps its offset and strides
    final.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        out = _flat_head(final, flat)
    out.backward(dy.to(out.dtype))
    return {"out": out.detach(), "dX": flat.grad, "dW": final.weight.grad, "db": final.bias.grad}


def _check_values(got, final, flat, dy, what):
    x, w, b, g = flat.to(F64), final.weight.detach().to(F64), final.bias.detach().to(F64), dy.to(F64)
    B, K = flat.shape
    J = w.shape[0]
    within_bound(got["out"], x @ w.t() + b, x.abs() @ w.abs().t() + b.abs(), K + 1, f"{what} out")
    within_bound(got["dX"], g @ w, g.abs() @ w.abs(), J, f"{what} dX")
    within_bound(got["dW"], g.t() @ x, g.abs().t() @ x.abs(), B, f"{what} dW")
    within_bound(got["db"], g.sum(0), g.abs().sum(0), B, f"{what} db")
    assert all(got[k].dtype == BF16 for k in got)


@pytest.mark.parametrize("J", [4, 16])
def test_route_always_takes_the_bf16_kernels(gpu, monkeypatch, J):
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    final = _head(gpu, 4096, J)
    flat, dy = _operands(gpu, 4, 4096, J)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        got = _run(final, flat, dy)
    assert spy.calls["psf_flat_head_bf16"] == (1 if J <= 8 else 0) and spy.calls["psf_flat_head_bwd_bf16"] == 1, dict(spy.calls)
    assert all(spy.calls[e] == 0 for e in OLD), dict(spy.calls)
    _check_values(got, final, flat, dy, f"always J={J}")


def test_route_never_is_the_stock_module(gpu, monkeypatch):
    from sparsefactorization_amd import psfnet
    assert psfnet.bf16_head_route == "never"
    final = _head(gpu, 4096, 4)
    flat, dy = _operands(gpu, 4, 4096, 4)
    spy = Spy(monkeypatch)
    got = _run(final, flat, dy)
    assert all(spy.calls[e] == 0 for e in NEW + OLD), dict(spy.calls)
    assert torch.equal(got["out"], final(flat))
    assert all(got[k].dtype == BF16 and bool(torch.isfinite(got[k].float()).all()) for k in got)


def test_what_the_route_does_not_cover_takes_the_stock_module(gpu, monkeypatch):
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    spy = Spy(monkeypatch)

    def stock(final, flat, dy, amp=False, what=""):
        spy.reset()
        got = _run(final, flat, dy, amp)
        assert all(spy.calls[e] == 0 for e in NEW), (what, dict(spy.calls))
        with torch.autocast("cuda", dtype=BF16, enabled=amp):
            assert torch.equal(got["out"], final(flat)), what
        return got

    final = _head(gpu, 4096, 4)
    flat, dy = _operands(gpu, 4, 4096, 4)
    # a view at a 2-byte storage offset: contiguous, but no 8-byte vectors
    store = torch.zeros(4 * 4096 + 4, dtype=BF16, device=gpu)
    odd = store[1:1 + 4 * 4096].view(4, 4096)
    odd.copy_(flat)
    assert odd.is_contiguous() and odd.data_ptr() % 8 == 2
    stock(final, odd, dy, what="unaligned")
    # K = 4092: below the gate
    f92 = _head(gpu, 4092, 4)
    x92 = flat[:, :4092].contiguous()
    stock(f92, x92, dy, what="K = 4092")
    # autocast on: the stock module decides the dtypes
    got = stock(final, flat, dy, amp=True, what="autocast")
    assert got["out"].dtype == BF16 and all(spy.calls[e] == 0 for e in OLD)
    # an f32 head: its f32 kernels as ever; and with bf16 activations under autocast, the stock module
    f32 = _head(gpu, 4096, 4, dtype=torch.float32)
    spy.reset()
    got = _run(f32, flat.float(), dy.float())
    assert all(spy.calls[e] == 0 for e in NEW) and all(spy.calls[e] == 1 for e in OLD), dict(spy.calls)
    assert got["out"].dtype == torch.float32
    spy.reset()
    got = _run(f32, flat, dy, amp=True)
    assert all(spy.calls[e] == 0 for e in NEW), dict(spy.calls)
    # a weight that is a view at an odd offset, and a non-contiguous input
    wstore = torch.zeros(4 * 4096 + 4, dtype=BF16, device=gpu)
    fodd = _head(gpu, 4096, 4)
    wview = wstore[1:1 + 4 * 4096].view(4, 4096)
    wview.copy_(fodd.weight.detach())
    fodd.weight = nn.Parameter(wview)
    stock(fodd, flat, dy, what="weight view")
    spy.reset()
    _run(final, torch.zeros(4096, 4, dtype=BF16, device=gpu).t(), dy)
    assert all(spy.calls[e] == 0 for e in NEW)


def test_fallbacks_inside_the_function(gpu, monkeypatch):
    """B > 1024: the kernel forward, the two ``mm`` calls backward."""
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    final = _head(gpu, 4096, 3)
    flat, dy = _operands(gpu, 1025, 4096, 3)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        got = _run(final, flat, dy)
    assert spy.calls["psf_flat_head_bf16"] == 1 and spy.calls["psf_flat_head_bwd_bf16"] == 0, dict(spy.calls)
    _check_values(got, final, flat, dy, "B = 1025")


def test_non_linear_head_first_layer(gpu, monkeypatch):
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    torch.manual_seed(5)
    final = nn.Sequential(nn.Linear(4096, 16), nn.GELU(), nn.Linear(16, 3)).to(gpu).to(BF16)
    flat, _ = _operands(gpu, 4, 4096, 3)
    spy = Spy(monkeypatch)
    x = flat.clone().requires_grad_(True)
    out = psfnet._flat_head(final, x)
    out.float().sum().backward()
    assert spy.calls["psf_flat_head_bf16"] == 0 and spy.calls["psf_flat_head_bwd_bf16"] == 1, dict(spy.calls)
    first = psfnet._flat_head(final[0], flat)  # (its values: the J = 16 case above)
    assert out.dtype == BF16 and torch.equal(out, final[1:](first))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in final.parameters()) and x.grad is not None


def _order_net(gpu, n_vec):
    from sparsefactorization_amd import psf_training
    torch.manual_seed(0)
    return psf_training.build_model("order", n_vec, use_cuda=False).to(gpu).to(BF16)


def test_bf16_order_model_takes_the_head_kernels(gpu, monkeypatch):
    """Temporal Order at N = 512: K = 512 x 8 = 4096, J = 4, B = 4."""
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    net = _order_net(gpu, 512)
    gen = torch.Generator().manual_seed(1)
    X, Y = torch.randint(0, 6, (4, 512, 1), generator=gen).to(gpu), torch.randint(0, 4, (4,), generator=gen).to(gpu)
    seen = []
    real = psfnet._flat_head
    monkeypatch.setattr(psfnet, "_flat_head", lambda final, flat: (seen.append(flat.detach().clone()), real(final, flat))[1])
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        logits = net(X)
        nn.CrossEntropyLoss()(logits.squeeze(), Y).backward()
    assert spy.calls["psf_flat_head_bf16"] == 1 and spy.calls["psf_flat_head_bwd_bf16"] == 1, dict(spy.calls)
    assert all(spy.calls[e] == 0 for e in OLD)
    assert logits.dtype == BF16 and bool(torch.isfinite(logits.float()).all())
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.dtype == BF16 and bool(torch.isfinite(p.grad.float()).all()), name
    assert len(seen) == 1 and seen[0].shape == (4, 4096)
    x, w, b = seen[0].to(F64), net.final.weight.detach().to(F64), net.final.bias.detach().to(F64)
    within_bound(logits.detach(), x @ w.t() + b, x.abs() @ w.abs().t() + b.abs(), 4096 + 1, "model logits")


def test_head_replays_from_a_graph(gpu, monkeypatch):
    """One forward + backward of the head (K = 4096, B = 4, J = 4) captured after a warm-up on a side stream: three replays leave
    the eager bits in out, dX and dW."""
    from sparsefactorization_amd import psfnet
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    final = _head(gpu, 4096, 4)
    flat, dy = _operands(gpu, 4, 4096, 4)
    eager = _run(final, flat, dy)
    x = flat.detach().clone().requires_grad_(True)
    w, b = final.weight, final.bias

    def step():
        out = psfnet._flat_head(final, x)
        return (out, *torch.autograd.grad(out, [x, w], dy))

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up (allocations)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    spy = Spy(monkeypatch)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    assert spy.calls["psf_flat_head_bf16"] == 1 and spy.calls["psf_flat_head_bwd_bf16"] == 1
    for _ in range(3):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
    torch.cuda.synchronize()
    for name, got in zip(("out", "dX", "dW"), captured):
        assert torch.equal(got.view(torch.int16), eager[name].view(torch.int16)), name


def test_driver_trains_in_bf16_from_a_graph(gpu, monkeypatch, capsys):
    import json

    from sparsefactorization_amd import psf_training, psfnet, token_linear
    from sparsefactorization_amd.train import ChunkedAdam
    monkeypatch.setattr(token_linear, "bf16_route", token_linear.bf16_route)  # main sets both: put back afterwards
    monkeypatch.setattr(psfnet, "bf16_head_route", psfnet.bf16_head_route)
    with pytest.raises(SystemExit):
        psf_training.main(["--problem", "adding", "--bf16"])
    assert psfnet.bf16_head_route == "never" and token_linear.bf16_route == "never"
    spy = Spy(monkeypatch)
    res = psf_training.main(["--problem", "order", "--n-vec", "512", "--bf16", "--graph", "--json",
                             "--max-steps", "4", "--train-seqs", "160", "--eval-seqs", "40"])
    assert psfnet.bf16_head_route == "always" and token_linear.bf16_route == "always"
    params = list(res["net"].parameters())
    assert params and all(p.dtype == BF16 for p in params)
    opt = res["optimizer"]
    assert isinstance(opt, ChunkedAdam)
    for p in params:
        assert opt.state[p]["master"].dtype == torch.float32 and opt.state[p]["master"].shape == p.shape
    assert spy.calls["psf_flat_head_bf16"] >= 1 and spy.calls["psf_flat_head_bwd_bf16"] >= 1, dict(spy.calls)
    assert math.isfinite(res["stats"]["loss"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["dtype"] == "bf16" and line["hip_graph"] is True and math.isfinite(line["loss"])
