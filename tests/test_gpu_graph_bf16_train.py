"""GPU: a bf16 token model trains from a HIP graph — token_linear.bf16_route = "always" (lookup and table gradient on the
library's bf16 instances) plus make_adam(..., capturable=True, master_weights=True) (f32 master weights in ChunkedAdam).

  a. a module in which nothing goes through a BLAS (TokenEmbedding + positional add + elementwise operators + a sum loss): 10
     replays are bit-equal to 10 eager steps from the same start — parameters, master, exp_avg, exp_avg_sq. That pins the
     warm-up undo of ``master`` as well: GraphedStep's three warm-up steps create it, and the undo must put back the restored
     parameter's value, not zero.
  b. the Temporal-Order PSFNet at N = 128, B = 8 in bf16: the capture succeeds, and 20 graphed steps on one fixed batch follow
     the eager losses within 4 x the largest per-step difference between two eager runs (the project's factor for another
     summation order; exact equality where the two eager runs agree exactly).

On the parent both fail in GraphedStep's constructor (check_capturable refuses the bf16 table; make_adam has no
master_weights). In a file of its own, sorted behind tests/test_gpu_coresidence.py, for the reason given in
tests/test_gpu_graph_bf16_bwd.py: a graph replay makes the HIP runtime take hardware queues for itself.
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture
def bf16_route():
    from sparsefactorization_amd import token_linear
    assert token_linear.bf16_route == "never"
    token_linear.bf16_route = "always"
    yield
    token_linear.bf16_route = "never"


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


class _AllLibrary(torch.nn.Module):
    """Lookup + positional add (psf_embed_tokens_bf16), then elementwise operators only."""

    def __init__(self, vocab, n, width):
        super().__init__()
        from sparsefactorization_amd.token_linear import TokenEmbedding
        self.embedding = TokenEmbedding(vocab, width)
        self.pos_embedding = torch.nn.Embedding(n, width)  # a parameter holder, as in PSFNet: never looked up
        self.scale = torch.nn.Parameter(torch.ones(width))

    def forward(self, idx):
        from sparsefactorization_amd.token_linear import embed_tokens
        x = embed_tokens(idx, self.embedding, self.pos_embedding.weight)
        return torch.tanh(x) * self.scale + 0.25 * x * x


def _sum_loss(pred, target):
    return ((pred - target) ** 2).sum()


def _eager_step(net, opt, loss, X, Y):
    opt.zero_grad(set_to_none=True)
    out = loss(net(X).squeeze(), Y)
    out.backward()
    opt.step()
    return out.detach()


def test_graphed_steps_of_an_all_library_module_are_the_eager_bits(gpu, bf16_route):
    from sparsefactorization_amd.train import ChunkedAdam, GraphedStep, make_adam
    B, N, V, E = 4, 96, 6, 16
    torch.manual_seed(3)
    net_g = _AllLibrary(V, N, E).to(gpu).to(BF16)
    net_e = copy.deepcopy(net_g)
    start = [p.detach().clone() for p in net_g.parameters()]
    gen = torch.Generator().manual_seed(4)
    X = torch.randint(0, V, (B, N), generator=gen).to(gpu)
    Y = torch.randn(B, N, E, generator=gen).to(BF16).to(gpu)
    opt_g = make_adam(net_g.parameters(), 1e-3, capturable=True, master_weights=True)
    opt_e = make_adam(net_e.parameters(), 1e-3, capturable=True, master_weights=True)
    assert isinstance(opt_g, ChunkedAdam) and isinstance(opt_e, ChunkedAdam)
    step = GraphedStep(net_g, opt_g, _sum_loss, X, Y, warmup_steps=3)
    # the warm-up is undone: parameters at their start, every master the f32 value of its parameter, moments zero, count 0
    for p, s0 in zip(net_g.parameters(), start):
        assert np.array_equal(_bits(p), _bits(s0))
        st = opt_g.state[p]
        assert st["master"].dtype == torch.float32 and np.array_equal(_bits(st["master"]), _bits(s0.float())), "master after the warm-up undo"
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 0.0
    for k in range(10):
        loss_g = float(step(X, Y))
        loss_e = float(_eager_step(net_e, opt_e, _sum_loss, X, Y))
        assert loss_g == loss_e, (k, loss_g, loss_e)
    torch.cuda.synchronize(gpu)
    for (name, pg), pe, s0 in zip(net_g.named_parameters(), net_e.parameters(), start):
        assert pg.dtype == BF16
        assert np.array_equal(_bits(pg), _bits(pe)), name
        assert not np.array_equal(_bits(pg), _bits(s0)), f"{name} did not move"
        for key in ("master", "exp_avg", "exp_avg_sq"):
            a, b = opt_g.state[pg][key], opt_e.state[pe][key]
            assert a.dtype == torch.float32 and np.array_equal(_bits(a), _bits(b)), (name, key)
        assert float(opt_g.state[pg]["step"]) == float(opt_e.state[pe]["step"]) == 10.0
        assert np.array_equal(_bits(pg), _bits(opt_g.state[pg]["master"].to(BF16))), f"{name} is its master, rounded"


def _order_run(gpu, graphed, steps=20, B=8, N=128):
    """(per-step losses, the net, its starting parameters) of the bf16 Temporal-Order PSFNet on one fixed batch."""
    from sparsefactorization_amd import psf_training
    from sparsefactorization_amd.train import ChunkedAdam, GraphedStep, make_adam
    torch.manual_seed(0)
    net = psf_training.build_model("order", N, use_cuda=False).to(gpu).to(BF16)
    start = {k: p.detach().clone() for k, p in net.named_parameters()}
    gen = torch.Generator().manual_seed(1)
    X = torch.randint(0, 6, (B, N, 1), generator=gen).to(gpu)
    Y = torch.randint(0, 4, (B,), generator=gen).to(gpu)
    loss = torch.nn.CrossEntropyLoss()
    opt = make_adam(net.parameters(), 1e-3, capturable=True, master_weights=True)
    assert isinstance(opt, ChunkedAdam)
    if graphed:
        step = GraphedStep(net, opt, loss, X, Y, warmup_steps=3)  # the capture must succeed
        losses = [float(step(X, Y)) for _ in range(steps)]
    else:
        losses = [float(_eager_step(net, opt, loss, X, Y)) for _ in range(steps)]
    return np.array(losses, dtype=np.float64), net, start


def test_the_bf16_temporal_order_model_trains_from_a_graph(gpu, bf16_route):
    """Measured on the MI355X (profiles/bf16_train_graph_ab.md): the two eager runs and the graphed run gave the same 20 losses,
    so the bar was exact equality."""
    eager_a, _, _ = _order_run(gpu, graphed=False)
    eager_b, _, _ = _order_run(gpu, graphed=False)
    graph, net, start = _order_run(gpu, graphed=True)
    spread = float(np.abs(eager_a - eager_b).max())
    diff = float(np.abs(graph - eager_a).max())
    print(f"BF16_GRAPH_ORDER: eager-eager spread {spread:.3e}, graph-eager difference {diff:.3e}; first loss {graph[0]:.4f}, last {graph[-1]:.4f}")
    if spread == 0.0:
        assert np.array_equal(graph, eager_a), (graph, eager_a)
    else:
        assert diff <= 4 * spread, (diff, spread)
    for name, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), name
    assert graph[-1] < graph[0]
    w = net.embedding.weight
    assert w.dtype == BF16 and not np.array_equal(_bits(w), _bits(start["embedding.weight"])), \
        "embedding.weight did not move: at lr = 1e-3 it cannot under a pure-bf16 Adam, and must with master weights"
