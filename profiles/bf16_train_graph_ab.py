"""Graph-captured bf16 training (``token_linear.bf16_route = "always"`` + ``make_adam(..., master_weights=True)``): three A/Bs.

    step    the Temporal-Order PSFNet in bf16 at B = 64, N = 128 and N = 1024: one training step (zero_grad, forward, loss,
            backward, ChunkedAdam step on f32 master weights) issued eagerly against the same step replayed from the HIP graph
            that ``train.GraphedStep`` captures. Two copies of one seeded model, the two modes alternating per round.
    wgrad   the table gradient at T = 64 x 16384, V = 6, E = 32 from one bf16 d(out): ``psf_embed_tokens_bwd_bf16`` (workspace
            and output allocated once) against ``aten::embedding_dense_backward`` on the same bf16 tensor, alternating.
    adam    ``psf_adam_step_master`` (bf16 parameter and gradient, f32 master and moments) against ``psf_adam_step_f32`` on two
            524 288-element tensors — pos_embedding and final of a PSFNet at N = 16384 — alternating.

HIP events around ``iters`` calls after one warm-up call, ``--rounds`` rounds; every timed window is 0.1 s or longer. Prints one
JSON line per (part, size, arm): median us per call over the rounds and the min - max spread, then the ratio. Without --part the
parts run one after another, each in a child process of its own under a time limit; the first failure ends the run (nothing
more is started on a GPU that has faulted).

    python profiles/bf16_train_graph_ab.py [--rounds 7] [--part step_128|step_1024|wgrad|adam]
"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("step_128", "step_1024", "wgrad", "adam")
CHILD_LIMIT_S = 240


def _timed(fn, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def _report(part, size, arms, times, iters, extra=None):
    med = {a: statistics.median(times[a]) for a in arms}
    for a in arms:
        print(json.dumps({"part": part, **size, "arm": a, "us": round(med[a], 2),
                          "spread_us": [round(min(times[a]), 2), round(max(times[a]), 2)], "rounds": len(times[a]), "iters": iters[a]}),
              flush=True)
    print(json.dumps({"part": part, **size, f"{arms[0]}_over_{arms[1]}": round(med[arms[0]] / med[arms[1]], 3), **(extra or {})}), flush=True)


def run_step(N, rounds, B=64):
    import torch
    from sparsefactorization_amd import psf_training, token_linear
    from sparsefactorization_amd.train import ChunkedAdam, GraphedStep, make_adam
    dev = torch.device("cuda:0")
    token_linear.bf16_route = "always"
    torch.manual_seed(0)
    net_e = psf_training.build_model("order", N, use_cuda=False).to(dev).to(torch.bfloat16)
    net_g = copy.deepcopy(net_e)
    gen = torch.Generator().manual_seed(1)
    X = torch.randint(0, 6, (B, N, 1), generator=gen).to(dev)
    Y = torch.randint(0, 4, (B,), generator=gen).to(dev)
    loss = torch.nn.CrossEntropyLoss()
    opt_e = make_adam(net_e.parameters(), 1e-3, capturable=True, master_weights=True)
    opt_g = make_adam(net_g.parameters(), 1e-3, capturable=True, master_weights=True)
    assert isinstance(opt_e, ChunkedAdam)
    graphed = GraphedStep(net_g, opt_g, loss, X, Y, warmup_steps=3)

    def eager():
        opt_e.zero_grad(set_to_none=True)
        out = loss(net_e(X).squeeze(), Y)
        out.backward()
        opt_e.step()
        return out.detach()

    # the two copies take the same steps: the losses of the first three side by side, before the timing
    first = [(float(graphed(X, Y)), float(eager())) for _ in range(3)]
    arms = ("eager", "graph")
    fns = {"eager": eager, "graph": graphed.graph.replay}
    iters = {"eager": 100 if N <= 128 else 50, "graph": 1000 if N <= 128 else 200}
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:
            times[a].append(_timed(fns[a], iters[a]))
    n_params = sum(1 for p in net_e.parameters() if p.grad is not None)
    _report("step", {"B": B, "N": N}, arms, times, iters, {"parameters_stepped": n_params, "first_losses_graph_eager": first})


def run_wgrad(rounds, T=64 * 16384, V=6, E=32):
    import torch
    from sparsefactorization_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(2)
    idx = torch.randint(0, V, (T,), generator=gen).to(dev)
    dout = torch.randn(T, E, generator=gen).to(torch.bfloat16).to(dev)
    nbytes = lib.psf_embed_tokens_bwd_workspace(T, V, E)
    ws = torch.empty(nbytes // 4, device=dev)
    dW = torch.empty(V, E, dtype=torch.bfloat16, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def mine():
        _lib.check(lib.psf_embed_tokens_bwd_bf16(idx.data_ptr(), dout.data_ptr(), T, V, E, dW.data_ptr(), ws.data_ptr(), nbytes, stream),
                   "psf_embed_tokens_bwd_bf16")

    kept = []

    def aten():
        kept[:] = [torch.ops.aten.embedding_dense_backward(dout, idx, V, -1, False)]

    mine()
    aten()
    torch.cuda.synchronize()
    ref = torch.zeros(V, E, dtype=torch.float64, device=dev).index_add_(0, idx, dout.double())
    err = {name: float(((t.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max()) for name, t in (("library", dW), ("aten", kept[0]))}
    arms = ("aten", "library")
    fns = {"aten": aten, "library": mine}
    iters = {"aten": 40, "library": 2000}
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:
            times[a].append(_timed(fns[a], iters[a]))
    _report("wgrad", {"T": T, "V": V, "E": E}, arms, times, iters, {"largest_relative_error_against_float64": err})


def run_adam(rounds, n=524288, count=2):
    import torch
    from sparsefactorization_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3)
    mk = lambda dtype, scale=1.0: [(scale * torch.randn(n, generator=gen)).to(dtype).to(dev) for _ in range(count)]  # noqa: E731
    f32, bf16 = torch.float32, torch.bfloat16
    p32, g32, m32, v32 = mk(f32), mk(f32), mk(f32, 0.1), [t.square() for t in mk(f32)]
    master, pb, gb, mb, vb = mk(f32), mk(bf16), mk(bf16), mk(f32, 0.1), [t.square() for t in mk(f32)]
    tab = lambda ts: (ctypes.c_void_p * count)(*[t.data_ptr() for t in ts])  # noqa: E731
    sizes = (ctypes.c_int64 * count)(*[n] * count)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t32, tmaster = [tab(ts) for ts in (p32, g32, m32, v32)], [tab(ts) for ts in (master, pb, gb, mb, vb)]
    hyper = (1e-3, 0.9, 0.999, 1e-8, 10.0, None, stream)

    def step_f32():
        _lib.check(lib.psf_adam_step_f32(*t32, sizes, count, *hyper), "psf_adam_step_f32")

    def step_master():
        _lib.check(lib.psf_adam_step_master(*tmaster, sizes, count, *hyper), "psf_adam_step_master")

    arms = ("master", "f32")
    fns = {"master": step_master, "f32": step_f32}
    iters = {"master": 10000, "f32": 10000}
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:
            times[a].append(_timed(fns[a], iters[a]))
    # bytes per element: f32 reads p, g, m, v and writes p, m, v (28); master reads master, m, v + a bf16 g and writes them + a bf16 p (28)
    _report("adam", {"elements": n, "tensors": count}, arms, times, iters, {"bytes_per_element": {"master": 28, "f32": 28}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", default=None, choices=PARTS)
    args = ap.parse_args()
    if args.part:
        if args.part.startswith("step_"):
            run_step(int(args.part[5:]), args.rounds)
        else:
            {"wgrad": run_wgrad, "adam": run_adam}[args.part](args.rounds)
        return 0
    for part in PARTS:  # one child per part, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(args.rounds)]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"part": part, "error": f"no result within {CHILD_LIMIT_S} s"}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"part": part, "error": f"exit status {rc}"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
