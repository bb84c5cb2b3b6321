"""The bf16 producer MLPs of a training call, forward + backward: the opt-in fused route (psf_mlp_fwd_bf16 +
psf_mlp_bwd_bf16, ``fused_mlp.bf16_train_route = "always"``) against the stacked route it would replace ("never", the default).

One process per size, the two settings alternating per round on the same seeded bf16 modules, the same input and the same
output gradients; a call is ``ys = fused_mlp.apply(x, blocks); torch.autograd.backward(ys, dys)`` with the parameters' and
x's gradients cleared before it. Two ways of running it:
    eager   HIP events around ``iters`` calls, one warm-up call per setting and round: what a training step pays, the host's
            issue of the launches and the allocations included
    graph   the same call captured once per setting in a torch.cuda.graph and replayed ``iters`` times: the kernels alone
Before the timing the two settings' gradients are compared (they make the same roundings and may differ where an f32 sum
lands on a bf16 tie). Prints one JSON line per (size, mode, setting): median us per call over the rounds and the min - max
spread, and per size the ratios.

Without --size the sizes run one after another, each in a child process of its own under a time limit; the first failure
ends the run (nothing more is started on a GPU that has faulted).

    python profiles/bf16_mlp_bwd_ab.py [--rounds 7] [--iters N] [--size NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADDING = (32, [(32, 8)] + [(32, 15)] * 14)       # E, [(h, O)]: g + 14 link MLPs of the Adding / Order model
IMDB = (32, [(128, 32)] + [(128, 13)] * 12)      # the IMDb / Pathfinder widths (E = 32: inside the backward's limit)
SIZES = {  # name: (B, N, (E, layers), eager calls per round, graph replays per round): every timed window is 0.1 s or longer
    "adding_64x16384": (64, 16384, ADDING, 10, 100),   # (with "always"; several times that with "never")
    "adding_8x1024": (8, 1024, ADDING, 200, 2000),
    "adding_8x128": (8, 128, ADDING, 200, 2000),
    "imdb_32x1024": (32, 1024, IMDB, 200, 500),
}
SETTINGS = ("never", "always")
CHILD_LIMIT_S = 240


def run_size(name, rounds, iters):
    import torch
    from torch import nn
    from sparsefactorization_amd import fused_mlp

    B, N, (E, layers), default_iters, default_replays = SIZES[name]
    replays = iters or default_replays
    iters = iters or default_iters
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    class Block(nn.Module):
        def __init__(self, h, O):
            super().__init__()
            self.network = nn.Sequential(nn.Linear(E, h), nn.GELU(), nn.Linear(h, O))

    blocks = [Block(h, O).to(torch.bfloat16).to(dev) for h, O in layers]
    params = [p for b in blocks for p in b.parameters()]
    x = torch.randn(B, N, E).to(torch.bfloat16).to(dev).requires_grad_(True)
    dys = [torch.randn(B, N, O).to(torch.bfloat16).to(dev) for _, O in layers]
    want = {"never": "stacked", "always": "bf16_train"}

    def step():
        x.grad = None
        for p in params:
            p.grad = None
        torch.autograd.backward(fused_mlp.apply(x, blocks), dys)

    def grads():
        return [x.grad.clone()] + [p.grad.clone() for p in params]

    def eager():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        step()
        torch.cuda.synchronize()
        s.record()
        for _ in range(iters):
            step()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / iters

    def replay(graph):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        graph.replay()
        torch.cuda.synchronize()
        s.record()
        for _ in range(replays):
            graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / replays

    got = {}
    for setting in SETTINGS:
        fused_mlp.bf16_train_route = setting
        assert fused_mlp.route(x, blocks) == want[setting], (setting, fused_mlp.route(x, blocks))
        step()
        torch.cuda.synchronize()
        got[setting] = grads()
    differ = sum(int((p != q).sum()) for p, q in zip(got["never"], got["always"]))
    total = sum(p.numel() for p in got["never"])
    # per tensor, relative to the tensor's largest element (weight gradients are sums over T that cancel: relative to the element
    # itself a one-step difference of a near-zero sum is arbitrarily large)
    worst = max(float((p.float() - q.float()).abs().max() / q.float().abs().max().clamp_min(1e-30)) for p, q in zip(got["never"], got["always"]))
    del got

    times = {("eager", s): [] for s in SETTINGS}
    for _ in range(rounds):
        for setting in SETTINGS:
            fused_mlp.bf16_train_route = setting
            times[("eager", setting)].append(eager())

    graphs = {}
    side = torch.cuda.Stream(device=dev)
    for setting in SETTINGS:  # warm-up on a side stream, then one capture per setting
        fused_mlp.bf16_train_route = setting
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        x.grad = None
        for p in params:
            p.grad = None
        graphs[setting] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[setting]):
            step()
    fused_mlp.bf16_train_route = "never"
    times.update({("graph", s): [] for s in SETTINGS})
    for _ in range(rounds):
        for setting in SETTINGS:
            times[("graph", setting)].append(replay(graphs[setting]))

    med = {k: statistics.median(ts) for k, ts in times.items()}
    for (mode, setting), ts in times.items():
        print(json.dumps({"size": name, "T": B * N, "E": E, "K": len(layers), "h": layers[0][0], "mode": mode, "bf16_train_route": setting,
                          "us": round(med[(mode, setting)], 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)], "rounds": rounds,
                          "iters": replays if mode == "graph" else iters}), flush=True)
    print(json.dumps({"size": name, "never_over_always_eager": round(med[("eager", "never")] / med[("eager", "always")], 3),
                      "never_over_always_graph": round(med[("graph", "never")] / med[("graph", "always")], 3),
                      "differing_gradient_elements": differ, "of": total, "largest_difference_over_tensor_max": worst}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--size", default=None, choices=sorted(SIZES))
    args = ap.parse_args()
    if args.size:
        run_size(args.size, args.rounds, args.iters)
        return 0
    for name in SIZES:  # one child per size, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--size", name, "--rounds", str(args.rounds), "--iters", str(args.iters)]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"size": name, "error": f"no result within {CHILD_LIMIT_S} s"}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"size": name, "error": f"exit status {rc}"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
