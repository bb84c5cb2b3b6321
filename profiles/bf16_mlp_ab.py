"""The bf16 producer MLPs of an inference call: the fused launch (psf_mlp_fwd_bf16) against the stacked route it replaces.

One process per size, the two routes alternating per round on the same seeded bf16 modules and the same input, under
no_grad, HIP events around ``iters`` calls, one warm-up call per route and round. Routes:
    stacked   fused_mlp.stacked_apply — one stacked library GEMM, one GELU kernel, K small library GEMMs: what a bf16
              PSFNet ran before the fused kernel existed (the yardstick)
    fused     fused_mlp.fused_mlp_forward_bf16 — the packing kernel plus one launch, the hidden layer in registers
Before the timing the two routes' outputs are compared (they may differ only where an f32 sum lands on a bf16 tie).
Prints one JSON line per (size, route): median us per call over the rounds, the min - max spread, and per size the ratio.

Without --size the sizes run one after another, each in a child process of its own under a time limit; the first failure
ends the run (nothing more is started on a GPU that has faulted).

    python profiles/bf16_mlp_ab.py [--rounds 9] [--iters N] [--size NAME]
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
IMDB = (32, [(128, 32)] + [(128, 13)] * 12)      # the IMDb / Pathfinder widths
SIZES = {  # name: (B, N, (E, layers), iters per round)
    "adding_64x16384": (64, 16384, ADDING, 20),
    "adding_8x1024": (8, 1024, ADDING, 200),
    "adding_8x128": (8, 128, ADDING, 200),
    "imdb_32x1024": (32, 1024, IMDB, 50),
}
CHILD_LIMIT_S = 240


def run_size(name, rounds, iters):
    import torch
    from torch import nn
    from sparsefactorization_amd import fused_mlp

    B, N, (E, layers), default_iters = SIZES[name]
    iters = iters or default_iters
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    class Block(nn.Module):
        def __init__(self, h, O):
            super().__init__()
            self.network = nn.Sequential(nn.Linear(E, h), nn.GELU(), nn.Linear(h, O))

    blocks = [Block(h, O).to(torch.bfloat16).to(dev) for h, O in layers]
    x = torch.randn(B, N, E).to(torch.bfloat16).to(dev)
    routes = {"stacked": fused_mlp.stacked_apply, "fused": fused_mlp.fused_mlp_forward_bf16}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(x, blocks)
        torch.cuda.synchronize()
        s.record()
        for _ in range(iters):
            fn(x, blocks)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / iters

    with torch.no_grad():
        assert fused_mlp.route(x, blocks) == "bf16_forward" and fused_mlp.stackable(x, blocks)  # (both would take it)
        a, b = routes["stacked"](x, blocks), routes["fused"](x, blocks)
        torch.cuda.synchronize()
        differ = sum(int((p != q).sum()) for p, q in zip(a, b))
        total = sum(p.numel() for p in a)
        worst = max(float((p.float() - q.float()).abs().max()) for p, q in zip(a, b))
        del a, b
        times = {r: [] for r in routes}
        for _ in range(rounds):
            for r, fn in routes.items():
                times[r].append(timed(fn))
    med = {r: statistics.median(ts) for r, ts in times.items()}
    for r, ts in times.items():
        print(json.dumps({"size": name, "T": B * N, "E": E, "K": len(layers), "h": layers[0][0], "route": r,
                          "us": round(med[r], 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)], "rounds": rounds,
                          "iters": iters}), flush=True)
    print(json.dumps({"size": name, "stacked_over_fused": round(med["stacked"] / med["fused"], 3),
                      "differing_elements": differ, "of": total, "largest_difference": worst}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
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
