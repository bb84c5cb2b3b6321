"""The whole bf16 mixer of a short sequence: the single launch (psf_mixer_fwd_bf16) against the two calls it replaces.

One process per size, the two routes alternating per round on the same seeded bf16 modules and the same input, under
no_grad, HIP events around ``iters`` calls, one warm-up call per route and round. Routes:
    two_calls  fused_mlp.fused_mlp_forward_bf16 + chord.chord_chain — what a bf16 PSFNet runs with
               fused_mixer.bf16_route = "never" (the yardstick): pack, producer and chain kernels, M + 1 producer outputs
    mixer      fused_mixer.mixer_forward_bf16 — pack plus one launch, V0, every W_m and V on chip
Each route is timed twice: eager (host-bound at these sizes) and replayed from a captured graph (the kernels).
Before the timing the two routes' results are compared: they must be the same bits.
Prints one JSON line per (size, mode, route): median us per forward over the rounds and the min - max spread, and per
(size, mode) the ratio.

Without --size the sizes run one after another, each in a child process of its own under a time limit; the first failure
ends the run (nothing more is started on a GPU that has faulted).

    python profiles/bf16_mixer_ab.py [--rounds 9] [--iters N] [--size NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (B, N, iters per round). The Adding network: E = 32, hidden 32, C = 8, M = log2 N steps of L = M + 1 links.
SIZES = {
    "adding_8x128": (8, 128, 200),
    "adding_64x128": (64, 128, 200),
    "adding_40x512": (40, 512, 200),
    "adding_40x1024": (40, 1024, 100),  # reported as not covered unless psf_mixer_fwd_bf16_plan takes it
    # one workgroup per sequence: what more sequences than CUs (256) do to the comparison
    "adding_512x128": (512, 128, 100),
    "adding_320x512": (320, 512, 50),
}
E, H, C = 32, 32, 8
CHILD_LIMIT_S = 240


def run_size(name, rounds, iters):
    import torch
    from torch import nn
    from sparsefactorization_amd import chord, fused_mixer, fused_mlp

    B, N, default_iters = SIZES[name]
    iters = iters or default_iters
    M = N.bit_length() - 1
    L = M + 1
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    class Block(nn.Module):
        def __init__(self, h, O):
            super().__init__()
            self.network = nn.Sequential(nn.Linear(E, h), nn.GELU(), nn.Linear(h, O))

    g = Block(H, C).to(torch.bfloat16).to(dev)
    fs = [Block(H, L).to(torch.bfloat16).to(dev) for _ in range(M)]
    x = torch.randn(B, N, E).to(torch.bfloat16).to(dev)

    def two_calls():
        ys = fused_mlp.fused_mlp_forward_bf16(x, [g, *fs])
        return chord.chord_chain(ys[1:], ys[0], True)

    def mixer():
        return fused_mixer.mixer_forward_bf16(x, g, fs, True)

    with torch.no_grad():
        if not fused_mixer.covered_bf16(x, g, fs):
            print(json.dumps({"size": name, "N": N, "covered": False}), flush=True)
            return
        assert fused_mlp.bf16_eligible(x, [g, *fs])
        a, b = two_calls(), mixer()
        torch.cuda.synchronize()
        assert a.dtype == b.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16)), "the routes differ"
        routes = {"two_calls": two_calls, "mixer": mixer}

        def graphed(fn):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = fn()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int16), a.view(torch.int16)), "a replay differs from the eager call"
            return graph.replay

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            torch.cuda.synchronize()
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3 / iters

        modes = {"eager": routes, "graph": {r: graphed(fn) for r, fn in routes.items()}}
        for mode, fns in modes.items():
            times = {r: [] for r in fns}
            for _ in range(rounds):
                for r, fn in fns.items():
                    times[r].append(timed(fn))
            med = {r: statistics.median(ts) for r, ts in times.items()}
            for r, ts in times.items():
                print(json.dumps({"size": name, "B": B, "N": N, "M": M, "L": L, "mode": mode, "route": r, "us": round(med[r], 2),
                                  "spread_us": [round(min(ts), 2), round(max(ts), 2)], "rounds": rounds, "iters": iters}), flush=True)
            print(json.dumps({"size": name, "mode": mode, "two_calls_over_mixer": round(med["two_calls"] / med["mixer"], 3),
                              "same_bits": True}), flush=True)


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
