"""The bf16 forward chain: one LDS-resident launch against the per-step launches, with the f32 one launch as the yardstick.

One process, the routes alternating per round on the same seeded operands (the bf16 ones are the f32 ones rounded), HIP
events. Routes (knobs chain_fused / chain_cc):
    bf16_steps    0 / 0   M per-step launches: the bf16 chain before the one-launch kernels existed
    bf16_one_cc0  2 / 0   one launch, the planner's automatic instance
    bf16_one_cc1  2 / 1   one launch, one channel group (8 channels) per workgroup
    bf16_one_cc2  2 / 2   one launch, the large instances (chord_chain_rows_k) wherever they fit
    bf16_auto     1 / 0   what a user gets: the measured gate
    f32_one       2 / 0   the f32 one launch
A one-launch route whose kernel is the one a route before it already ran is skipped (same instance). Each shape runs with
only the last result kept (inference: two buffers take turns) and with every step kept (training).
Prints one JSON line per (shape, mode, route): median us per chain and per step over the rounds and the min - max spread.

    python profiles/bf16_chain_ab.py [--rounds 7] [--iters 20] [--shape NAME] [--mode last|keep] [--routes a,b]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsefactorization_amd as sfa  # noqa: E402
from sparsefactorization_amd import _lib  # noqa: E402

SHAPES = {  # name: (B, N, L, C, M, V0 is a broadcast eye)
    "listops_2000x128": (32, 2000, 12, 128, 11, False),
    "listops_2048x64": (32, 2048, 12, 64, 11, False),
    "pathfinder_1024x32": (64, 1024, 11, 32, 10, False),
    "text_4097x32_b32": (32, 4097, 14, 32, 12, False),
    "text_4097x32_b16": (16, 4097, 14, 32, 12, False),
    "attention_map_1024x1024": (8, 1024, 11, 1024, 10, True),
    "synthetic_128x8": (40, 128, 8, 8, 7, False),
    "synthetic_1024x8": (40, 1024, 11, 8, 10, False),
    "synthetic_2048x8": (40, 2048, 12, 8, 11, False),
}
ROUTES = {  # name: (dtype, chain_fused, chain_cc)
    "bf16_steps": (torch.bfloat16, 0, 0),
    "bf16_one_cc0": (torch.bfloat16, 2, 0),
    "bf16_one_cc1": (torch.bfloat16, 2, 1),
    "bf16_one_cc2": (torch.bfloat16, 2, 2),
    "bf16_auto": (torch.bfloat16, 1, 0),
    "f32_one": (torch.float32, 2, 0),
}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--mode", default=None, choices=["last", "keep"])
    ap.add_argument("--routes", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    wanted = args.routes.split(",") if args.routes else list(ROUTES)
    for name, (B, N, L, C, M, eye) in SHAPES.items():
        if args.shape and name != args.shape:
            continue
        g = torch.Generator(device="cpu").manual_seed(0)
        W32 = [(0.3 * torch.randn(B, N, L, generator=g)).to(dev) for _ in range(M)]
        V32 = torch.eye(N, C, device=dev) if eye else torch.randn(B, N, C, generator=g).to(dev)
        operands = {dt: ([w.to(dt) for w in W32], V32.to(dt)) for dt in (torch.float32, torch.bfloat16)}
        routes, seen = {}, set()
        for r in wanted:
            dt, cf, cc = ROUTES[r]
            sfa.set_tuning("chain_fused", cf)
            sfa.set_tuning("chain_cc", cc)
            desc = _lib.describe_chain_fwd(B, N, L, C, M, elem_bytes=2 if dt == torch.bfloat16 else 4).split(" one launch")[0]
            if r.startswith("bf16_one"):
                if "chain" not in desc or desc in seen:
                    continue  # does not fit, or the instance a route before this one already runs
                seen.add(desc)
            routes[r] = desc
        sfa.set_tuning("chain_fused", 1)
        sfa.set_tuning("chain_cc", 0)
        for mode in ("last", "keep"):
            if args.mode and mode != args.mode:
                continue
            times = {r: [] for r in routes}
            for _ in range(args.rounds):
                for r in routes:
                    dt, cf, cc = ROUTES[r]
                    Ws, V = operands[dt]
                    sfa.set_tuning("chain_fused", cf)
                    sfa.set_tuning("chain_cc", cc)
                    times[r].append(timed(lambda: sfa.chord._chain_forward_raw(V, False, None, Ws, mode == "keep"), args.iters))
            sfa.set_tuning("chain_fused", 1)
            sfa.set_tuning("chain_cc", 0)
            for r, ts in times.items():
                us = statistics.median(ts)
                print(json.dumps({"shape": name, "B": B, "N": N, "L": L, "C": C, "M": M, "mode": mode, "route": r,
                                  "us": round(us, 2), "us_per_step": round(us / M, 2),
                                  "spread_us": [round(min(ts), 2), round(max(ts), 2)],
                                  "spread_us_per_step": [round(min(ts) / M, 2), round(max(ts) / M, 2)],
                                  "kernel": routes[r] + (" (automatic route, last kept)" if r == "bf16_auto" else "")}), flush=True)


if __name__ == "__main__":
    main()
