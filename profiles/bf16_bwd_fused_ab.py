"""The bf16 backward step: two window kernels (knob bwd_fused = 0) against the fused step (bwd_fused = 2), in one process.

Operands as the chain's backward has them: W, V and dW are new every launch (sets spanning 2.5 x the Infinity Cache, 48 at the
most), dZ is the dV the launch before wrote (two buffers taking turns). The legs alternate per round; HIP events; one JSON line
per (shape, leg): median us per step over the rounds and the spread. Legs: the two kernels, the fused step as the automatic
rule would launch it, the fused step at each workgroups-per-CU limit (bwd_fused_wg_limit) and front count (bwd_fronts).
Then the bf16 training-chain backward (M steps, residual) through psf_chord_chain_bwd_bf16 against chord.py's per-step loop
(knob chain_bwd_fused = 0), timed on the host clock around a synchronised batch of backward passes.

    python profiles/bf16_bwd_fused_ab.py [--rounds 7] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsefactorization_amd as sfa  # noqa: E402
from sparsefactorization_amd import _lib  # noqa: E402
from sparsefactorization_amd.chord import _launch_bwd  # noqa: E402

SHAPES = {  # name: (B, N, L, C)
    "order": (40, 16384, 15, 8),
    "genome": (16, 16384, 15, 32),
    "listops128": (32, 2000, 12, 128),
    "listops64": (32, 2048, 12, 64),
    "pathfinder": (64, 1024, 11, 32),
    "imdb": (32, 4097, 14, 32),
    # the widths and lengths between those, for the gate
    "n16384_c16": (32, 16384, 15, 16),
    "n4096_c8": (64, 4096, 13, 8),
    "n1024_c8": (64, 1024, 11, 8),
    "n4096_c64": (16, 4096, 13, 64),
    "n2048_c128": (32, 2048, 12, 128),
}
CHAINS = {"order_train": (40, 16384, 15, 8, 14), "pathfinder_train": (32, 1024, 11, 32, 10), "adding_n128": (40, 128, 8, 8, 7)}
FOOTPRINT = int(2.5 * 256 * 2 ** 20)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def knobs(**kv):
    for k, v in kv.items():
        sfa.set_tuning(k, v)


def step_legs(name, B, N, L, C, rounds, dev, quick):
    g = torch.Generator(device="cpu").manual_seed(0)
    per_set = 2 * B * N * (2 * L + C)
    sets = max(2, min(48, -(-FOOTPRINT // per_set)))
    Ws = [(torch.randn(B, N, L, generator=g) / L ** 0.5).to(torch.bfloat16).to(dev) for _ in range(sets)]
    Vs = [torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev) for _ in range(sets)]
    dWs = [torch.empty_like(Ws[0]) for _ in range(sets)]
    z0 = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev)
    zz = [z0.clone(), torch.empty_like(z0)]
    it = [0]

    def step():
        s = it[0] % sets
        it[0] += 1
        _launch_bwd(zz[it[0] & 1], Ws[s], Vs[s], dWs[s], zz[1 - (it[0] & 1)], B, N, L, C, N * C, None)

    knobs(bwd_fused=2)
    fused_name = _lib.describe_bwd(B, N, L, C, elem_bytes=2)
    knobs(bwd_fused=0)
    two_name = _lib.describe_bwd(B, N, L, C, elem_bytes=2)
    legs = {"two_kernels": dict(bwd_fused=0, bwd_fused_wg_limit=0, bwd_fronts=0)}
    if "fused" in fused_name:
        legs["fused"] = dict(bwd_fused=2, bwd_fused_wg_limit=0, bwd_fronts=0)
        if not quick:
            for wg in (2, 3, 4, 5):
                legs[f"fused_wg{wg}"] = dict(bwd_fused=2, bwd_fused_wg_limit=wg, bwd_fronts=0)
            for fr in (1, 2, 4):
                legs[f"fused_fronts{fr}"] = dict(bwd_fused=2, bwd_fused_wg_limit=0, bwd_fronts=fr)
    iters = max(100, 4 * sets)
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for leg, kv in legs.items():
            knobs(**kv)
            zz[0].copy_(z0)  # every leg starts its dZ chain from the same rows
            times[leg].append(timed(step, iters))
    knobs(bwd_fused=1, bwd_fused_wg_limit=0, bwd_fronts=0)
    for leg, ts in times.items():
        print(json.dumps({"shape": name, "B": B, "N": N, "L": L, "C": C, "leg": leg, "us_per_step": round(statistics.median(ts), 2),
                          "spread_us": [round(min(ts), 2), round(max(ts), 2)], "operand_sets": sets,
                          "kernel": two_name if leg == "two_kernels" else fused_name,
                          "automatic_route": _lib.describe_bwd(B, N, L, C, elem_bytes=2)}), flush=True)


def chain_legs(name, B, N, L, C, M, rounds, dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    Ws = [(torch.randn(B, N, L, generator=g) / L ** 0.5).to(torch.bfloat16).to(dev).requires_grad_(True) for _ in range(M)]
    V0 = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev).requires_grad_(True)
    dOut = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(dev)
    out = sfa.chord_chain(Ws, V0, True)

    def bwd():
        torch.autograd.grad(out, [V0, *Ws], dOut, retain_graph=True)

    def wall(iters):
        for _ in range(3):
            bwd()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            bwd()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / iters

    times = {"python_loop": [], "library_entry": []}
    for _ in range(rounds):
        for leg, knob in (("python_loop", 0), ("library_entry", 1)):
            knobs(chain_bwd_fused=knob)
            times[leg].append(wall(20))
    knobs(chain_bwd_fused=1)
    for leg, ts in times.items():
        print(json.dumps({"chain": name, "B": B, "N": N, "L": L, "C": C, "M": M, "residual": True, "leg": leg,
                          "us_per_backward_chain": round(statistics.median(ts), 1), "spread_us": [round(min(ts), 1), round(max(ts), 1)],
                          "step_kernel": _lib.describe_bwd(B, N, L, C, elem_bytes=2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the two routes only: no workgroup / front sweeps")
    ap.add_argument("--shapes", default="", help="comma-separated subset of the step shapes")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"device": _lib.device_info(), "build": _lib.build_info()[-80:]}), flush=True)
    for name, (B, N, L, C) in SHAPES.items():
        if args.shapes and name not in args.shapes.split(","):
            continue
        step_legs(name, B, N, L, C, args.rounds, dev, args.quick)
        torch.cuda.empty_cache()
    for name, (B, N, L, C, M) in CHAINS.items():
        chain_legs(name, B, N, L, C, M, args.rounds, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
