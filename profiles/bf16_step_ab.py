"""bf16 against f32 on the chord path, in one process, on the same seeded operands (the bf16 ones are the f32 ones rounded).

Alternates f32 and bf16 per round and times with HIP events: the forward step, the forward chain of M steps (every step
kept, as training runs it) and the backward step (dV + dW), at the headline shape, the Order training shape and ListOps-64.
Prints one line per (shape, leg, dtype): median us per call over the rounds, algorithmic bytes and the fraction of 8 TB/s.

    python profiles/bf16_step_ab.py [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsefactorization_amd as sfa  # noqa: E402

SHAPES = {  # name: (B, N, L, C, M)
    "headline": (64, 16384, 15, 8, 14),
    "order_train": (40, 16384, 15, 8, 14),
    "listops64": (32, 2048, 12, 64, 11),
}
HBM = 8.0e12


def step_bytes(B, N, L, C, esz, leg):
    if leg == "fwd":  # W once, V once, the residual once, out once (the ideal: every V row fetched once)
        return esz * B * N * (L + 3 * C)
    if leg == "chain":  # per step, no residual
        return esz * B * N * (L + 2 * C)
    if leg == "bwd":  # dV: dZ + W + dV; dW: dZ + V + dW
        return esz * B * N * (2 * L + 4 * C)
    raise ValueError(leg)


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, (B, N, L, C, M) in SHAPES.items():
        g = torch.Generator(device="cpu").manual_seed(0)
        W32 = [(0.3 * torch.randn(B, N, L, generator=g)).to(dev) for _ in range(M)]
        V32 = torch.randn(B, N, C, generator=g).to(dev)
        dZ32 = torch.randn(B, N, C, generator=g).to(dev)
        ops = {}
        for dt in (torch.float32, torch.bfloat16):
            Ws = [w.to(dt) for w in W32]
            V, dZ = V32.to(dt), dZ32.to(dt)
            bw = lambda Ws=Ws, V=V, dZ=dZ: sfa.chord.spmm_backward_raw(  # noqa: E731
                dZ, Ws[0], V, (B, N, L, C, N * C), None, True, True, V.shape)
            ops[dt] = {
                "fwd": lambda Ws=Ws, V=V: sfa.chord_spmm(Ws[0], V, V),
                "chain": lambda Ws=Ws, V=V: sfa.chord._chain_forward_raw(V, False, None, Ws, True),
                "bwd": bw,
            }
        times = {(leg, dt): [] for dt in ops for leg in ops[dt]}
        for _ in range(args.rounds):
            for dt in (torch.float32, torch.bfloat16):
                for leg, fn in ops[dt].items():
                    times[(leg, dt)].append(timed(fn, args.iters if leg != "chain" else max(2, args.iters // 5)))
        for (leg, dt), ts in times.items():
            esz = 4 if dt == torch.float32 else 2
            us = statistics.median(ts)
            per_step = us / M if leg == "chain" else us
            nbytes = step_bytes(B, N, L, C, esz, leg)
            print(json.dumps({"shape": name, "B": B, "N": N, "L": L, "C": C, "M": M, "leg": leg,
                              "dtype": "f32" if esz == 4 else "bf16", "us": round(us, 2), "us_per_step": round(per_step, 2),
                              "alg_bytes_per_step": nbytes, "frac_8TBs": round(nbytes / (per_step * 1e-6) / HBM, 3),
                              "spread_us": [round(min(ts), 2), round(max(ts), 2)], "kernel": sfa.describe_fwd(B, N, L, C, esz)
                              if leg != "bwd" else None}), flush=True)


if __name__ == "__main__":
    main()
