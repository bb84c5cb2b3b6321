"""Attention-map queries: (a) the one-launch transposed chain against the per-step launches it replaces, and (b) the row / column
queries against the dense-map route of ChangedPSF.forward. Results: profiles/attention_queries_ab.md.

(a) psf_chord_chain_tr_f32 / _bf16 (one launch, csrc/chain_tr_lds.h) against M calls of psf_chord_spmm_bwd_* with dW = NULL —
    what a caller had before the entry. Each arm is captured in a HIP graph (one chain per graph), so the host's issue of
    the launches is outside the window: HIP events around ``iters`` replays, the two arms alternating per round on the same
    seeded operands, after their results have been compared bit for bit (a difference ends the run). Median us per chain over
    the rounds and the min - max spread. Shapes: B = 64, N = 1024, L = 12, M = 11 (Pathfinder) with R = 4 and R = 64, and
    B = 40, N = 128, L = 8, M = 7 (Adding / Temporal Order) with R = 4; bf16 with R = 8 in place of 4.
(b) attention_cols / attention_rows against the dense map as ChangedPSF.forward builds it (chord_chain on eye(N), the identity
    padded to a multiple of four columns), on the same random links: Pathfinder (N = 1024, L = 12, M = 11) with 18 columns at
    B = 8; the text task (N = 4097, L = 13, M = 12) with one row at B = 1 and B = 8. EAGER calls as a script makes them (the
    one-hot operand, the allocations and the launches are inside the window), HIP events around ``iters`` calls; peak memory is
    torch.cuda.max_memory_allocated over one call, less what was allocated before it (the links).

Each part runs in a child process of its own under a time limit; the first failure ends the run (nothing more is started on a
GPU that has faulted).

    python profiles/attention_queries_ab.py [--rounds 7] [--part a|b]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A_SHAPES = [("pathfinder_r4", 64, 1024, 12, 11, 4, 6000), ("pathfinder_r64", 64, 1024, 12, 11, 64, 2500), ("adding_r4", 40, 128, 8, 7, 4, 12000)]
# (iters: the shorter arm's timed window is 0.1 s or longer at 20 / 54 / 10 us per chain)
CHILD_LIMIT_S = 240


def part_a(rounds):
    import torch
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for dtype, suffix in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        vec = 16 // torch.empty((), dtype=dtype).element_size()
        for name, B, N, L, M, R, iters in A_SHAPES:
            R = max(R, vec)
            torch.manual_seed(0)
            Ws = [(torch.randn(B, N, L) / L ** 0.5).to(dtype).to(dev) for _ in range(M)]
            Q = torch.zeros(B, N, R, dtype=dtype, device=dev)
            Q[:, torch.arange(R) * (N // R), torch.arange(R)] = 1  # one-hot columns, as attention_rows makes them
            out, bufs = torch.empty_like(Q), [torch.empty_like(Q), torch.empty_like(Q)]
            w_tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Ws])
            assert lib.psf_chord_chain_tr_supported(N, L, R, M, Q.element_size()) == 1
            chain, step = getattr(lib, "psf_chord_chain_tr_" + suffix), getattr(lib, "psf_chord_spmm_bwd_" + suffix)

            def one_launch():
                _lib.check(chain(w_tab, Q.data_ptr(), out.data_ptr(), None, M, B, N, L, R, None, _lib.stream_ptr(dev)), "chain_tr")

            def per_step():
                y = Q
                for m in range(M - 1, -1, -1):
                    dst = bufs[m & 1]
                    _lib.check(step(y.data_ptr(), Ws[m].data_ptr(), None, None, dst.data_ptr(), B, N, L, R, N * R, None,
                                    _lib.stream_ptr(dev)), "spmm_bwd")
                    y = dst

            arms = {"one_launch": one_launch, "per_step": per_step}
            graphs = {}
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for fn in arms.values():
                    fn()  # warm-up: first launches may raise an instance's LDS limit
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
            differ = int((out.view(bits) != bufs[0].view(bits)).sum())
            if differ:
                print(json.dumps({"part": "a", "shape": name, "dtype": suffix, "error": f"{differ} of {out.numel()} elements differ"}), flush=True)
                return 1
            for arm, fn in arms.items():
                graphs[arm] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[arm]):
                    fn()

            def timed(g):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                g.replay()
                torch.cuda.synchronize()
                s.record()
                for _ in range(iters):
                    g.replay()
                e.record()
                torch.cuda.synchronize()
                return s.elapsed_time(e) * 1e3 / iters

            times = {arm: [] for arm in arms}
            for _ in range(rounds):
                for arm in arms:
                    times[arm].append(timed(graphs[arm]))
            med = {arm: statistics.median(ts) for arm, ts in times.items()}
            for arm, ts in times.items():
                print(json.dumps({"part": "a", "shape": name, "dtype": suffix, "B": B, "N": N, "L": L, "M": M, "R": R, "arm": arm,
                                  "us": round(med[arm], 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)], "rounds": rounds,
                                  "iters": iters}), flush=True)
            print(json.dumps({"part": "a", "shape": name, "dtype": suffix, "per_step_over_one_launch": round(med["per_step"] / med["one_launch"], 3),
                              "differing_elements": differ}), flush=True)
            del graphs
    return 0


def part_b(rounds):
    import torch
    import sparsefactorization_amd as sfa
    dev = torch.device("cuda:0")
    cols18 = [0, 1, 31, 32, 33, 100, 255, 256, 257, 511, 512, 640, 777, 800, 901, 1000, 1022, 1023]

    def dense(Ws, N):  # ChangedPSF.forward's map
        cp = (N + 3) // 4 * 4
        eye = torch.zeros(N, cp, dtype=Ws[0].dtype, device=dev)
        eye.diagonal().fill_(1)
        return sfa.chord_chain(Ws, eye, False)[..., :N]

    jobs = [("pathfinder_cols18", 8, 1024, 12, 11, "cols", cols18, 1600), ("text_row0", 1, 4097, 13, 12, "rows", [0], 1200),
            ("text_row0", 8, 4097, 13, 12, "rows", [0], 1200)]  # (iters: 0.1 s or longer at 68 / 99 us per query)
    for name, B, N, L, M, kind, index, iters in jobs:
        torch.manual_seed(0)
        Ws = [(torch.randn(B, N, L) / L ** 0.5).to(dev) for _ in range(M)]
        query = (lambda: sfa.attention_cols(Ws, index)) if kind == "cols" else (lambda: sfa.attention_rows(Ws, index))
        arms = {"query": query, "dense": lambda: dense(Ws, N)}
        with torch.no_grad():
            q, d = query(), dense(Ws, N)
            torch.cuda.synchronize()
            ref = d[..., index] if kind == "cols" else d[:, index, :]
            err = float((q - ref).abs().max() / ref.abs().max())
            equal = bool(torch.equal(q, ref))
            del q, d, ref
            peak = {}
            for arm, fn in arms.items():
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                r = fn()
                torch.cuda.synchronize()
                peak[arm] = torch.cuda.max_memory_allocated() - base
                del r
            times = {arm: [] for arm in arms}
            for _ in range(rounds):
                for arm, fn in arms.items():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()
                    torch.cuda.synchronize()
                    s.record()
                    for _ in range(iters):
                        fn()
                    e.record()
                    torch.cuda.synchronize()
                    times[arm].append(s.elapsed_time(e) * 1e3 / iters)
        med = {arm: statistics.median(ts) for arm, ts in times.items()}
        for arm, ts in times.items():
            print(json.dumps({"part": "b", "job": name, "B": B, "N": N, "L": L, "M": M, "kind": kind, "n_index": len(index), "arm": arm,
                              "us": round(med[arm], 1), "spread_us": [round(min(ts), 1), round(max(ts), 1)],
                              "peak_bytes": peak[arm], "rounds": rounds, "iters": iters}), flush=True)
        print(json.dumps({"part": "b", "job": name, "B": B, "dense_over_query_time": round(med["dense"] / med["query"], 2),
                          "dense_over_query_peak": round(peak["dense"] / max(peak["query"], 1), 1),
                          "query_vs_dense_rel_inf": err, "query_equals_dense_bits": equal}), flush=True)
        del Ws
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", default=None, choices=["a", "b"])
    args = ap.parse_args()
    if args.part:
        import faulthandler
        faulthandler.enable()  # a traceback on stderr if the process dies on a signal
        return {"a": part_a, "b": part_b}[args.part](args.rounds)
    for part in ("a", "b"):  # one child per part, each under its own limit; stop at the first failure
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
