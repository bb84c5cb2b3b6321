"""The bf16 backward chain of a short sequence under autograd: the opt-in one launch (psf_chord_chain_bwd_lds_bf16,
``chord.bf16_chain_bwd_route = "always"``) against the per-step route it would replace ("never", the default:
psf_chord_chain_bwd_bf16, M per-step launches and one residual sum).

Metric: us per backward chain. One process per size, the two settings alternating per round on the same seeded bf16 operands
(residual on, as the synthetic models run it); a call is ``torch.autograd.grad(out, [V0, *Ws], dOut, retain_graph=True)`` on a
chord_chain forward made once, so only the backward is in the timed window: HIP events around ``iters`` calls, one warm-up call
per setting and round. This is the EAGER figure: the kernels plus the host's issue of the launches, the pointer tables and the
allocations. There is no graph-replay mode here (profiles/bf16_chain_bwd_ab.md says why); tests/test_gpu_graph_bf16_chain_bwd.py
shows that the one-launch route replays from a graph to the eager bits.
Before the timing the two settings' gradients are compared bit for bit (the contract is identical bits; a difference ends the
run). Prints one JSON line per (size, setting): median us per call over the rounds and the min - max spread, and per size the
ratio.

Sizes: the synthetic shapes, C = 8, M = log2 N steps of L = log2 N + 1 links (psf_training.py: n_W = int(log2(n_vec))), at
N = 128, 512 and 1024, each at B = 8 and B = 64.

Without --size the sizes run one after another, each in a child process of its own under a time limit; the first failure ends
the run (nothing more is started on a GPU that has faulted).

    python profiles/bf16_chain_bwd_ab.py [--rounds 7] [--iters N] [--size NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {}  # name: (B, N, M, L, C, calls per round): every timed window is 0.1 s or longer
for _n in (128, 512, 1024):
    for _b in (8, 64):
        _m = _n.bit_length() - 1
        SIZES[f"n{_n}_b{_b}"] = (_b, _n, _m, _m + 1, 8, 2000)
SETTINGS = ("never", "always")
CHILD_LIMIT_S = 150


def run_size(name, rounds, iters):
    import torch
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib, chord

    import faulthandler
    faulthandler.enable()  # a traceback on stderr if the process dies on a signal

    def note(what):  # progress on stderr: where a run that ends early had got to
        print(f"{name}: {what}", file=sys.stderr, flush=True)

    B, N, M, L, C, default_iters = SIZES[name]
    iters = iters or default_iters
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ws = [(0.4 * torch.randn(B, N, L)).to(torch.bfloat16).to(dev).requires_grad_(True) for _ in range(M)]
    v0 = torch.randn(B, N, C).to(torch.bfloat16).to(dev).requires_grad_(True)
    dout = torch.randn(B, N, C).to(torch.bfloat16).to(dev)
    assert _lib.load().psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 1
    out = sfa.chord_chain(ws, v0, True)

    def step():
        return torch.autograd.grad(out, [v0, *ws], dout, retain_graph=True)

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

    got = {}
    for setting in SETTINGS:
        chord.bf16_chain_bwd_route = setting
        got[setting] = [g.clone() for g in step()]
        torch.cuda.synchronize()
    differ = sum(int((p.view(torch.int16) != q.view(torch.int16)).sum()) for p, q in zip(got["never"], got["always"]))
    total = sum(p.numel() for p in got["never"])
    del got
    note("routes compared")
    if differ:
        print(json.dumps({"size": name, "error": f"{differ} of {total} gradient elements differ between the routes"}), flush=True)
        return 1

    times = {("eager", s): [] for s in SETTINGS}
    for _ in range(rounds):
        for setting in SETTINGS:
            chord.bf16_chain_bwd_route = setting
            times[("eager", setting)].append(eager())

    note("timed")
    chord.bf16_chain_bwd_route = "never"
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for (mode, setting), ts in times.items():
        print(json.dumps({"size": name, "B": B, "N": N, "M": M, "L": L, "C": C, "mode": mode, "bf16_chain_bwd_route": setting,
                          "us": round(med[(mode, setting)], 2), "spread_us": [round(min(ts), 2), round(max(ts), 2)], "rounds": rounds,
                          "iters": iters}), flush=True)
    print(json.dumps({"size": name, "never_over_always_eager": round(med[("eager", "never")] / med[("eager", "always")], 3),
                      "differing_gradient_elements": differ, "of": total}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--size", default=None, choices=sorted(SIZES))
    args = ap.parse_args()
    if args.size:
        return run_size(args.size, args.rounds, args.iters)
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
