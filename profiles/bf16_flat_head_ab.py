"""The bf16 FLATTEN head (``psfnet.bf16_head_route = "always"``: psf_flat_head_bf16, psf_flat_head_bwd_bf16): three A/Bs.

    head_fwd     ``_flat_head`` on the bf16 kernels against the stock bf16 ``nn.Linear`` (the library GEMM), forward only, at
                 K = 131072 with (B, J) = (64, 1), (40, 4), (64, 4) and K = 524288 with (16, 2); as a user calls it (the workspace
                 and the output are allocated per call)
    head_fwdbwd  the same with the backward: dX, dW and db from one bf16 d(out)
    head_vs_f32  the raw entries, buffers allocated once: psf_flat_head_bf16 against psf_flat_head_f32 on the same values — what
                 8-byte loads of half the bytes cost against the f32 kernel's 16-byte loads

The arms alternate per round in one process. HIP events around ``iters`` calls after a warm-up call; ``iters`` is sized from a
short trial so that every timed window is 0.1 s or longer. Prints one JSON line per (part, size, arm): median us per call over
the rounds and the min - max spread, then the ratio. Without --part the parts run one after another, each in a child process
of its own under a time limit; the first failure ends the run (nothing more is started on a GPU that has faulted).

    python profiles/bf16_flat_head_ab.py [--rounds 7] [--part head_fwd|head_fwdbwd|head_vs_f32]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("head_fwd", "head_fwdbwd", "head_vs_f32")
SHAPES = ((64, 131072, 1), (40, 131072, 4), (64, 131072, 4), (16, 524288, 2))  # (B, K, J)
CHILD_LIMIT_S = 240
WINDOW_US = 0.2e6


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


def _iters(fn):
    """Calls per timed window: 0.2 s worth at the pace of the faster of two short trials (after a warm-up of its own), so that a
    trial that caught a slow moment still leaves the window above 0.1 s."""
    _timed(fn, 3)
    return max(10, int(WINDOW_US / max(min(_timed(fn, 20), _timed(fn, 20)), 1e-3)) + 1)


def _ab(part, size, fns, rounds, extra=None):
    arms = tuple(fns)
    iters = {a: _iters(fns[a]) for a in arms}
    times = {a: [] for a in arms}
    for _ in range(rounds):
        for a in arms:
            times[a].append(_timed(fns[a], iters[a]))
    med = {a: statistics.median(times[a]) for a in arms}
    for a in arms:
        print(json.dumps({"part": part, **size, "arm": a, "us": round(med[a], 2),
                          "spread_us": [round(min(times[a]), 2), round(max(times[a]), 2)], "rounds": rounds, "iters": iters[a],
                          "window_ms": round(med[a] * iters[a] / 1e3, 1)}), flush=True)
    base = arms[0]
    print(json.dumps({"part": part, **size, **{f"{base}_over_{a}": round(med[base] / med[a], 3) for a in arms[1:]}, **(extra or {})}),
          flush=True)


def _head_operands(B, K, J, dev):
    import torch
    torch.manual_seed(7)
    final = torch.nn.Linear(K, J).to(dev).to(torch.bfloat16)
    gen = torch.Generator().manual_seed(8)
    flat = torch.randn(B, K, generator=gen).to(torch.bfloat16).to(dev)
    dy = torch.randn(B, J, generator=gen).to(torch.bfloat16).to(dev)
    return final, flat, dy


def run_head_ab(rounds, backward):
    import torch
    from sparsefactorization_amd import psfnet
    dev = torch.device("cuda:0")
    psfnet.bf16_head_route = "always"
    part = "head_fwdbwd" if backward else "head_fwd"
    for B, K, J in SHAPES:
        final, flat, dy = _head_operands(B, K, J, dev)
        x = flat.clone().requires_grad_(backward)
        final.requires_grad_(backward)
        kept = []

        def run(head):
            if backward:
                x.grad = None
                final.zero_grad(set_to_none=True)
                head(final, x).backward(dy)
            else:
                with torch.no_grad():
                    kept[:] = [head(final, x)]

        out_lib = psfnet._flat_head(final, x)
        assert "FlatHeadBf16Fn" in type(out_lib.grad_fn).__name__ if backward else out_lib.dtype == torch.bfloat16
        ref = flat.double() @ final.weight.detach().double().t() + final.bias.detach().double()
        err = {name: float((o.detach().double() - ref).abs().max() / ref.abs().max())
               for name, o in (("library", out_lib), ("stock", final(x)))}
        _ab(part, {"B": B, "K": K, "J": J}, {"stock": lambda: run(lambda f, t: f(t)), "library": lambda: run(psfnet._flat_head)}, rounds,
            {"max_error_of_the_logits_over_max_logit_against_float64": err})


def run_head_vs_f32(rounds):
    import torch
    from sparsefactorization_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B, K, J in SHAPES:
        final, flat, _ = _head_operands(B, K, J, dev)
        w, b = final.weight.detach(), final.bias.detach()
        x32, w32, b32 = flat.float(), w.float(), b.float()
        nbytes = lib.psf_flat_head_workspace(B, K, J)
        ws = torch.empty(nbytes // 4, device=dev)
        out16, out32 = torch.empty(B, J, dtype=torch.bfloat16, device=dev), torch.empty(B, J, device=dev)

        def bf16():
            _lib.check(lib.psf_flat_head_bf16(flat.data_ptr(), w.data_ptr(), b.data_ptr(), out16.data_ptr(), B, K, J, ws.data_ptr(), nbytes,
                                              stream), "psf_flat_head_bf16")

        def f32():
            _lib.check(lib.psf_flat_head_f32(x32.data_ptr(), w32.data_ptr(), b32.data_ptr(), out32.data_ptr(), B, K, J, ws.data_ptr(), nbytes,
                                             stream), "psf_flat_head_f32")

        bf16()
        f32()
        torch.cuda.synchronize()
        same = bool(torch.equal(out16.view(torch.int16), out32.to(torch.bfloat16).view(torch.int16)))
        _ab("head_vs_f32", {"B": B, "K": K, "J": J}, {"f32": f32, "bf16": bf16}, rounds,
            {"bf16_is_the_f32_result_rounded_once": same, "bytes_read": {"f32": 4 * (B + J) * K, "bf16": 2 * (B + J) * K}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", default=None, choices=PARTS)
    args = ap.parse_args()
    if args.part:
        if args.part == "head_vs_f32":
            run_head_vs_f32(args.rounds)
        else:
            run_head_ab(args.rounds, args.part == "head_fwdbwd")
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
