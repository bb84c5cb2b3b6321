"""Where the one-launch last-result chain wins: psf_chord_chain_fwd_f32 (per-step launches, two buffers) against
psf_chord_chain_last_f32 (csrc/fwd_chain_regs.h) through the raw entries, N = 16384, L = 15, M = 14, residual on, over grids
of 32 to 1024 workgroups (B * C / 2): below one round of one workgroup per CU, around it, just above it and at whole
multiples, at C = 8, 4 and 12. HIP events, 30 chains per figure, three alternating rounds, equal bits. Each line also carries
what psf_chord_chain_last_supported answers for the grid under the default knobs, so the rule of
csrc/fwd_chain_regs_launch.h can be read against the measurement: profiles/chain_regs_ab.md.

    python profiles/chain_regs_ab.py        (on the GPU; one JSON line per grid, as kept in profiles/chain_regs_ab.log)"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparsefactorization_amd import _lib  # noqa: E402

N, L, M = 16384, 15, 14
GRIDS = [(8, b) for b in (8, 16, 32, 48, 56, 60, 61, 64, 65, 72, 96, 122, 128, 129, 144, 192, 256)] + \
        [(4, b) for b in (122, 128, 130)] + [(12, b) for b in (36, 41, 42, 43, 64, 85)]
dev = torch.device("cuda:0")
lib = _lib.load()
vp = ctypes.c_void_p
print(_lib.device_info(), flush=True)
for C, B in GRIDS:
    torch.manual_seed(B)
    Ws = [0.3 * torch.randn(B, N, L, device=dev) for _ in range(M)]
    V0 = torch.randn(B, N, C, device=dev)
    bufs = [torch.empty(B, N, C, device=dev) for _ in range(2)]
    out = torch.empty(B, N, C, device=dev)
    wt = (vp * M)(*[w.data_ptr() for w in Ws])
    ot = (vp * M)(*[bufs[m % 2].data_ptr() for m in range(M)])
    s = torch.cuda.current_stream(dev).cuda_stream

    def steps():
        rc = lib.psf_chord_chain_fwd_f32(wt, V0.data_ptr(), ot, M, 1, B, N, L, C, N * C, None, s)
        assert rc == 0, rc

    def last():
        rc = lib.psf_chord_chain_last_f32(wt, V0.data_ptr(), out.data_ptr(), M, 1, B, N, L, C, N * C, None, s)
        assert rc == 0, (rc, _lib.last_error())

    def timed(fn, reps):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    row = {"C": C, "B": B, "wgs": B * C // 2, "steps_us": [], "last_us": []}
    for rnd in range(3):  # alternate
        row["steps_us"].append(round(timed(steps, 30), 1))
        row["last_us"].append(round(timed(last, 30), 1))
    steps()
    last()
    torch.cuda.synchronize()
    row["equal"] = bool(torch.equal(out, bufs[(M - 1) % 2]))
    row["ratio"] = round(statistics.median(row["steps_us"]) / statistics.median(row["last_us"]), 3)
    row["rule"] = int(lib.psf_chord_chain_last_supported(B, N, L, C, M, 16, 1, N * C, 1))
    print(json.dumps(row), flush=True)
    del Ws, V0, bufs, out
    torch.cuda.empty_cache()
