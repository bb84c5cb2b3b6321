#!/usr/bin/env python3
"""The mixer-plan refactor against a checkout of its parent commit: the same launches, and the host time of an eager forward.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/mixer_plan_ab.py --launches TREE
    python profiles/mixer_plan_ab.py --trace OUT            # kernel, grid, workgroup, LDS bytes per launch, in launch order
    python profiles/mixer_plan_ab.py --host other/parent [processes per tree]

``--launches`` runs ONE forward of each small mixer shape (tests/test_gpu_mixer.py: two_tiles, c16_two_tiles, odd, c4, l4_e4,
pathfinder, imdb, lds_n64, lds_c4_h128; two_tiles again with mixer_lds = 0 and with fwd_split = 0; a token recipe at N = 128
evaluated in the kernel; the bf16 mixer at N = 128 and at 512 x 16) from the package in TREE, through names both commits have.
The per-step tile decision (full tiles / predicated tiles / one launch or two) is not visible through the ABI; the launch list is.

``--host``: whole processes alternate, parent and this tree (the method of profiles/producer_route_ab.py); per process and
workload 50 iterations to warm up, then the median of 300 iterations timed one by one on the wall clock with the device
synchronised after each. Workloads: the eager no-grad mixer forward (find + forward, as psfnet calls them) in f32 at BASELINE
configs[0] (N = 128, B = 40), in f32 at Pathfinder's widths (1024 x 32, hidden 128, B = 16) and in bf16 at N = 128, B = 40 with
bf16_route = "always". Verdict per workload: the tree's median of medians may exceed the parent's by no more than the parent's own
spread (largest minus smallest of its per-process medians)."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, B, N, E, h, C, L, M, residual): tests/test_gpu_mixer.py
F32 = [("two_tiles", 2, 512, 32, 32, 8, 10, 9, True), ("c16_two_tiles", 2, 256, 32, 32, 16, 9, 8, True), ("odd", 2, 600, 12, 40, 12, 9, 5, True),
       ("c4", 2, 1000, 8, 24, 4, 10, 4, False), ("l4_e4", 3, 512, 4, 8, 4, 4, 3, False), ("pathfinder", 3, 1024, 32, 128, 32, 12, 11, False),
       ("imdb", 2, 4097, 32, 128, 32, 13, 12, True), ("lds_n64", 7, 64, 32, 32, 8, 7, 6, True), ("lds_c4_h128", 3, 256, 16, 128, 4, 9, 8, True)]
HOST = ("f32 cfg1 N=128 B=40", "f32 pathfinder 1024x32 B=16", "bf16 N=128 B=40")


def _setup(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import fused_mixer
    from sparsefactorization_amd.psfnet import MLPBlock
    assert os.path.abspath(sfa.__file__).startswith(os.path.abspath(tree) + os.sep), sfa.__file__
    dev = torch.device("cuda:0")

    def blocks(E, h, C, L, M, dtype=torch.float32):
        torch.manual_seed(11)
        return MLPBlock([h, 'GELU'], E, C).to(dev, dtype), [MLPBlock([h, 'GELU'], E, L).to(dev, dtype) for _ in range(M)]
    return torch, sfa, fused_mixer, dev, blocks


def launches(tree):
    torch, sfa, fm, dev, blocks = _setup(tree)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, B, N, E, h, C, L, M, res in F32:
            g, fs = blocks(E, h, C, L, M)
            x = torch.randn(B, N, E, generator=gen).to(dev)
            fm.mixer_forward(x, g, fs, res)
            if name == "two_tiles":
                for knob in ("mixer_lds", "fwd_split"):
                    with sfa._lib.tuning(**{knob: 0}):
                        fm.mixer_forward(x, g, fs, res)
        g, fs = blocks(32, 32, 8, 8, 7)
        r = fm.Recipe.tokens(torch.randint(0, 6, (3, 128), generator=gen).to(dev), torch.randn(6, 32, generator=gen).to(dev),
                             torch.randn(128, 32, generator=gen).to(dev))
        fm.recipe_in_kernel = True
        fm.mixer_forward_in(r, g, fs, True)
        for B, N, E, C, L, M in ((3, 128, 32, 8, 8, 7), (2, 512, 32, 16, 10, 9)):
            g, fs = blocks(E, 32, C, L, M, torch.bfloat16)
            fm.mixer_forward_bf16(torch.randn(B, N, E, generator=gen).to(dev, torch.bfloat16), g, fs, True)
        torch.cuda.synchronize()
    print("LAUNCHES DONE", flush=True)


def trace(out):
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if not name.startswith("__amd_rocclr_"):  # (the runtime's own copies: the uploads of the inputs, the same program in both)
            print("{} grid=({},{},{}) wg=({},{},{}) lds={}".format(name, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                                                                   r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"],
                                                                   r["LDS_Block_Size"]))


def child(tree):
    torch, sfa, fm, dev, blocks = _setup(tree)
    fm.route = fm.bf16_route = "always"

    def timed(fn):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(300):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e6

    out = {}
    with torch.no_grad():
        for name, (B, N, E, h, C, L, M), dtype in zip(HOST, ((40, 128, 32, 32, 8, 8, 7), (16, 1024, 32, 128, 32, 12, 11), (40, 128, 32, 32, 8, 8, 7)),
                                                      (torch.float32, torch.float32, torch.bfloat16)):
            g, fs = blocks(E, h, C, L, M, dtype)
            x = torch.randn(B, N, E, device=dev).to(dtype)
            if dtype == torch.bfloat16:
                out[name] = timed(lambda: fm.mixer_forward_bf16(x, g, fs, True, fm.find_bf16(x, g, fs)))
            else:
                out[name] = timed(lambda: fm.mixer_forward_in(fm.Recipe.data(x), g, fs, True, fm.find(fm.Recipe.data(x), g, fs)))
    print("RESULT " + json.dumps(out), flush=True)


def host(parent, n):
    trees = {"parent": parent, "tree": HERE}
    got = {name: [] for name in trees}
    for i in range(n):
        for name in (("parent", "tree") if i % 2 == 0 else ("tree", "parent")):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", trees[name]], capture_output=True, text=True,
                                 timeout=120, cwd=trees[name])
            if run.returncode != 0:  # nothing more is started on the device after a failure
                sys.exit(f"{name} process {i} ended with {run.returncode}:\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
            got[name].append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(name, i, got[name][-1], flush=True)
    ok_all = True
    for w in HOST:
        p, t = [g[w] for g in got["parent"]], [g[w] for g in got["tree"]]
        mp, mt, sp = statistics.median(p), statistics.median(t), max(p) - min(p)
        ok_all = ok_all and mt - mp <= sp
        print(f"## {w}\n\n| | per-process medians (us) | median | spread |\n|---|---|---|---|\n"
              f"| parent | {' '.join(f'{v:.1f}' for v in p)} | {mp:.1f} | {sp:.1f} |\n"
              f"| tree | {' '.join(f'{v:.1f}' for v in t)} | {mt:.1f} | {max(t) - min(t):.1f} |\n\n"
              f"tree - parent = {mt - mp:+.1f} us against the parent's spread of {sp:.1f} us\n")
    return 0 if ok_all else 3  # (1: a process failed)


if __name__ == "__main__":
    if sys.argv[1] == "--launches":
        launches(sys.argv[2])
    elif sys.argv[1] == "--trace":
        trace(sys.argv[2])
    elif sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(host(os.path.abspath(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5))
