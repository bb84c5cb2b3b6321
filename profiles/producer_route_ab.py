#!/usr/bin/env python3
"""Host time of the Python route layer (fused_mlp.ROUTES, fused_mixer.find) against a checkout of the parent commit:

    python profiles/producer_route_ab.py other/parent [out.md] [processes per tree]

The kernels are the parent's (csrc is unchanged: both trees load a build of the same sources, the parent's checkout a copy of
this tree's libpsf_chord.so), so what can move is the time the host needs to issue a forward or a step. Five eager workloads
that are bound by the host (profiles/bf16_mlp_ab.md): the no-grad forward of the cfg1 synthetic model
(Adding, N = 128, B = 40), of the Pathfinder LRA model at B = 16 and of the CIFAR-10 LRA model at B = 32, and the training step
of the last two. Whole processes alternate, parent and this tree; per process and workload: 50 iterations to warm up, then the
median of 200 iterations timed one by one (wall clock, the device synchronised after each).

Verdict per workload: the tree's median of per-process medians may exceed the parent's by no more than the parent's own spread
(largest minus smallest of its per-process medians).

    python profiles/producer_route_ab.py --paired other/parent [out.md] [parent|tree: whose model is built first]

is the same comparison inside ONE process, for the workloads whose per-process medians fall into two modes (the training steps:
0.9 or 1.3 ms per step, whichever tree): the parent's package is imported a second time under another name, the same seeded
model is built from each, and the two take turns, twelve rounds of 100 timed iterations each. What the process landed on is
then the same for both; printed per workload: the per-round medians and the median of the paired differences."""
import importlib
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

WORKLOADS = ("cfg1 forward", "pathfinder forward B=16", "cifar10 forward B=32", "pathfinder step B=16", "cifar10 step B=32")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import torch
    import sparsefactorization_amd
    from sparsefactorization_amd import lra_training, psf_training
    from sparsefactorization_amd.train import make_adam
    assert os.path.abspath(sparsefactorization_amd.__file__).startswith(os.path.abspath(tree) + os.sep)
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(200):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e6

    out = {}
    torch.manual_seed(42)
    net = psf_training.build_model("adding", 128).to(dev).eval()
    X, _ = psf_training.make_split("adding", 40, 128, dev, 1000)
    with torch.no_grad():
        out[WORKLOADS[0]] = timed(lambda: net(X))
    for task, batch, fwd, step in (("pathfinder", 16, WORKLOADS[1], WORKLOADS[3]), ("cifar10", 32, WORKLOADS[2], WORKLOADS[4])):
        cfg = lra_training.config[task]
        torch.manual_seed(42)
        net = lra_training.build_model(task).to(dev)
        X, Y = lra_training.synthetic_split(task, batch, dev, 1)
        if cfg["model"]["pooling_type"] == "CLS":
            X = lra_training.add_cls_token(X, cfg["model"]["vocab_size"])
        net.eval()
        with torch.no_grad():
            out[fwd] = timed(lambda: net(X))
        net.train()
        opt = make_adam(net.parameters(), cfg["training"]["learning_rate"])
        loss = torch.nn.CrossEntropyLoss()

        def one():
            opt.zero_grad(set_to_none=True)
            loss(net(X).squeeze(), Y).backward()
            opt.step()
        out[step] = timed(one)
    print("RESULT " + json.dumps(out), flush=True)


def paired(parent, path, first="parent", rounds=12):
    import torch

    def load_as(name, tree):
        pkg = os.path.join(tree, "sparsefactorization_amd")
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        sys.modules[name] = mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return name
    names = {"parent": load_as("sfa_parent", parent), "tree": load_as("sfa_tree", HERE)}
    names = {arm: names[arm] for arm in sorted(names, key=lambda a: a != first)}  # whose model is built first
    dev = torch.device("cuda:0")
    lines = ["", f"# The same in one process (`--paired`), the {first}'s model built first", "",
             f"Both packages in one process, the same seeded model from each, {rounds} rounds in alternating order; per round and tree the",
             "median of 100 iterations (50 to warm up before the first round). us per iteration.", ""]
    for task, batch in (("pathfinder", 16), ("cifar10", 32)):
        arms = {}
        for arm, name in names.items():
            lt, tr = importlib.import_module(name + ".lra_training"), importlib.import_module(name + ".train")
            cfg = lt.config[task]
            torch.manual_seed(42)
            net = lt.build_model(task).to(dev)
            assert type(net).__module__.startswith(name)
            X, Y = lt.synthetic_split(task, batch, dev, 1)
            arms[arm] = (net, tr.make_adam(net.parameters(), cfg["training"]["learning_rate"]), X, Y)
        loss = torch.nn.CrossEntropyLoss()

        def forward(net, opt, X, Y):
            with torch.no_grad():
                net(X)

        def step(net, opt, X, Y):
            opt.zero_grad(set_to_none=True)
            loss(net(X).squeeze(), Y).backward()
            opt.step()
        for what, fn in (("forward", forward), ("step", step)):
            for net, *_ in arms.values():
                net.train(what == "step")
            med = {arm: [] for arm in arms}
            for rd in range(-1, rounds):  # (round -1 warms up)
                for arm in (("parent", "tree") if rd % 2 == 0 else ("tree", "parent")):
                    ts = []
                    for _ in range(50 if rd < 0 else 100):
                        t0 = time.perf_counter()
                        fn(*arms[arm])
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                    if rd >= 0:
                        med[arm].append(statistics.median(ts) * 1e6)
            diff = [t - p for p, t in zip(med["parent"], med["tree"])]
            lines += [f"## {task} {what} B={batch}", ""] + [f"* {arm}: {' '.join(f'{v:.1f}' for v in med[arm])} — median "
                                                          f"{statistics.median(med[arm]):.1f}" for arm in arms]
            lines += [f"* tree - parent per round: {' '.join(f'{v:+.1f}' for v in diff)} — median {statistics.median(diff):+.1f}", ""]
    with open(path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main(parent, path, n):
    trees = {"parent": parent, "tree": HERE}
    got = {name: [] for name in trees}
    for i in range(n):
        for name in (("parent", "tree") if i % 2 == 0 else ("tree", "parent")):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", trees[name]], capture_output=True, text=True,
                                 timeout=300, cwd=trees[name])
            if run.returncode != 0:  # nothing more is started on the device after a failure
                sys.exit(f"{name} process {i} ended with {run.returncode}:\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
            got[name].append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            print(name, i, got[name][-1], flush=True)
    lines = ["# Host time of the producer route table against its parent", "",
             f"`profiles/producer_route_ab.py`: {n} processes per tree, alternating; per process the median of 200 iterations after 50",
             "to warm up, each timed on the wall clock with the device synchronised after it. us per iteration.", ""]
    worst = True
    for w in WORKLOADS:
        p, t = [g[w] for g in got["parent"]], [g[w] for g in got["tree"]]
        mp, mt, sp, st = statistics.median(p), statistics.median(t), max(p) - min(p), max(t) - min(t)
        ok = mt - mp <= sp
        worst = worst and ok
        lines += [f"## {w}", "", "| | per-process medians | median of medians | spread (max - min) | smallest |", "|---|---|---|---|---|",
                  f"| parent | {' '.join(f'{v:.1f}' for v in p)} | {mp:.1f} | {sp:.1f} | {min(p):.1f} |",
                  f"| tree | {' '.join(f'{v:.1f}' for v in t)} | {mt:.1f} | {st:.1f} | {min(t):.1f} |", "",
                  f"tree - parent = {mt - mp:+.1f} us against the parent's spread of {sp:.1f} us: "
                  + ("no difference." if ok else "SLOWER than the parent's own noise allows."), ""]
    lines += ["## Verdict", "", "No workload is slower than the parent by more than the parent's own run-to-run spread." if worst
              else "At least one workload is slower than the parent's spread allows (see above)."]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if worst else 1


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    elif sys.argv[1] == "--paired":
        paired(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "profiles", "producer_route_ab.md"),
               sys.argv[4] if len(sys.argv) > 4 else "parent")
    else:
        sys.exit(main(os.path.abspath(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "producer_route_ab.md"),
                      int(sys.argv[3]) if len(sys.argv) > 3 else 5))
