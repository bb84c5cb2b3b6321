"""``token_linear.bf16_linear_route`` (psf_linear_wgrad_bf16, psf_affine_rows_bf16) against the parent's path: three A/Bs.

    kernel       the raw entry psf_linear_wgrad_bf16 (both launches; outputs and workspace allocated once) against the stock bf16
                 weight-gradient formulas ``dy.t() @ x`` and ``dy.sum(0)`` (the library GEMM), with psf_linear_wgrad_strided_f32 on
                 the widened operands for scale: T = 40 * 16384 with (m, n) = (2, 32), (32, 32), (32, 8), (128, 128) and
                 T = 40 * 2048 with (64, 64). Also prints the algorithmic bytes 2 T (m + n), the call's TB/s and its share of the
                 8 TB/s peak, and both results' largest error against a float64 product at the timed size.
    step_order   one bf16 Temporal-Order training step (zero_grad, forward, loss, backward, master-weight Adam), B = 40, at
    step_adding  N = 16384 and N = 1024, eager and captured by train.GraphedStep, with the switch at "never" and at "always";
                 the same for the Adding model fed bf16 inputs, its squared error taken in f32 (at "never" its init_linear is
                 the stock nn.Linear). token_linear.bf16_route and psfnet.bf16_head_route are "always" in both arms.

The arms alternate per round in one process. HIP events around ``iters`` calls (50 kernel calls, 10 steps) after five warm-up
calls of every arm; one JSON line per case: the median over the rounds and the min - max spread per arm, then the ratio. Without
--part the parts run one after another, each in a child process of its own under a time limit; the first failure ends the run
(nothing more is started on a GPU that has faulted).

    python profiles/bf16_linear_wgrad_ab.py [--part kernel|step_order|step_adding] > profiles/bf16_linear_wgrad_ab.log
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("kernel", "step_order", "step_adding")
KERNEL_SHAPES = ((40 * 16384, 2, 32), (40 * 16384, 32, 32), (40 * 16384, 32, 8), (40 * 16384, 128, 128), (40 * 2048, 64, 64))  # (T, m, n)
STEP_SIZES = (16384, 1024)
BATCH = 40
CHILD_LIMIT_S = 300
PEAK_TBPS = 8.0


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def ab(arms, iters, rounds):
    import torch
    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, iters))
    return {k: {"us": round(statistics.median(v), 2), "spread_us": [round(min(v), 2), round(max(v), 2)]} for k, v in res.items()}


def kernel_case(T, m, n, rounds):
    import torch
    from sparsefactorization_amd import _lib
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(T, m, device=dev, generator=g).to(bf16)
    dy = torch.randn(T, n, device=dev, generator=g).to(bf16)
    xf, dyf = x.float(), dy.float()
    s = torch.cuda.current_stream().cuda_stream
    nb = lib.psf_linear_wgrad_bf16_workspace(T, m, n)
    ws = torch.empty(nb // 4, device=dev)
    dW, db = torch.empty(n, m, device=dev, dtype=bf16), torch.empty(n, device=dev, dtype=bf16)
    nbf = lib.psf_linear_wgrad_workspace(T, m, n)
    wsf = torch.empty(nbf // 4, device=dev)
    dWf, dbf = torch.empty(n, m, device=dev), torch.empty(n, device=dev)

    def library():
        _lib.check(lib.psf_linear_wgrad_bf16(x.data_ptr(), m, dy.data_ptr(), n, T, m, n, dW.data_ptr(), db.data_ptr(), ws.data_ptr(), nb, s),
                   "psf_linear_wgrad_bf16")

    def f32_kernel():
        _lib.check(lib.psf_linear_wgrad_strided_f32(xf.data_ptr(), m, dyf.data_ptr(), n, T, m, n, dWf.data_ptr(), dbf.data_ptr(),
                                                    wsf.data_ptr(), nbf, s), "psf_linear_wgrad_strided_f32")

    def stock():
        return dy.t() @ x, dy.sum(0)

    r = ab({"stock": stock, "library": library, "f32_kernel": f32_kernel}, 50, rounds)
    library()
    sw, _ = stock()
    torch.cuda.synchronize()
    ref = dy.double().t() @ x.double()
    nbytes = 2 * T * (m + n)
    tbps = nbytes / r["library"]["us"] * 1e-6
    r.update(part="kernel", T=T, m=m, n=n, rounds=rounds, iters=50, stock_over_library=round(r["stock"]["us"] / r["library"]["us"], 2),
             algorithmic_bytes=nbytes, library_TBps=round(tbps, 3), share_of_peak=round(tbps / PEAK_TBPS, 3),
             max_abs_error_against_float64={"library": float((dW.double() - ref).abs().max()), "stock": float((sw.double() - ref).abs().max())})
    print(json.dumps(r), flush=True)


def step_case(problem, N, graphed, rounds):
    import torch
    from sparsefactorization_amd import psf_training, psfnet, token_linear as tl
    from sparsefactorization_amd.train import GraphedStep, make_adam
    dev, bf16 = torch.device("cuda:0"), torch.bfloat16
    tl.bf16_route = "always"
    psfnet.bf16_head_route = "always"
    arms = {}
    for route in ("never", "always"):
        tl.bf16_linear_route = route
        psf_training.seed_everything(42)
        net = psf_training.build_model(problem, N).to(dev).to(bf16)
        opt = make_adam(net.parameters(), 1e-3, capturable=True, master_weights=True)
        X, Y = psf_training.make_split(problem, BATCH, N, dev, 1000)
        if X.is_floating_point():
            X = X.to(bf16)
        loss = (lambda p, y: torch.nn.functional.mse_loss(p.float(), y)) if problem == "adding" else torch.nn.CrossEntropyLoss()
        if graphed:  # the capture keeps the route it was made under
            step = GraphedStep(net, opt, loss, X, Y)
            arms[route] = (lambda step=step, X=X, Y=Y: step(X, Y))
        else:
            def eager(net=net, opt=opt, loss=loss, X=X, Y=Y, route=route):
                tl.bf16_linear_route = route
                opt.zero_grad(set_to_none=True)
                out = loss(net(X).squeeze(), Y)
                out.backward()
                opt.step()
            arms[route] = eager
    r = ab(arms, 10, rounds)
    tl.bf16_linear_route = "never"
    r.update(part=f"step_{problem}", problem=problem, N=N, B=BATCH, graphed=graphed, rounds=rounds, iters=10,
             never_over_always=round(r["never"]["us"] / r["always"]["us"], 3))
    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=PARTS)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if args.part is None:
        for part in PARTS:
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--rounds", str(args.rounds)], timeout=CHILD_LIMIT_S)
            if proc.returncode != 0:
                sys.exit(f"part {part} exited {proc.returncode}: stopping")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it has no fallback")
    if args.part == "kernel":
        for T, m, n in KERNEL_SHAPES:
            kernel_case(T, m, n, args.rounds)
    else:
        problem = args.part[len("step_"):]
        for N in STEP_SIZES:
            for graphed in (False, True):
                step_case(problem, N, graphed, min(args.rounds, 5))


if __name__ == "__main__":
    main()
