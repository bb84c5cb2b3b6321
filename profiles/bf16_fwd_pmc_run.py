"""The bf16 forward step at the headline shape (B=64, N=16384, L=15, C=8, with the residual), launched `iters` times — the
program that profiles/bf16_step_ab.md's counter runs wrap (rocprofv3 --pmc ... -- python profiles/bf16_fwd_pmc_run.py).

    python profiles/bf16_fwd_pmc_run.py [B N L C iters]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sparsefactorization_amd as sfa  # noqa: E402


def main():
    B, N, L, C, iters = (int(a) for a in (sys.argv[1:6] if len(sys.argv) > 5 else (64, 16384, 15, 8, 100)))
    g = torch.Generator().manual_seed(0)
    dev = torch.device("cuda:0")
    W = (0.3 * torch.randn(B, N, L, generator=g)).to(dev, torch.bfloat16)
    V = torch.randn(B, N, C, generator=g).to(dev, torch.bfloat16)
    R = torch.randn(B, N, C, generator=g).to(dev, torch.bfloat16)
    for _ in range(iters):
        sfa.chord_spmm(W, V, R)
    torch.cuda.synchronize()
    print(sfa.describe_fwd(B, N, L, C, 2))


if __name__ == "__main__":
    main()
