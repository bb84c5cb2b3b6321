"""GPU: a bf16 chain backward captured into a HIP graph replays to the eager bits (psf_chord_chain_bwd_bf16 issues only stream
launches: the M per-step kernels and the residual sum).

In a file of its own, sorted behind tests/test_gpu_coresidence.py: instantiating and replaying a graph makes the HIP runtime
take hardware queues for itself, and a co-residence test that runs afterwards can find its two fresh streams on one queue —
serialised, so it has nothing to observe. The suite's other graph tests sort behind that file too."""
import pytest
import torch

from test_gpu_bf16_bwd_fused import _autograd_chain, _chain_operands, _same_bits

pytestmark = pytest.mark.gpu


def test_chain_backward_replays_from_a_graph(gpu):
    import sparsefactorization_amd as sfa
    B, N, L, C, M = 2, 1024, 11, 8, 5
    Ws, V0, dOut = _chain_operands(gpu, B, N, L, C, M, 260)
    eager = _autograd_chain(Ws, V0, dOut, True)
    ws = [w.detach().clone().requires_grad_(True) for w in Ws]
    v0 = V0.detach().clone().requires_grad_(True)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(sfa.chord_chain(ws, v0, True), [v0, *ws], dOut)  # warm-up (allocations)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = torch.autograd.grad(sfa.chord_chain(ws, v0, True), [v0, *ws], dOut)
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager, captured)):
        _same_bits(b, a, f"replayed, tensor {i}")
