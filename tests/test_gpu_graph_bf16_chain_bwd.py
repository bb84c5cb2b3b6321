"""GPU: with chord.bf16_chain_bwd_route = "always", a bf16 chain backward captured into a HIP graph replays to the eager bits
(psf_chord_chain_bwd_lds_bf16 issues one stream launch, allocates nothing and does not synchronise).

In a file of its own, sorted behind tests/test_gpu_coresidence.py, for the reason test_gpu_graph_bf16_bwd.py gives: a graph's
instantiation and replay make the HIP runtime take hardware queues for itself."""
import numpy as np
import pytest
import torch

import bf16_edges as be
import chain_bwd_bf16_cases as cb

pytestmark = pytest.mark.gpu


def _bf16_tensor(a, gpu):
    return torch.from_numpy(be.rne_bits(a).view(np.int16)).to(gpu).view(torch.bfloat16).reshape(a.shape)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def test_one_launch_chain_backward_replays_from_a_graph(gpu, monkeypatch):
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import _lib, chord
    case = cb.GRAPH
    B, N, M, L, C, res, _off = case
    Wn, V0n, dOutn = cb.operands(case)
    ws = [_bf16_tensor(w, gpu).requires_grad_(True) for w in Wn]
    v0 = _bf16_tensor(V0n, gpu).requires_grad_(True)
    dOut = _bf16_tensor(dOutn, gpu)
    lib = _lib.load()
    calls, real = [], lib.psf_chord_chain_bwd_lds_bf16

    def counted(*args):
        calls.append(real(*args))
        return calls[-1]
    monkeypatch.setattr(lib, "psf_chord_chain_bwd_lds_bf16", counted)
    never = [_bits(t) for t in torch.autograd.grad(sfa.chord_chain(ws, v0, res), [v0, *ws], dOut)]
    assert calls == []
    chord.bf16_chain_bwd_route = "always"
    try:
        side = torch.cuda.Stream(device=gpu)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = torch.autograd.grad(sfa.chord_chain(ws, v0, res), [v0, *ws], dOut)  # warm-up (allocations)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eager = [_bits(t) for t in eager]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = torch.autograd.grad(sfa.chord_chain(ws, v0, res), [v0, *ws], dOut)
    finally:
        chord.bf16_chain_bwd_route = "never"
    assert calls == [0, 0]  # the warm-up and the capture both took the one launch
    for t in captured:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b, c) in enumerate(zip(eager, captured, never)):
        assert be.same_bits(_bits(b), a) == 0, f"replayed, tensor {i}"
        assert be.same_bits(a, c) == 0, f"eager against the default route, tensor {i}"
