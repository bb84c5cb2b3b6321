"""GPU: psf_chord_chain_tr_f32 / _bf16 captured into a HIP graph replay to the eager bits, on the one launch and on the
per-step route (the entries allocate nothing and do not synchronise: include/psf_chord.h, "Streams").

In a file of its own, sorted behind tests/test_gpu_coresidence.py, for the reason test_gpu_graph_bf16_bwd.py gives: a graph's
instantiation and replay make the HIP runtime take hardware queues for itself."""
import ctypes

import numpy as np
import pytest
import torch

import attention_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["pathfinder", "n1025"])
def test_entry_replays_from_a_graph(gpu, name, dtype):
    from sparsefactorization_amd import _lib
    lib = _lib.load()
    bf = dtype == torch.bfloat16
    case = next(c for c in (ac.BF16_CASES if bf else ac.F32_CASES) if c[0] == name)
    Wn, Qn, _ = ac.operands(case, bf)
    Ws = [torch.from_numpy(np.array(W)).to(gpu).to(dtype) for W in Wn]
    Q = torch.from_numpy(np.array(Qn)).to(gpu).to(dtype)
    B, N, R = Q.shape
    M, L = len(Ws), Ws[0].shape[2]
    out, scratch = torch.empty_like(Q), torch.empty_like(Q)
    fn = lib.psf_chord_chain_tr_bf16 if bf else lib.psf_chord_chain_tr_f32
    w_tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Ws])

    def launch():
        rc = fn(w_tab, Q.data_ptr(), out.data_ptr(), scratch.data_ptr(), M, B, N, L, R, None, _lib.stream_ptr(gpu))
        assert rc == 0, _lib.last_error()

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()  # eager, and the warm-up: the first launch of an instance may raise its LDS limit
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.float().cpu().numpy()
    assert ac.same_bits(eager, ac.expected(case, bf)) == 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        out.fill_(float("nan"))
        scratch.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert ac.same_bits(out.float().cpu().numpy(), eager) == 0
