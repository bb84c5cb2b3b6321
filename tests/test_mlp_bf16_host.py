"""CPU: the fused bf16 producer forward's host side — psf_mlp_fwd_bf16 / psf_mlp_fwd_bf16_workspace are exported and bound,
validate before any HIP call with psf_mlp_fwd_f32's codes (include/psf_chord.h), and fused_mlp.bf16_eligible takes only what
the kernel covers."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
i32, vp = ctypes.c_int32, ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def arr(vals):
    return (i32 * len(vals))(*vals)


def ptrs(n, v=16):
    return (vp * n)(*([v] * n))


def test_the_two_symbols_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("psf_mlp_fwd_bf16", "psf_mlp_fwd_bf16_workspace"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert len(lib.psf_mlp_fwd_bf16.argtypes) == len(lib.psf_mlp_fwd_f32.argtypes) == 14
    assert lib.psf_mlp_fwd_bf16_workspace.restype is ctypes.c_int64
    assert lib.psf_version() == 2  # additive: the ABI version stays
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        header = fh.read()
    assert re.search(r"#define PSF_ABI_VERSION\s+2\b", header)
    assert re.search(r"int psf_mlp_fwd_bf16\(const uint16_t\* X, int64_t T, int32_t E, int32_t K,", header)
    assert b"fused MLP fwd<bf16>" in lib.psf_build_info()


def test_workspace_limits(lib):
    ws = lib.psf_mlp_fwd_bf16_workspace
    h, O = arr([32, 33, 128]), arr([8, 15, 32])
    for E in (8, 32, 64):
        n = ws(E, 3, h, O)
        assert n > 0 and n % 16 == 0
    assert ws(32, 3, h, O) == (1 + 2 + 4) * 6912  # one image per 32 hidden rows
    for E in (4, 12, 68, 72):
        assert ws(E, 3, h, O) == -1
    assert ws(32, 0, h, O) == -1 and ws(32, 33, arr([32] * 33), arr([8] * 33)) == -1
    assert ws(32, 32, arr([32] * 32), arr([8] * 32)) > 0
    assert ws(32, 3, arr([32, 0, 32]), O) == -1 and ws(32, 3, arr([32, 129, 32]), O) == -1
    assert ws(32, 3, h, arr([8, 0, 8])) == -1 and ws(32, 3, h, arr([8, 33, 8])) == -1
    assert ws(32, 3, None, O) == -1 and ws(32, 3, h, None) == -1


def test_entry_validates_before_touching_the_gpu(lib):
    """The f32 twin's codes, in its order, and a psf_last_error text — no HIP call has been made at that point."""
    f = lib.psf_mlp_fwd_bf16
    one, two = vp(16), vp(32)
    h, O = arr([32, 32, 128]), arr([8, 15, 32])
    ws = lib.psf_mlp_fwd_bf16_workspace(32, 3, h, O)
    t = [ptrs(3) for _ in range(5)]

    def call(X=one, T=100, E=32, K=3, A=t[0], a=t[1], B=t[2], b=t[3], hh=h, OO=O, Y=t[4], w=two, wb=ws):
        return f(X, T, E, K, A, a, B, b, hh, OO, Y, w, wb, None)

    for kw in (dict(X=None), dict(A=None), dict(a=None), dict(B=None), dict(b=None), dict(hh=None), dict(OO=None), dict(Y=None),
               dict(w=None)):
        assert call(**kw) == E_NULL, kw
        assert b"NULL" in lib.psf_last_error()
    assert call(T=0) == E_SHAPE and b"T >= 1" in lib.psf_last_error()
    assert call(E=12) == E_SHAPE and call(E=72) == E_SHAPE and call(K=0) == E_SHAPE
    assert call(hh=arr([32, 129, 32])) == E_SHAPE and call(OO=arr([8, 33, 8])) == E_SHAPE
    assert call(X=vp(24)) == E_ALIGN and b"X must be 16-byte aligned" in lib.psf_last_error()
    assert call(wb=ws - 16) == E_SHAPE and b"workspace" in lib.psf_last_error()
    assert call(w=vp(40)) == E_SHAPE
    assert call(A=(vp * 3)(16, None, 16)) == E_NULL and b"NULL layer pointer" in lib.psf_last_error()
    assert call(Y=(vp * 3)(16, 16, None)) == E_NULL
    assert call(Y=(vp * 3)(16, 24, 16)) == E_ALIGN and b"Y[k] must be 16-byte aligned" in lib.psf_last_error()
    assert call(Y=(vp * 3)(16, 16, 30)) == E_ALIGN  # an odd-O row offset: 2-byte aligned is not enough
    assert call(B=(vp * 3)(16, 17, 16)) == E_ALIGN and b"2-byte aligned" in lib.psf_last_error()
    # the f32 twin answers the shared cases with the same codes
    g = lib.psf_mlp_fwd_f32
    ws32 = lib.psf_mlp_fwd_workspace(32, 3, h, O)
    assert g(None, 100, 32, 3, t[0], t[1], t[2], t[3], h, O, t[4], two, ws32, None) == E_NULL
    assert g(one, 0, 32, 3, t[0], t[1], t[2], t[3], h, O, t[4], two, ws32, None) == E_SHAPE
    assert g(vp(24), 100, 32, 3, t[0], t[1], t[2], t[3], h, O, t[4], two, ws32, None) == E_ALIGN
    assert g(one, 100, 32, 3, t[0], t[1], t[2], t[3], h, O, t[4], two, ws32 - 16, None) == E_SHAPE


class _Block(nn.Module):
    """MLPBlock's shape: ``network`` = Linear, GELU, Linear."""

    def __init__(self, E, h, O, bias=True, deep=False, approximate="none"):
        super().__init__()
        layers = [nn.Linear(E, h, bias=bias), nn.GELU(approximate=approximate)]
        if deep:
            layers += [nn.Linear(h, h), nn.GELU()]
        self.network = nn.Sequential(*layers, nn.Linear(h, O, bias=bias))


def test_bf16_eligible_is_false_off_the_route(lib, monkeypatch):
    from sparsefactorization_amd import fused_mlp
    blocks = [_Block(32, 32, 8).bfloat16(), _Block(32, 32, 15).bfloat16()]
    x = torch.zeros(4, 16, 32, dtype=torch.bfloat16)
    with torch.no_grad():
        assert not fused_mlp.bf16_eligible(x, blocks)  # a CPU tensor
        # everything but the device: a tensor that says it is on the GPU
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        assert fused_mlp.bf16_eligible(x, blocks)
        assert not fused_mlp.bf16_eligible(x.float(), blocks)                                   # f32 x
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 32, 8), _Block(32, 32, 15)])          # f32 parameters
        mixed = _Block(32, 32, 8).bfloat16()
        mixed.network[2].bias.data = mixed.network[2].bias.data.float()
        assert not fused_mlp.bf16_eligible(x, [mixed])                                          # one f32 parameter
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 32, 8, deep=True).bfloat16()])        # the deep form
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 32, 8, bias=False).bfloat16()])       # no biases
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 32, 8, approximate="tanh").bfloat16()])
        assert not fused_mlp.bf16_eligible(torch.zeros(4, 512, dtype=torch.bfloat16), [_Block(512, 32, 8).bfloat16()])  # E = 512
        assert not fused_mlp.bf16_eligible(torch.zeros(4, 12, dtype=torch.bfloat16), [_Block(12, 32, 8).bfloat16()])    # E % 8
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 129, 8).bfloat16()])
        assert not fused_mlp.bf16_eligible(x, [_Block(32, 32, 33).bfloat16()])
        assert not fused_mlp.bf16_eligible(x[0, 0], blocks)                                     # dim < 2
        assert not fused_mlp.bf16_eligible(x, [])
        monkeypatch.setattr(fused_mlp, "bf16_enabled", False)
        assert not fused_mlp.bf16_eligible(x, blocks)
        monkeypatch.setattr(fused_mlp, "bf16_enabled", True)
        monkeypatch.setattr(fused_mlp, "enabled", False)
        assert not fused_mlp.bf16_eligible(x, blocks)
        monkeypatch.setattr(fused_mlp, "enabled", True)
        assert fused_mlp.bf16_eligible(x, blocks)
    assert not fused_mlp.bf16_eligible(x, blocks)  # gradients enabled on trainable parameters
    for b in blocks:
        b.requires_grad_(False)
    assert fused_mlp.bf16_eligible(x, blocks)      # nothing to train: the route is taken with autograd on too
    # the f32 routes keep their meaning: none of them takes a bf16 call
    with torch.no_grad():
        assert not fused_mlp.eligible(x, blocks) and not fused_mlp.wide_ok(x, blocks)
        assert fused_mlp.stackable(x, blocks)
