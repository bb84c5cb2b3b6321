"""CPU: the host side of the bf16 FLATTEN head — nothing here launches a kernel.

  a. psf_flat_head_bf16 and psf_flat_head_bwd_bf16 are exported and bound like their f32 neighbours (the f32 workspace position as a
     DeviceAddr), and refuse NULL, shape and alignment errors with the f32 entries' codes before any HIP call. Every pointer here
     is fake: a call that got past its checks would launch on it, so only refused calls are made.
  b. psfnet.bf16_head_route defaults to "never"; another value than "never" / "always" raises ValueError at the head.
"""
import ctypes

import pytest
import torch
from torch import nn

NEW_ENTRIES = ("psf_flat_head_bf16", "psf_flat_head_bwd_bf16")
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_the_two_entries_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), f"libpsf_chord.so does not export {name}"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    for a, b in (("psf_flat_head_bf16", "psf_flat_head_f32"), ("psf_flat_head_bwd_bf16", "psf_flat_head_bwd_f32")):
        assert len(_lib.SIGNATURES[a][0]) == len(_lib.SIGNATURES[b][0]) and _lib.SIGNATURES[a][1] is ctypes.c_int
    # the f32 workspace of a _bf16 entry is no bf16 tensor: bound as DeviceAddr, so that tests/ptr_audit.py does not read it as one
    assert [i for i, t in enumerate(_lib.SIGNATURES["psf_flat_head_bf16"][0]) if t is _lib.DeviceAddr] == [7]
    assert not any(t is _lib.DeviceAddr for t in _lib.SIGNATURES["psf_flat_head_bwd_bf16"][0])


def test_ptr_audit_reads_the_bf16_positions_and_skips_the_workspace():
    import ptr_audit
    from sparsefactorization_amd import _lib
    fwd = [ptr_audit.wanted("psf_flat_head_bf16", i, _lib.SIGNATURES) for i in range(10)]
    assert fwd[:4] == [(torch.bfloat16,)] * 4 and fwd[7] == () and fwd[9] == ()
    bwd = [ptr_audit.wanted("psf_flat_head_bwd_bf16", i, _lib.SIGNATURES) for i in range(9)]
    assert bwd[:5] == [(torch.bfloat16,)] * 5 and bwd[8] == ()


@pytest.mark.parametrize("entry", ["psf_flat_head_bf16", "psf_flat_head_f32"])
def test_forward_entry_validates_before_touching_the_gpu(lib, entry):
    """The bf16 entry and, with the same arguments, its f32 neighbour: the same codes (alignment: 8 bytes against 16)."""
    vp = ctypes.c_void_p
    one, two, three, four = vp(16), vp(32), vp(48), vp(64)
    f = getattr(lib, entry)   # (X, W, bias, out, B, K, J, workspace, workspace_bytes, stream)
    B, K, J = 8, 4096, 4
    need = lib.psf_flat_head_workspace(B, K, J)
    assert need == (K // 1024) * B * J * 4
    for hole in (0, 1, 3, 7):
        args = [one, two, None, three, B, K, J, four, need, None]
        args[hole] = None
        assert f(*args) == E_NULL, hole
    assert entry[:-4].encode() in lib.psf_last_error()
    assert f(one, two, None, three, B, 6, J, four, 1 << 30, None) == E_SHAPE          # K = 6
    assert f(one, two, None, three, B, 0, J, four, 1 << 30, None) == E_SHAPE
    assert f(one, two, None, three, B, K, 9, four, 1 << 30, None) == E_SHAPE          # forward J = 9
    assert f(one, two, None, three, B, K, 0, four, 1 << 30, None) == E_SHAPE
    assert f(one, two, None, three, 0, K, J, four, 1 << 30, None) == E_SHAPE
    assert f(one, two, None, three, B, K, J, four, need - 4, None) == E_SHAPE and b"workspace" in lib.psf_last_error()
    assert f(vp(12), two, None, three, B, K, J, four, need, None) == E_ALIGN           # a pointer at address 12
    assert f(one, vp(12), None, three, B, K, J, four, need, None) == E_ALIGN
    if entry.endswith("_bf16"):
        assert b"8-byte" in lib.psf_last_error()
        assert f(one, vp(20), None, three, B, K, J, four, need, None) == E_ALIGN       # 4-byte aligned only
        assert f(vp(18), two, None, three, B, K, J, four, need, None) == E_ALIGN       # one element off
    else:
        assert f(one, vp(24), None, three, B, K, J, four, need, None) == E_ALIGN       # f32: 8 bytes are not enough


@pytest.mark.parametrize("entry", ["psf_flat_head_bwd_bf16", "psf_flat_head_bwd_f32"])
def test_backward_entry_validates_before_touching_the_gpu(lib, entry):
    vp = ctypes.c_void_p
    dy, x, w, dx, dw = vp(16), vp(32), vp(48), vp(64), vp(80)
    g = getattr(lib, entry)   # (dY, X, W, dX, dW, B, K, J, stream)
    B, K, J = 8, 4096, 4
    assert g(None, x, w, dx, dw, B, K, J, None) == E_NULL
    assert g(dy, x, w, None, None, B, K, J, None) == E_NULL                            # nothing wanted
    assert g(dy, None, w, None, dw, B, K, J, None) == E_NULL                           # dW wanted without X
    assert g(dy, x, None, dx, None, B, K, J, None) == E_NULL and b"dX needs W" in lib.psf_last_error()   # dX wanted without W
    assert g(dy, x, w, dx, dw, B, 6, J, None) == E_SHAPE                               # K = 6
    assert g(dy, x, w, dx, dw, B, 0, J, None) == E_SHAPE
    assert g(dy, x, w, dx, dw, B, K, 17, None) == E_SHAPE                              # backward J = 17
    assert g(dy, x, w, dx, dw, B, K, 0, None) == E_SHAPE
    assert g(dy, x, w, dx, dw, 1025, K, J, None) == E_SHAPE                            # B = 1025
    assert g(dy, x, w, dx, dw, 0, K, J, None) == E_SHAPE
    assert entry[:-4].encode() in lib.psf_last_error()
    for hole in range(1, 5):                                                           # X, W, dX, dW at address 12
        args = [dy, x, w, dx, dw, B, K, J, None]
        args[hole] = vp(12)
        assert g(*args) == E_ALIGN, hole
    # an operand that is not read is not judged: dW only looks at X and dW, dX only at W and dX
    assert g(dy, x, vp(12), None, dw, B, 6, J, None) == E_SHAPE
    if entry.endswith("_bf16"):
        assert g(dy, x, w, dx, vp(20), B, K, J, None) == E_ALIGN and b"8-byte" in lib.psf_last_error()
    else:
        assert g(dy, x, w, dx, vp(88), B, K, J, None) == E_ALIGN


def test_route_default_and_validation(monkeypatch):
    from sparsefactorization_amd import psfnet
    assert psfnet.bf16_head_route == "never"
    final, flat = nn.Linear(8, 2), torch.zeros(3, 8)
    assert torch.equal(psfnet._flat_head(final, flat), final(flat))
    monkeypatch.setattr(psfnet, "bf16_head_route", "always")
    assert torch.equal(psfnet._flat_head(final, flat), final(flat))                    # f32 on the CPU: the stock module
    assert torch.equal(psfnet._flat_head(final.bfloat16(), flat.bfloat16()), final(flat.bfloat16()))   # bf16 on the CPU too
    for bad in ("sometimes", "Always", "", None, True):
        monkeypatch.setattr(psfnet, "bf16_head_route", bad)
        with pytest.raises(ValueError, match="bf16_head_route"):
            psfnet._flat_head(final, flat)


def test_bf16_flag_of_the_driver_refuses_the_adding_problem():
    from sparsefactorization_amd import psf_training
    with pytest.raises(SystemExit, match="--bf16 needs --problem order"):
        psf_training.main(["--problem", "adding", "--bf16"])
