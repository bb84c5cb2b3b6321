"""CPU: the bf16 entry points of include/psf_chord.h — the planner names a bf16 kernel, and argument validation returns
PSF_E_* codes before any HIP call (NULL, shape, alias and alignment), as for the _f32 twins. No compute is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _describe(lib, B, N, L, C, elem_bytes):
    buf = ctypes.create_string_buffer(256)
    rc = lib.psf_describe_fwd(B, N, L, C, elem_bytes, buf, 256)
    return rc, buf.value.decode()


def test_describe_fwd_names_the_bf16_window_kernel_at_the_headline_shape(lib):
    rc, name = _describe(lib, 64, 16384, 15, 8, 2)
    assert rc == 0, lib.psf_last_error()
    # C = 8 is one 16-byte group: TG = 1, 512-row tiles (256 threads x 2 rows), 11 near links and 4 far ones
    assert name.startswith("chord_fwd_win_k<bf16,L=15,TG=1,R=2,NT=256> TR=512 near=11 far=4"), name


@pytest.mark.parametrize("C,tg", [(16, 2), (32, 4), (64, 8), (128, 16), (256, 16)])
def test_describe_fwd_bf16_channel_groups(lib, C, tg):
    rc, name = _describe(lib, 4, 4096, 12, C, 2)
    assert rc == 0, lib.psf_last_error()
    assert name.startswith(f"chord_fwd_win_k<bf16,L=12,TG={tg},R=2,NT=256>"), name


def test_describe_fwd_bf16_generic_routes(lib):
    assert _describe(lib, 2, 300, 9, 6, 2) == (0, "chord_fwd_generic_k<bf16,VEC=1>")   # C % 8 != 0
    assert _describe(lib, 2, 777, 22, 8, 2) == (0, "chord_fwd_generic_k<bf16,VEC=8>")  # L beyond the window kernels
    assert _describe(lib, 2, 100, 9, 8, 2) == (0, "chord_fwd_generic_k<bf16,VEC=8>")   # N shorter than two tiles
    assert _describe(lib, 64, 16384, 15, 8, 3)[0] == -2                                 # no 3-byte element


def test_describe_fwd_f32_unchanged(lib):
    rc, name = _describe(lib, 64, 16384, 15, 8, 4)
    assert rc == 0 and name.startswith("chord_fwd_win_k<f32,L=15,TG=2,R=2,NT=256> TR=256"), name


def test_bf16_entry_points_validate_before_touching_the_gpu(lib):
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(17)  # not 2-byte aligned
    f = lib.psf_chord_spmm_fwd_bf16
    assert f(None, one, None, two, 1, 8, 4, 8, 64, None, None) == -1         # PSF_E_NULL
    assert f(one, one, None, two, 1, 0, 4, 8, 0, None, None) == -2           # PSF_E_SHAPE (N < 1)
    assert f(one, one, None, two, 1, 8, 65, 8, 64, None, None) == -2         # PSF_E_SHAPE (L > 64)
    assert f(one, one, None, two, 1, 8, 4, 8, 7, None, None) == -2           # PSF_E_SHAPE (batch stride)
    assert f(one, two, None, two, 1, 8, 4, 8, 64, None, None) == -3          # PSF_E_ALIAS
    assert f(odd, one, None, two, 1, 8, 4, 8, 64, None, None) == -4          # PSF_E_ALIGN
    assert f(one, one, odd, two, 1, 8, 4, 8, 64, None, None) == -4           # PSF_E_ALIGN (residual)
    assert f(one, one, None, two, 0, 8, 4, 8, 64, None, None) == 0           # B = 0: nothing to do

    g = lib.psf_chord_spmm_bwd_bf16
    assert g(None, one, one, two, two, 1, 8, 4, 8, 64, None, None) == -1     # dZ NULL
    assert g(one, None, one, None, two, 1, 8, 4, 8, 64, None, None) == -1    # dV without W
    assert g(one, one, None, two, None, 1, 8, 4, 8, 64, None, None) == -1    # dW without V
    assert g(two, one, one, None, two, 1, 8, 4, 8, 64, None, None) == -3     # dV aliases dZ
    assert g(one, one, one, None, odd, 1, 8, 4, 8, 64, None, None) == -4     # misaligned dV
    assert g(one, one, one, two, two, 1, 8, 0, 8, 64, None, None) == -2      # L < 1

    tab = lambda *p: (ctypes.c_void_p * len(p))(*p)  # noqa: E731
    h = lib.psf_chord_chain_fwd_bf16
    assert h(None, one, tab(two.value), 1, 0, 1, 8, 4, 8, 64, None, None) == -1
    assert h(tab(one.value), one, tab(None), 1, 0, 1, 8, 4, 8, 64, None, None) == -1
    assert h(tab(one.value), one, tab(one.value), 1, 0, 1, 8, 4, 8, 64, None, None) == -3   # out aliases V0
    assert h(tab(one.value), one, tab(two.value), 1, 1, 2, 8, 4, 8, 0, None, None) == -2    # broadcast V0 as residual
    assert h(tab(one.value), one, tab(two.value), -1, 0, 1, 8, 4, 8, 64, None, None) == -2  # M < 0
    assert h(tab(odd.value), one, tab(two.value), 1, 0, 1, 8, 4, 8, 64, None, None) == -4   # misaligned W
    assert h(tab(one.value), one, tab(two.value), 0, 0, 1, 8, 4, 8, 64, None, None) == 0    # M = 0

    s = lib.psf_sum_tensors_bf16
    assert s(None, 1, 8, two, None) == -1
    assert s(tab(one.value), 1, 8, None, None) == -1
    assert s(tab(None), 1, 8, two, None) == -1
    assert s(tab(one.value), 0, 8, two, None) == -2          # count < 1
    assert s(tab(*([one.value] * 33)), 33, 8, two, None) == -2  # count > 32
    assert s(tab(one.value), 1, 12, two, None) == -2         # n not a multiple of 8
    assert s(tab(ctypes.c_void_p(18).value), 1, 8, two, None) == -4  # source not 16-byte aligned
    assert s(tab(one.value), 1, 8, ctypes.c_void_p(4098), None) == -4
    assert s(tab(one.value), 1, 0, two, None) == 0


def test_python_dtype_surface():
    import torch
    from sparsefactorization_amd import chord
    assert chord._suffix(torch.empty(0, dtype=torch.bfloat16)) == "_bf16"
    assert chord._suffix(torch.empty(0, dtype=torch.float32)) == "_f32"
    with pytest.raises(TypeError):
        chord._suffix(torch.empty(0, dtype=torch.float16))
    W = torch.zeros(1, 8, 4, dtype=torch.bfloat16)
    with pytest.raises(TypeError):  # mixed dtypes stay refused
        chord.spmm_forward_raw(W, torch.zeros(1, 8, 8), None, None)
