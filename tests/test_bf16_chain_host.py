"""CPU: the planner and the describe entry of the bf16 one-launch forward chain (csrc/fwd_chain_lds_bf16.h).
psf_describe_chain_fwd_dtype names the kernel a chain would run; nothing is launched."""
import contextlib
import ctypes
import os
import re

import pytest


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


@pytest.fixture
def knobs(lib):
    """Set tuning knobs for one test; restored afterwards."""
    from sparsefactorization_amd import _lib
    with contextlib.ExitStack() as stack:
        yield lambda key, value: stack.enter_context(_lib.tuning(**{key: value}))


def _describe(lib, B, N, L, C, M, elem_bytes):
    buf = ctypes.create_string_buffer(256)
    rc = lib.psf_describe_chain_fwd_dtype(B, N, L, C, M, elem_bytes, buf, 256)
    return rc, buf.value.decode()


def _describe_f32(lib, B, N, L, C, M):
    buf = ctypes.create_string_buffer(256)
    rc = lib.psf_describe_chain_fwd(B, N, L, C, M, buf, 256)
    return rc, buf.value.decode()


def test_names_the_bf16_lds_kernel_for_a_synthetic_shape(lib, knobs):
    knobs("chain_fused", 2)  # wherever it fits: independent of the measured gate
    rc, name = _describe(lib, 40, 1024, 11, 8, 10, 2)
    assert rc == 0, lib.psf_last_error()
    # C = 8 is ONE group of 8 channels: 1024 slots, two rows per thread on 512 threads, one workgroup per sequence
    assert name.startswith("chord_chain_lds_k<bf16,L=11,CC=1,R=2> one launch for all 10 steps, 512 threads, 1 workgroup(s)"), name
    # sixteen channels: two groups per workgroup
    rc, name = _describe(lib, 40, 1024, 11, 16, 10, 2)
    assert rc == 0 and name.startswith("chord_chain_lds_k<bf16,L=11,CC=2,R=2> one launch for all 10 steps, 1024 threads, 1 workgroup(s)"), name
    # three rows per thread: N = 1025 with two groups (2050 slots), up to L = 18 in bf16
    rc, name = _describe(lib, 4, 1025, 18, 16, 4, 2)
    assert rc == 0 and name.startswith("chord_chain_lds_k<bf16,L=18,CC=2,R=3>"), name


def test_names_the_bf16_rows_kernels(lib, knobs):
    knobs("chain_fused", 2)
    knobs("chain_cc", 2)  # the large instances wherever they fit
    rc, name = _describe(lib, 32, 2000, 12, 128, 11, 2)
    assert rc == 0, lib.psf_last_error()
    assert name.startswith("chord_chain_rows_k<bf16,L=12,G=2,R=2> one launch for all 11 steps, 1024 threads x 2 rows x 16 channels, "
                           "8 workgroup(s) per sequence"), name
    rc, name = _describe(lib, 2, 1500, 9, 24, 3, 2)  # an odd number of 8-channel groups
    assert rc == 0 and "chord_chain_rows_k<bf16,L=9,G=2,R=2>" in name and "2 workgroup(s) per sequence" in name, name
    rc, name = _describe(lib, 32, 4097, 14, 32, 12, 2)
    assert rc == 0, lib.psf_last_error()
    assert name.startswith("chord_chain_rows_k<bf16,L=14,G=1,R=5> one launch for all 12 steps, 832 threads x 5 rows x 8 channels, "
                           "4 workgroup(s) per sequence"), name
    rc, name = _describe(lib, 2, 4160, 20, 8, 2, 2)
    assert rc == 0 and "chord_chain_rows_k<bf16,L=20,G=1,R=5>" in name, name


@pytest.mark.parametrize("B,N,L,C,M,fused", [
    (4, 1024, 11, 12, 10, 2),   # C % 8 != 0
    (4, 4161, 11, 8, 10, 2),    # N beyond the long-row instance
    (4, 1024, 21, 8, 10, 2),    # L beyond the compiled link counts
    (4, 1024, 11, 8, 1, 2),     # a single step is a step
    (4, 1024, 11, 8, 10, 0),    # knob: never
    (4, 1025, 19, 16, 4, 2),    # three rows per thread (2050 slots) would spill at L = 19: declined
])
def test_per_step_names_where_the_one_launch_does_not_apply(lib, knobs, B, N, L, C, M, fused):
    knobs("chain_fused", fused)
    knobs("chain_cc", 2)
    rc, name = _describe(lib, B, N, L, C, M, 2)
    assert rc == 0, lib.psf_last_error()
    assert "chain" not in name and ("chord_fwd_win_k<bf16" in name or "chord_fwd_generic_k<bf16" in name), name
    buf = ctypes.create_string_buffer(256)
    assert lib.psf_describe_fwd(B, N, L, C, 2, buf, 256) == 0
    assert name == buf.value.decode()


def test_three_rows_per_thread_stop_at_eighteen_links(lib, knobs):
    knobs("chain_fused", 2)
    assert "R=3" in _describe(lib, 4, 2049, 18, 8, 4, 2)[1]
    assert "chord_chain_lds_k<bf16,L=18,CC=1,R=3>" in _describe(lib, 4, 2049, 18, 8, 4, 2)[1]
    assert "chord_chain" not in _describe(lib, 4, 2049, 19, 8, 4, 2)[1]  # (f32 stops at L = 14 there)
    assert "chord_chain_lds_k<f32,L=14,CC=1,R=3>" in _describe(lib, 4, 2049, 14, 4, 4, 4)[1]
    assert "chord_chain" not in _describe(lib, 4, 2049, 15, 4, 4, 4)[1]


F32_SHAPES = [(32, 2000, 12, 128, 11), (40, 2048, 12, 8, 11), (32, 1024, 11, 32, 10), (32, 4097, 14, 32, 12),
              (8, 4097, 14, 32, 12),  # the five of test_fused_lds_chain_large_instance_rule
              (40, 128, 8, 8, 7), (40, 1024, 11, 8, 10), (2, 1025, 11, 8, 4), (2, 2049, 12, 4, 4), (64, 16384, 15, 8, 14),
              (1, 1024, 11, 1024, 10), (3, 300, 9, 6, 5), (2, 777, 22, 8, 3)]


@pytest.mark.parametrize("cc", [0, 1, 2])
def test_elem_bytes_4_is_the_f32_entry(lib, knobs, cc):
    knobs("chain_cc", cc)
    for shape in F32_SHAPES:
        rc, name = _describe(lib, *shape, 4)
        assert (rc, name) == _describe_f32(lib, *shape) and rc == 0, (shape, name)
        assert "bf16" not in name


def test_errors(lib):
    assert _describe(lib, 4, 1024, 11, 8, 10, 3)[0] == -2   # no 3-byte element
    assert _describe(lib, 4, 1024, 11, 8, 10, 8)[0] == -2   # no f64 one-launch plan to describe
    assert lib.psf_describe_chain_fwd_dtype(4, 1024, 11, 8, 10, 2, None, 256) == -1
    assert _describe(lib, 4, 0, 11, 8, 10, 2)[0] == -2


def test_header_declares_and_lib_binds_the_entry(lib):
    from sparsefactorization_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "psf_chord.h")) as fh:
        header = fh.read()
    assert re.search(r"int psf_describe_chain_fwd_dtype\(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t elem_bytes,\s*"
                     r"char\* buf,\s*int32_t cap\);", header)
    assert re.search(r"#define PSF_ABI_VERSION\s+2\b", header)
    assert lib.psf_describe_chain_fwd_dtype.argtypes is not None and len(lib.psf_describe_chain_fwd_dtype.argtypes) == 8
    assert _lib.describe_chain_fwd(40, 1024, 11, 8, 10) == _describe_f32(lib, 40, 1024, 11, 8, 10)[1]
    assert "bf16" in _lib.describe_chain_fwd(40, 1024, 11, 8, 10, elem_bytes=2)
