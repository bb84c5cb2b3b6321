"""CPU: the host side of the bf16 fused backward step and of the bf16 backward chain entry (csrc/bwd_fused_bf16.h,
psf_chord.hip: pick_fused_step_bf16, psf_chord_chain_bwd_bf16, psf_describe_bwd). psf_describe_bwd names the kernel(s) a
backward step would run; the chain entry's argument checks are reached before anything is launched. No device is touched."""
import contextlib
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIAS, E_UNSUPPORTED = -1, -2, -3, -7


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


def _describe(lib, B, N, L, C, elem_bytes):
    buf = ctypes.create_string_buffer(256)
    rc = lib.psf_describe_bwd(B, N, L, C, elem_bytes, buf, 256)
    return rc, buf.value.decode()


def test_error_codes_are_the_headers():
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        header = fh.read()
    for name, value in (("PSF_E_NULL", E_NULL), ("PSF_E_SHAPE", E_SHAPE), ("PSF_E_ALIAS", E_ALIAS), ("PSF_E_UNSUPPORTED", E_UNSUPPORTED)):
        m = re.search(r"\b%s\s*=?\s*\(?(-?\d+)\)?" % name, header)
        assert m and int(m.group(1)) == value, name


def test_the_two_entries_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("psf_chord_chain_bwd_bf16", "psf_describe_bwd"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert len(lib.psf_chord_chain_bwd_bf16.argtypes) == len(lib.psf_chord_chain_bwd_f32.argtypes) == 15
    assert len(lib.psf_describe_bwd.argtypes) == 7
    assert lib.psf_version() == 2  # additive: the ABI version stays
    assert _lib.describe_bwd(2, 1024, 11, 8) == _describe(lib, 2, 1024, 11, 8, 4)[1]
    assert "bf16" in _lib.describe_bwd(2, 1024, 11, 8, elem_bytes=2)


def test_header_compiles_as_strict_c99_with_both_entries(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "use.c"
    src.write_text('#include "psf_chord.h"\n'
                   "typedef int (*chain_t)(const uint16_t*, const uint16_t* const*, const uint16_t*, const uint16_t* const*,\n"
                   "                       uint16_t* const*, uint16_t*, uint16_t* const*, int32_t, int32_t, int64_t, int64_t, int32_t,\n"
                   "                       int64_t, const int64_t*, void*);\n"
                   "typedef int (*desc_t)(int64_t, int64_t, int32_t, int64_t, int32_t, char*, int32_t);\n"
                   "chain_t a = psf_chord_chain_bwd_bf16;\ndesc_t b = psf_describe_bwd;\n"
                   "int version(void) { return PSF_ABI_VERSION; }\n")
    proc = subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        assert re.search(r"#define PSF_ABI_VERSION\s+2\b", fh.read())


@pytest.mark.parametrize("B,N,L,C,want", [
    (2, 1024, 11, 8, "chord_bwd_fused_k<bf16,L=11,TG=1,NT=256> TR=256 near=10 far=1 fronts=1"),
    (2, 256, 9, 32, "chord_bwd_fused_k<bf16,L=9,TG=4,NT=256> TR=64 near=8 far=1 fronts=1"),
    (3, 64, 7, 128, "chord_bwd_fused_k<bf16,L=7,TG=16,NT=256> TR=16 near=6 far=1 fronts=1"),
])
def test_names_the_fused_kernel_where_it_applies(lib, knobs, B, N, L, C, want):
    knobs("bwd_fused", 2)  # wherever it applies: independent of the measured gate
    rc, name = _describe(lib, B, N, L, C, 2)
    assert rc == 0, lib.psf_last_error()
    assert name == want


def test_fronts_follow_the_knob(lib, knobs):
    knobs("bwd_fused", 2)
    for fronts in (1, 2, 4):
        knobs("bwd_fronts", fronts)
        name = _describe(lib, 4, 16384, 15, 8, 2)[1]
        assert name == f"chord_bwd_fused_k<bf16,L=15,TG=1,NT=256> TR=256 near=10 far=5 fronts={fronts}", name


def test_names_the_two_window_kernels_with_the_knob_off(lib, knobs):
    knobs("bwd_fused", 0)
    for shape in ((2, 1024, 11, 8), (4, 16384, 15, 8)):
        rc, name = _describe(lib, *shape, 2)
        assert rc == 0
        L = shape[2]
        assert name == f"chord_dw_win_k<bf16,L={L},TG=1,R=1,NT=256> + chord_dv_win_k<bf16,L={L},TG=1,R=2,NT=256>", name
    rc, name = _describe(lib, 2, 256, 9, 32, 2)
    assert name == "chord_dw_win_k<bf16,L=9,TG=4,R=1,NT=256> + chord_dv_win_k<bf16,L=9,TG=4,R=2,NT=256>", name


@pytest.mark.parametrize("B,N,L,C", [
    (2, 256, 9, 8),     # N < two tiles of 256 rows
    (2, 1024, 21, 8),   # L beyond the compiled link counts
    (2, 513, 10, 8),    # N no multiple of the tile: there is no bf16 edge instance
    (2, 1024, 11, 24),  # rows of 24 channels: not 8 << k
    (2, 1024, 11, 12),  # C % 8 != 0
])
def test_two_kernel_route_where_the_fused_step_does_not_apply(lib, knobs, B, N, L, C):
    """Whatever dW and dV kernels the shape takes today (window kernels where they apply, the generic ones beyond their limits:
    N < two tiles, L > 20), never the fused one — and the same string whatever the knob says."""
    names = []
    for fused in (2, 1, 0):
        knobs("bwd_fused", fused)
        rc, name = _describe(lib, B, N, L, C, 2)
        assert rc == 0, lib.psf_last_error()
        assert "fused" not in name and re.fullmatch(r"chord_dw_(win|generic)_k<bf16,[^>]*> \+ chord_dv_(win|generic)_k<bf16,[^>]*>", name), name
        names.append(name)
    assert names[0] == names[1] == names[2]


def test_f32_and_f64_routes(lib, knobs):
    rc, name = _describe(lib, 40, 16384, 15, 8, 4)
    assert rc == 0 and name == "chord_bwd_fused_k<f32,L=15,TG=2,NT=256> TR=128 near=9 far=6 fronts=2", name
    assert _describe(lib, 32, 4097, 13, 32, 4)[1].startswith("chord_bwd_fused_edge_k<f32,L=13,TG=8,NT=256>")
    knobs("bwd_fused", 0)
    name = _describe(lib, 40, 16384, 15, 8, 4)[1]
    assert name == "chord_dw_win_k<f32,L=15,TG=2,R=1,NT=256> + chord_dv_win_k<f32,L=15,TG=2,R=1,NT=512>", name
    assert _describe(lib, 2, 2048, 12, 64, 4)[1].startswith("chord_dw_chunk_k<f32,L=12,TG=8,R=1,NT=256> + chord_dv_win_k<f32,")
    assert _describe(lib, 2, 1024, 11, 8, 8)[1] == "chord_dw_generic_k<f64,VEC=2> + chord_dv_generic_k<f64,VEC=2>"
    assert _describe(lib, 2, 1024, 11, 7, 4)[1] == "chord_dw_generic_k<f32,VEC=1> + chord_dv_generic_k<f32,VEC=1>"


def test_describe_errors(lib):
    assert _describe(lib, 2, 1024, 11, 8, 3)[0] == E_SHAPE
    assert _describe(lib, 2, 0, 11, 8, 2)[0] == E_SHAPE
    assert lib.psf_describe_bwd(2, 1024, 11, 8, 2, None, 256) == E_NULL


def _table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _chain_call(lib, M, residual, dOut=0x10000, W=None, X=None, dW=None, dX="auto", V0=0x20000, dV0=0x30000, B=2, N=1024, L=11, C=8):
    """Fake (never dereferenced) device addresses: every check below returns before a launch."""
    W = _table([0x100000 + 0x10000 * m for m in range(max(M, 1))]) if W is None else W
    X = _table([0x400000 + 0x10000 * m for m in range(max(M, 1))]) if X is None else X
    dW = _table([0x800000 + 0x10000 * m for m in range(max(M, 1))]) if dW is None else dW
    if dX == "auto":
        dX = _table([0xc00000 + 0x10000 * m for m in range(max(M, 1))])
    return lib.psf_chord_chain_bwd_bf16(dOut, W, V0, X, dW, dV0, dX, M, residual, B, N, L, C, None, None)


def test_chain_entry_validates_before_it_launches(lib, knobs):
    assert _chain_call(lib, 0, 0) == E_SHAPE                      # M = 0
    assert _chain_call(lib, 3, 0, dOut=None) == E_NULL
    assert _chain_call(lib, 3, 0, V0=None) == E_NULL
    assert _chain_call(lib, 3, 0, dV0=None) == E_NULL
    for which in ("W", "X", "dW"):                               # NULL tables
        rc = lib.psf_chord_chain_bwd_bf16(0x10000, None if which == "W" else _table([1, 2, 3]), 0x20000,
                                          None if which == "X" else _table([1, 2, 3]), None if which == "dW" else _table([1, 2, 3]),
                                          0x30000, _table([1, 2, 3]), 3, 0, 2, 1024, 11, 8, None, None)
        assert rc == E_NULL, which
    assert _chain_call(lib, 3, 0, N=0) == E_SHAPE
    assert _chain_call(lib, 3, 0, L=65) == E_SHAPE
    assert _chain_call(lib, 3, 0, dX=None) == E_UNSUPPORTED      # no gradient buffers: the caller runs the steps
    assert _chain_call(lib, 32, 1) == E_UNSUPPORTED              # 33 residual terms: beyond psf_sum_tensors_bf16
    assert _chain_call(lib, 3, 1, N=1023, C=1) == E_UNSUPPORTED  # B*N*C % 8 != 0 with the residual
    w = [0x100000, 0x110000, 0x120000]
    assert _chain_call(lib, 3, 0, W=_table(w), dW=_table([0x800000, w[1], 0x820000])) == E_ALIAS
    assert b"step 1" in lib.psf_last_error()
    assert _chain_call(lib, 3, 0, W=_table([w[0], None, w[2]])) == E_NULL
    assert _chain_call(lib, 3, 0, dX=_table([0xc00000, 0xc10000, None])) == E_NULL
    assert _chain_call(lib, 3, 1, B=0) == 0                      # an empty batch is no work
    knobs("chain_bwd_fused", 0)
    assert _chain_call(lib, 3, 0) == E_UNSUPPORTED               # knob off
    assert _chain_call(lib, 0, 0) == E_SHAPE                     # (validation still comes first)
