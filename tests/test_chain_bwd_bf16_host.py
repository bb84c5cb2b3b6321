"""CPU: the host side of the one-launch bf16 backward chain entry (psf_chord.hip: psf_chord_chain_bwd_lds_bf16 and
psf_chord_chain_bwd_lds_bf16_supported; csrc/bwd_chain_lds_bf16_inst.hip: chain_bwd_lds_bf16_fits). The shape query needs no
device, and every argument check of the entry returns before anything is launched. No device is touched."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIAS, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -4, -7


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_error_codes_are_the_headers():
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        header = fh.read()
    for name, value in (("PSF_E_NULL", E_NULL), ("PSF_E_SHAPE", E_SHAPE), ("PSF_E_ALIAS", E_ALIAS), ("PSF_E_ALIGN", E_ALIGN),
                        ("PSF_E_UNSUPPORTED", E_UNSUPPORTED)):
        m = re.search(r"\b%s\s*=?\s*\(?(-?\d+)\)?" % name, header)
        assert m and int(m.group(1)) == value, name


def test_the_two_entries_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("psf_chord_chain_bwd_lds_bf16", "psf_chord_chain_bwd_lds_bf16_supported"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    # the per-step entry's arguments without dX_steps
    assert len(lib.psf_chord_chain_bwd_lds_bf16.argtypes) == len(lib.psf_chord_chain_bwd_bf16.argtypes) - 1 == 14
    assert len(lib.psf_chord_chain_bwd_lds_bf16_supported.argtypes) == 4
    assert lib.psf_version() == 2  # additive: the ABI version stays


def test_route_attribute_defaults_to_never():
    from sparsefactorization_amd import chord
    assert chord.bf16_chain_bwd_route == "never"


def test_header_compiles_as_strict_c99_with_both_entries(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "use.c"
    src.write_text('#include "psf_chord.h"\n'
                   "typedef int (*chain_t)(const uint16_t*, const uint16_t* const*, const uint16_t*, const uint16_t* const*,\n"
                   "                       uint16_t* const*, uint16_t*, int32_t, int32_t, int64_t, int64_t, int32_t,\n"
                   "                       int64_t, const int64_t*, void*);\n"
                   "typedef int (*query_t)(int64_t, int32_t, int64_t, int32_t);\n"
                   "chain_t a = psf_chord_chain_bwd_lds_bf16;\nquery_t b = psf_chord_chain_bwd_lds_bf16_supported;\n"
                   "int version(void) { return PSF_ABI_VERSION; }\n")
    proc = subprocess.run([cc, "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        assert re.search(r"#define PSF_ABI_VERSION\s+2\b", fh.read())


@pytest.mark.parametrize("N,L,C,M", [(1024, 20, 16, 64), (1, 2, 8, 1), (128, 8, 8, 14)])
def test_supported_shapes(lib, N, L, C, M):
    assert lib.psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 1


@pytest.mark.parametrize("N,L,C,M", [
    (1025, 11, 8, 2),   # N beyond the rows a workgroup holds
    (128, 8, 4, 2),     # C = 4: half a slot
    (128, 8, 12, 2),
    (128, 8, 24, 2),    # three slot groups
    (128, 1, 8, 2),     # L below the compiled link counts
    (128, 21, 8, 2),    # ... and above them
    (128, 8, 8, 0),
    (128, 8, 8, 65),    # M beyond kChainMaxSteps
])
def test_unsupported_shapes(lib, N, L, C, M):
    assert lib.psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == 0


def test_supported_follows_the_rule_everywhere(lib):
    import chain_bwd_bf16_cases as cb
    for N in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4096):
        for L in (1, 2, 3, 19, 20, 21):
            for C in (4, 8, 12, 16, 24, 32):
                for M in (0, 1, 64, 65):
                    assert lib.psf_chord_chain_bwd_lds_bf16_supported(N, L, C, M) == int(cb.covered(N, L, C, M)), (N, L, C, M)


def test_knob_off_answers_zero_and_unsupported(lib):
    from sparsefactorization_amd import _lib
    before = _lib.get_tuning("chain_bwd_fused")
    assert before == 1
    with _lib.tuning(chain_bwd_fused=0):
        assert lib.psf_chord_chain_bwd_lds_bf16_supported(128, 8, 8, 14) == 0
        assert _call(lib, 3) == E_UNSUPPORTED
        assert _call(lib, 0) == E_SHAPE  # (validation still comes first)
    assert _lib.get_tuning("chain_bwd_fused") == before  # put back
    assert lib.psf_chord_chain_bwd_lds_bf16_supported(128, 8, 8, 14) == 1


def _table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _call(lib, M, residual=0, dOut=0x10000, W=None, X=None, dW=None, V0=0x20000, dV0=0x30000, B=2, N=1024, L=11, C=8):
    """Fake (never dereferenced) device addresses: every check below returns before a launch."""
    W = _table([0x100000 + 0x10000 * m for m in range(max(M, 1))]) if W is None else W
    X = _table([0x400000 + 0x10000 * m for m in range(max(M, 1))]) if X is None else X
    dW = _table([0x800000 + 0x10000 * m for m in range(max(M, 1))]) if dW is None else dW
    return lib.psf_chord_chain_bwd_lds_bf16(dOut, W, V0, X, dW, dV0, M, residual, B, N, L, C, None, None)


def test_entry_validates_before_it_launches(lib):
    assert _call(lib, 0) == E_SHAPE                      # M = 0
    assert _call(lib, 3, dOut=None) == E_NULL
    assert _call(lib, 3, V0=None) == E_NULL
    assert _call(lib, 3, dV0=None) == E_NULL
    for which in ("W", "X", "dW"):                       # NULL tables
        rc = lib.psf_chord_chain_bwd_lds_bf16(0x10000, None if which == "W" else _table([1, 2, 3]), 0x20000,
                                              None if which == "X" else _table([1, 2, 3]), None if which == "dW" else _table([1, 2, 3]),
                                              0x30000, 3, 0, 2, 1024, 11, 8, None, None)
        assert rc == E_NULL, which
    assert _call(lib, 3, N=0) == E_SHAPE
    assert _call(lib, 3, L=65) == E_SHAPE
    assert _call(lib, 3, B=-1) == E_SHAPE
    # shapes the kernel does not cover: declined, never run some other way
    for kw in ({"N": 1025}, {"C": 4}, {"C": 12}, {"C": 24}, {"L": 1}, {"L": 21}, {"M": 65}):
        kw = dict(kw)
        assert _call(lib, kw.pop("M", 3), **kw) == E_UNSUPPORTED, kw
    assert _call(lib, 3, 1, B=0) == 0                    # an empty batch is no work
    # per-step pointers (B > 0, still before any launch)
    w = [0x100000, 0x110000, 0x120000]
    assert _call(lib, 3, W=_table(w), dW=_table([0x800000, w[1], 0x820000])) == E_ALIAS
    assert b"step 1" in lib.psf_last_error()
    assert _call(lib, 3, W=_table([w[0], None, w[2]])) == E_NULL
    assert _call(lib, 3, dW=_table([0x800000, 0x810000, None])) == E_NULL
    assert _call(lib, 3, X=_table([None, 0x410000, None])) == E_NULL        # X_steps[2]; X_steps[0] is ignored
    # alignment: dOut, dV0, V0 and every X_m 16 bytes; W_m and dW_m two
    assert _call(lib, 3, dOut=0x10008) == E_ALIGN
    assert _call(lib, 3, dV0=0x30002) == E_ALIGN
    assert _call(lib, 3, V0=0x20008) == E_ALIGN
    assert _call(lib, 3, X=_table([0x400008, 0x410000, 0x420008])) == E_ALIGN
    assert b"step 2" in lib.psf_last_error()                                # (X_steps[0] = 0x400008 was not looked at)
    assert _call(lib, 3, W=_table([w[0], w[1] + 1, w[2]])) == E_ALIGN
    assert _call(lib, 3, dW=_table([0x800001, 0x810000, 0x820000])) == E_ALIGN
