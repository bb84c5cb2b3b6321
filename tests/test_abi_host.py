"""CPU: the C-ABI library loads and exports every symbol of include/psf_chord.h; host-only entry points and
argument validation (everything that returns before the first HIP call); Python host logic and module surface.
No compute is launched here.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "psf_chord.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(psf_[a-z0-9_]+)\s*\(", text)))


def test_exports_every_declared_symbol(lib):
    from sparsefactorization_amd import _lib
    declared = _declared_functions()
    assert len(declared) >= 14
    for name in declared:
        assert hasattr(lib, name), f"libpsf_chord.so does not export {name}"
    assert sorted(_lib.SIGNATURES) == declared  # the ctypes table binds exactly the header
    assert lib.psf_version() == 2
    assert b"gfx950" in lib.psf_build_info()


def test_chord_indices_host_routine_matches_reference(lib):
    g = load_golden("chord_indices.npz")
    for n, l in g["full_cases"]:
        n, l = int(n), int(l)
        rows = (ctypes.c_int64 * (n * l))()
        cols = (ctypes.c_int64 * (n * l))()
        assert lib.psf_chord_indices(n, l, rows, cols) == 0
        assert np.array_equal(np.frombuffer(rows, dtype=np.int64), g[f"rows_{n}_{l}"])
        assert np.array_equal(np.frombuffer(cols, dtype=np.int64), g[f"cols_{n}_{l}"])


def test_python_helper_returns_reference_types(lib):
    import sparsefactorization_amd as sfa
    g = load_golden("psfnet_adding_n128.npz")
    rows, cols = sfa.get_chord_indices_assym(128, 8)
    assert isinstance(rows, list) and isinstance(cols, list)
    assert np.array_equal(torch.tensor((rows, cols)).numpy(), g["chord_indicies"])


def test_offsets(lib):
    from sparsefactorization_amd import _lib
    assert _lib.chord_offsets(16384, 15) == [0] + [2 ** k for k in range(14)]
    assert _lib.chord_offsets(1024, 12)[-1] == 0          # 2^10 mod 1024: duplicate self link
    assert _lib.chord_offsets(100, 9) == [0, 1, 2, 4, 8, 16, 32, 64, 28]
    assert _lib.chord_offsets(1, 4) == [0, 0, 0, 0]
    assert _lib.chord_offsets(3, 64)[63] == pow(2, 62, 3)


def test_argument_validation_returns_codes_not_crashes(lib):
    f = lib.psf_chord_spmm_fwd_f32
    one = ctypes.c_void_p(16)
    two = ctypes.c_void_p(32)
    assert f(None, one, None, two, 1, 8, 4, 4, 32, None, None) == -1          # PSF_E_NULL
    assert f(one, one, None, two, 1, 0, 4, 4, 0, None, None) == -2            # PSF_E_SHAPE (N < 1)
    assert f(one, one, None, two, 1, 8, 65, 4, 32, None, None) == -2          # L > PSF_MAX_LINKS
    assert f(one, one, None, two, 1, 8, 4, 4, 7, None, None) == -2            # bad batch stride
    assert f(one, two, None, two, 1, 8, 4, 4, 32, None, None) == -3           # PSF_E_ALIAS
    assert f(ctypes.c_void_p(18), one, None, two, 1, 8, 4, 4, 32, None, None) == -4  # PSF_E_ALIGN
    assert f(one, one, None, two, 0, 8, 4, 4, 32, None, None) == 0            # empty batch: nothing to do
    assert f(one, two, None, two, 1, 8, 4, 4, 32, None, None) == -3 and b"alias" in lib.psf_last_error()
    # producer-side entry point: validation happens before any HIP call too
    assert lib.psf_linear_wgrad_workspace(1 << 20, 32, 15) > 0
    assert lib.psf_linear_wgrad_workspace(1 << 20, 129, 15) == -1
    assert lib.psf_linear_wgrad_f32(None, one, 64, 8, 8, two, None, two, 1 << 20, None) == -1
    assert b"non-NULL" in lib.psf_last_error()
    assert lib.psf_linear_wgrad_f32(one, one, 64, 8, 300, two, None, two, 1 << 20, None) == -2
    assert lib.psf_linear_wgrad_f32(one, one, 1 << 20, 32, 32, two, None, two, 16, None) == -2
    b = lib.psf_chord_spmm_bwd_f32
    assert b(None, one, one, two, two, 1, 8, 4, 4, 32, None, None) == -1
    assert b(one, None, one, None, two, 1, 8, 4, 4, 32, None, None) == -1     # dV needs W
    assert b(one, one, one, None, one, 1, 8, 4, 4, 32, None, None) == -3      # dV aliases dZ
    c = lib.psf_chord_chain_fwd_f32
    assert c(None, one, None, 2, 0, 1, 8, 4, 4, 32, None, None) == -1
    assert c(None, None, None, 0, 0, 1, 8, 4, 4, 32, None, None) == 0          # M == 0


C99_CONSUMER = r"""
/* A consumer of include/psf_chord.h that is not Python: what a maintainer of the reference would link where
   spmul/spmul_cuda.cu:163-166 binds forward_host / backward_host with pybind11. Host-only calls: no GPU needed. */
#include <stdio.h>
#include <string.h>
#include "psf_chord.h"
#include "psf_chord_tuning.h"

#define PSF_COUNT(key, lo, hi, def) +1

int main(void) {
  int64_t off[12];
  float w[4] = {0}, v[4] = {0};
  if (psf_version() != PSF_ABI_VERSION) return 1;
  if (psf_chord_offsets(1024, 12, off) != PSF_OK) return 2;
  if (off[0] != 0 || off[1] != 1 || off[11] != 0) return 3;          /* 2^10 mod 1024: the duplicate self link */
  if (psf_chord_spmm_fwd_f32(NULL, v, NULL, w, 1, 8, 4, 4, 32, NULL, NULL) != PSF_E_NULL) return 4;
  if (strstr(psf_last_error(), "NULL") == NULL) return 5;
  if (psf_chord_spmm_fwd_f32(w, v, NULL, v, 1, 8, 4, 4, 32, NULL, NULL) != PSF_E_ALIAS) return 6;
  if (psf_chord_spmm_fwd_f32(w, v, NULL, w + 1, 1, 0, 4, 4, 0, NULL, NULL) != PSF_E_SHAPE) return 7;
  if ((0 PSF_TUNING_KNOBS(PSF_COUNT)) != 21) return 8;              /* the catalogue expands in C99 */
  if (psf_get_tuning("bwd_fused") != 1 || psf_set_tuning("no_such_knob", 0) != PSF_E_TUNING) return 9;
  printf("psf_version=%d offsets[11]=%lld\n", psf_version(), (long long)off[11]);
  return 0;
}
"""


def test_header_is_c99_and_a_plain_c_program_links_the_library(lib, tmp_path):
    """include/psf_chord.h is the boundary, and its consumer need not be Python: the header (and the knob catalogue beside it,
    psf_chord_tuning.h) compiles as strict C99
    (-std=c99 -pedantic -Wall -Werror), a C program links libpsf_chord.so and gets the ABI version, the chord offsets of
    Pathfinder's shape (N = 1024, L = 12: offset 2^10 = 0 mod N, the duplicate self link the reference keeps —
    SyntheticExperiments/psf.py:7-32) and the argument-error codes, all before any HIP call."""
    import shutil
    import subprocess
    from sparsefactorization_amd import build
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "consumer.c"
    src.write_text(C99_CONSUMER)
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(build.LIB_PATH)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", libdir, "-l:libpsf_chord.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"consumer exited {run.returncode}: {run.stdout} {run.stderr}"
    assert run.stdout.strip() == "psf_version=2 offsets[11]=0"


def test_entry_points_are_callable_from_two_threads_at_once(lib):
    """include/psf_chord.h, "Threads": host-only entry points and the validation paths of the device entry points hammered
    from two threads while a third flips a knob; every call must return what it returns single-threaded, and each thread
    keeps its own error string."""
    import threading
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)
    want = [0] + [2 ** k for k in range(14)]
    errors = []

    def offsets_worker():
        buf = (ctypes.c_int64 * 15)()
        for _ in range(3000):
            if lib.psf_chord_offsets(16384, 15, buf) != 0 or list(buf) != want:
                errors.append("offsets")
            if lib.psf_describe_fwd(64, 16384, 15, 8, 4, ctypes.create_string_buffer(128), 128) != 0:
                errors.append("describe")

    def validation_worker():
        for _ in range(3000):
            if lib.psf_chord_spmm_fwd_f32(one, two, None, two, 1, 8, 4, 4, 32, None, None) != -3:   # PSF_E_ALIAS
                errors.append("alias code")
            if b"alias" not in lib.psf_last_error():
                errors.append("alias message")
            if lib.psf_chord_chain_fwd_f32(None, None, None, 0, 0, 1, 8, 4, 4, 32, None, None) != 0:
                errors.append("empty chain")

    def knob_worker():
        for i in range(3000):
            if lib.psf_set_tuning(b"xcd_remap", i & 1) != 0:
                errors.append("set_tuning")
            if lib.psf_chord_spmm_fwd_f32(None, one, None, two, 1, 8, 4, 4, 32, None, None) != -1 or b"non-NULL" not in lib.psf_last_error():
                errors.append("null message")
        lib.psf_set_tuning(b"xcd_remap", 1)

    threads = [threading.Thread(target=f) for f in (offsets_worker, validation_worker, knob_worker)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, sorted(set(errors))


def test_mixer_entry_point_states_its_limits_without_touching_the_gpu(lib):
    """psf_mixer_fwd_workspace returns -1 outside the fused path's limits (include/psf_chord.h); psf_mixer_fwd_f32 rejects
    NULL tables, short workspaces, misaligned and aliased buffers before any HIP call."""
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    h = (i32 * 3)(32, 32, 32)
    assert lib.psf_mixer_fwd_workspace(16384, 32, 2, h, 8, 15) == 3 * 14080
    assert lib.psf_mixer_fwd_workspace(1024, 32, 2, (i32 * 3)(128, 128, 128), 32, 12) == 12 * 14080
    assert lib.psf_mixer_fwd_workspace(128, 32, 2, h, 8, 8) == 3 * 14080   # BASELINE configs[0]: the single-launch LDS kernel
    assert lib.psf_mixer_fwd_workspace(100, 32, 2, h, 8, 8) == -1      # neither: N < two tiles of 256 rows, not a multiple of 32
    assert lib.psf_mixer_fwd_workspace(256, 32, 2, h, 16, 8) == 3 * 14080  # C = 16: two 128-row tiles, per-step kernels
    assert lib.psf_mixer_fwd_workspace(128, 32, 2, h, 16, 8) == -1     # C = 16 and N < two tiles
    assert lib.psf_mixer_fwd_workspace(512, 32, 2, h, 8, 10) > 0       # exactly two tiles
    assert lib.psf_mixer_fwd_workspace(16384, 48, 2, h, 8, 15) == -1   # E > 32
    assert lib.psf_mixer_fwd_workspace(16384, 30, 2, h, 8, 15) == -1   # E not a multiple of 4
    assert lib.psf_mixer_fwd_workspace(16384, 32, 2, h, 64, 15) == -1  # C > 32
    assert lib.psf_mixer_fwd_workspace(16384, 32, 2, h, 8, 21) == -1   # L > 20
    assert lib.psf_mixer_fwd_workspace(16384, 32, 2, (i32 * 3)(32, 200, 32), 8, 15) == -1  # hidden > 128
    assert lib.psf_mixer_fwd_workspace(16384, 32, 2, None, 8, 15) == -1
    one, two, three = vp(16), vp(32), vp(48)
    tab = (vp * 3)(16, 16, 16)
    outs = (vp * 2)(32, 48)
    f = lib.psf_mixer_fwd_f32
    ws = 3 * 14080
    assert f(None, 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, one, outs, three, ws, None) == -1
    assert f(one, 1, 100, 32, 2, tab, tab, tab, tab, h, 8, 8, 1, two, outs, three, ws, None) == -2 and b"fused path" in lib.psf_last_error()
    assert f(one, 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, outs, three, ws - 16, None) == -2  # workspace too small
    assert f(vp(20), 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, outs, three, ws, None) == -4    # X misaligned
    assert f(one, 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, (vp * 2)(32, 32), three, ws, None) == -3  # out aliases V0
    assert f(one, 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, (vp * 2)(64, 64), three, ws, None) == -3  # step in == out
    assert f(one, 0, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, outs, three, ws, None) == 0        # empty batch
    # an input recipe (psf_mixer_input kinds 1, 2) is evaluated by the single-launch kernel only: on the per-step path the entry
    # says so, names the two row-writing entry points, and has launched nothing
    from sparsefactorization_amd import _lib
    rec = _lib.MixerInput(_lib.MIXER_IN_TOKENS, 6, 16, 32, None, None)
    g = lib.psf_mixer_fwd_in_f32
    assert g(ctypes.byref(rec), 1, 16384, 32, 2, tab, tab, tab, tab, h, 8, 15, 1, two, outs, three, ws, None) == -2
    assert b"psf_embed_tokens_f32" in lib.psf_last_error() and b"single-launch" in lib.psf_last_error()
    for gone in ("psf_chord_chain_fwd_far_f32", "psf_chord_spmm_bwd_far_f32", "psf_chord_bwd_far_first_link"):
        assert not hasattr(lib, gone), f"{gone} was removed in ABI version 2"


def test_producer_entry_points_validate_before_touching_the_gpu(lib):
    """psf_mlp_fwd_f32 / psf_mlp_bwd_f32 / psf_linear_wgrad_strided_f32: sizes outside the kernels' limits, NULL
    tables and short workspaces come back as PSF_E_* codes (no HIP call has been made at that point)."""
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    one, two = vp(16), vp(32)

    def arr(vals):
        return (i32 * len(vals))(*vals)

    def ptrs(n, v=16):
        return (vp * n)(*([v] * n))

    h, O = arr([32, 32, 128]), arr([8, 15, 32])
    fwd_ws = lib.psf_mlp_fwd_workspace(32, 3, h, O)
    assert fwd_ws > 0 and fwd_ws % 16 == 0
    assert lib.psf_mlp_fwd_workspace(64, 3, h, O) > 0             # E = 64: f32-MFMA variant only
    assert lib.psf_mlp_fwd_workspace(68, 3, h, O) == -1            # E > 64
    assert lib.psf_mlp_fwd_workspace(30, 3, h, O) == -1            # E not a multiple of 4
    assert lib.psf_mlp_fwd_workspace(32, 33, h, O) == -1           # K > 32
    assert lib.psf_mlp_fwd_workspace(32, 3, arr([32, 129, 32]), O) == -1   # h > 128
    assert lib.psf_mlp_fwd_workspace(32, 3, h, arr([8, 33, 8])) == -1      # out > 32
    f = lib.psf_mlp_fwd_f32
    tabs = [ptrs(3) for _ in range(5)]
    assert f(None, 100, 32, 3, tabs[0], tabs[1], tabs[2], tabs[3], h, O, tabs[4], two, fwd_ws, None) == -1
    assert f(one, 0, 32, 3, tabs[0], tabs[1], tabs[2], tabs[3], h, O, tabs[4], two, fwd_ws, None) == -2       # T < 1
    assert f(vp(20), 100, 32, 3, tabs[0], tabs[1], tabs[2], tabs[3], h, O, tabs[4], two, fwd_ws, None) == -4  # X alignment
    assert f(one, 100, 32, 3, tabs[0], tabs[1], tabs[2], tabs[3], h, O, tabs[4], two, fwd_ws - 16, None) == -2
    assert b"workspace" in lib.psf_last_error()
    assert f(one, 100, 32, 3, (vp * 3)(16, None, 16), tabs[1], tabs[2], tabs[3], h, O, tabs[4], two, fwd_ws, None) == -1

    bwd_ws = lib.psf_mlp_bwd_workspace(100000, 32, 3, h, O)
    assert bwd_ws > 0
    assert lib.psf_mlp_bwd_workspace(100000, 64, 3, h, O) == -1    # the backward covers E <= 32
    assert lib.psf_mlp_bwd_workspace(0, 32, 3, h, O) == -1
    # the partial-sum buffer grows with T: one slot per workgroup of 4 waves x 1 or 2 tiles
    assert lib.psf_mlp_bwd_workspace(10 ** 6, 32, 3, h, O) > bwd_ws
    g = lib.psf_mlp_bwd_f32
    t = [ptrs(3) for _ in range(8)]
    assert g(one, 100000, 32, 3, t[0], t[1], t[2], h, O, t[3], two, t[4], t[5], t[6], t[7], two, bwd_ws - 16, None) == -2
    assert g(one, 100000, 32, 3, t[0], t[1], t[2], h, O, None, two, t[4], t[5], t[6], t[7], two, bwd_ws, None) == -1
    assert g(one, 100000, 32, 3, t[0], t[1], t[2], h, O, (vp * 3)(16, 16, None), two, t[4], t[5], t[6], t[7], two,
             bwd_ws, None) == -1
    assert b"NULL" in lib.psf_last_error()

    assert lib.psf_embed_tokens_bwd_workspace(65536, 225, 32) > 0
    assert lib.psf_embed_tokens_bwd_workspace(65536, 513, 32) == -1     # vocabulary beyond the LDS table
    assert lib.psf_embed_tokens_bwd_f32(one, one, 65536, 225, 32, two, two, 16, None) == -2   # short workspace
    assert lib.psf_embed_tokens_bwd_f32(None, one, 65536, 225, 32, two, two, 1 << 30, None) == -1
    assert lib.psf_embed_tokens_f32(one, one, None, two, 100, 10, 6, 30, None) == -2           # E % 4 != 0
    assert lib.psf_embed_tokens_f32(one, vp(20), None, two, 100, 10, 6, 32, None) == -4        # table alignment

    s = lib.psf_linear_wgrad_strided_f32
    assert s(one, 31, one, 15, 1 << 20, 32, 15, two, None, two, 1 << 30, None) == -2   # ldx < m
    assert s(one, 480, one, 14, 1 << 20, 32, 15, two, None, two, 1 << 30, None) == -2  # ldy < n
    assert b"strides" in lib.psf_last_error()


def test_wide_producer_entry_points_validate_before_touching_the_gpu(lib):
    """psf_mlp_wide_fwd_f32 / psf_mlp_wide_bwd_f32 (csrc/mlp_wide.hip) refuse, in this order and before any HIP call: a NULL
    table (-1), a shape outside the limits (-2), X off 16 bytes or saved / workspace off 256 (-4), a saved or workspace area
    one byte short (-2), a NULL pointer of any kind in a table (-1), and — forward only — A[k] off 16 bytes (-4). Every pointer
    here is fake: a call that got past its checks would launch on them."""
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    K, T, E = 2, 100, 32

    def arr(vals):
        return (i32 * len(vals))(*vals)

    def tab(hole=None, v=64):
        return (vp * K)(*[None if k == hole else v for k in range(K)])

    h, O = arr([32, 128]), arr([8, 40])
    n_saved, n_fwd, n_bwd = (f(T, E, K, h, O) for f in (lib.psf_mlp_wide_saved_bytes, lib.psf_mlp_wide_fwd_workspace,
                                                        lib.psf_mlp_wide_bwd_workspace))
    assert min(n_saved, n_fwd, n_bwd) > 0
    X, SAVED, WS = vp(16), vp(1 << 20), vp(1 << 24)   # 16-byte and 256-byte aligned

    # ---- forward: (X, T, E, K, A, a, B, b, h, O, Y, saved, saved_bytes, workspace, workspace_bytes, stream)
    f = lib.psf_mlp_wide_fwd_f32

    def fwd(**kw):
        a = dict(X=X, T=T, E=E, K=K, A=tab(), a=tab(), B=tab(), b=tab(), h=h, O=O, Y=tab(), saved=SAVED, n_saved=n_saved, ws=WS, n_ws=n_fwd)
        a.update(kw)
        rc = f(a["X"], a["T"], a["E"], a["K"], a["A"], a["a"], a["B"], a["b"], a["h"], a["O"], a["Y"], a["saved"], a["n_saved"],
               a["ws"], a["n_ws"], None)
        assert rc != 0 and b"psf_mlp_wide_fwd" in lib.psf_last_error(), kw
        return rc

    for name in ("X", "A", "a", "B", "b", "h", "O", "Y", "ws"):                      # 1. a NULL table, before the shape ...
        assert fwd(**{name: None}) == -1, name
        assert fwd(**{name: None}, T=0) == -1, name
    for kw in (dict(T=0), dict(E=8), dict(E=1040), dict(E=520), dict(K=0), dict(K=25), dict(h=arr([0, 128])), dict(h=arr([32, 129])),
               dict(O=arr([0, 40])), dict(O=arr([8, 129]))):                          # 2. ... the shape before the alignment ...
        assert fwd(**kw) == -2, kw
        assert fwd(**kw, X=vp(20), n_ws=0) == -2, kw
    for kw in (dict(X=vp(20)), dict(X=vp(24)), dict(saved=vp((1 << 20) + 16)), dict(ws=vp((1 << 24) + 128))):
        assert fwd(**kw) == -4, kw                                                    # 3. ... the alignment before the sizes ...
        assert fwd(**kw, n_ws=0, n_saved=0) == -4, kw
    for kw in (dict(n_saved=n_saved - 1), dict(n_ws=n_fwd - 1), dict(saved=None, n_saved=0, n_ws=n_fwd),
               dict(saved=None, n_saved=0, n_ws=n_fwd + n_saved - 1)):
        assert fwd(**kw) == -2 and b"too small" in lib.psf_last_error(), kw          # 4. ... the sizes before the layers
        assert fwd(**kw, A=tab(hole=0)) == -2, kw
    for name in ("A", "a", "B", "b", "Y"):                                            # 5. a NULL pointer of every kind, any layer
        for k in range(K):
            assert fwd(**{name: tab(hole=k)}) == -1 and b"NULL layer pointer" in lib.psf_last_error(), (name, k)
    for k in range(K):                                                                # 6. the forward's A[k] off 16 bytes
        bad = (vp * K)(*[68 if j == k else 64 for j in range(K)])
        assert fwd(A=bad) == -4 and b"first-layer weights" in lib.psf_last_error(), k
        for name in ("a", "B", "b", "Y"):                                             # (nothing else needs more than a float's)
            assert fwd(A=bad, **{name: tab(v=68)}) == -4 and fwd(A=tab(hole=k), **{name: tab(v=68)}) == -1

    # ---- backward: (saved, saved_bytes, T, E, K, A, B, h, O, dY, dX, dA, da, dB, db, workspace, workspace_bytes, stream)
    g = lib.psf_mlp_wide_bwd_f32

    def bwd(**kw):
        a = dict(saved=SAVED, n_saved=n_saved, T=T, E=E, K=K, A=tab(), B=tab(), h=h, O=O, dY=tab(), dX=vp(32), dA=tab(), da=tab(),
                 dB=tab(), db=tab(), ws=WS, n_ws=n_bwd)
        a.update(kw)
        rc = g(a["saved"], a["n_saved"], a["T"], a["E"], a["K"], a["A"], a["B"], a["h"], a["O"], a["dY"], a["dX"], a["dA"], a["da"],
               a["dB"], a["db"], a["ws"], a["n_ws"], None)
        assert rc != 0 and b"psf_mlp_wide_bwd" in lib.psf_last_error(), kw
        return rc

    for name in ("saved", "A", "B", "h", "O", "dY", "dA", "da", "dB", "db", "ws"):
        assert bwd(**{name: None}) == -1, name
        assert bwd(**{name: None}, T=0) == -1, name
    for kw in (dict(T=0), dict(E=520), dict(K=25), dict(h=arr([32, 129])), dict(O=arr([0, 40]))):
        assert bwd(**kw) == -2, kw
        assert bwd(**kw, saved=vp((1 << 20) + 16)) == -2, kw
    for kw in (dict(saved=vp((1 << 20) + 16)), dict(ws=vp((1 << 24) + 128))):
        assert bwd(**kw) == -4, kw
        assert bwd(**kw, n_ws=0, n_saved=0) == -4, kw
    for kw in (dict(n_saved=n_saved - 1), dict(n_ws=n_bwd - 1)):
        assert bwd(**kw) == -2 and b"too small" in lib.psf_last_error(), kw
        assert bwd(**kw, dY=tab(hole=1)) == -2, kw
    for name in ("A", "B", "dY", "dA", "da", "dB", "db"):
        for k in range(K):
            assert bwd(**{name: tab(hole=k)}) == -1 and b"NULL layer pointer" in lib.psf_last_error(), (name, k)
            assert bwd(**{name: tab(hole=k)}, dX=None) == -1, (name, k)


def test_adam_step_is_validated_in_full_before_the_first_launch(lib):
    """psf_adam_step_f32 puts 40 tensors into a launch. A fault behind the first 40 (or 80) tensors of a list comes back as its
    code before anything is launched: these pointers are fake, so wherever there is a device a launch on the tensors in front
    of the fault would be an illegal access (tests/test_gpu_adam.py shows on real tensors that none of them has changed)."""
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    f = lib.psf_adam_step_f32
    hyper = (1e-3, 0.9, 0.999, 1e-8)

    def tables(count, fault=None, at=None):
        tabs = [[4096 + 64 * (4 * k + j) for k in range(count)] for j in range(4)]
        sizes = [16] * count
        if fault == "null":
            tabs[2][at] = None
        elif fault == "align":
            tabs[1][at] += 2
        elif fault == "negative":
            sizes[at] = -1
        elif fault == "blocks":  # 2^31 - 1 workgroups of 4096 elements, and one more, inside one launch
            sizes[at - 1], sizes[at] = 4096 * (2 ** 31 - 1), 1
        return [(vp * max(count, 1))(*t) for t in tabs] + [(i64 * max(count, 1))(*sizes)]

    for fault, code in (("null", -1), ("negative", -1), ("align", -4), ("blocks", -2)):
        for at in (40, 79, 80):
            if fault == "blocks" and at in (40, 80):
                continue  # (the count is per launch: index at - 1 would sit in the launch before)
            assert f(*tables(81, fault, at), 81, *hyper, 1.0, None, None) == code, (fault, at)
            assert b"psf_adam_step" in lib.psf_last_error()
    t81 = tables(81)
    for step in (0.5, 0.0, -1.0, float("nan")):
        assert f(*t81, 81, *hyper, step, None, None) == -2 and b"step" in lib.psf_last_error()   # PSF_E_SHAPE
    assert f(*t81, -1, *hyper, 1.0, None, None) == -2                                             # count < 0
    assert f(*t81, 0, *hyper, 1.0, None, None) == 0 and f(None, None, None, None, None, 0, *hyper, 0.5, None, None) == 0
    for j in range(5):                                                                            # a NULL table
        t = list(t81)
        t[j] = None
        assert f(*t, 81, *hyper, 1.0, None, None) == -1


# The keys of the library: the parent's nineteen chord knobs (its twenty-one less the two timing-lab keys, which left with the
# labs) and the two that the producer entry points read.
KNOB_KEYS = ["fwd_variant", "bwd_variant", "xcd_remap", "fwd_split", "fwd_wide", "dw_variant", "dv_threads", "bwd_fused",
             "bwd_fused_wg_limit", "dw_tgs", "fwd_wg_limit", "chain_zigzag", "mixer_wg_limit", "mixer_lds", "bwd_fronts",
             "fwd_rows", "chain_fused", "chain_cc", "chain_bwd_fused", "mlp_variant", "wide_fuse"]

CATALOGUE_PRINTER = r"""
#include <stdio.h>
#include "psf_chord_tuning.h"
#define PSF_ROW(key, lo, hi, def) printf("%s %d %d %d\n", #key, lo, hi, def);
int main(void) {
  PSF_TUNING_KNOBS(PSF_ROW)
  return 0;
}
"""


@pytest.fixture(scope="module")
def catalogue(tmp_path_factory):
    """include/psf_chord_tuning.h as a C consumer sees it: [(key, lo, hi, default)], printed by a strict-C99 program."""
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc") or "/opt/rocm/llvm/bin/clang"
    tmp = tmp_path_factory.mktemp("catalogue")
    (tmp / "rows.c").write_text(CATALOGUE_PRINTER)
    proc = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp / "rows.c"), "-o", str(tmp / "rows")], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    out = subprocess.run([str(tmp / "rows")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    return [(k, int(lo), int(hi), int(d)) for k, lo, hi, d in (line.split() for line in out.stdout.splitlines())]


def test_knob_catalogue_is_what_the_library_accepts(lib, catalogue):
    """Every row of PSF_TUNING_KNOBS against the loaded library: the default is what psf_get_tuning answers, both ends of the
    range are accepted, one step beyond either end is PSF_E_TUNING and leaves the value alone, and the value is put back."""
    E_TUNING = -6
    assert len(catalogue) == len({k for k, *_ in catalogue})  # one entry per key
    for key, lo, hi, default in catalogue:
        k = key.encode()
        assert lo <= default <= hi, key
        assert lib.psf_get_tuning(k) == default, key
        try:
            for v in (lo, hi):
                assert lib.psf_set_tuning(k, v) == 0 and lib.psf_get_tuning(k) == v, (key, v)
            for v in (lo - 1, hi + 1):
                assert lib.psf_set_tuning(k, v) == E_TUNING and lib.psf_get_tuning(k) == hi, (key, v)
                assert key.encode() in lib.psf_last_error()
        finally:
            assert lib.psf_set_tuning(k, default) == 0
        assert lib.psf_get_tuning(k) == default, key


def test_knob_key_set(lib, catalogue):
    """The catalogue's keys are exactly the 21 written above, and the library knows no other: the two timing-lab keys are
    rejected exactly like a key that never existed."""
    E_TUNING = -6
    assert len(KNOB_KEYS) == 21
    assert sorted(k for k, *_ in catalogue) == sorted(KNOB_KEYS)
    for key in KNOB_KEYS:
        assert lib.psf_get_tuning(key.encode()) >= 0, key
    answers = {}
    for key in ("no_such_knob", "mixer_ablate", "bwd_ablate"):
        rc_set, err_set = lib.psf_set_tuning(key.encode(), 0), lib.psf_last_error().decode()
        rc_get, err_get = lib.psf_get_tuning(key.encode()), lib.psf_last_error().decode()
        assert rc_set == E_TUNING and rc_get == E_TUNING, key
        answers[key] = (rc_set, err_set.replace(key, "KEY"), rc_get, err_get.replace(key, "KEY"))
    assert answers["mixer_ablate"] == answers["bwd_ablate"] == answers["no_such_knob"]
    assert "unknown tuning key 'KEY'" in answers["no_such_knob"][1]


def test_tuning_context_manager_restores_on_error(lib):
    import sparsefactorization_amd as sfa
    assert sfa.tuning is sfa._lib.tuning
    with sfa.tuning(fwd_variant=1, chain_cc=2):
        assert (sfa.get_tuning("fwd_variant"), sfa.get_tuning("chain_cc")) == (1, 2)
    assert (sfa.get_tuning("fwd_variant"), sfa.get_tuning("chain_cc")) == (0, 0)
    with pytest.raises(ZeroDivisionError):
        with sfa.tuning(bwd_fused=0):
            assert sfa.get_tuning("bwd_fused") == 0
            1 / 0
    assert sfa.get_tuning("bwd_fused") == 1
    with pytest.raises(sfa.PSFLibraryError):  # a refused value: what was set before it is put back
        with sfa.tuning(fwd_variant=2, bwd_variant=7):
            pass
    assert (sfa.get_tuning("fwd_variant"), sfa.get_tuning("bwd_variant")) == (0, 0)


def test_tuning_knobs(lib):
    import sparsefactorization_amd as sfa
    assert sfa.get_tuning("mlp_variant") == 0
    sfa.set_tuning("mlp_variant", 3)
    assert sfa.get_tuning("mlp_variant") == 3
    sfa.set_tuning("mlp_variant", 0)
    with pytest.raises(sfa.PSFLibraryError):
        sfa.set_tuning("mlp_variant", 4)
    assert sfa.get_tuning("fwd_variant") == 0
    sfa.set_tuning("fwd_variant", 1)
    assert "generic" in sfa.describe_fwd(64, 16384, 15, 8)
    sfa.set_tuning("fwd_variant", 0)
    assert "win" in sfa.describe_fwd(64, 16384, 15, 8)
    with pytest.raises(sfa.PSFLibraryError):
        sfa.set_tuning("no_such_knob", 1)
    with pytest.raises(sfa.PSFLibraryError):
        sfa.set_tuning("fwd_variant", 99)


def test_no_cpu_fallback(lib):
    """CPU tensors must raise: the product has no CPU path (the oracle is test infrastructure only)."""
    import sparsefactorization_amd as sfa
    W, V = torch.zeros(1, 8, 4), torch.zeros(1, 8, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.chord_spmm(W, V)
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.chord_chain([W], V)
    idx = torch.tensor(sfa.get_chord_indices_assym(8, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.spmm(idx, W.reshape(1, 32), 8, 8, V)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "sparsefactorization_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\.*oracle", text, flags=re.M), f
                assert "liboracle" not in text and "chord_oracle" not in text, f


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from sparsefactorization_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libpsf_chord.so"))
    with pytest.raises(_lib.PSFLibraryError, match="not built"):
        _lib.load()


def test_offsets_from_index_validation():
    from sparsefactorization_amd.chord import offsets_from_index
    import sparsefactorization_amd as sfa
    idx = torch.tensor(sfa.get_chord_indices_assym(100, 9))
    assert offsets_from_index(idx, 100) == (0, 1, 2, 4, 8, 16, 32, 64, 28)
    bad = idx.clone()
    bad[0, 3] = 7
    with pytest.raises(ValueError, match="rows"):
        offsets_from_index(bad, 100)
    bad = idx.clone()
    bad[1, 20] += 1
    with pytest.raises(ValueError, match="cols"):
        offsets_from_index(bad, 100)
    with pytest.raises(ValueError):
        offsets_from_index(idx[:, :-1], 100)


# ---------------------------------------------------------------------------------------------------
# module surface: constructor signatures, attribute names, state_dict layout, shipped checkpoints
# ---------------------------------------------------------------------------------------------------
def _layouts():
    out = {}
    for line in load_golden("checkpoint_layouts.npz")["layouts"]:
        ck, key, shape = str(line).split("|")
        out.setdefault(ck, {})[key] = tuple(int(s) for s in shape.split("x")) if shape else ()
    return out


PATHFINDER = dict(vocab_size=225, embedding_size=32, n_vec=1024, n_W=11, Ws=[128, 'GELU'], V=[128, 'GELU'],
                  n_channels_V=32, n_class=2, pooling_type="FLATTEN", head=['linear'], use_cuda=False,
                  use_residuals=False, dropout1_p=0, dropout2_p=0, dropout3_p=0, init_embedding_weights=False,
                  use_pos_embedding=True, problem="pathfinder")
IMDB = dict(vocab_size=97, embedding_size=32, n_vec=4097, n_W=12, Ws=[128, 'GELU'], V=[128, 'GELU'],
            n_channels_V=32, n_class=2, pooling_type="CLS", head=['linear'], use_cuda=False, use_residuals=True,
            dropout1_p=0.4, dropout2_p=0, dropout3_p=0, init_embedding_weights=True, use_pos_embedding=False,
            problem="imdb")


@pytest.mark.parametrize("ckpt,cfg", [("pathfinder_epoch27.pt", PATHFINDER), ("imdb_epoch138.pt", IMDB)])
def test_state_dict_layout_matches_shipped_checkpoints(lib, ckpt, cfg):
    """LRA/psf_training_config.py:60-117 configs; layouts recorded from LRA/attention_maps/*.pt."""
    from sparsefactorization_amd.lra_psf import PSFNet
    net = PSFNet(**cfg)
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert mine == _layouts()[ckpt]
    assert "chord_indicies" not in mine
    assert net.chord_indicies.shape == (2, cfg["n_vec"] * (cfg["n_W"] + 1))
    assert net.n_links == cfg["n_W"] + 1


def test_synthetic_module_surface(lib):
    from sparsefactorization_amd.synthetic_psf import PSFNet, MLPBlock, MakeMLP, get_chord_indices_assym  # noqa: F401
    g = load_golden("psfnet_adding_n128.npz")
    torch.manual_seed(42)
    net = PSFNet(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=128, n_W=7, Ws=[32, 'GELU'],
                 V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
                 use_cuda=False, use_residuals=True, use_pos_embedding=False, problem="adding")
    want = {k[4:]: g[k] for k in g.files if k.startswith("sd::")}
    sd = net.state_dict()
    assert set(sd) == set(want)
    # same construction order as the reference => the same seed draws the same initial weights
    for k, v in want.items():
        assert np.array_equal(sd[k].numpy(), v), k
    assert np.array_equal(net.chord_indicies.numpy(), g["chord_indicies"])
    for attr in ("fs", "g", "final", "embedding", "pos_embedding", "init_linear", "n_W", "n_links", "n_vec"):
        assert hasattr(net, attr)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in want.items()}, strict=True)


def test_attention_block_surface(lib):
    from sparsefactorization_amd.attention_block import PSFNet
    net = PSFNet(vocab_size=256, embedding_size=16, max_seq_len=100, use_cuda=False, use_residuals=False,
                 dropout1_p=0, dropout2_p=0, dropout3_p=0)
    assert net.n_W == 7 and net.n_links == 8
    keys = set(net.state_dict())
    assert {"embedding.weight", "apc_embedding.weight", "g.network.0.weight", "fs.6.network.2.bias"} <= keys


def test_genome_surface(lib):
    from sparsefactorization_amd.genome_psf import PSFNet
    cfg = dict(IMDB)
    cfg.pop("problem")
    cfg.update(n_vec=64, n_W=6)
    net = PSFNet(**cfg)
    assert net.embedding.padding_idx is None


def test_library_carries_the_hash_of_its_sources_and_a_stale_one_is_reported(monkeypatch):
    """psf_build_info ends in csrc=<sha256 of csrc/ + the header>; build.needs_build and _lib.load compare it with the
    tree, so an edited kernel source cannot silently run on an old binary."""
    import warnings
    from sparsefactorization_amd import _lib, build
    lib = _lib.load()
    assert ("csrc=" + build.csrc_hash()).encode() in lib.psf_build_info()
    assert build.built_hash() == build.csrc_hash() and not build.needs_build()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _lib._warn_if_stale(lib)  # fresh: silent
    monkeypatch.setattr(build, "csrc_hash", lambda: "0" * 64)
    assert build.needs_build()
    with pytest.warns(RuntimeWarning, match="built from other sources"):
        _lib._warn_if_stale(lib)


def test_fused_mixer_handoff_is_per_thread_and_uncovered_blocks_raise(lib, monkeypatch):
    """fused_mixer hands what its eligibility check found to the forward that follows as an argument (``find`` ->
    ``mixer_forward_in(..., found)``): the module keeps no state between the two calls, so two threads serving two models each
    get their own layers back, and blocks the path does not cover raise a ValueError naming the requirement instead of a
    TypeError."""
    import threading
    from sparsefactorization_amd import fused_mixer
    from sparsefactorization_amd.psfnet import MLPBlock
    assert not any(hasattr(fused_mixer, name) for name in ("_handoff", "_key", "_pending", "threading"))
    g, fs = MLPBlock([32, 'GELU'], 32, 8), [MLPBlock([32, 'GELU'], 32, 12) for _ in range(3)]
    found = fused_mixer._block_pairs(32, g, fs)
    assert found is not None and found[0][0] == 3 and found[0][2:] == (8, 12) and len(found[1]) == 4
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))  # everything but the device
    monkeypatch.setattr(fused_mixer, "route", "always")
    models = [(g, fs), (MLPBlock([16, 'GELU'], 32, 4), [MLPBlock([16, 'GELU'], 32, 9) for _ in range(2)])]
    seen, barrier = {}, threading.Barrier(2, timeout=20)

    def serve(i):
        gi, fi = models[i]
        with torch.no_grad():
            r = fused_mixer.Recipe.data(torch.zeros(2, 64, 32))
            assert fused_mixer.eligible_recipe(r, gi, fi)
            barrier.wait()  # both threads have asked before either takes its answer
            first = fused_mixer.find(r, gi, fi)
            barrier.wait()
            seen[i] = (first, fused_mixer.find(r, gi, fi))
    threads = [threading.Thread(target=serve, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i, (gi, fi) in enumerate(models):
        for sizes, pairs in seen[i]:
            assert (sizes[0], list(sizes[1]), sizes[2], sizes[3]) == ((3, [32] * 4, 8, 12), (2, [16] * 3, 4, 9))[i]
            assert all(a is b for got, blk in zip(pairs, [gi, *fi]) for a, b in zip(got, (blk.network[0], blk.network[2])))
    monkeypatch.setattr(fused_mixer, "route", "never")
    with torch.no_grad():
        assert fused_mixer.find(fused_mixer.Recipe.data(torch.zeros(2, 64, 32)), g, fs) is None
    monkeypatch.undo()
    odd = [MLPBlock([32, 'GELU'], 32, 12), MLPBlock([32, 'GELU'], 32, 13)]  # link MLPs that disagree on L
    assert fused_mixer._block_pairs(32, g, odd) is None
    with pytest.raises(ValueError, match="does not cover these blocks"):
        fused_mixer.mixer_forward(torch.zeros(1, 64, 32), g, odd, True)


def test_interleaved_fronts_visit_every_tile_once():
    """Geom::ileave (csrc/psf_common.h: decode_block; knob "bwd_fronts"): position t of an XCD's walk through a batch element
    is row block (t mod 2^s) * tiles / 2^s + t / 2^s. Restated here: for every tile count the host accepts (2^s | tiles) the
    map is a bijection, consecutive positions are tiles / 2^s apart (the fronts) and each front advances one tile per 2^s
    positions — speed only, never correctness; the GPU test test_fused_backward_fronts_only_reorder_workgroups checks the bits."""
    for s in (1, 2, 3):
        for tiles in (1 << s, 2 << s, 6 << s, 64, 128, 512, 1000 << s):
            if tiles % (1 << s):
                continue
            walk = [(t & ((1 << s) - 1)) * (tiles >> s) + (t >> s) for t in range(tiles)]
            assert sorted(walk) == list(range(tiles))
            assert walk[1] - walk[0] == tiles >> s
            if tiles > (1 << s):
                assert walk[1 << s] == 1
