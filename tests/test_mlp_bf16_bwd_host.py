"""CPU: the host side of the fused bf16 producer backward — psf_mlp_bwd_bf16's limits and argument validation (everything that
returns before the first HIP call), its declarations as C99, and the route ``fused_mlp`` gives a call with the opt-in switch
``bf16_train_route`` at "never" (the recorded parent's answers, all of them) and at "always" (exactly the bf16 training calls
inside the kernel's limits move to "bf16_train"). No device is touched: nothing is launched."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

import producer_route_grid as grid
from conftest import ROOT

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "producer_routes_parent.json")
i32, vp = ctypes.c_int32, ctypes.c_void_p
NULL, SHAPE, ALIGN = -1, -2, -4  # PSF_E_NULL, PSF_E_SHAPE, PSF_E_ALIGN


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def arr(vals):
    return (i32 * len(vals))(*vals)


def ptrs(n, v=16):
    return (vp * n)(*([v] * n))


def ws_of(lib, T, E, hs, Os):
    return lib.psf_mlp_bwd_bf16_workspace(T, E, len(hs), arr(hs), arr(Os))


def test_workspace_states_every_limit_from_both_sides(lib):
    for E, ok in ((0, False), (8, True), (32, True), (40, False), (36, False)):
        assert (ws_of(lib, 1000, E, [32], [8]) > 0) == ok, f"E = {E}"
        assert ok or ws_of(lib, 1000, E, [32], [8]) == -1
    for h, ok in ((0, False), (1, True), (128, True), (129, False)):
        assert (ws_of(lib, 1000, 32, [32, h], [8, 8]) > 0) == ok, f"h = {h}"
        assert ok or ws_of(lib, 1000, 32, [32, h], [8, 8]) == -1
    for O, ok in ((0, False), (1, True), (32, True), (33, False)):
        assert (ws_of(lib, 1000, 32, [32, 32], [8, O]) > 0) == ok, f"O = {O}"
        assert ok or ws_of(lib, 1000, 32, [32, 32], [8, O]) == -1
    for K, ok in ((0, False), (1, True), (32, True), (33, False)):
        assert (ws_of(lib, 1000, 32, [32] * K, [8] * K) > 0) == ok, f"K = {K}"
        assert ok or ws_of(lib, 1000, 32, [32] * K, [8] * K) == -1
    assert ws_of(lib, 0, 32, [32], [8]) == -1 and ws_of(lib, 1, 32, [32], [8]) > 0
    assert lib.psf_mlp_bwd_bf16_workspace(1000, 32, 1, None, arr([8])) == -1
    # 16-byte multiples; one partial-sum slot per workgroup, so it grows with T and with the number of 32-row units
    small, large = ws_of(lib, 1000, 32, [32], [8]), ws_of(lib, 10 ** 6, 32, [32], [8])
    assert small % 16 == 0 and large > small and ws_of(lib, 1000, 32, [33], [8]) == 2 * small


def call(lib, X=16, T=1000, E=32, K=3, A=None, a=None, B=None, h=None, O=None, dY=None, dX=32, dA=None, da=None, dB=None,
         db=None, ws=48, ws_bytes=None):
    """psf_mlp_bwd_bf16 on made-up addresses (never dereferenced by the host: every case below fails validation)."""
    h = arr([32, 33, 128]) if h is None else h
    O = arr([8, 15, 32]) if O is None else O
    tab = lambda t: ptrs(K) if t is None else t
    need = lib.psf_mlp_bwd_bf16_workspace(T, E, K, h, O)
    return lib.psf_mlp_bwd_bf16(vp(X) if X else None, T, E, K, tab(A), tab(a), tab(B), h, O, tab(dY), vp(dX) if dX else None,
                                tab(dA), tab(da), tab(dB), tab(db), vp(ws) if ws else None,
                                need if ws_bytes is None else ws_bytes, None)


def test_validation_order_and_codes_before_any_hip_call(lib):
    need = ws_of(lib, 1000, 32, [32, 33, 128], [8, 15, 32])
    assert need > 0
    # 1. NULL tables
    assert call(lib, X=0) == NULL and b"psf_mlp_bwd_bf16" in lib.psf_last_error()
    assert call(lib, ws=0) == NULL
    for name in ("A", "a", "B", "dY", "dA", "da", "dB", "db"):
        bad = lib.psf_mlp_bwd_bf16(vp(16), 1000, 32, 3, *[None if n == name else ptrs(3) for n in ("A", "a", "B")], arr([32, 33, 128]),
                                   arr([8, 15, 32]), None if name == "dY" else ptrs(3), vp(32),
                                   *[None if n == name else ptrs(3) for n in ("dA", "da", "dB", "db")], vp(48), need, None)
        assert bad == NULL, name
    # ... before the shape: a NULL table with a bad shape is still PSF_E_NULL
    assert call(lib, X=0, E=36) == NULL
    # 2. shape
    for kw in (dict(T=0), dict(E=36), dict(E=40), dict(E=0), dict(h=arr([32, 129, 32])), dict(O=arr([8, 33, 8])), dict(O=arr([0, 8, 8]))):
        assert call(lib, ws_bytes=1 << 40, **kw) == SHAPE, kw
    assert b"E in {8,16,24,32}" in lib.psf_last_error()
    assert lib.psf_mlp_bwd_bf16(vp(16), 1000, 32, 33, ptrs(33), ptrs(33), ptrs(33), arr([32] * 33), arr([8] * 33), ptrs(33), vp(32),
                                ptrs(33), ptrs(33), ptrs(33), ptrs(33), vp(48), 1 << 40, None) == SHAPE
    # ... before the alignment: a misaligned X with a bad shape is PSF_E_SHAPE
    assert call(lib, X=18, T=0) == SHAPE
    # 3. X, dX, dY[k]: 16-byte alignment
    assert call(lib, X=24) == ALIGN and call(lib, dX=40) == ALIGN
    assert call(lib, dY=(vp * 3)(16, 16, 18)) == ALIGN and b"dY" in lib.psf_last_error()
    # ... before the workspace
    assert call(lib, X=24, ws_bytes=16) == ALIGN
    # 4. workspace
    assert call(lib, ws_bytes=need - 16) == SHAPE and b"workspace" in lib.psf_last_error()
    assert call(lib, ws=40) == SHAPE
    # 5. per MLP: NULL, then 2-byte alignment; a short workspace comes first
    assert call(lib, A=(vp * 3)(16, None, 16)) == NULL and b"layer" in lib.psf_last_error()
    assert call(lib, A=(vp * 3)(16, None, 16), ws_bytes=need - 16) == SHAPE
    assert call(lib, db=(vp * 3)(16, 16, None)) == NULL and call(lib, dY=(vp * 3)(None, 16, 16)) == NULL
    assert call(lib, a=(vp * 3)(16, 17, 16)) == ALIGN and call(lib, dB=(vp * 3)(16, 16, 33)) == ALIGN
    # dX may be NULL: such a call gets past the whole validation of the tables (the next fault is reported)
    assert call(lib, dX=0, ws_bytes=need - 16) == SHAPE and call(lib, dX=0, a=(vp * 3)(16, 17, 16)) == ALIGN


C99_CONSUMER = r"""
#include <stddef.h>
#include "psf_chord.h"
int main(void) {
  int32_t h[1] = {32}, O[1] = {8};
  int64_t (*ws)(int64_t, int32_t, int32_t, const int32_t*, const int32_t*) = psf_mlp_bwd_bf16_workspace;
  int (*f)(const uint16_t*, int64_t, int32_t, int32_t, const uint16_t* const*, const uint16_t* const*, const uint16_t* const*,
           const int32_t*, const int32_t*, const uint16_t* const*, uint16_t*, uint16_t* const*, uint16_t* const*,
           uint16_t* const*, uint16_t* const*, void*, int64_t, void*) = psf_mlp_bwd_bf16;
  if (ws(1000, 32, 1, h, O) <= 0 || ws(1000, 40, 1, h, O) != -1) return 1;
  if (f(NULL, 1000, 32, 1, NULL, NULL, NULL, h, O, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) != PSF_E_NULL) return 2;
  return 0;
}
"""


def test_header_still_compiles_as_c99_with_the_new_declarations(lib, tmp_path):
    from sparsefactorization_amd import build
    gcc = shutil.which("gcc")
    assert gcc is not None, "the C99 check needs gcc"
    src, exe = tmp_path / "consumer.c", tmp_path / "consumer"
    src.write_text(C99_CONSUMER)
    libdir = os.path.dirname(build.LIB_PATH)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", libdir, "-l:libpsf_chord.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"consumer exited {run.returncode}: {run.stdout} {run.stderr}"


# ---------------------------------------------------------------- routes
@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)["answers"]


def test_route_table_has_the_new_entry_in_its_place():
    from sparsefactorization_amd import fused_mlp
    names = list(fused_mlp.ROUTES)
    assert names[names.index("bf16_forward") + 1] == "bf16_train" and names[names.index("bf16_train") + 1] == "stacked"
    assert fused_mlp.ROUTES["bf16_train"] == ("bf16_trainable", "fused_mlp_apply_bf16")
    assert fused_mlp.bf16_train_route == "never"
    lim = fused_mlp._BF16_TRAIN
    assert lim == fused_mlp._BF16._replace(e_max=32, k_max=fused_mlp.MAX_K) and lim.e_max == 32 and lim.k_max == 32


def test_never_is_the_default_and_gives_the_recorded_routes(recorded):
    from sparsefactorization_amd import fused_mlp
    assert fused_mlp.bf16_train_route == "never"
    got = {lab: (answer, named) for lab, answer, named in grid.answers(fused_mlp, also=fused_mlp.route)}
    assert list(got) == list(recorded)
    wrong = [(lab, got[lab], recorded[lab]) for lab in recorded
             if got[lab][0] != recorded[lab] or str(got[lab][1]) != recorded[lab].split(":")[1]]
    assert not wrong, wrong[:10]
    x, blocks = grid.build(grid._case("bf16", "train"))
    with grid.asked_on_the_gpu(fused_mlp, grid._case("bf16", "train")):
        assert not fused_mlp.bf16_trainable(x, blocks) and fused_mlp.route(x, blocks) == "stacked"


def _moves(c) -> bool:
    """Whether case ``c`` of the grid is a bf16 training call inside _BF16_TRAIN, from the case's own description."""
    return (c["x"] == "bf16" and c["params"] == "bf16" and c["odd"] is None and c["form"] == "plain" and not c["empty"]
            and c["mode"] in ("train", "frozen_x") and c["off"] not in ("enabled", "bf16_enabled", "train_enabled")
            and (c["shape"] is None or len(c["shape"]) >= 2) and c["E"] % 8 == 0 and 8 <= c["E"] <= 32
            and 1 <= c["h"] <= 128 and 1 <= c["O"] <= 32 and 1 <= c["K"] <= 32)


def test_always_moves_exactly_the_bf16_training_calls_inside_the_limits(recorded, monkeypatch):
    from sparsefactorization_amd import fused_mlp
    monkeypatch.setattr(fused_mlp, "bf16_train_route", "always")
    cases = {grid.label(c): c for c in grid.cases()}
    moved = 0
    for lab, answer, named in grid.answers(fused_mlp, also=fused_mlp.route):
        bits, was = recorded[lab].split(":")
        assert answer == recorded[lab], f"{lab}: a predicate of the parent changed its answer"
        if _moves(cases[lab]):
            moved += 1
            assert was == "stacked" or (was == "None" and cases[lab]["K"] == 1), (lab, was)  # (a single MLP is not stacked)
            assert named == "bf16_train", f"{lab}: route() = {named}"
        else:
            assert str(named) == was, f"{lab}: route() = {named}, the parent's is {was}"
    # both sides of every limit were asked: E 8 and 32 in, 36 and 64 out; K 32 in, 33 out; h 128 in, 129 out; O 32 in, 33 out
    assert moved >= 20
    for inside, outside in ((dict(E=32), dict(E=36)), (dict(E=8), dict(E=6)), (dict(E=32), dict(E=64)), (dict(K=32), dict(K=33)),
                            (dict(h=128), dict(h=129)), (dict(O=32), dict(O=33))):
        assert _moves(grid._case("bf16", "train", **inside)) and not _moves(grid._case("bf16", "train", **outside))
        assert grid.label(grid._case("bf16", "train", **inside)) in cases and grid.label(grid._case("bf16", "train", **outside)) in cases
