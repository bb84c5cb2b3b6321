"""CPU: the instance grid of tests/instance_grid.py is what the library can name, every cell has a recipe, and the operands of
the GPU module's bit-for-bit verdicts are exact at the grid's shapes. Host only: the describe entries and the CPU oracle."""
import itertools
import re

import numpy as np
import pytest

import bf16_edges as be
import instance_grid as ig
import x3_exact as xe
from oracle import chord_oracle as oc
from sparsefactorization_amd import _lib
from sparsefactorization_amd._lib import tuning
from test_gpu_launch_table import ROUTE_DEFAULTS

SWEEP_L = (4, 12, 20)
SWEEP_C = {4: [4 << t for t in range(7)] + [12, 20, 36, 136, 260], 2: [8 << t for t in range(6)] + [12, 20, 36, 136, 260]}
SWEEP_N = sorted({n for k in range(14) for n in (2 ** k - 1, 2 ** k, 2 ** k + 1) if 1 <= n <= 8192})
_STEP = re.compile(r"(chord_(?:fwd_win|dv_win|dw_win|dw_chunk|bwd_fused_edge|bwd_fused)_k)<(f32|bf16),L=\d+,TG=(\d+),(?:R=(\d+),)?NT=(\d+)>")
_FAMILY_OF = {v: k for k, v in ig.KERNEL.items()}


def _knob_sets():
    sets = [{}] + [ig._mode_knobs(f, c, m) for f, cs in ig.STEP_GRID.items() for c in cs for m in ig.MODES[ig.kind(f)]]
    return [dict(t) for t in sorted({tuple(sorted(s.items())) for s in sets})]


def test_the_step_grid_is_what_describe_can_name():
    """Every (kernel, element, TG, R, NT) that psf_describe_fwd / _bwd name over the sweep has a grid row, and every grid row is
    named: a newly compiled configuration without a row fails here, and so does a row that nothing reaches."""
    named = set()
    for kn in _knob_sets():
        with tuning(**{**ROUTE_DEFAULTS, **kn}):
            for eb, L, N in itertools.product((4, 2), SWEEP_L, SWEEP_N):
                for C in SWEEP_C[eb]:
                    for s in (_lib.describe_fwd(ig.B, N, L, C, elem_bytes=eb), _lib.describe_bwd(ig.B, N, L, C, elem_bytes=eb)):
                        for kernel, el, tg, r, nt in _STEP.findall(s):
                            named.add((f"{_FAMILY_OF[kernel]}_{el}", (int(tg), int(r or 1), int(nt))))
    table = {(f, c) for f, cs in ig.STEP_GRID.items() for c in cs}
    assert named == table, (sorted(named - table), sorted(table - named))


def _chain_config(s):
    m = re.search(r"chord_chain_lds_k<(f32|bf16),L=\d+,CC=(\d+),R=(\d+)> .*?, (\d+) threads,", s)
    if m:
        r = int(m.group(3))
        return m.group(1), ("lds", int(m.group(2)), r, int(m.group(4)) > 512 if r == 2 else None)
    m = re.search(r"chord_chain_rows_k<(f32|bf16),L=\d+,G=(\d+),R=(\d+)>", s)
    return (m.group(1), ("rows", int(m.group(2)), int(m.group(3)), None)) if m else None


def test_the_chain_grid_is_what_describe_can_name():
    """The same for psf_describe_chain_fwd_dtype. N: around the powers of two and around the planner's own limits
    (fwd_chain_lds_launch.h: kChainLdsMaxSlots = 2112 and its half, kChainLongRows = 4160)."""
    named = set()
    lengths = sorted(set(SWEEP_N) | {1056, 1057, 2112, 2113, 4160, 4161})
    for cc in (0, 1, 2):
        with tuning(**{**ROUTE_DEFAULTS, "chain_fused": 2, "chain_cc": cc}):
            for eb, L, N in itertools.product((4, 2), (2,) + SWEEP_L, lengths):
                for C in SWEEP_C[eb]:
                    got = _chain_config(_lib.describe_chain_fwd(ig.B, N, L, C, ig.M, elem_bytes=eb))
                    if got:
                        named.add(got)
    table = {(el, c) for el in ("f32", "bf16") for c in ig.CHAIN_GRID}
    assert named == table, (sorted(named - table, key=str), sorted(table - named, key=str))


def test_every_step_cell_has_a_recipe_for_every_mode():
    """No cell is left out because its shape was hard to find; the shapes are the smallest: N <= two tiles + one row, at most 1025
    (the full+ragged run: up to half a 16-byte group of rows, test_split_runs_stay_next_to_the_aligned_length; the fused steps'
    run with a far link on another block: four tiles, at most 1024 rows)."""
    missing, runs = [], 0
    for f, c, L in ig.step_cells():
        assert ig.modes(f, c, L), (f, c, L)
        assert ig.kind(f) != "fwd" or ("full" in ig.modes(f, c, L)) == (ig.near_links(c, L) < L)  # (MODE 0 needs a far link)
        for mode in ig.modes(f, c, L):
            r = ig.recipe(f, c, L, mode)
            runs += 1
            if r is None:
                missing.append((f, c, L, mode))
                continue
            Bc, N, C, kn = r
            TR = ig.tile_rows(c)
            assert Bc == ig.B and C == ig.channels(f, c) and N >= 2 * TR
            assert N <= {"split": 2 * TR + 8 // ig.elem_bytes(f), "far": 4 * TR}.get(mode, 2 * TR + 1) <= 1028, (f, c, L, mode, N)
            assert (N % TR == 0) == (mode not in ("edge", "split")), (f, c, L, mode, N)
            with tuning(**kn):
                ig.confirm(f, c, L, mode, N, C)
    assert not missing, missing
    # forward: 5 runs where the aligned launch has a far link, else 4; dV, dW, chunk: 3; fused: 2 where it has a far link, else 1; edge: 2
    assert runs == 3275


def test_the_cell_totals():
    cells = ig.step_cells()
    per = {f: sum(1 for g, _c, _L in cells if g == f) for f in ig.STEP_GRID}
    assert per == {"fwd_f32": 187, "dv_f32": 170, "dw_f32": 119, "chunk_f32": 34, "fused_f32": 102, "fused_edge_f32": 102,
                   "fwd_bf16": 85, "dv_bf16": 85, "dw_bf16": 85, "fused_bf16": 85}
    for el, total in ig.STEP_TOTALS.items():
        assert sum(n for f, n in per.items() if ig.elem(f) == el) == total
    assert sum(ig.STEP_TOTALS.values()) == 1054 == len(set(ig.instance(f, c, L) for f, c, L in cells))
    assert len(ig.mixer_cells()) == 68
    assert len(ig.chain_cells()) == 380 == 2 * 19 * len(ig.CHAIN_GRID)


def test_every_chain_cell_has_a_recipe_and_the_refused_ones_are_these():
    """chord_chain_lds_k with three rows per thread is declined beyond L = 14 (f32) and 18 (bf16): the only cells decided by
    the planner's rule and not by a run. There describe names another kernel at the N that the last accepted L takes."""
    refused = []
    for el, c, L in ig.chain_cells():
        r = ig.chain_recipe(el, c, L)
        assert r is not None, (el, c, L)
        Bc, N, C, kn = r
        assert Bc == ig.B and N <= ig.CHAIN_N_MAX and C in (4, 8, 16)
        with tuning(**kn):
            s = _lib.describe_chain_fwd(Bc, N, L, C, ig.M, elem_bytes=4 if el == "f32" else 2)
        assert ig.chain_shows(el, c, L, s) == (not ig.chain_refused(el, c, L)), (el, c, L, s)
        if ig.chain_refused(el, c, L):
            assert "chord_chain" not in s, s
            refused.append((el, c[1], L))
    assert refused == [("f32", cc, L) for cc in (1, 2) for L in range(15, 21)] + [("bf16", cc, L) for cc in (1, 2) for L in (19, 20)]
    for L, taken in ((14, True), (15, False)):  # "beyond L = 14 the 768-thread f32 instance spills": both sides of the rule
        for c in (("lds", 1, 3, None), ("lds", 2, 3, None)):
            Bc, N, C, kn = ig.chain_recipe("f32", c, L)
            with tuning(**kn):
                s = ig.describe(ig.chain_family("f32", c), N, L, Bc, C)
            assert ig.chain_refused("f32", c, L) == (not taken) and ig.chain_shows("f32", c, L, s) == taken, s


def test_split_runs_stay_next_to_the_aligned_length():
    """The full+ragged run is one row longer wherever B N L stays a whole number of 16-byte groups, else a few."""
    for f in ("fwd_f32", "fwd_bf16"):
        vec = 16 // ig.elem_bytes(f)
        for c in ig.STEP_GRID[f]:
            for L in ig.WIN_L:
                N0, N = ig.recipe(f, c, L, "aligned")[1], ig.recipe(f, c, L, "split")[1]
                assert (ig.B * N * L) % vec == 0 and all((ig.B * n * L) % vec for n in range(N0 + 1, N)), (f, c, L, N0, N)
                assert N - N0 <= vec // 2


@pytest.mark.parametrize("C", ig.MIXER_C)
def test_the_mixer_cells_are_exact(C):
    """The form of test_x3_exact_cpu.py: test_the_mixer_cases_are_exact, at the grid's shapes; and the per-step kernels take
    every one of them (psf_mixer_fwd_plan = 1 under mixer_lds = 0)."""
    with tuning(mixer_lds=0):
        assert all(ig.mixer_plan(N, C, L) == 1 for L in ig.MIXER_L for N in ig.mixer_lengths(C))
    assert ig.mixer_lengths(C)[0] == {4: 512, 8: 512, 16: 256, 32: 128}[C]
    for L in (4, 11, 20):
        for N in ig.mixer_lengths(C):
            for kind in ig.MIXER_KINDS:
                case = ig.mixer_case(kind, N, C, L)
                xe.check_exact(case)
                assert max(np.abs(y).max() for y in case.reference()["Y"][1:]) * L < 2  # |W| L < 2: the chain does not grow


DW_SHAPES = [("dv_f32", (64, 2, 256), 20, "edge"), ("dw_f32", (64, 1, 256), 4, "full"), ("dv_f32", (1, 2, 256), 20, "edge"),
             ("chunk_f32", (16, 1, 256), 13, "edge"), ("dw_bf16", (16, 1, 256), 12, "full"), ("fused_f32", (32, 1, 256), 20, "aligned")]


@pytest.mark.parametrize("family,config,L,mode", DW_SHAPES)
def test_the_integer_dw_cases_stay_exact_at_the_widest_rows(family, config, L, mode):
    """_bwd_case's operands (test_gpu_launch_table.py) at the grid's shapes: every dW sum an f32 integer far below 2^24, equal
    to the oracle's f32 result, so one dW is correct in any summation order."""
    Bc, N, C, _kn = ig.recipe(family, config, L, mode)
    assert (family, config, L, mode) != DW_SHAPES[0] or (N, C) == (17, 256)
    dZ, V, W = be.int_case((Bc, N, C), 50 + L), be.int_case((Bc, N, C), 51 + L), be.normal_case((Bc, N, L), 52, 0.5)
    exact, _ = be.dw_sums(dZ, V, L)
    dF, _dV = oc.spmul_bwd(dZ, W, V)
    assert np.abs(exact).max() <= 225 * C < 2.0 ** 24 and np.array_equal(exact.astype(np.float32), dF)
