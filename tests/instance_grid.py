"""The grid of compiled chord kernel instances and, per cell, the smallest shape that runs it (host only: describe entries).

The step kernels are templates over the link count L and a launch configuration (lanes per row TG, rows per thread R,
workgroup size NT); their compile-time geometry (near/far split, W staging loop, LDS size) depends on both together, so every
(kernel, L, TG, R, NT) cell is code of its own. This module lists the cells (tables mirroring the launchers' constants, each
with its source) and finds for each one the smallest N, with the route knobs that reach the configuration, at which
psf_describe_* names exactly that instance. tests/test_instance_grid_host.py holds the tables against what the library can
name and the totals; tests/test_gpu_instance_grid.py runs every cell.

FAMILIES, _describe, _confirm and ROUTE_DEFAULTS are tests/test_gpu_launch_table.py's, untouched; the families that module
does not have (the dV and the dW window kernel on their own) go through `describe` and `confirm` below, which ask its
entries under the family of the same describe entry and element type.

What the smallest shapes leave out: at N = two tiles every far offset of the chord pattern, 2^k mod N, is 0, so in the aligned
runs (and the runs with a view one element off) every far link reads the row's own block. Far links on other blocks come with
the edge, full+ragged and off-grid runs (N + 1: the far offsets are 2^k mod (N + 1)) and, for the fused steps, whose aligned
instance has no such run (bf16 has no edge instance at all), with one run at four tiles (far offset: two tiles).
"""
import ctypes
import functools
import re

from sparsefactorization_amd._lib import tuning
from test_gpu_launch_table import B, CHAIN_L, FAMILIES, M, ROUTE_DEFAULTS, WIN_L, _confirm, _describe

__all__ = ["B", "M", "WIN_L", "CHAIN_L", "STEP_GRID", "CHAIN_GRID", "MIXER_C", "recipe", "modes", "confirm"]

# dV and dW alone: a dV cell of wide rows runs next to the chunk dW and the other way round, so each is named on its own.
# They are asked through the launch table's family of the same describe entry and element type (C is always given).
_ENTRY_OF = {"dv_f32": "win_f32", "dw_f32": "win_f32", "dv_bf16": "win_bf16", "dw_bf16": "win_bf16"}
assert not set(_ENTRY_OF) & set(FAMILIES)


def describe(family, N, L, batch, C):
    return _describe(_ENTRY_OF.get(family, family), N, L, batch, C)

# ---------------------------------------------------------------- the step kernels: (TG, R, NT) per family
_TG_F32 = [1 << t for t in range(0, 6 + 1)]    # fwd_window_launch.h: kWinTgsMax = 6, every TGS at 256 threads
_TG_BF16 = [1 << t for t in range(0, 4 + 1)]   # fwd_window_launch.h: kWinTgsMaxBf16 = 4 (bwd_window_launch.h: kFusedBf16TgsMax = 4)
_WIDE = (1 << 3, 2, 1024)                      # fwd_window_launch.h: kWideTgs = 3, kWideThreads = 1024
_ROWS4 = [(1 << t, 4, 256) for t in (2, 3, 4)]  # fwd_window_launch.h: win_rows4_compiled (PSF_ROWS4_TGS_MIN 2 .. MAX 4)
_DV_MID = [(1 << t, 1, 512) for t in (0, 1)]   # bwd_window_launch.h: kDvMidThreads = 512, kDvMidTgsMax = 1
_CHUNK = [(1 << t, 1, 256) for t in (3, 4)]    # bwd_window_launch.h: kDwChunkTgsMin = 3, kDwChunkTgsMax = 4
_TG_FUSED = [1 << t for t in range(0, 5 + 1)]  # bwd_window_launch.h: kFusedTgsMax = 5 (aligned and edge instance)

STEP_GRID = {
    "fwd_f32": [(tg, 2, 256) for tg in _TG_F32] + _ROWS4 + [_WIDE],
    "dv_f32": [(tg, 2, 256) for tg in _TG_F32] + _DV_MID + [_WIDE],
    "dw_f32": [(tg, 1, 256) for tg in _TG_F32],   # dW: 256 threads x 1 row (bwd_window_launch.h)
    "chunk_f32": _CHUNK,
    "fused_f32": [(tg, 1, 256) for tg in _TG_FUSED],
    "fused_edge_f32": [(tg, 1, 256) for tg in _TG_FUSED],
    "fwd_bf16": [(tg, 2, 256) for tg in _TG_BF16],
    "dv_bf16": [(tg, 2, 256) for tg in _TG_BF16],
    "dw_bf16": [(tg, 1, 256) for tg in _TG_BF16],
    "fused_bf16": [(tg, 1, 256) for tg in _TG_BF16],
}
KERNEL = {"fwd": "chord_fwd_win_k", "dv": "chord_dv_win_k", "dw": "chord_dw_win_k", "chunk": "chord_dw_chunk_k",
          "fused": "chord_bwd_fused_k", "fused_edge": "chord_bwd_fused_edge_k"}
STEP_TOTALS = {"f32": 714, "bf16": 340}  # cells: configurations x 17 link counts (kWinLmin = 4 .. kWinLmax = 20)


def kind(family):
    return family.rsplit("_", 1)[0]


def elem(family):
    return family.rsplit("_", 1)[1]


def elem_bytes(family):
    return 4 if elem(family) == "f32" else 2


def instance(family, config, L):
    """The instance as describe prints it (psf_chord.hip: print_win; the fused steps have one row per thread and print no R)."""
    tg, r, nt = config
    rows = "" if kind(family).startswith("fused") else f"R={r},"
    return f"{KERNEL[kind(family)]}<{elem(family)},L={L},TG={tg},{rows}NT={nt}>"


def tile_rows(config):
    tg, r, nt = config
    return nt // tg * r  # fwd_window_launch.h: win_tile_rows


def near_links(config, L):
    """psf_chord.hip: near_links — offsets 0, 1, 2, .., 2^(KN-2) <= TR."""
    return min(L, tile_rows(config).bit_length() + 1)


def channels(family, config):
    """Rows of exactly one 16-byte group per lane: 4 << tgs (f32), 8 << tgs (bf16); the 1024-thread chunks take C >= 64."""
    if config == _WIDE:
        return 64
    return (4 if elem(family) == "f32" else 8) * config[0]


def knobs(family, config):
    """The route knobs that reach a configuration (on top of ROUTE_DEFAULTS)."""
    k, f32, C = kind(family), elem(family) == "f32", channels(family, config)
    out = {}
    if k == "fwd" and f32:
        if config == _WIDE:
            out["fwd_wide"] = 1
        elif C >= 64:
            out["fwd_wide"] = 4        # whole rows: neither the 1024-thread nor the 256-thread chunks
        if config[1] == 4:
            out["fwd_rows"] = 4
    elif k in ("dv", "dw", "chunk"):
        out["bwd_fused"] = 0
        if k == "dv" and f32:
            if config == _WIDE:
                out["fwd_wide"] = 1
            out["dv_threads"] = 0 if config[2] == 512 else 1
        if k == "dw" and f32:
            out["dw_variant"] = 1      # rows of >= 32 channels stay on chord_dw_win_k
        if k == "chunk":
            out["dw_tgs"] = 4 if config[0] == 8 else 5
    elif k == "fused":
        out["bwd_fused"] = 2
    elif k == "fused_edge":
        out["bwd_fused"] = 1
    return out


# what a family's cell runs; "full" (forward, MODE 0: an off-grid last offset) only where the aligned launch has a far link
# and "far" (fused steps: four tiles, the far offset two tiles) likewise
MODES = {"fwd": ("aligned", "edge", "split", "full", "shift"), "dv": ("full", "edge", "shift"), "dw": ("full", "edge", "shift"),
         "chunk": ("full", "edge", "shift"), "fused": ("aligned", "far"), "fused_edge": ("edge", "shift")}
_TILES = {"aligned": "tiles=full, aligned", "edge": "tiles=edge", "split": "tiles=full+ragged", "full": "tiles=full, aligned",
          "shift": "tiles=full, aligned"}


def modes(family, config, L):
    needs_far = {"fwd": "full", "fused": "far"}.get(kind(family))
    return tuple(m for m in MODES[kind(family)] if m != needs_far or near_links(config, L) < L)


def _mode_knobs(family, config, mode):
    k = knobs(family, config)
    if kind(family) == "fwd" and mode == "split":
        k["fwd_split"] = 2  # full tiles on MODE 0 / 2, the ragged tail on the edge instance, in two launches
    return k


def _must(family, config, L, mode):
    """The strings describe has to show for a cell's run. describe takes every operand as 16-byte aligned and the offsets as
    the chord pattern's, so "shift" and the forward's "full" are confirmed on the aligned launch of the same shape."""
    also = [instance(family, config, L)]
    if kind(family) == "fwd":
        also.append(_TILES[mode])
    return tuple(also)


@functools.lru_cache(maxsize=None)
def _base_n(family, config, L):
    """The smallest N of whole tiles at which describe names the cell's instance (forward: with aligned full tiles). The fused
    edge step: the aligned step's N (bwd_fused = 2), which the edge instance takes one row further on or with a W off its
    16-byte boundary."""
    fam, TR = ("fused_" + elem(family) if kind(family) == "fused_edge" else family), tile_rows(config)
    mode = MODES[kind(fam)][0]
    must = _must(fam, config, L, mode)
    C = channels(fam, config)
    with tuning(**{**ROUTE_DEFAULTS, **_mode_knobs(fam, config, mode)}):
        for N in range(1, 2 * TR + 2):
            if N % TR == 0 and all(x in describe(fam, N, L, B, C) for x in must):
                return N
    return None


@functools.lru_cache(maxsize=None)
def recipe(family, config, L, mode):
    """(B, N, C, knobs) of a step cell's run, or None where describe does not name the cell's instance there."""
    assert mode in modes(family, config, L), (family, config, L, mode)
    N = _base_n(family, config, L)
    if N is None:
        return None
    C, kn = channels(family, config), {**ROUTE_DEFAULTS, **_mode_knobs(family, config, mode)}
    with tuning(**kn):
        if mode == "edge":
            N += 1
        elif mode == "far":
            N *= 2
        elif mode == "split":
            # one row more where that keeps B N L a whole number of 16-byte groups (else every tile takes the edge instance:
            # psf_chord.hip, pick_window), otherwise the first ragged N that does
            N = next((n for n in range(N + 1, N + tile_rows(config)) if _TILES[mode] in describe(family, n, L, B, C)), N + 1)
        # (the edge step with W one element off: describe cannot see it; the same shape one row longer names the instance)
        s = describe(family, N + (kind(family) == "fused_edge" and mode == "shift"), L, B, C)
    if not all(x in s for x in _must(family, config, L, mode)):
        return None
    if kind(family) == "fwd" and int(re.search(r"far=(\d+)", s).group(1)) != L - near_links(config, L):
        return None
    return B, N, C, kn


def confirm(family, config, L, mode, N, C):
    """Under the cell's knobs (set by the caller): describe names the cell's instance for this run."""
    edge_shift = kind(family) == "fused_edge" and mode == "shift"
    if family in _ENTRY_OF:
        s = describe(family, N, L, B, C)
        assert all(x in s for x in _must(family, config, L, mode)), f"{family} N={N} L={L}: {s}"
        return s
    s = _confirm(family, N + edge_shift, L, _must(family, config, L, mode), B, C)
    if edge_shift:  # ... and the aligned shape itself is the aligned step's: only W's address sends it to the edge instance
        assert instance("fused_" + elem(family), config, L) in describe(family, N, L, B, C), (family, config, L)
    return s


def step_cells(families=None):
    return [(f, c, L) for f in (families or STEP_GRID) for c in STEP_GRID[f] for L in WIN_L]


def cell_id(family, config, L):
    return f"{family}-TG{config[0]}-R{config[1]}-NT{config[2]}-L{L}"


# ---------------------------------------------------------------- the one-launch forward chains
# fwd_chain_lds_inst.hip: launch_R — chord_chain_lds_k<L, CC, R, RES, NTMAX>: R = 1 (512), R = 2 on <= 512 threads (512),
# R = 2 on more (1024), R = 3 on <= 768 threads (768); chord_chain_rows_k<G = 2, R = 2> and <G = 1, R = kChainLongRowsPerThread = 5>
CHAIN_GRID = [("lds", cc, r, big_wg) for cc in (1, 2) for r, big_wg in ((1, None), (2, False), (2, True), (3, None))] + \
             [("rows", 2, 2, None), ("rows", 1, 5, None)]
# fwd_chain_lds_inst.hip: plan_chain_lds — three rows per thread stop at L = 14 in f32 and at kChainLdsRows3LmaxBf16 = 18 in bf16
CHAIN_ROWS3_LMAX = {"f32": 14, "bf16": 18}
CHAIN_N_MAX = 2113  # fwd_chain_lds_launch.h: kChainLdsMaxSlots + 1, the first N of chord_chain_rows_k<G = 1>


def chain_refused(el, config, L):
    """The cells that plan_chain_lds turns away: decided by its rule, not by a run."""
    return config[0] == "lds" and config[2] == 3 and L > CHAIN_ROWS3_LMAX[el]


def chain_family(el, config):
    return ("chain_" if config[0] == "lds" else "rows_") + el


def chain_knobs(config):
    """chain_fused = 2 takes the one launch wherever it fits; chain_cc = 1 keeps one channel group per workgroup, 2 takes two
    and the whole-row instances beyond 1056 / 2112 rows."""
    return {**ROUTE_DEFAULTS, "chain_fused": 2, "chain_cc": 1 if config[:2] == ("lds", 1) else 2}


def chain_channels(el, config):
    return (4 if el == "f32" else 8) * config[1]  # one 16-byte group per CC / G


def chain_shows(el, config, L, s):
    """Whether a describe string names the chain cell: kernel, CC / G, R and, for chord_chain_lds_k, the side of 512 threads."""
    which, cc, r, big_wg = config
    if which == "rows":
        return f"chord_chain_rows_k<{el},L={L},G={cc},R={r}>" in s
    if f"chord_chain_lds_k<{el},L={L},CC={cc},R={r}>" not in s:
        return False
    return big_wg is None or (int(re.search(r", (\d+) threads,", s).group(1)) > 512) == big_wg  # (R = 2 alone has two NTMAX)


@functools.lru_cache(maxsize=None)
def _chain_n(el, config, L):
    fam, C = chain_family(el, config), chain_channels(el, config)
    with tuning(**chain_knobs(config)):
        for N in range(1, CHAIN_N_MAX + 1):
            if chain_shows(el, config, L, describe(fam, N, L, B, C)):
                return N
    return None


def chain_recipe(el, config, L):
    """(B, N, C, knobs) of a chain cell: the smallest N that takes it. A refused cell: the N of the same configuration at
    the last link count the planner accepts, where describe must then name another kernel."""
    N = _chain_n(el, config, CHAIN_ROWS3_LMAX[el] if chain_refused(el, config, L) else L)
    return None if N is None else (B, N, chain_channels(el, config), chain_knobs(config))


def chain_cells():
    return [(el, c, L) for el in ("f32", "bf16") for c in CHAIN_GRID for L in CHAIN_L]


def chain_id(el, config, L):
    which, cc, r, big_wg = config
    return f"{which}_{el}-{'G' if which == 'rows' else 'CC'}{cc}-R{r}{'-wide' if big_wg else ''}-L{L}"


# ---------------------------------------------------------------- the step kernel that computes its own W tile
MIXER_C = (4, 8, 16, 32)               # fwd_mlp_step_inst.hip is built with -DPSF_TGS=0..3: rows of 4 << TGS channels
MIXER_L = range(4, 21)                 # fwd_mlp_step_launch.h: kMlpStepLmin = 4 .. kMlpStepLmax = 20
MIXER_E = MIXER_H = 8
MIXER_KINDS = ("x", "w")


def mixer_tile_rows(C):
    tgs = (C // 4).bit_length() - 1
    return (256 >> tgs) * (1 if tgs == 0 else 2)  # fwd_mlp_step_launch.h: mlp_step_tile_rows — 256, 256, 128, 64


def mixer_lengths(C):
    """Two tiles (the aligned instance) and one row more (the predicated one)."""
    return 2 * mixer_tile_rows(C), 2 * mixer_tile_rows(C) + 1


def mixer_plan(N, C, L):
    """psf_mixer_fwd_plan for g and M link MLPs of MIXER_H hidden rows (under the caller's knobs): 1 = the per-step kernels."""
    from sparsefactorization_amd import _lib
    hs = (ctypes.c_int32 * (M + 1))(*[MIXER_H] * (M + 1))
    return _lib.load().psf_mixer_fwd_plan(N, MIXER_E, M, hs, C, L)


def mixer_case(kind_, N, C, L):
    import x3_exact as xe
    return xe.mixer_case(kind_, B, N, MIXER_E, MIXER_H, C, L, M, seed=N + MIXER_E + MIXER_H)


def mixer_cells():
    return [(C, L) for C in MIXER_C for L in MIXER_L]
