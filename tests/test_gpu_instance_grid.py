"""GPU: every compiled instance of the chord step kernels, the one-launch forward chains and the mixer step kernel runs once
against the CPU oracle, bit for bit, at the smallest shape that reaches it.

tests/test_gpu_launch_table.py runs every link count L at one launch configuration per family: enough for the (L -> instance)
mapping, not for the kernels, whose compile-time geometry (near/far split, W staging loop, LDS size) depends on L and on the
configuration (lanes per row TG, rows per thread R, workgroup size NT) together. tests/instance_grid.py lists every
(kernel, L, TG, R, NT) cell and finds its shape and route knobs from the describe entries; tests/test_instance_grid_host.py
holds that table against what the library can name. Before every run describe must name the cell's own instance, so a route
change can never turn a case into a second test of a neighbour. (describe takes operands as 16-byte aligned and offsets as the
chord pattern's: the runs with a view one element off, and the forward's off-grid last offset, are confirmed on the plain
launch of the same shape; which instance a misaligned operand is sent to is the planner's rule, read in psf_chord.hip, and not
something describe can show.) The runs with views move W as well as dW, on purpose: a misaligned W sends the dV window kernel's
full tiles to its edge instance with a non-zero staging offset, as a misaligned dW does for the dW kernels.

Only bits are compared; there is no tolerance in this file. The verdicts are test_gpu_launch_table.py's: f32 the oracle's
bits, bf16 rne_bits of the oracle's f32 result, dW on the integer operands of bf16_edges.int_case (one correct answer in any
summation order). The mixer step kernel, which that module could only hold to 1e-5, takes the exact operands of
tests/x3_exact.py (mixer_case) and the verdict of test_gpu_x3_exact.py: bit-equal to the oracle's chain fed with the exact W, V0.

Cells: 714 f32 and 340 bf16 step cells (forward 187 + 85, dV 170 + 85, dW 119 + 85, chunk dW 34, fused step 102 + 85, fused
edge step 102), 380 chain cells (16 of them declined by the planner's rule and run through whatever takes them instead), 68
mixer-step cells: 1502 test ids. Measured on an MI355X: the module takes 8 s of wall time (1502 passed in 8.13 s; the slowest id,
the first, 0.19 s), so the runs of a cell stay separate launches.
"""
import numpy as np
import pytest
import torch

import bf16_edges as be
import instance_grid as ig
from oracle import chord_oracle as oc
from sparsefactorization_amd._lib import tuning
from test_gpu_launch_table import _assert_bits, _bwd_case, _chain_case, _confirm, _dev, _dtype, _fwd_case

pytestmark = pytest.mark.gpu

BAND = 64  # elements of NaN on either side of a shifted view


def _off_by_one(t):
    """(arena, view): the tensor's values in a view one element off a 16-byte boundary, inside NaN bands (the form of
    _banded_input(.., shift=1) in test_gpu_guard_bands.py)."""
    n = t.numel()
    arena = torch.full((n + 2 * BAND + 8,), float("nan"), device=t.device, dtype=t.dtype)
    view = arena[BAND + 1:BAND + 1 + n].view(t.shape)
    assert arena.data_ptr() % 16 == 0 and view.data_ptr() % 16 == t.element_size()
    view.copy_(t)
    return arena, view


def _bands_nan(arena, n):
    return bool(torch.isnan(arena[:BAND + 1]).all()) and bool(torch.isnan(arena[BAND + 1 + n:]).all())


def _fwd_shifted(gpu, eb, N, L, C, what):
    """_fwd_case with W one element off: full tiles on the edge instance, staged from a non-zero misalignment."""
    import sparsefactorization_amd as sfa
    W, V, R = be.normal_case((ig.B, N, L), 1, 0.5), be.normal_case((ig.B, N, C), 2), be.normal_case((ig.B, N, C), 3)
    ref = oc.spmul_fwd(W, V, None)
    _arena, Wd = _off_by_one(_dev(W, eb, gpu))
    for res in (None, R):
        got = sfa.chord_spmm(Wd, _dev(V, eb, gpu), None if res is None else _dev(res, eb, gpu))
        _assert_bits(got, ref if res is None else ref + res, eb, f"{what} residual={res is not None}")


def _bwd_shifted(gpu, eb, N, L, C, what, shift_dw):
    """_bwd_case with W, and where asked dW, in views one element off (the operands' exactness: _bwd_case on the same shape,
    and test_instance_grid_host.py)."""
    from sparsefactorization_amd.chord import _launch_bwd
    dZ, V, W = be.int_case((ig.B, N, C), 50 + L), be.int_case((ig.B, N, C), 51 + L), be.normal_case((ig.B, N, L), 52, 0.5)
    dF, dV = oc.spmul_bwd(dZ, W, V)
    _wa, Wd = _off_by_one(_dev(W, eb, gpu))
    gV = torch.full((ig.B, N, C), float("nan"), device=gpu, dtype=_dtype(eb))
    gW = torch.full((ig.B, N, L), float("nan"), device=gpu, dtype=_dtype(eb))
    arena = None
    if shift_dw:
        arena, gW = _off_by_one(gW)
    _launch_bwd(_dev(dZ, eb, gpu), Wd, _dev(V, eb, gpu), gW, gV, ig.B, N, L, C, N * C, None)
    _assert_bits(gW, dF, eb, f"{what} dW")
    _assert_bits(gV, dV, eb, f"{what} dV")
    assert arena is None or _bands_nan(arena, gW.numel()), f"{what}: dW written outside its view"


def _ids(cells, fn):
    return [fn(*c) for c in cells]


# ---------------------------------------------------------------- a. the step kernels
_FWD = ig.step_cells(["fwd_f32", "fwd_bf16"])
_BWD = ig.step_cells([f for f in ig.STEP_GRID if ig.kind(f) != "fwd"])


@pytest.mark.parametrize("family,config,L", _FWD, ids=_ids(_FWD, ig.cell_id))
def test_forward_cell(gpu, family, config, L):
    """With and without residual: aligned tiles; one row more in one launch (edge instance); a ragged length in two launches
    (full tiles, then the tail on the edge instance); where the aligned launch has a far link, the last offset off the tile grid
    (MODE 0 on every tile); the aligned length with W one element off (full tiles on the edge instance, mis != 0)."""
    from sparsefactorization_amd import _lib
    eb = ig.elem_bytes(family)
    for mode in ig.modes(family, config, L):
        _B, N, C, knobs = ig.recipe(family, config, L, mode)
        what = f"{ig.instance(family, config, L)} N={N} C={C} {mode}"
        with tuning(**knobs):
            ig.confirm(family, config, L, mode, N, C)
            if mode == "shift":
                _fwd_shifted(gpu, eb, N, L, C, what)
                continue
            off = None
            if mode == "full":
                off = _lib.chord_offsets(N, L)
                off[-1] = (off[-1] + 1) % N
            _fwd_case(gpu, eb, N, L, C, off, what)


@pytest.mark.parametrize("family,config,L", _BWD, ids=_ids(_BWD, ig.cell_id))
def test_backward_cell(gpu, family, config, L):
    """dV / dW window kernels and the chunk dW: full tiles, one row more, W and dW in views one element off. The fused step: its
    aligned shape (two tiles: every far offset is 0) and, where it has a far link, four tiles (the far offset is two tiles). The
    fused edge step: one row more, and the aligned shape with W one element off."""
    eb = ig.elem_bytes(family)
    for mode in ig.modes(family, config, L):
        _B, N, C, knobs = ig.recipe(family, config, L, mode)
        what = f"{ig.instance(family, config, L)} N={N} C={C} {mode}"
        with tuning(**knobs):
            ig.confirm(family, config, L, mode, N, C)
            if mode == "shift":
                _bwd_shifted(gpu, eb, N, L, C, what, shift_dw=ig.kind(family) != "fused_edge")
            else:
                _bwd_case(gpu, eb, ig.B, N, L, C, what)


# ---------------------------------------------------------------- b. the one-launch forward chains
_CHAIN = ig.chain_cells()


@pytest.mark.parametrize("el,config,L", _CHAIN, ids=_ids(_CHAIN, ig.chain_id))
def test_chain_cell(gpu, el, config, L):
    """Residual and not (_chain_case). Where plan_chain_lds declines three rows per thread (f32: L > 14, bf16: L > 18) describe
    must name another kernel, and the result still carries the oracle's bits."""
    eb = 4 if el == "f32" else 2
    _B, N, C, knobs = ig.chain_recipe(el, config, L)
    fam = ig.chain_family(el, config)
    with tuning(**knobs):
        s = ig.describe(fam, N, L, ig.B, C)
        if ig.chain_refused(el, config, L):
            assert "chord_chain" not in s and "_k<" in s, s
        else:
            _confirm(fam, N, L, (), ig.B, C)
            assert ig.chain_shows(el, config, L, s), s
        _chain_case(gpu, eb, N, L, C, f"{ig.chain_id(el, config, L)} N={N} C={C} [{s.split('>')[0]}>]")


# ---------------------------------------------------------------- c. the step kernel that computes its own W tile
_MIXER = ig.mixer_cells()


@pytest.mark.parametrize("C,L", _MIXER, ids=[f"C{C}-L{L}" for C, L in _MIXER])
def test_mixer_step_cell(gpu, C, L):
    """chord_fwd_mlp_k<L, TGS, RES, EDGE>: two tiles (the aligned instance) and one row more (the predicated one), residual and
    not, on exact operands: fused_mixer.mixer_forward equals the oracle's chain fed with the exact W_m and V0, bit for bit."""
    from sparsefactorization_amd import fused_mixer
    from test_gpu_x3_exact import _blocks, _eq
    for N in ig.mixer_lengths(C):
        rows, cols = oc.chord_indices(N, L)
        for kind in ig.MIXER_KINDS:
            case = ig.mixer_case(kind, N, C, L)  # exact: test_instance_grid_host.py
            blocks = _blocks(gpu, case)
            g, fs = blocks[0], blocks[1:]
            ys = [y.astype(np.float32).reshape(ig.B, N, -1) for y in case.reference()["Y"]]
            x = torch.from_numpy(case.X.reshape(ig.B, N, ig.MIXER_E)).to(gpu)
            with tuning(mixer_lds=0), torch.no_grad():
                assert ig.mixer_plan(N, C, L) == 1 and fused_mixer.covered(x, g, fs)
                for residual in (False, True):
                    want = oc.chain(np.stack([rows, cols]), np.stack(ys[1:]), ys[0], residual)[-1]
                    _eq(fused_mixer.mixer_forward(x, g, fs, residual), want, f"mixer C={C} L={L} N={N} {kind} residual={residual}")
