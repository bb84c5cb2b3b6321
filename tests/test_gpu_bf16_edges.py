"""GPU: the hardening suite of the f32 chord steps, carried over to the bf16 steps (forward, dV, dW, the fused dV + dW step).

  1. guard bands: every output a view into an int16 arena of a NaN bit pattern, at element shifts 0, 1 and 4;
  2. stale LDS: every step right after launches that leave NaN in the LDS of every CU (f32 and bf16 layouts);
  3. dW pinned: bit for bit on integer data whose sums are exact in any order, and on random data inside the float64
     bracket bf16_rne(exact -+ C 2^-24 sum|dZ V|) — no other tolerance;
  4. NaN, Inf, signed zeros and the ends of f32's product range on the window and generic backward routes;
  5. limit shapes: L = 4 and L = 20, N C 2 bytes at 2^31 (where the window kernel leaves its scalar block addresses), batch
     elements beyond 2^31 bytes;
  6. a dispatcher sweep over random (B, N, L, C).

Expected values come from oracle.chord_oracle (f32 on the upcast inputs, rounded once) or from float64 arithmetic on the
definition, never from another route of the library. Where the operands are aligned the route is asserted with
psf_describe_fwd / psf_describe_bwd, so a case cannot silently stop covering the kernel it was written for. The tools
(tests/bf16_edges.py) are tested on the CPU by test_bf16_edges_host.py.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bf16_edges as be
from oracle import chord_oracle as oc
from sparsefactorization_amd._lib import tuning

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- routes
def WIN(tg, tiles=None):
    return ("win", tg, tiles)


def GEN(vec):
    return ("gen", vec, None)


FULL, EDGE = "full, aligned (scalar block addresses)", "edge"

# (B, N, L, C): (forward, dW, dV, TG of the fused step under bwd_fused = 2 or None). Tile rows are 512/256/128/64/32 for the
# forward and dV and 256/128/64/32/16 for dW at C = 8/16/32/64/128; the window needs N >= 2 tiles.
ROUTES = {
    (2, 1024, 11, 8): (WIN(1, FULL), WIN(1), WIN(1), 1),         # full tiles
    (2, 1025, 11, 8): (WIN(1, EDGE), WIN(1), WIN(1), None),      # ragged last tile; N L odd: dW all-edge
    (3, 600, 10, 8): (GEN(8), WIN(1), GEN(8), None),             # dW on the window kernel, forward and dV generic
    (2, 515, 9, 24): (WIN(4, EDGE), WIN(4), WIN(4), None),       # C / 8 = 3: idle lanes
    (2, 300, 9, 40): (WIN(8, EDGE), WIN(8), WIN(8), None),       # C / 8 = 5: idle lanes on all three window kernels
    (2, 54, 8, 88): (GEN(8), WIN(16), GEN(8), None),             # window dW with 5 of 16 lanes idle
    (2, 2048, 12, 16): (WIN(2, FULL), WIN(2), WIN(2), 2),
    (2, 257, 12, 32): (WIN(4, EDGE), WIN(4), WIN(4), None),
    (3, 130, 7, 64): (WIN(8, EDGE), WIN(8), WIN(8), None),
    (2, 64, 6, 128): (WIN(16, FULL), WIN(16), WIN(16), 16),
    (2, 67, 6, 128): (WIN(16, EDGE), WIN(16), WIN(16), None),
    (1, 300, 12, 264): (WIN(16, EDGE), GEN(8), WIN(16), None),   # 128-channel chunks plus an 8-channel tail; dW generic
    (2, 777, 22, 8): (GEN(8), GEN(8), GEN(8), None),             # L beyond the window kernels
    (2, 300, 9, 6): (GEN(1), GEN(1), GEN(1), None),
    (2, 5, 3, 3): (GEN(1), GEN(1), GEN(1), None),
    (1, 1, 1, 8): (GEN(8), GEN(8), GEN(8), None),
    (2, 777, 3, 8): (GEN(8), GEN(8), GEN(8), None),              # L below the window kernels
    (1, 4097, 13, 8): (WIN(1, EDGE), WIN(1), WIN(1), None),
    # parts 3 to 5
    (2, 1025, 11, 32): (WIN(4, EDGE), WIN(4), WIN(4), None),
    (2, 300, 9, 24): (WIN(4, EDGE), WIN(4), WIN(4), None),
    (2, 256, 9, 32): (WIN(4, FULL), WIN(4), WIN(4), 4),
    (3, 1024, 11, 8): (WIN(1, FULL), WIN(1), WIN(1), 1),
    (2, 513, 10, 128): (WIN(16, EDGE), WIN(16), WIN(16), None),
    (2, 1100, 11, 256): (WIN(16, EDGE), GEN(8), WIN(16), None),
    (3, 8, 4, 8): (GEN(8), GEN(8), GEN(8), None),
    (2, 1024, 4, 8): (WIN(1, FULL), WIN(1), WIN(1), 1),
    (1, 1 << 19, 20, 8): (WIN(1, FULL), WIN(1), WIN(1), 1),
    (1, (1 << 16) + 1, 17, 8): (WIN(1, EDGE), WIN(1), WIN(1), None),
    (2, 1 << 19, 20, 1024): (WIN(16, FULL), GEN(8), WIN(16), None),
    (1, 1 << 19, 20, 2048): (WIN(16, "full"), GEN(8), WIN(16), None),  # N C 2 == 2^31: no scalar block addresses
}
STEP_SHAPES = list(ROUTES)[:18]


def _kernel(what, L, spec):
    kind, n, _ = spec
    if kind == "gen":
        return f"chord_{what}_generic_k<bf16,VEC={n}>"
    return f"chord_{what}_win_k<bf16,L={L},TG={n},R={1 if what == 'dw' else 2},NT=256>"


def _assert_routes(B, N, L, C):
    """The kernels of aligned operands at this shape under the current knobs are the ones the case was written for."""
    from sparsefactorization_amd import _lib
    fwd, dw, dv, fused = ROUTES[(B, N, L, C)]
    generic = GEN(8 if C % 8 == 0 else 1)
    if _lib.get_tuning("fwd_variant") == 1:
        fwd = generic
    if _lib.get_tuning("bwd_variant") == 1:
        dw, dv, fused = generic, generic, None
    name = _lib.describe_fwd(B, N, L, C, elem_bytes=2)
    assert name.startswith(_kernel("fwd", L, fwd)), name
    if fwd[2] is not None:
        assert name.endswith("tiles=" + fwd[2]), name
    name = _lib.describe_bwd(B, N, L, C, elem_bytes=2)
    if fused is not None and _lib.get_tuning("bwd_fused") == 2:
        assert name.startswith(f"chord_bwd_fused_k<bf16,L={L},TG={fused},NT=256> "), name
    else:
        assert name == _kernel("dw", L, dw) + " + " + _kernel("dv", L, dv), name


# ---------------------------------------------------------------- references (computed once per shape, read-only)
@functools.lru_cache(maxsize=None)
def _ref(B, N, L, C, offsets=None):
    W, V = be.normal_case((B, N, L), 1, 0.5), be.normal_case((B, N, C), 2)
    R, dZ = be.normal_case((B, N, C), 3), be.normal_case((B, N, C), 4)
    off = None if offsets is None else list(offsets)
    out = oc.spmul_fwd(W, V, off)
    dF, dV = oc.spmul_bwd(dZ, W, V, off)
    exact, absum = be.dw_sums(dZ, V, L, off)
    lo, hi = be.dw_bracket(exact, absum, C)
    r = SimpleNamespace(W=W, V=V, R=R, dZ=dZ, out=be.rne_bits(out), outR=be.rne_bits(out + R), dV=be.rne_bits(dV), dF=dF, lo=lo,
                        hi=hi, loose=float((lo != hi).mean()))
    for a in vars(r).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def _bt(a, gpu):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(torch.bfloat16).to(gpu)  # (a copy: the references are read-only)


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _assert_bits(got_bits, want_bits, what):
    bad = be.same_bits(got_bits.ravel(), want_bits.ravel())
    assert bad == 0, f"{what}: {bad} of {want_bits.size} elements differ from the oracle's bits"


def _assert_dw_ref(got_bits, ref, what):
    """Bracket (b) with the bounds computed once per shape."""
    got = be.bits_f32(got_bits).reshape(ref.lo.shape)
    with np.errstate(invalid="ignore"):
        bad = int((~((ref.lo <= got) & (got <= ref.hi))).sum())
    assert ref.loose <= be.MAX_LOOSE, f"{what}: {ref.loose:.1%} of the brackets hold more than one bf16 value"
    assert bad == 0, f"{what}: {bad} of {got.size} elements outside bf16_rne(exact -+ C 2^-24 sum|dZ V|)"


def _fwd(W, V, R, out, B, N, L, C, offsets=None):
    from sparsefactorization_amd import _lib
    rc = _lib.load().psf_chord_spmm_fwd_bf16(W.data_ptr(), V.data_ptr(), None if R is None else R.data_ptr(), out.data_ptr(), B, N, L, C,
                                             N * C, _lib.offsets_array(offsets), _lib.stream_ptr(W.device))
    _lib.check(rc, "psf_chord_spmm_fwd_bf16")


# ---------------------------------------------------------------- 1. guard bands
def _arena(shape, gpu, shift):
    """(arena, bf16 view of `shape` at element shift `shift`, (lo, hi)): the sentinel everywhere."""
    total, lo, hi = be.arena_span(int(np.prod(shape)), shift)
    buf = torch.full((total,), be.SENTINEL, dtype=torch.int16, device=gpu)
    view = buf[lo:hi].view(torch.bfloat16).view(*shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (2 * shift) % 16
    return buf, view, (lo, hi)


def _operand(a, gpu, shift):
    _, view, _ = _arena(a.shape, gpu, shift)
    view.copy_(_bt(a, gpu))
    return view


def _inside(arena, what):
    """The output's bits after the bands were found intact and every element written."""
    buf, _, (lo, hi) = arena
    a = buf.cpu().numpy().view(np.uint16)
    below, above, unwritten = be.band_report(a, lo, hi)
    assert below == 0 and above == 0, f"{what}: {below} elements written below the output, {above} above it"
    assert unwritten == 0, f"{what}: {unwritten} elements of the output were never written"
    return a[lo:hi]


def _guard_band_case(gpu, B, N, L, C, wshift, vshift, offsets=None):
    from sparsefactorization_amd.chord import _launch_bwd
    ref = _ref(B, N, L, C, offsets)
    off = None if offsets is None else list(offsets)
    Wt = _operand(ref.W, gpu, wshift)
    Vt, Rt, dZt = (_operand(a, gpu, vshift) for a in (ref.V, ref.R, ref.dZ))
    tag = f"shifts W {wshift} V {vshift}"
    for res, want in ((Rt, ref.outR), (None, ref.out)):
        o = _arena((B, N, C), gpu, vshift)
        _fwd(Wt, Vt, res, o[1], B, N, L, C, off)
        _assert_bits(_inside(o, f"out, {tag}"), want, f"out, residual {res is not None}, {tag}")
    for fused, want_dw, want_dv in ((0, True, True), (2, True, True), (0, True, False), (0, False, True)):
        gw = _arena((B, N, L), gpu, wshift) if want_dw else None
        gv = _arena((B, N, C), gpu, vshift) if want_dv else None
        with tuning(bwd_fused=fused):
            if wshift == vshift == 0 and offsets is None and want_dw and want_dv:
                _assert_routes(B, N, L, C)
            _launch_bwd(dZt, Wt, Vt, gw and gw[1], gv and gv[1], B, N, L, C, N * C, off)
        what = f"bwd_fused={fused} dW={want_dw} dV={want_dv}, {tag}"
        if gv:
            _assert_bits(_inside(gv, "dV, " + what), ref.dV, "dV, " + what)
        if gw:
            _assert_dw_ref(_inside(gw, "dW, " + what), ref, "dW, " + what)


# all operands and results at the same shift; then W and dW alone off their boundary (the window kernels' misaligned W tile,
# the dW kernel's element-wise ends) with the row operands aligned
SHIFTS = [(0, 0), (1, 1), (4, 4), (1, 0), (4, 0)]


@pytest.mark.parametrize("wshift,vshift", SHIFTS)
@pytest.mark.parametrize("B,N,L,C", STEP_SHAPES)
def test_steps_stay_inside_their_outputs(gpu, B, N, L, C, wshift, vshift):
    _guard_band_case(gpu, B, N, L, C, wshift, vshift)


@pytest.mark.parametrize("wshift,vshift", SHIFTS)
def test_steps_with_far_offsets_off_the_tile_stay_inside_their_outputs(gpu, wshift, vshift):
    """Chord near links (the window kernels) with far offsets that are no multiples of the tile."""
    off = tuple([0] + [1 << k for k in range(9)] + [777, -3001])
    _guard_band_case(gpu, 2, 4096, 12, 8, wshift, vshift, off)


# ---------------------------------------------------------------- 2. stale LDS
_poison_cache = {}


def _poison(gpu):
    """NaN in the LDS of every CU: the two f32 launches of test_gpu_stale_lds.py, then the bf16 LDS-resident chain on an all-NaN
    V0, so that both element layouts are left behind."""
    import sparsefactorization_amd as sfa
    from test_gpu_stale_lds import _poison as poison_f32
    poison_f32(gpu)
    if not _poison_cache:
        B, N, C, L = 2048, 512, 16, 10
        assert "chord_chain_lds_k<bf16" in sfa._lib.describe_chain_fwd(B, N, L, C, 2, elem_bytes=2)
        _poison_cache["bf16"] = ([torch.zeros(B, N, L, device=gpu, dtype=torch.bfloat16) for _ in range(2)],
                                 torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16))
    with torch.no_grad():
        Ws, V0 = _poison_cache["bf16"]
        out = sfa.chord_chain(Ws, V0, True)
        assert bool(torch.isnan(out[0, 0, 0]))


@pytest.mark.parametrize("B,N,L,C", STEP_SHAPES)
def test_steps_after_nan_in_every_lds(gpu, B, N, L, C):
    from sparsefactorization_amd.chord import _launch_bwd
    ref = _ref(B, N, L, C)
    Wt, Vt, Rt, dZt = (_bt(a, gpu) for a in (ref.W, ref.V, ref.R, ref.dZ))
    _assert_routes(B, N, L, C)
    for res, want in ((Rt, ref.outR), (None, ref.out)):
        out = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
        _poison(gpu)
        _fwd(Wt, Vt, res, out, B, N, L, C)
        _assert_bits(_bits(out), want, f"out, residual {res is not None}")
    for fused in (0, 2):
        gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
        gV = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
        with tuning(bwd_fused=fused):
            _assert_routes(B, N, L, C)
            _poison(gpu)
            _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, N * C, None)
        _assert_bits(_bits(gV), ref.dV, f"dV, bwd_fused={fused}")
        _assert_dw_ref(_bits(gW), ref, f"dW, bwd_fused={fused}")


# ---------------------------------------------------------------- 3. dW, pinned
@pytest.mark.parametrize("shape,fused,broadcast", be.KNOWN_ANSWER)
def test_dw_known_answers_bit_for_bit(gpu, shape, fused, broadcast):
    """Integers in [-15, 15]: every partial sum in any order is an exact f32 integer, so dW has one correct value."""
    from sparsefactorization_amd.chord import _launch_bwd
    B, N, L, C = shape
    dZ, V = be.known_answer_operands(shape, broadcast)
    W = be.normal_case((B, N, L), 52)
    exact, _ = be.dw_sums(dZ, V, L)
    assert np.abs(exact).max() < 2.0 ** 24
    Wt, Vt, dZt = _bt(W, gpu), _bt(V, gpu), _bt(dZ, gpu)
    gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
    gV = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
    with tuning(bwd_fused=fused):
        _assert_routes(B, N, L, C)
        _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, 0 if broadcast else N * C, None)
    _assert_bits(_bits(gW), be.rne_bits(exact.astype(np.float32)), "dW")
    _assert_bits(_bits(gV), be.rne_bits(oc.spmul_bwd(dZ, W, np.ascontiguousarray(np.broadcast_to(V, (B, N, C))))[1]), "dV")


@pytest.mark.parametrize("bwd_variant,fused", [(0, 0), (0, 2), (1, 0)])
@pytest.mark.parametrize("B,N,L,C", [(2, 1024, 11, 8), (2, 515, 9, 24), (2, 513, 10, 128), (2, 1100, 11, 256), (2, 300, 9, 6)])
def test_dw_random_data_inside_the_float64_bracket(gpu, B, N, L, C, bwd_variant, fused):
    from sparsefactorization_amd.chord import _launch_bwd
    ref = _ref(B, N, L, C)
    print(f"share of brackets with more than one value at C={C}: {ref.loose:.2%}")
    gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
    with tuning(bwd_fused=fused, bwd_variant=bwd_variant):
        _assert_routes(B, N, L, C)
        _launch_bwd(_bt(ref.dZ, gpu), _bt(ref.W, gpu), _bt(ref.V, gpu), gW, None, B, N, L, C, N * C, None)
    _assert_dw_ref(_bits(gW), ref, "dW")


# ---------------------------------------------------------------- 4. special values
@pytest.mark.parametrize("run", be.SPECIAL_RUNS)
@pytest.mark.parametrize("B,N,L,C", be.SPECIAL_SHAPES)
def test_special_values_on_every_route(gpu, B, N, L, C, run):
    """out (with and without the residual) and dV: the oracle's bits, NaN in the same places, the same sign of zero. dW: where
    no partial sum can overflow (sum|dZ V| below FLT_MAX, always so without 2^126) the oracle's NaN / +Inf / -Inf pattern
    exactly and bracket (b) on the finite elements."""
    from sparsefactorization_amd.chord import _launch_bwd
    W, V, R, dZ = be.special_operands(B, N, L, C, run)
    # the header's condition for the fused multiply-add to equal mul-then-add, on the host before anything is launched
    assert be.product_range_ok(W, V) and be.product_range_ok(W, dZ) and be.product_range_ok(dZ, V)
    with np.errstate(all="ignore"):
        out = oc.spmul_fwd(W, V)
        want_out, want_outR = be.rne_bits(out), be.rne_bits(out + R)
        dF, dV = oc.spmul_bwd(dZ, W, V)
        want_dV = be.rne_bits(dV)
        exact, absum = be.dw_sums(dZ, V, L)
    # dW elements whose partial sums stay finite in any order: all terms finite and sum|terms| (1 + C 2^-24) below FLT_MAX
    with np.errstate(invalid="ignore"):
        safe = np.isfinite(absum) & (absum * (1 + C * 2.0 ** -24) < be.FLT_MAX)
    if run == "dz":  # 2^126 in dZ: a sum may overflow in one order and not in another; a NaN term gives NaN in any order
        ordered = np.isnan(absum) | safe
    else:            # no overflow anywhere: NaN and Inf come from the operands alone, the same in any order
        assert bool((safe | ~np.isfinite(absum)).all())
        ordered = np.ones_like(safe)
    assert safe.sum() >= 8 and np.isnan(dF).any() and np.isinf(dF).any() and np.isnan(dV).any()
    Wt, Vt, Rt, dZt = (_bt(a, gpu) for a in (W, V, R, dZ))
    for variant in (0, 1):
        with tuning(fwd_variant=variant):
            _assert_routes(B, N, L, C)
            for res, want in ((None, want_out), (Rt, want_outR)):
                got = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
                _fwd(Wt, Vt, res, got, B, N, L, C)
                _assert_bits(_bits(got), want, f"out, fwd_variant={variant} residual={res is not None}")
    for bwd_variant, fused in ((0, 1), (0, 0), (0, 2), (1, 1)):
        gW = torch.zeros((B, N, L), device=gpu, dtype=torch.bfloat16)
        gV = torch.zeros((B, N, C), device=gpu, dtype=torch.bfloat16)
        with tuning(bwd_variant=bwd_variant, bwd_fused=fused):
            _assert_routes(B, N, L, C)
            _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, N * C, None)
        what = f"bwd_variant={bwd_variant} bwd_fused={fused}"
        _assert_bits(_bits(gV), want_dV, "dV, " + what)
        got = be.bits_f32(_bits(gW)).reshape(B, N, L)
        for name, pat in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
            bad = int(((pat(got) != pat(dF)) & ordered).sum())
            assert bad == 0, f"dW, {what}: {name} in {bad} other places than in the oracle"
        bad, loose = be.bracket_report(_bits(gW), exact, absum, C, where=safe)
        assert loose <= be.MAX_LOOSE and bad == 0, f"dW, {what}: {bad} finite elements outside their bracket"


# ---------------------------------------------------------------- 5. limit shapes
@pytest.mark.parametrize("B,N,L,C", [(3, 8, 4, 8), (2, 1024, 4, 8), (1, 1 << 19, 20, 8), (1, (1 << 16) + 1, 17, 8)])
def test_limit_shapes(gpu, B, N, L, C):
    """L at both ends of the window kernels, the longest sequence, 2^16 + 1: forward and dV bit for bit, dW by bracket (b)."""
    from sparsefactorization_amd.chord import _launch_bwd
    ref = _ref(B, N, L, C)
    Wt, Vt, Rt, dZt = (_bt(a, gpu) for a in (ref.W, ref.V, ref.R, ref.dZ))
    for res, want in ((Rt, ref.outR), (None, ref.out)):
        out = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
        _fwd(Wt, Vt, res, out, B, N, L, C)
        _assert_bits(_bits(out), want, f"out, residual {res is not None}")
    for fused in (0, 2):
        gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
        gV = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
        with tuning(bwd_fused=fused):
            _assert_routes(B, N, L, C)
            _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, N * C, None)
        _assert_bits(_bits(gV), ref.dV, f"dV, bwd_fused={fused}")
        _assert_dw_ref(_bits(gW), ref, f"dW, bwd_fused={fused}")
    _ref.cache_clear()  # the long sequences' references are not small


@pytest.mark.parametrize("B,N,L,C", [(2, 1 << 19, 20, 1024), (1, 1 << 19, 20, 2048)])
def test_two_gigabyte_operands(gpu, B, N, L, C):
    """Each of V, the residual, dZ, out and dV is 2 GB. In the first case the last batch element starts 2^30 bytes into every
    operand and half of its rows lie beyond 2^31 bytes while N C 2 < 2^31; in the second N C 2 == 2^31 exactly, where the
    window kernels leave their scalar block addresses. Rows of the last batch element are sampled and recomputed in float64
    on the device: out and dV must have the bits of bf16_rne(float64) wherever the float64 value is further than
    L 2^-24 sum|terms| from a rounding boundary (at least 90 % of the elements), and be one of the boundary's two neighbours
    elsewhere (where a sum cancels, the slack spans several values of the fine grid near zero — 5 of 8192 sampled elements in
    the first case — and any value between the two ends passes: bf16_edges.decide_rows); dW must lie in bracket (b) (at this C most brackets hold several values: no share is asserted) and within the
    bar of test_gpu_bf16.py, one bf16 ulp plus 1e-5 max|dW|."""
    from sparsefactorization_amd.chord import _launch_bwd
    _ref.cache_clear()
    torch.cuda.empty_cache()
    _assert_routes(B, N, L, C)
    g = torch.Generator(device=gpu).manual_seed(5)
    Wt = (0.2 * torch.randn(B, N, L, device=gpu, generator=g)).to(torch.bfloat16)
    Vt, Rt, dZt = (torch.randn(B, N, C, device=gpu, generator=g, dtype=torch.bfloat16) for _ in range(3))
    out = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
    gV = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
    gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
    try:
        _fwd(Wt, Vt, Rt, out, B, N, L, C)
        _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, N * C, None)
        assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(gV).any()) and not bool(torch.isnan(gW).any())
        b = B - 1
        rows = torch.tensor(be.sample_rows(N), device=gpu)
        Wd = Wt[b].double()
        want = Rt[b, rows].double()
        absF = want.abs()
        wantV = torch.zeros(len(rows), C, dtype=torch.float64, device=gpu)
        absV = torch.zeros_like(wantV)
        wantW = torch.zeros(len(rows), L, dtype=torch.float64, device=gpu)
        absW = torch.zeros_like(wantW)
        dZr = dZt[b, rows].double()
        for k, o in enumerate(be.chord_offsets(N, L)):
            src, back = (rows + o) % N, (rows - o) % N
            Vs = Vt[b, src].double()
            t = Wd[rows, k, None] * Vs
            want, absF = want + t, absF + t.abs()
            p = dZr * Vs
            wantW[:, k], absW[:, k] = p.sum(-1), p.abs().sum(-1)
            t = Wd[back, k, None] * dZt[b, back].double()
            wantV, absV = wantV + t, absV + t.abs()
        for name, got, exact, absum in (("out", out[b, rows], want, absF), ("dV", gV[b, rows], wantV, absV)):
            wrong, share = be.decide_rows(_bits(got), exact.cpu().numpy(), L * 2.0 ** -24 * absum.cpu().numpy())
            print(f"{name}: decidable share {share:.2%}")
            assert share >= be.MIN_DECIDABLE, f"{name}: only {share:.1%} of the sampled elements are decidable"
            assert wrong == 0, f"{name}: {wrong} sampled elements are neither neighbour of bf16_rne(float64)"
        exactW, absW = wantW.cpu().numpy(), absW.cpu().numpy()
        got = _bits(gW[b, rows])
        bad, loose = be.bracket_report(got, exactW, absW, C)
        print(f"dW: share of brackets with more than one value {loose:.2%}")
        assert bad == 0, f"dW: {bad} sampled elements outside bf16_rne(exact -+ C 2^-24 sum|dZ V|)"
        nearest = be.rne64(exactW).astype(np.float64)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(nearest), 2.0 ** -126))) - 7)
        err = np.abs(be.bits_f32(got).astype(np.float64).reshape(nearest.shape) - nearest)
        assert (err <= ulp + 1e-5 * np.abs(exactW).max()).all()
    finally:
        del Wt, Vt, Rt, dZt, out, gV, gW
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- 6. dispatcher sweep
def _random_shapes(n, seed):
    """test_gpu_parity.py's draw with bf16's channel sets: 1..13, multiples of 8 up to 96, multiples of 64 up to 512, odd
    multiples of 4."""
    rng = np.random.default_rng(seed)
    shapes = []
    for _ in range(n):
        N = int(rng.choice([rng.integers(1, 64), rng.integers(64, 700), rng.integers(700, 6000)]))
        L = int(rng.integers(1, 25))
        C = int(rng.choice([rng.integers(1, 14), 8 * rng.integers(1, 13), 64 * rng.integers(1, 9), 4 * (2 * rng.integers(0, 35) + 1)]))
        B = int(rng.integers(1, 4))
        shapes.append((B, N, L, C))
    return shapes


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_shapes_forward_and_backward(gpu, seed):
    """30 random (B, N, L, C) per seed, with and without the residual: out and dV bit for bit against the oracle, dW by
    bracket (b) up to C = 256 and by the bar of test_gpu_bf16.py above."""
    from sparsefactorization_amd.chord import _launch_bwd
    from test_gpu_bf16 import _assert_dw
    for (B, N, L, C) in _random_shapes(30, 100 + seed):
        tag = f"B={B} N={N} L={L} C={C}"
        W, V = be.normal_case((B, N, L), 7 * seed + 1, 0.5), be.normal_case((B, N, C), 7 * seed + 2)
        R, dZ = be.normal_case((B, N, C), 7 * seed + 3), be.normal_case((B, N, C), 7 * seed + 4)
        Wt, Vt, Rt, dZt = (_bt(a, gpu) for a in (W, V, R, dZ))
        want = oc.spmul_fwd(W, V)
        for res, ref in ((Rt, want + R), (None, want)):
            out = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
            _fwd(Wt, Vt, res, out, B, N, L, C)
            _assert_bits(_bits(out), be.rne_bits(ref), f"out, residual {res is not None}, {tag}")
        gW = torch.full((B, N, L), float("nan"), device=gpu, dtype=torch.bfloat16)
        gV = torch.full((B, N, C), float("nan"), device=gpu, dtype=torch.bfloat16)
        _launch_bwd(dZt, Wt, Vt, gW, gV, B, N, L, C, N * C, None)
        dF, dV = oc.spmul_bwd(dZ, W, V)
        _assert_bits(_bits(gV), be.rne_bits(dV), "dV, " + tag)
        if C <= 256:
            be.assert_dw_bracket(_bits(gW), dZ, V, L, what="dW, " + tag)
        else:
            _assert_dw(gW, dF)
