"""CPU self-tests of the cases of test_gpu_wide_mlp_edges.py (tests/wide_cases.py) and of the wide plan itself.

Without a GPU they show four things. Agreement: the plain-Python mirror of make_wide_plan gives the byte counts of the three
psf_mlp_wide_* size functions (host-only calls) on a grid that holds every limit and every refusal. The split-K property:
every split that the plan hands the weight-gradient GEMM has a K range — on the mirror for every token count and tile count,
and on the library itself, whose split count is read back from psf_mlp_wide_bwd_workspace. Reach: the case table holds the
limits it names. The canaries: one write into a band, one unwritten element and one byte outside a scratch area are
reported.
"""
import ctypes

import numpy as np
import pytest
import torch

import wide_cases as wc
import x3_exact as xe


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _sizes(lib, T, E, layers):
    K = len(layers)
    h = (ctypes.c_int32 * max(K, 1))(*[hh for hh, _ in layers])
    O = (ctypes.c_int32 * max(K, 1))(*[oo for _, oo in layers])
    return tuple(f(T, E, K, h, O) for f in (lib.psf_mlp_wide_saved_bytes, lib.psf_mlp_wide_fwd_workspace, lib.psf_mlp_wide_bwd_workspace))


def _mirror(T, E, layers):
    p = wc.plan(T, E, layers)
    return (-1, -1, -1) if p is None else (p["saved"], p["fwd_ws"], p["bwd_ws"])


GRID_T = [1, 255, 256, 257, 300, 5700, 8800, 22100, 25344, 25700, 25856, 26368, 23552, 32800, 33000, 64000, 99999]
GRID_E = [16, 48, 64, 128, 144, 512, 528, 1024]
GRID_LAYERS = [[(1, 1)], [(96, 33), (33, 1), (128, 20)], [(128, 128)] * 24, [(128, 12)] * 24, [(128, 12)] * 12, [(32, 8)], [(128, 8)],
               [(128, 128)] + [(128, 12)] * 11, [(100, 12), (33, 40)], [(64, 64), (127, 33), (5, 17)], [(128, 32)] * 23]
REFUSED = [(0, 16, [(1, 1)]), (-5, 16, [(1, 1)]), (100, 8, [(1, 1)]), (100, 1040, [(1, 1)]), (100, 520, [(1, 1)]), (100, 0, [(1, 1)]),
           (100, 16, []), (100, 16, [(1, 1)] * 25), (100, 16, [(0, 1)]), (100, 16, [(129, 1)]), (100, 16, [(1, 0)]), (100, 16, [(1, 129)]),
           (100, 16, [(128, 128), (128, 129)])]


def test_mirror_matches_the_library_on_every_limit_and_refusal(lib):
    n = 0
    for T in GRID_T:
        for E in GRID_E:
            for layers in GRID_LAYERS:
                got, want = _mirror(T, E, layers), _sizes(lib, T, E, layers)
                assert got == want, (T, E, layers)
                assert min(want) > 0 and all(v % 256 == 0 for v in want), (T, E, layers)
                n += 1
    for name, (T, E, layers) in wc.CASES.items():
        assert _mirror(T, E, layers) == _sizes(lib, T, E, layers), name
    for T, E, layers in REFUSED:
        assert wc.plan(T, E, layers) is None and _sizes(lib, T, E, layers) == (-1, -1, -1), (T, E, layers)
    assert n == len(GRID_T) * len(GRID_E) * len(GRID_LAYERS)


def test_plane_limit_is_on_the_padded_token_count(lib):
    """include/psf_chord.h: T_pad * E and T_pad * (sum of h[k], each rounded up to 32) below 2^30, T_pad = T rounded up to
    256 — one bf16 term plane of X or of G below 2 GiB."""
    one = [(1, 1)]
    assert _sizes(lib, 1 << 20, 1024, one) == (-1, -1, -1) and wc.plan(1 << 20, 1024, one) is None
    below = (1 << 20) - 256
    assert _mirror(below, 1024, one) == _sizes(lib, below, 1024, one) and min(_sizes(lib, below, 1024, one)) > 0
    # T itself below the limit, T_pad on it: refused
    assert _sizes(lib, below + 1, 1024, one) == (-1, -1, -1) and wc.plan(below + 1, 1024, one) is None
    # the same for the stacked hidden rows: J = 24 x 128 = 3072, J x T_pad = 2^30 at T_pad = 349 525.33..: first multiple of 256 on it
    full = [(128, 1)] * 24
    t_bad = -(-(1 << 30) // 3072 // 256) * 256
    assert 3072 * t_bad >= 1 << 30 > 3072 * (t_bad - 256)
    assert _sizes(lib, t_bad, 16, full) == (-1, -1, -1) and wc.plan(t_bad, 16, full) is None
    assert _mirror(t_bad - 256, 16, full) == _sizes(lib, t_bad - 256, 16, full) and min(_sizes(lib, t_bad - 256, 16, full)) > 0
    # hidden widths count rounded up to 32 each: 24 x 97 rows fill the same planes as 24 x 128
    assert _sizes(lib, t_bad, 16, [(97, 1)] * 24) == (-1, -1, -1)


# ---------------------------------------------------------------- split-K
T_PADS = range(256, 100352 + 1, 256)   # every T_pad up to 100 352 >= 100 000


def _empty(chunks, splits):
    return [(sp, b, e) for sp, (b, e) in enumerate(wc.split_ranges(chunks, splits)) if e <= b]


def test_every_split_of_the_mirror_plan_has_a_k_range():
    """For every T_pad and every tile count: every split's [sp * per, min((sp + 1) * per, chunks)) is non-empty, one round of
    workgroups holds all (tile, split) items, and the kernel's per is the plan's."""
    counts = wc.tile_counts()
    assert counts[0] == 1 and counts[-1] == 48 and {1, 2, 3, 4, 5, 6, 7, 12, 36, 48} <= set(counts)
    for t_pad in T_PADS:
        chunks = t_pad // wc.CHUNK
        for tiles in counts:
            s = wc.split_rule(chunks, tiles)
            assert 1 <= s <= wc.SPLITS_MAX and s * tiles <= wc.WORKGROUPS and s <= max(chunks // wc.MIN_CHUNKS, 1), (t_pad, tiles)
            assert not _empty(chunks, s), (t_pad, tiles, s)
            ranges = wc.split_ranges(chunks, s)
            assert ranges[0][0] == 0 and ranges[-1][1] == chunks and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            # never fewer chunks per split than the rule before the fix gave: only splits without a K range left
            s0 = wc.split_rule(chunks, tiles, parent=True)
            assert -(-chunks // s) == -(-chunks // s0) and s <= s0


def test_the_rule_before_the_fix_left_splits_without_a_k_range():
    """The shapes of the defect: splits = min(256 / tiles, chunks / 32, 64) alone. (nk of the last split as the kernel computes it.)"""
    def last_nk(t_pad, tiles):
        chunks = t_pad // wc.CHUNK
        b, e = wc.split_ranges(chunks, wc.split_rule(chunks, tiles, parent=True))[-1]
        return e - b
    for tiles in (1, 2, 3, 4, 5):
        assert (last_nk(25344, tiles), last_nk(25856, tiles), last_nk(26368, tiles)) == (0, -1, -2)
    assert (last_nk(22272, 6), last_nk(23552, 6)) == (-2, -4)
    assert all(last_nk(33024, tiles) <= 0 for tiles in (1, 2, 3, 4))
    assert all(last_nk(t_pad, tiles) > 0 for t_pad in T_PADS for tiles in wc.tile_counts() if tiles >= 7)


def test_every_split_of_the_library_plan_has_a_k_range(lib):
    """The same property on the library: psf_mlp_wide_bwd_workspace less everything but the split slabs is splits x one slab."""
    for tiles in wc.tile_counts():
        E, layers = wc.shape_with_tiles(tiles)
        K = len(layers)
        h = (ctypes.c_int32 * K)(*[hh for hh, _ in layers])
        O = (ctypes.c_int32 * K)(*[oo for _, oo in layers])
        for t_pad in T_PADS:
            p = wc.plan(t_pad, E, layers)
            assert p["tiles"] == tiles and p["T_pad"] == t_pad
            slabs, rem = divmod(lib.psf_mlp_wide_bwd_workspace(t_pad, E, K, h, O) - p["bwd_ws_less_splits"], p["split_slab"])
            assert rem == 0 and slabs >= 1, (t_pad, tiles)
            assert not _empty(p["chunks"], slabs), (t_pad, tiles, slabs)
            assert slabs == p["splits"], (t_pad, tiles)


# ---------------------------------------------------------------- reach of the case table
def test_case_table_reaches_what_it_claims():
    p = {name: wc.plan(*case) for name, case in wc.CASES.items()}
    assert all(v is not None for v in p.values())
    assert set(wc.TABLE) | set(wc.ALIGN) | set(wc.NULL_DX) | set(wc.FUSE) | {wc.LOCAL} | set(wc.STALE) | set(wc.REPEAT) == set(wc.CASES)
    assert set(wc.EXACT) <= set(wc.TABLE) and len(wc.TABLE_RUNS) == len(wc.TABLE) + len(wc.EXACT)
    assert (p["smallest"]["T_pad"], p["smallest"]["J"], p["smallest"]["U"]) == (256, 32, 8)
    assert p["units"]["U"] == wc.MAX_UNITS == 96 and p["units"]["n_slots"] == [0, 0, wc.SLOT_CLASS] and wc.SLOT_CLASS == 384
    assert p["wrap0"]["groups"] == 23 and p["wrap0"]["n_slots"] == [96, 0, 0] and 23 * 96 > 256 * 8   # more items than waves
    assert (p["widest"]["J_pad"], p["widest"]["tiles_e"], p["widest"]["tiles"], p["widest"]["E_pad"]) == (3072, 4, 48, 1024)
    assert p["uneven"]["splits"] == 17 and [e - b for b, e in wc.split_ranges(p["uneven"]["chunks"], 17)] == [33] * 16 + [32]
    for name, t_pad, tiles in (("empty1", 25856, 1), ("empty6", 22272, 6), ("cap64", 33024, 1)):
        assert (p[name]["T_pad"], p[name]["tiles"]) == (t_pad, tiles)
        before = wc.plan(*wc.CASES[name], parent_splits=True)
        assert _empty(before["chunks"], before["splits"]), name            # the defect's shapes ...
        assert not _empty(p[name]["chunks"], p[name]["splits"]), name      # ... and the fixed plan on them
        assert p[name]["bwd_ws"] < before["bwd_ws"]
    assert wc.plan(*wc.CASES["cap64"], parent_splits=True)["splits"] == wc.SPLITS_MAX == 64 and p["cap64"]["splits"] == 63
    # the further tests' cases
    assert all(o % 4 == 0 for _, o in wc.CASES["o4"][2]) and any(o % 4 for _, o in wc.CASES["odd"][2])
    assert all(-(-h // 32) == 4 for h, _ in wc.CASES["fuse4"][2]) and {o <= 32 for _, o in wc.CASES["fuse4"][2]} == {True, False}
    T, _E, layers = wc.CASES[wc.LOCAL]
    assert T == 300 and wc.LOCAL_TOKENS == [0, 31, 32, 255, 256, T - 1] and all(h % 32 for h, _ in layers)
    assert p[wc.LOCAL]["J_pad"] > p[wc.LOCAL]["J"] > sum(h for h, _ in layers) and p[wc.LOCAL]["T_pad"] > T
    assert [wc.CASES[n][0] for n in wc.STALE] == [1, 255, 257]


@pytest.mark.parametrize("name", sorted(wc.EXACT))
def test_known_answer_cases_are_exact(name):
    T, E, layers = wc.CASES[name]
    case = xe.make_case(wc.EXACT[name], T, E, layers, seed=xe.seed("wide", T, E))
    xe.check_exact(case)
    X, params, dYs, ref, exact = wc.problem(name, wc.EXACT[name])
    assert exact and np.array_equal(X, case.X) and all(np.array_equal(a, b) for a, b in zip(dYs, case.dYs))
    assert not X.flags.writeable


def test_float64_reference_of_a_seeded_case():
    X, params, dYs, ref, exact = wc.problem("local")
    T, E, layers = wc.CASES["local"]
    assert not exact and X.shape == (T, E) and [d.shape for d in dYs] == [(T, o) for _, o in layers]
    assert [tuple(a.shape for a in ps) for ps in params] == [((h, E), (h,), (o, h), (o,)) for h, o in layers]
    A, a, B, b = (t.astype(np.float64) for t in params[1])
    H = X.astype(np.float64) @ A.T + a
    y = torch.nn.functional.gelu(torch.from_numpy(H)).numpy() @ B.T + b
    assert np.allclose(ref["Y"][1], y, rtol=0, atol=1e-12) and ref["Y"][1].dtype == np.float64
    assert np.allclose(ref["grads"][1][3], dYs[1].astype(np.float64).sum(0), rtol=0, atol=1e-12)
    assert wc.problem("local") is wc.problem("local")


# ---------------------------------------------------------------- the canaries report what they are there for
def test_canaries_report_one_stray_write_and_one_unwritten_element():
    cpu = torch.device("cpu")
    for shift in (0, 1):
        buf, view, span = wc.banded((7, 5), cpu, shift)
        # `shift` floats off the boundary that the allocation and the 256-byte band give it
        assert (view.data_ptr() - buf.data_ptr()) == 4 * (wc.BAND + shift) and span == (wc.BAND + shift, wc.BAND + shift + 35)
        assert wc.band_damage(buf, span) == 0 and wc.unwritten(buf, span) == 35 and bool(torch.isnan(buf).all())
        view.copy_(torch.arange(35.0).view(7, 5))
        assert wc.band_damage(buf, span) == 0 and wc.unwritten(buf, span) == 0
        view[3, 2] = float("nan")   # a computed NaN is a written element: not the canary's bits
        assert wc.unwritten(buf, span) == 0
        wc._words(view)[6, 4] = wc.CANARY
        assert wc.unwritten(buf, span) == 1
        for at in (span[0] - 1, span[1], 0, buf.numel() - 1):
            keep = buf[at].clone()
            buf[at] = 0.0
            assert wc.band_damage(buf, span) == 1, at
            buf[at] = float("nan")   # NaN of other bits is damage too
            assert wc.band_damage(buf, span) == 1, at
            wc._words(buf)[at] = wc.CANARY
            assert wc.band_damage(buf, span) == 0 and bool(torch.isnan(keep))
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    v = wc.banded_input(a, cpu, 1)
    assert np.array_equal(v.numpy(), a) and v.is_contiguous()


def test_scratch_canaries_report_one_byte_outside():
    cpu = torch.device("cpu")
    for n in (0, 256, 4608):
        buf, view = wc.scratch(n, cpu)
        assert view.numel() == n and buf.numel() == n + 2 * wc.SCRATCH_BAND and wc.SCRATCH_BAND >= 64 * 1024
        assert view.storage_offset() == wc.SCRATCH_BAND and wc.SCRATCH_BAND % 256 == 0   # as aligned as the allocation
        assert wc.scratch_damage(buf, n) == 0
        if n:
            assert bool(torch.isnan(view.view(torch.float32)).all()) and bool(torch.isnan(view.view(torch.bfloat16)).all())
            view.zero_()
            assert wc.scratch_damage(buf, n) == 0
        for at in (wc.SCRATCH_BAND - 1, wc.SCRATCH_BAND + n, 0, buf.numel() - 1):
            buf[at] = 0
            assert wc.scratch_damage(buf, n) == 1, at
            buf[at] = 0xFF
    assert wc.same_bits(np.float32([0.0, 1.0]), np.float32([0.0, 1.0])) and not wc.same_bits(np.float32([0.0]), np.float32([-0.0]))
