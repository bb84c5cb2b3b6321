"""CPU self-tests of the known-answer cases of test_gpu_helpers_exact.py (tests/helper_cases.py).

They show, without a GPU, that every case is exact (small integers, sum |terms| < 2^24, an integral expected answer that f32
holds), that the lists reach the code paths they are there for (computed from the constants the kernels document: sub-table
counts, 64-column chunks, 128-token slices capped at 2048, the two chunk lengths of the head, the capped grids of the stride
loops, the LDS sizes), and that five emulated defects each change at least one expected answer.
"""
import numpy as np
import pytest

import helper_cases as hc

ALL = hc.EMB_GRAD + hc.EMB_FWD + hc.AFFINE + hc.HEAD_FWD + hc.HEAD_BWD + hc.WGRAD


def _operands(case):
    names = {hc.EmbGrad: ("dout",), hc.EmbFwd: ("table", "pos_rows"), hc.Affine: ("x", "w", "b"), hc.HeadFwd: ("x", "w", "b"),
             hc.HeadBwd: ("dy", "x", "w"), hc.WGrad: ("x", "dy")}[type(case)]
    return {n: getattr(case, n)() for n in names}


MAGNITUDE = {(hc.EmbGrad, "dout"): 4, (hc.EmbFwd, "table"): 2000, (hc.EmbFwd, "pos_rows"): 2000, (hc.Affine, "x"): 7,
             (hc.Affine, "w"): 7, (hc.Affine, "b"): 7, (hc.HeadFwd, "x"): 2, (hc.HeadFwd, "w"): 2, (hc.HeadFwd, "b"): 100,
             (hc.HeadBwd, "dy"): 3, (hc.HeadBwd, "x"): 3, (hc.HeadBwd, "w"): 3, (hc.WGrad, "x"): 3, (hc.WGrad, "dy"): 2}


def test_ids_are_unique():
    for lst in (hc.EMB_GRAD, hc.EMB_FWD, hc.AFFINE, hc.HEAD_FWD, hc.HEAD_BWD, hc.WGRAD):
        assert len({c.id for c in lst}) == len(lst)


@pytest.mark.parametrize("case", ALL, ids=[f"{type(c).__name__}-{c.id}" for c in ALL])
def test_every_case_is_exact(case):
    """Operands are integers inside their documented magnitudes, sum |terms| < 2^24, the expected answer integral and exact in f32."""
    for name, a in _operands(case).items():
        if a is None:
            continue
        assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)), name
        assert np.abs(a).max() <= MAGNITUDE[type(case), name], name
    assert case.bound() < hc.LIMIT
    want = case.expected()
    for w in want if isinstance(want, tuple) else (want,):
        assert hc.as_f32(w).shape == w.shape


def test_as_f32_refuses_what_f32_cannot_hold():
    assert hc.as_f32(np.array([hc.LIMIT - 1, -3])).tolist() == [float(hc.LIMIT - 1), -3.0]
    for bad in (np.array([hc.LIMIT]), np.array([0.5])):
        with pytest.raises(AssertionError):
            hc.as_f32(bad)


def test_embedding_gradient_list_covers_what_it_claims():
    cases = hc.EMB_GRAD
    assert 28 <= len(cases) <= 36
    assert {c.T for c in cases} == {1, 127, 128, 129, 999, 4096, 262144, 262145, 300001, 300}
    assert {c.E for c in cases} >= {1, 2, 3, 5, 8, 12, 16, 17, 32, 33, 64, 65, 100, 4096}
    assert {c.V for c in cases} >= {1, 6, 192, 193, 225, 512}
    assert {c.pattern for c in cases} == set(hc.EMB_PATTERNS)
    for E in {c.E for c in cases}:
        assert len({c.T for c in cases if c.E == E}) >= 2, E
    for c in cases:
        if c.T > 200000:
            assert (c.V, c.E) == (6, 4)
        if c.E == 4096:
            assert c.V == 4 and c.T <= 300
        if c.V == 512:
            assert (c.E, c.T) == (64, 4096)
    # every layout of the LDS table: 1, 2, 4, ..., 64 sub-tables; idle columns inside a sub-table (E no power of two)
    assert {hc.emb_subtables(c.E) for c in cases} == {1, 2, 4, 8, 16, 32, 64}
    assert [hc.emb_subtables(E) for E in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 4096)] == [64, 32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1, 1, 1]
    assert any(c.E < 64 and c.E & (c.E - 1) for c in cases)
    # a partial last chunk of 64 columns; one chunk, two, and 64 of them
    assert any(c.E > 64 and c.E % hc.EMB_CHUNK for c in cases)
    assert {-(-c.E // hc.EMB_CHUNK) for c in cases} >= {1, 2, 64}
    # the dynamic-LDS boundary (48 KB: V = 192 | 193), the largest vocabulary of the models (225) and the limit V = 512 (128 KB)
    assert hc.emb_lds_bytes(192) == 48 * 1024 and hc.emb_lds_bytes(512) == 128 * 1024
    assert {192, 193, 225, 512} <= {c.V for c in cases}
    # fewer tokens than one slice, a ragged last slice, the last T of 128-token slices, and capped slices with empty ones
    assert any(c.T < hc.EMB_TOKENS_PER_SLICE for c in cases) and any(c.T % hc.EMB_TOKENS_PER_SLICE for c in cases if c.T > 128)
    assert any(c.T == hc.EMB_TOKENS_PER_SLICE * hc.EMB_SLICES_MAX for c in cases)
    capped = [c for c in cases if -(-c.T // hc.EMB_TOKENS_PER_SLICE) > hc.EMB_SLICES_MAX]
    assert len(capped) >= 2
    for c in capped:
        assert hc.emb_slices(c.T) == hc.EMB_SLICES_MAX and hc.emb_slice_len(c.T) > hc.EMB_TOKENS_PER_SLICE
        assert (hc.EMB_SLICES_MAX - 1) * hc.emb_slice_len(c.T) >= c.T, "no slice starts at or past T"
    # the patterns do what they say, and the last token carries the largest magnitude
    for c in cases:
        idx, d = c.idx(), c.dout()
        assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < c.V
        assert np.all(np.abs(d[-1]) == 4) and (c.T == 1 or np.abs(d[:-1]).max() <= 3)
        assert c.E == 1 or len(set(d[-1].tolist())) == 2
        want = c.expected()
        if c.pattern == "one_row":
            assert len(set(idx.tolist())) == 1 and not want[np.arange(c.V) != idx[0]].any()
        elif c.pattern == "missing":
            assert not (idx % 2).any() and not want[1::2].any()
            assert c.V < 2 or want[1::2].size
        elif c.pattern == "ends":
            assert set(idx.tolist()) <= {0, c.V - 1} and not want[1:c.V - 1].any()
    assert any(c.pattern == "missing" and c.V >= 192 for c in cases) and any(c.pattern == "ends" and c.V >= 192 for c in cases)


def test_stride_loop_lists_take_a_second_trip():
    one_trip = hc.STRIDE_GRID * hc.STRIDE_THREADS
    assert [(c.B, c.N, c.V, c.E, c.pos) for c in hc.EMB_FWD] == [(1, 1, 1, 4, False), (3, 7, 6, 4, True), (7, 10000, 6, 128, True),
                                                                (2, 2049, 512, 32, False)]
    assert any(c.vectors() > one_trip for c in hc.EMB_FWD) and any(c.vectors() < hc.STRIDE_THREADS for c in hc.EMB_FWD)
    aff = hc.AFFINE
    assert {c.K for c in aff} == {1, 2, 3} and {(c.K, c.bias) for c in aff} == {(k, b) for k in (1, 2, 3) for b in (True, False)}
    assert {c.E for c in aff} == {4, 12, 16, 256, 516, 1024}
    for E in (516, 1024):
        assert {c.T for c in aff if c.E == E} == {1, 85, 86, 8193}
        assert all(c.positions_per_workgroup() == 1 for c in aff if c.E == E)
    assert any(c.T > hc.STRIDE_GRID * c.positions_per_workgroup() for c in aff if c.E == 516)       # one position per
    assert any(c.T > hc.STRIDE_GRID * c.positions_per_workgroup() for c in aff if c.E == 1024)      # workgroup
    assert any((c.T, c.E) == (600000, 4) for c in aff)
    assert any(c.T > hc.STRIDE_GRID * c.positions_per_workgroup() > hc.STRIDE_GRID for c in aff)      # ... and 64 per workgroup
    # 85 positions per workgroup at E = 12: one workgroup exactly full, and one position more
    assert {c.T for c in aff if c.E == 12} == {85, 86} and hc.Affine(85, 1, 12, True).positions_per_workgroup() == 85


def test_head_lists_cover_both_chunk_lengths_their_tails_and_the_backward_limit():
    fwd = hc.HEAD_FWD
    assert {c.K for c in fwd} >= {4, 1020, 1024, 1028, 4096 + 12} and {c.B for c in fwd} >= {1, 8, 9} and {c.J for c in fwd} >= {1, 3, 8}
    for chunk in (1024, 4096):
        mine = [c for c in fwd if c.chunk() == chunk]
        assert any(c.K % chunk for c in mine) and any(c.K > chunk and c.K % chunk for c in mine), chunk
    # which side of the rule (>= 1024 workgroups of 4096 floats x 8 rows) each large case falls on
    large = [c for c in fwd if c.B * c.K > (1 << 20)]
    assert len(large) == 4
    for c in large:
        wgs = -(-c.K // 4096) * -(-c.B // hc.HEAD_ROWS)
        assert (wgs >= 1024) == ((c.B, c.K, c.J) in hc.HEAD_FWD_LARGE_CHUNK) == (c.chunk() == 4096), c.id
    assert {-(-c.K // 4096) * -(-c.B // 8) for c in large} == {1024, 960}  # exactly at the rule, and one row group below
    assert {c.J for c in fwd if c.chunk() == 4096} == {1, 3, 8} and all(c.chunk() == 1024 for c in fwd if c.K < 4096)
    assert max(c.B * c.K * 4 for c in fwd) < 140e6
    assert any(c.B % hc.HEAD_ROWS == 1 for c in fwd) and any(not c.bias for c in fwd)
    # the same 120 rows and the same W on both sides of the rule
    a, b = (next(c for c in fwd if (c.B, c.K, c.J) == k) for k in hc.HEAD_FWD_ACROSS)
    assert a.chunk() == 4096 and b.chunk() == 1024
    xa = a.x()
    assert np.array_equal(xa[:b.B], b.x()) and np.array_equal(a.w(), b.w()) and np.array_equal(a.b(), b.b())
    assert np.array_equal(a.expected(x=xa)[:b.B], b.expected())
    bwd = hc.HEAD_BWD
    assert {c.B for c in bwd} == {1, 7, 8, 9, 1024} and {c.J for c in bwd} == {1, 5, 16} and {c.K for c in bwd} == {4, 252, 256, 260, 4096}
    assert any((c.B, c.K, c.J, c.want_dx, c.want_dw) == (1024, 4096, 16, True, True) for c in bwd)
    assert max(c.B * c.J * 4 for c in bwd) == 64 * 1024 and hc.HEAD_BWD_MAX_B * hc.HEAD_BWD_MAX_J * 4 == 64 * 1024
    assert sum(c.want_dx and not c.want_dw for c in bwd) >= 2 and sum(c.want_dw and not c.want_dx for c in bwd) >= 2
    assert all(c.want_dx or c.want_dw for c in bwd)


def test_weight_gradient_list_covers_what_it_claims():
    cases = hc.WGRAD
    assert 14 <= len(cases) <= 18
    assert {c.T for c in cases} == {1, 2, 15, 17, 31, 4097, 100003}
    assert {(c.m, c.n) for c in cases} == {(1, 1), (1, 128), (128, 1), (128, 128), (33, 65), (32, 15)}
    assert 3 * sum(c.strided for c in cases) >= len(cases) and 3 * sum(not c.need_bias for c in cases) >= len(cases)
    assert any(c.strided and not c.need_bias for c in cases) and any(c.strided and c.T > 4096 for c in cases)
    for c in cases:
        if c.strided:
            xw, yw = c.wide()
            assert xw.shape == (c.T, c.m + 3) and yw.shape == (c.T, c.n + 5)
            assert np.isnan(xw).sum() == 3 * c.T and np.isnan(yw).sum() == 5 * c.T
            assert np.array_equal(xw[:, c.X_OFF:c.X_OFF + c.m], c.x()) and np.array_equal(yw[:, c.DY_OFF:c.DY_OFF + c.n], c.dy())
            assert np.isnan(xw[:, 0]).all() and np.isnan(xw[:, -1]).all() and np.isnan(yw[:, 0]).all() and np.isnan(yw[:, -1]).all()


def test_the_data_are_asymmetric():
    """A transposed or permuted operand gives another answer: the expected results are not symmetric under the swaps a wrong tile makes."""
    c = next(c for c in hc.WGRAD if (c.T, c.m, c.n) == (17, 128, 128))
    dW, _ = c.expected()
    assert not np.array_equal(dW, dW.T) and not np.array_equal(dW, dW[::-1]) and not np.array_equal(dW, dW[:, ::-1])
    c = next(c for c in hc.HEAD_BWD if (c.B, c.K, c.J) == (8, 256, 16))
    dX, dW = c.expected()
    assert not np.array_equal(dX, dX[::-1]) and not np.array_equal(dW, dW[::-1])
    c = next(c for c in hc.EMB_GRAD if (c.T, c.V, c.E) == (999, 225, 16))
    want = c.expected()
    assert len({tuple(r) for r in want.tolist()}) > 200 and len({tuple(r) for r in want.T.tolist()}) == 16


# ---- emulated defects: each changes at least one case's expected answer ------------------------------------------------
def _slice_of(c):
    n = hc.emb_slice_len(c.T)
    return np.arange(c.T) // n, np.arange(c.T) % n, n


def test_defect_last_token_of_a_slice_dropped():
    changed = 0
    for c in hc.EMB_GRAD:
        _, within, n = _slice_of(c)
        keep = (within != n - 1) & (np.arange(c.T) != c.T - 1)
        changed += not np.array_equal(c.expected(keep=keep), c.expected())
    assert changed == len(hc.EMB_GRAD)  # the last token carries +-4 everywhere: every case sees it


def test_defect_one_subtable_not_added():
    """Tokens sit side by side in 64 / E' sub-tables; the last one left out of the sum."""
    seen = set()
    for c in hc.EMB_GRAD:
        subs = hc.emb_subtables(c.E)
        if subs == 1 or c.T < subs:
            continue
        _, within, _ = _slice_of(c)
        if not np.array_equal(c.expected(keep=within % subs != subs - 1), c.expected()):
            seen.add(subs)
    assert seen == {2, 4, 8, 16, 32, 64}


def test_defect_last_partial_chunk_of_columns_left_unwritten():
    changed = []
    for c in hc.EMB_GRAD:
        full = c.E // hc.EMB_CHUNK * hc.EMB_CHUNK
        if c.E > hc.EMB_CHUNK and full < c.E:
            want = c.expected()
            assert want[:, full:].any(), c.id  # what a kernel that skips the ragged chunk would leave behind is not the answer
            changed.append(c.E)
    assert set(changed) == {65, 100}


def test_defect_tail_chunk_of_the_head_skipped():
    for chunk in (1024, 4096):
        changed = 0
        for c in hc.HEAD_FWD:
            if c.chunk() == chunk and c.K > chunk and c.K % chunk:
                x, w = c.x(), c.w()
                full = np.arange(c.K // chunk * chunk)
                changed += not np.array_equal(c.expected(x=x, w=w, cols=full), c.expected(x=x, w=w))
        assert changed >= 2, chunk


def test_defect_last_batch_row_of_the_head_backward_skipped():
    for c in hc.HEAD_BWD:
        dX, dW = c.expected()
        dXs, dWs = c.expected(rows=np.arange(c.B - 1))
        assert np.isnan(dXs[-1]).all() and np.array_equal(dXs[:-1], dX[:-1])
        assert not np.array_equal(dWs, dW), c.id


def test_out_of_range_ids_stay_within_two_rows_of_the_table():
    """The clamping tests read, at worst, the NaN rows next to the table: never further than the band."""
    assert hc.CLAMP_BAND_ROWS >= 4
    for c in hc.EMB_GRAD_CLAMPED + hc.EMB_FWD_CLAMPED:
        idx = c.idx()
        bad = hc.with_out_of_range_ids(idx, c.V, seed=1)
        out = (bad < 0) | (bad >= c.V)
        assert set(bad[out].tolist()) == {-2, -1, c.V, c.V + 1}
        assert bad[0] == -1 and bad[-1] == c.V and np.array_equal(bad[~out], idx[~out])
        assert 0.003 * idx.size <= out.sum() <= 0.03 * idx.size
        assert bad.min() >= -hc.CLAMP_BAND_ROWS and bad.max() < c.V + hc.CLAMP_BAND_ROWS
        want = c.expected(idx=np.clip(bad, 0, c.V - 1))
        assert not np.array_equal(want, c.expected())  # the clamped tokens count: rows 0 and V - 1 receive them
