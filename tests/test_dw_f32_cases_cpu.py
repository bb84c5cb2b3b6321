"""CPU: the tools of test_gpu_dw_f32_exact.py (tests/dw_f32_cases.py) are right and sharp. No device is touched.

* the integer references are exact: every row dot stays below 2^24 in units of its scale, and the conversion to f32 / f64
  loses nothing;
* they are the CPU oracle's dF bit for bit (oracle.chord_oracle.spmul_bwd, f32 and f64, chord and explicit offsets);
* the oracle's own f32 dF lies inside the envelope on every real case: the reference alone passes what the GPU test imposes;
* every emulated defect changes the bits of the integer case and leaves the envelope on the real case of every case it applies
  to, in every family; a defect confined to the smallest row of a scaled-integer case is caught too;
* what the old bar (rel_inf <= 1e-5 over the whole tensor) would have let through, per family, on the scaled-integer case:
  drop_last_group in all five families, ragged_row_unwritten in the four that have ragged tiles, skip_chunk in the chunk family,
  stale_lane (with a stale value of the row's own size) in the window and generic families — the assertion below wants at
  least one per family and prints the list;
* psf_describe_bwd, under each describable case's knobs, names the kernel the table expects, and the table reaches all five
  f32 families and the f64 kernel."""
import numpy as np
import pytest

import dw_f32_cases as dc
from oracle import chord_oracle as oc

F32_FAMILIES = ("generic", "win", "chunk", "fused", "fused_edge")
IDS = [c.name for c in dc.CASES]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("case", dc.CASES, ids=IDS)
def test_integer_references_are_exact_and_equal_the_oracle(case):
    dt = dc.dtype_of(case)
    W = dc.w_case(case)
    dZi, Vi = dc.int_case(case)
    _, absum_i = dc.dw_sums(dZi, Vi, case.L, case.offsets)
    assert absum_i.max() < dc.LIMIT and absum_i.max() <= 127 * 127 * case.C  # the 2^24 bound, in units of the dot's scale
    for kind, make in dc.KINDS_EXACT.items():
        dZ, V = make(case)
        assert dZ.dtype == dt and V.dtype == dt and V.shape == ((case.N, case.C) if case.bcast else (case.B, case.N, case.C))
        exact, absum = dc.dw_sums(dZ, V, case.L, case.offsets)
        want = dc.exact_as(exact, dt)  # asserts that the conversion is exact
        nz = want[want != 0]
        assert np.isfinite(want).all() and (nz.size == 0 or np.abs(nz).min() >= 2.0 ** -126), kind  # normal
        if kind == "row_coded":
            assert absum.max() < dc.LIMIT
            b = 0 if case.bcast else np.arange(case.B)[:, None, None]
            src = (np.arange(case.N)[None, :, None] + np.array(dc.reduced_offsets(case))[None, None, :]) % case.N
            assert np.array_equal(exact, case.C * dc.row_code(b, src) * np.ones((case.B, 1, 1)))
        if kind == "scaled_int":  # one scale per dot: the scaled sums are the integer sums times a power of two
            ei, _ = dc.dw_sums(dZi, Vi, case.L, case.offsets)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(ei != 0, exact / ei, 1.0)
            m, _e = np.frexp(ratio)
            assert np.all(m == 0.5)
        dF, _ = oc.spmul_bwd(dZ, W, V, case.offsets)
        assert dF.dtype == dt and np.array_equal(_bits(dF), _bits(want)), kind


@pytest.mark.parametrize("name", ["gen_c6_n50_offsets", "chunk_c64_n70_offsets", "gen_c8_n300_near_not_chord"])
def test_f64_references_equal_the_oracle_with_explicit_offsets(name):
    """The table's f64 cases use chord offsets; the references hold in f64 with explicit ones too."""
    case = dc.BY_NAME[name]._replace(name=name + "_f64", route=dc.FAMILIES["generic_f64"] + ",VEC=2")
    assert dc.dtype_of(case) == np.float64 and case.offsets is not None
    for kind, make in dc.KINDS_EXACT.items():
        dZ, V = make(case)
        want = dc.exact_as(dc.dw_sums(dZ, V, case.L, case.offsets)[0], np.float64)
        dF, _ = oc.spmul_bwd(dZ, dc.w_case(case), V, case.offsets)
        assert dF.dtype == np.float64 and np.array_equal(_bits(dF), _bits(want)), kind


def test_scaled_rows_span_what_the_global_bar_cannot_see():
    case = dc.BY_NAME["win_c4_n600_l20"]
    dZ, V = dc.scaled_int_case(case)
    exact, _ = dc.dw_sums(dZ, V, case.L)
    mag = np.abs(exact[exact != 0])
    assert mag.max() / mag.min() > 2.0 ** 140


@pytest.mark.parametrize("case", [c for c in dc.CASES if dc.elem_bytes(c) == 4], ids=[c.name for c in dc.CASES if dc.elem_bytes(c) == 4])
def test_oracle_lies_inside_the_envelope_on_the_real_cases(case):
    W = dc.w_case(case)
    for kind, make in dc.KINDS_REAL.items():
        dZ, V = make(case)
        exact, absum = dc.dw_sums(dZ, V, case.L, case.offsets)
        dF, _ = oc.spmul_bwd(dZ, W, V, case.offsets)
        assert dc.envelope_ratio(dF, exact, absum, case.C).max() <= 1.0, kind
        if kind == "cancel" and case.C >= 8:  # the sums cancel: far smaller than the sum of their |terms|
            assert np.median(np.abs(exact) / absum) < 0.05


def test_envelope_is_the_derived_one():
    assert dc.gamma(8) == 8 * 2.0 ** -24 / (1 - 8 * 2.0 ** -24)
    absum = np.array([1.0, 4.0])
    assert np.array_equal(dc.envelope(absum, 8), (dc.gamma(8) + 8 * 2.0 ** -52) * absum)
    r = dc.envelope_ratio(np.array([np.nan, 4.0]), np.array([0.0, 4.0]), absum, 8)
    assert np.isinf(r[0]) and r[1] == 0.0


def _defect_runs(fam):
    """(defect name, case) pairs of a family to which the defect applies."""
    for case in dc.cases_of(fam):
        dZ, V = dc.int_case(case)
        for name, fn in dc.DEFECTS.items():
            if fn(case, dZ, V, np.array([case.N - 1])) is not None:
                yield name, case


@pytest.mark.parametrize("fam", F32_FAMILIES)
def test_every_emulated_defect_is_caught_in_every_family(fam):
    seen, old_bar_passes = set(), []
    for name, case in _defect_runs(fam):
        fn = dc.DEFECTS[name]
        seen.add(name)
        last = np.array([case.N - 1])
        # integer case: the bits change
        dZ, V = dc.int_case(case)
        want = dc.exact_f32(dc.dw_sums(dZ, V, case.L, case.offsets)[0])
        bad = fn(case, dZ, V, last).astype(np.float32)
        assert not np.array_equal(_bits(bad), _bits(want)), (name, case.name)
        # real case: outside the envelope
        dZ, V = dc.real_case(case)
        exact, absum = dc.dw_sums(dZ, V, case.L, case.offsets)
        bad = fn(case, dZ, V, last).astype(np.float32)
        assert dc.envelope_ratio(bad, exact, absum, case.C).max() > 1.0, (name, case.name)
        # scaled integers, the defect on the smallest row only where it is local: the bits change; the old bar may not see it
        dZ, V = dc.scaled_int_case(case)
        exact = dc.dw_sums(dZ, V, case.L, case.offsets)[0]
        want = dc.exact_f32(exact)
        row = dc.smallest_row(dZ)
        kw = {"stale": float(np.abs(exact[:, row, :]).max())} if name == "stale_lane" else {}
        bad = fn(case, dZ, V, row, **kw).astype(np.float32)
        assert not np.array_equal(_bits(bad), _bits(want)), (name, case.name, "scaled")
        if dc.rel_inf(bad, want) <= 1e-5:
            old_bar_passes.append((name, case.name))
    expected = set(dc.DEFECTS) - ({"skip_chunk"} if fam != "chunk" else set()) - ({"stale_lane"} if fam not in ("win", "generic") else set())
    expected -= {"ragged_row_unwritten"} if fam == "fused" else set()  # the aligned instance has full tiles only
    assert seen == expected, (fam, seen)
    print(f"{fam}: defects within rel_inf <= 1e-5 on the scaled-integer case: {sorted(set(n for n, _ in old_bar_passes))} "
          f"({len(old_bar_passes)} runs)")
    passed = {n for n, _ in old_bar_passes}
    assert {"drop_last_group", "ragged_row_unwritten"} & expected <= passed, (fam, passed)
    if fam == "chunk":
        assert "skip_chunk" in passed
    if fam in ("win", "generic"):
        assert "stale_lane" in passed


def test_at_least_six_defects_and_row_decoding():
    assert len(dc.DEFECTS) >= 6
    case = dc.BY_NAME["win_c8_n300_bcast"]
    dZ, V = dc.row_coded_case(case)
    got = dc.defect_far_link_neighbour(case, dZ, V)
    want = dc.dw_sums(dZ, V, case.L)[0]
    where = [tuple(int(i) for i in ix) for ix in np.argwhere(got != want)[:3]]
    for (b, p, k), should, named in dc.decode_rows(case, got, where):
        assert k == case.L - 1 and should == (p + dc.reduced_offsets(case)[k]) % case.N and named == [(should + 1) % case.N]


def test_table_reaches_what_it_claims():
    fams = {dc.family(c) for c in dc.CASES}
    assert fams == set(dc.FAMILIES)
    by = lambda f: dc.cases_of(f)  # noqa: E731
    tr = dc.tile_rows
    assert [tr(C) for C in (4, 8, 12, 16, 20, 32, 64, 128, 136, 256)] == [256, 128, 64, 64, 32, 32, 16, 8, 4, 4]
    win = by("win")
    assert {c.C for c in win} >= {4, 8, 12, 16, 20, 28, 32, 64, 128, 136, 256}
    assert any(c.N == 2 * tr(c.C) for c in win) and any(c.N == 2 * tr(c.C) + 1 for c in win)
    assert {c.L for c in win} >= {4, 5, 20}
    assert {c.C // 32 for c in by("chunk")} >= {1, 2, 3, 5, 32} and any((c.N * c.L) % 4 for c in by("chunk"))
    assert {c.C for c in by("generic")} >= {1, 6, 260} and {c.L for c in by("generic")} >= {3, 21}
    assert {c.C for c in by("fused")} == {4, 8, 16, 32, 64, 128}
    assert any(c.N == 3 * tr(c.C) for c in by("fused")) and any(c.N == 8 * tr(c.C) for c in by("fused"))
    assert {c.C for c in by("fused_edge")} >= {4, 32, 128}
    for c in dc.CASES:
        if dc.family(c) in ("win", "fused", "fused_edge"):
            assert c.N >= 2 * tr(c.C) and 4 <= c.L <= 20, c.name
        assert c.B in (1, 2, 3)
    assert {c.B for c in dc.CASES} == {1, 2, 3} and {dc.family(c) for c in dc.CASES if c.bcast} >= set(F32_FAMILIES)
    assert any(c.want == "dw" for c in dc.CASES) and any(c.dw_mis for c in dc.CASES) and any(c.op_mis[0] for c in dc.CASES)
    offs = [o for c in dc.CASES if c.offsets for o in c.offsets]
    assert min(offs) < 0 and any(c.offsets and max(c.offsets) >= c.N for c in dc.CASES)
    # L = 20 at small N: far links reduce to 0 or to a near offset and duplicate another link
    dup = {c.name: dc.duplicate_links(c) for c in dc.CASES if dc.duplicate_links(c)}
    assert len(dup) >= 10
    assert (4, 0) in dup["win_c256_n8_l20"]              # 8 mod 8 = 0: the copy of link 0
    assert any(j > 0 for _k, j in dup["fused_c4_n768_l20"])  # 2^k mod 3 TR is TR or 2 TR: copies of near and far links
    assert any(len(set(c.offsets)) < len(c.offsets) for c in dc.CASES if c.offsets)


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_described_routes_are_the_expected_kernels(lib):
    from sparsefactorization_amd import _lib
    saved = {k: _lib.get_tuning(k) for k in dc.KNOB_DEFAULTS}
    assert saved == dc.KNOB_DEFAULTS
    named, wrong = set(), []
    try:
        for case in dc.CASES:
            if not dc.describable(case):
                continue
            try:
                for k, v in dc.describe_knobs(case).items():
                    _lib.set_tuning(k, v)
                got = _lib.describe_bwd(case.B, case.N, case.L, case.C, dc.elem_bytes(case))
            finally:
                for k, v in saved.items():
                    _lib.set_tuning(k, v)
            if dc.route_matches(case, got):
                named.add(dc.family(case))
            else:
                wrong.append((case.name, case.route, got))
    finally:
        for k, v in saved.items():
            _lib.set_tuning(k, v)
    assert not wrong, wrong
    assert named == set(dc.FAMILIES)
    assert {k: _lib.get_tuning(k) for k in dc.KNOB_DEFAULTS} == saved


def test_chain_case_is_exact():
    W, V0, dOut, X1, dW = dc.chain_case()
    B, N, L, C, M = (dc.CHAIN[k] for k in "BNLCM")
    assert W.shape == (M, B, N, L) and set(np.unique(W)) == {-1.0, 0.0, 1.0} and dW.shape == (M, B, N, L)
    rows, cols = oc.chord_indices(N, L)
    steps = oc.chain(np.stack([rows, cols]), W, V0, False)
    assert np.array_equal(steps[0], X1)                     # X_1 of the oracle's chain
    dF1, dX1 = oc.spmul_bwd(dOut, W[1], X1)
    dF0, _ = oc.spmul_bwd(dX1, W[0], V0)
    assert np.array_equal(dF1, dW[1]) and np.array_equal(dF0, dW[0])
