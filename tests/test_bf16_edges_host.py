"""CPU: the tools of the bf16 edge tests (tests/bf16_edges.py) do what test_gpu_bf16_edges.py relies on. No kernel runs here:
correct results are emulated with numpy f32 sums in several orders, defects by truncation, by rounding after every addition,
by a stray two-byte write, by a gather that is one row off."""
import numpy as np
import pytest
import torch

import bf16_edges as be


def _f32_sums(terms):
    """sum over the last axis of f32 terms in three orders: sequential, reversed, pairwise (a tree)."""
    terms = np.asarray(terms, dtype=np.float32)
    seq = np.zeros(terms.shape[:-1], np.float32)
    rev = np.zeros(terms.shape[:-1], np.float32)
    for c in range(terms.shape[-1]):
        seq = (seq + terms[..., c]).astype(np.float32)
        rev = (rev + terms[..., terms.shape[-1] - 1 - c]).astype(np.float32)
    t = terms
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), np.float32)], -1)
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    return seq, rev, t[..., 0]


def _dw_terms(dZ, V, L):
    """[B, N, L, C] f32 products (exact: bf16 x bf16)."""
    N = dZ.shape[1]
    return np.stack([dZ * np.roll(V, -o, axis=-2) for o in be.chord_offsets(N, L)], axis=2).astype(np.float32)


def test_conversions_agree_with_torch_and_with_each_other():
    rng = np.random.default_rng(0)
    with np.errstate(over="ignore"):
        a = (rng.standard_normal(200000) * np.exp2(rng.integers(-140, 128, 200000))).astype(np.float32)
    a[:8] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 3.3895314e38, 1e-40, -1e-45]  # (3.39e38 rounds to +Inf in bf16)
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert be.same_bits(be.rne_bits(a), want) == 0
    assert np.array_equal(be.bits_f32(be.rne_bits(a))[1:], be.rne64(a.astype(np.float64))[1:])
    # ties go to the even neighbour; truncation differs from rounding exactly where the dropped half is >= 1/2 ulp
    assert be.rne_bits(np.float32(257.0)) == be.rne_bits(np.float32(256.0)) and be.bits_f32(be.rne_bits(np.float32(259.0))) == 260.0
    assert be.bits_f32(be.trunc_bits(np.float32(259.0))) == 258.0
    # a float64 just above a tie: direct rounding goes up, the detour through f32 lands on the tie and goes down to even
    x = 256.0 + 1.0 + 2.0 ** -30
    assert be.rne64(x) == 258.0 and be.bits_f32(be.rne_bits(np.float32(x))) == 256.0
    # same_bits: NaN meets NaN whatever the payload, zeros are told apart by their sign
    assert be.same_bits(np.array([0x7FC0, 0x0000], np.uint16), np.array([0x7FC1, 0x8000], np.uint16)) == 1


@pytest.mark.parametrize("shape,broadcast", sorted({(s, b) for s, _, b in be.KNOWN_ANSWER}))
def test_integer_construction_is_exact_and_holds_every_rounding_case(shape, broadcast):
    B, N, L, C = shape
    dZ, V = be.known_answer_operands(shape, broadcast)
    for t in (dZ, V):
        assert np.array_equal(be.as_bf16(t), t) and np.abs(t).max() <= 15
    exact, absum = be.dw_sums(dZ, V, L)
    assert absum.max() <= 225 * C < 2.0 ** 24
    terms = _dw_terms(dZ, np.broadcast_to(V, (B, N, C)), L)
    for s in _f32_sums(terms):  # every order gives the exact integer
        assert np.array_equal(s.astype(np.float64), exact)
    cls = be.rounding_classes(exact.astype(np.float32))
    for k in ("exact", "tie_up", "tie_down", "up", "down"):
        assert cls[k] > 0, (k, cls)
    assert cls["tie_up"] + cls["tie_down"] + cls["up"] + cls["down"] >= 0.05 * cls["n"]
    # and so truncation is told from rounding, bit for bit
    assert be.same_bits(be.trunc_bits(exact.astype(np.float32)), be.rne_bits(exact.astype(np.float32))) > 0


@pytest.mark.parametrize("C", [6, 8, 24, 128, 256])
def test_bracket_accepts_f32_sums_in_any_order_and_rejects_wrong_roundings(C):
    B, N, L = 2, 300, 9
    dZ, V = be.normal_case((B, N, C), 4), be.normal_case((B, N, C), 2)
    exact, absum = be.dw_sums(dZ, V, L)
    terms = _dw_terms(dZ, V, L)
    for s in _f32_sums(terms):
        bad, loose = be.bracket_report(be.rne_bits(s), exact, absum, C)
        assert bad == 0 and loose <= be.MAX_LOOSE, (bad, loose)
        be.assert_dw_bracket(be.rne_bits(s), dZ, V, L)
    seq = _f32_sums(terms)[0]
    bad, _ = be.bracket_report(be.trunc_bits(seq), exact, absum, C)
    assert bad >= 0.3 * exact.size, f"truncation violates the bracket on only {bad / exact.size:.1%} of the elements"
    with pytest.raises(AssertionError):
        be.assert_dw_bracket(be.trunc_bits(seq), dZ, V, L)
    acc = np.zeros(seq.shape, np.float32)  # a bf16 accumulator: rounded after every addition
    for c in range(C):
        acc = be.as_bf16(acc + terms[..., c])
    bad, _ = be.bracket_report(be.rne_bits(acc), exact, absum, C)
    assert bad > 0
    # a NaN where a number belongs is outside every bracket
    got = be.rne_bits(seq)
    got.reshape(-1)[5] = 0x7FC0
    assert be.bracket_report(got, exact, absum, C)[0] == 1


@pytest.mark.parametrize("shift", [0, 1, 4])
def test_band_checker_flags_one_stray_write_and_one_unwritten_element(shift):
    n = 1000
    total, lo, hi = be.arena_span(n, shift)
    assert lo * 2 >= 256 and (total - hi) * 2 >= 256 and (lo * 2) % 16 == (2 * shift) % 16
    arena = np.full(total, be.SENTINEL, np.uint16)
    arena[lo:hi] = be.rne_bits(be.normal_case((n,), 1))
    assert be.band_report(arena, lo, hi) == (0, 0, 0)
    for pos, want in ((lo - 1, (1, 0, 0)), (0, (1, 0, 0)), (hi, (0, 1, 0)), (total - 1, (0, 1, 0))):
        a = arena.copy()
        a[pos] = 0x3F80
        assert be.band_report(a, lo, hi) == want, pos
    a = arena.copy()
    a[pos] = 0x7FC0  # a stray NaN of another pattern is a write too
    assert be.band_report(a, lo, hi) == (0, 1, 0)
    for pos in (lo, lo + 517, hi - 1):
        a = arena.copy()
        a[pos] = be.SENTINEL
        assert be.band_report(a, lo, hi) == (0, 0, 1), pos
    assert be.SENTINEL != 0x7FC0 and np.isnan(be.bits_f32(np.uint16(be.SENTINEL)))


@pytest.mark.parametrize("run", be.SPECIAL_RUNS)
@pytest.mark.parametrize("B,N,L,C", be.SPECIAL_SHAPES)
def test_special_value_generator_meets_its_product_range(B, N, L, C, run):
    W, V, R, dZ = be.special_operands(B, N, L, C, run)
    for t in (W, V, R, dZ):
        assert np.array_equal(be.as_bf16(t)[~np.isnan(t)], t[~np.isnan(t)])
        plain = t[np.isfinite(t) & (np.abs(t) < 2.0 ** 100) & (np.abs(t) > 2.0 ** -100)]
        assert plain.size >= 0.97 * t.size and np.abs(plain).min() >= 1.0 and np.abs(plain).max() < 2.0
        assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any()
        assert (t[t == 0].view(np.uint32) == 0).any() and (t[t == 0].view(np.uint32) == 0x80000000).any()
    assert be.product_range_ok(W, V) and be.product_range_ok(W, dZ) and be.product_range_ok(dZ, V)
    wide = {"w": W, "dz": dZ, "dz_tame": dZ}[run]
    assert (np.abs(wide) == 2.0 ** -126).any() and (np.abs(wide) == 2.0 ** 126).any() == (run != "dz_tame")
    for t in {"w": (V, R, dZ), "dz": (W, V, R), "dz_tame": (W, V, R)}[run]:
        assert not ((np.abs(t) == 2.0 ** 126) | (np.abs(t) == 2.0 ** -126)).any()
    # the precondition is a real one: the ends of the range in two operands that meet break it
    assert not be.product_range_ok(W if run == "w" else dZ, W if run == "w" else dZ)
    # dW has NaN, both infinities and finite elements to check (few at C = 128, where a row meets 256 operands)
    exact, absum = be.dw_sums(dZ, V, L)
    assert np.isnan(exact).any() and np.isposinf(exact).any() and np.isneginf(exact).any() and np.isfinite(exact).sum() >= 8


def _sampled_case(seed=0, B=1, N=4096, L=12, C=64):
    """Small stand-in for the 2 GB cases: (rows, exact, slack, f32 result) of out = sum_k W V[n + off_k] + R at sampled rows."""
    rng = np.random.default_rng(seed)
    W, V, R = be.normal_case((N, L), seed + 1, 0.2), be.normal_case((N, C), seed + 2), be.normal_case((N, C), seed + 3)
    off = be.chord_offsets(N, L)

    def rows_of(rows):
        rows = np.asarray(rows)
        terms = [W[rows, k, None].astype(np.float64) * V[(rows + o) % N].astype(np.float64) for k, o in enumerate(off)]
        terms.append(R[rows].astype(np.float64))
        exact = np.sum(terms, axis=0)
        absum = np.sum(np.abs(terms), axis=0)
        acc = np.zeros(exact.shape, np.float32)
        for t in terms:  # links ascending, then the residual, every product exact
            acc = (acc + t.astype(np.float32)).astype(np.float32)
        return exact, L * 2.0 ** -24 * absum, acc

    return np.array(be.sample_rows(N)), rows_of


def test_sampled_row_verdict_of_the_large_cases():
    rows, rows_of = _sampled_case()
    assert len(set(rows.tolist())) == 8 and rows.min() == 0 and rows.max() == 4095
    exact, slack, acc = rows_of(rows)
    wrong, share = be.decide_rows(be.rne_bits(acc), exact, slack)
    assert wrong == 0 and share >= be.MIN_DECIDABLE
    # the f32 result in another order is accepted as well (it may differ only next to a rounding boundary)
    wrong, _ = be.decide_rows(be.rne_bits((acc.astype(np.float64) + 0.5 * slack).astype(np.float32)), exact, slack)
    assert wrong == 0
    # rounded by truncation
    wrong, _ = be.decide_rows(be.trunc_bits(acc), exact, slack)
    assert wrong >= 0.3 * exact.size
    # a gather that is one row off
    _, _, off_by_one = rows_of((rows + 1) % 4096)
    wrong, _ = be.decide_rows(be.rne_bits(off_by_one), exact, slack)
    assert wrong >= 0.9 * exact.size
    # one element one bf16 step off where it is decidable
    got = be.rne_bits(acc)
    lo, hi = be.rne64(exact - slack), be.rne64(exact + slack)
    i = int(np.flatnonzero((lo == hi).ravel())[0])
    got.reshape(-1)[i] += 1
    assert be.decide_rows(got, exact, slack)[0] == 1
    # a sum that cancels: the slack spans several values of the fine grid near zero; those between the ends pass, others fail
    x, sl = np.array([1e-7]), np.array([1e-5])
    for v, want in ((0.0, 0), (-9.9e-6, 0), (1.01e-5, 0), (1.02e-5, 1), (-1.0e-5, 1), (np.nan, 1)):
        assert be.decide_rows(be.rne_bits(np.float32(v)), x, sl)[0] == want, v
    # slack so wide that nothing is decidable: the share says so
    assert be.decide_rows(be.rne_bits(acc), exact, slack * 2.0 ** 16)[1] < be.MIN_DECIDABLE
