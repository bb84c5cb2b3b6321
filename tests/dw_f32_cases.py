"""Cases, operands, references and emulated defects for the f32 weight gradient of the chord step (test_gpu_dw_f32_exact.py;
checked themselves, without a GPU, by test_dw_f32_cases_cpu.py).

    dW[b,p,k] = sum_c dZ[b,p,c] * V[b,(p+off_k) mod N,c]

numpy only. Five f32 kernel families compute it (chord_dw_generic_k, chord_dw_win_k, chord_dw_chunk_k, chord_bwd_fused_k,
chord_bwd_fused_edge_k; plan_bwd in csrc/psf_chord.hip chooses) and a sixth, f64 chord_dw_generic_k, exists for gradcheck.

Operands (all seeded by the case's name):

* ``int_case``         dZ and V are integers in [-127, 127] without zero. Every product and every partial sum of a row dot is an
                       integer of magnitude <= 127^2 C < 2^24 (C <= 1024, asserted), exact in f32: the only correct dW is the exact
                       sum, bit for bit, in any order, with or without FMA contraction.
* ``scaled_int_case``  the same integers, dZ row p times 2^s(p) and V row q times 2^t(q), s and t drawn per row from [-40, 40]. One
                       dot has one scale, so it stays exact and normal; dW is still bit-exact although its rows span ~2^160.
* ``row_coded_case``   dZ = 1 and V[b,q,c] = code(b,q) = (q + 131 b) mod 8191 for every c, so dW[b,p,k] = C code(b,(p+off_k) mod N)
                       names the source row that was read (exact for C <= 2048). ``decode_rows`` turns a wrong dW back into rows.
* ``real_case``        standard normal dZ and V; ``cancel=True``: the second half of each row's channels repeats the first half
                       with V negated plus a 2^-12 perturbation, so a row sum is far smaller than the sum of its |terms|.

References: ``dw_sums`` gives (exact, absum) in float64, absum = sum_c |dZ V|. Offsets are any int64, reduced mod N, duplicates
kept; V may be [B,N,C] or [N,C]. For the integer kinds ``exact_f32`` / ``exact_as`` convert and assert that nothing is lost.

Envelope of the real kinds (``envelope``). A correct f32 dW is the f32 result of C products, each rounded (or fused into the add
that consumes it), summed in any order or tree. Every term then passes through at most C roundings (its own product and at most
C - 1 additions), each of relative size <= u = 2^-24, so by the standard bound (Higham, Accuracy and Stability, lemma 3.1)
|got - exact| <= gamma_C absum with gamma_C = C u / (1 - C u). The float64 reference carries its own error, <= C 2^-52 absum,
which is added. No other tolerance.

The case table (``CASES``) uses the smallest shapes at which each path exists. A window or fused tile is
TR = 256 >> ceil_log2(C / 4) rows, a chunk-kernel tile 32 or 16 rows, and a kernel needs N >= 2 TR. Which plan_bwd line decides
the route of a case that psf_describe_bwd cannot be asked about (it takes aligned operands and chord offsets):

* a misaligned dZ or V clears dw_ok ("const bool dw_ok = (C % el.vec == 0) && aligned_to(dZ, 16) && aligned_to(V, 16)"), and
  pick_dw_chunk / pick_window return false on !vec_ok: chord_dw_generic_k<f32,VEC=1>;
* a misaligned W or dW fails pick_fused_step's "aligned_to(W, 16) ... aligned_to(dW, 16)" and pick_fused_edge_step, which does
  not look at them, takes the step: chord_bwd_fused_edge_k; with the fused step off the dW kernels stay (all_edge set by
  "!aligned_to(dW, 16)" in pick_dw_chunk and "!aligned_to(W, 16)" in pick_window, where W is the dW buffer);
* explicit offsets pass near_links when the first KN are the chord pattern's; far offsets that are no multiple of the tile
  fail pick_fused_step's "offs.v[k] % TR != 0" (the edge instance takes the step) and clear pick->aligned of the window kernel;
  near offsets that are not the chord's send both gradients to the generic kernels ("if (!KN) return false");
* dW alone (dV NULL) skips "if (want_dw && want_dv)": the dW branch below it is the one bwd_fused = 0 reaches, which is how
  the route of such a case is described.

Emulated defects (``DEFECTS``): numpy functions that compute dW the way a kernel with one mistake would. Each is applied to the
reference computation, never to a kernel.
"""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
LIMIT = 1 << 24
CODE_MOD = 8191
CODE_BATCH = 131

# knobs a case may set, with the shipped defaults (include/psf_chord_tuning.h)
KNOB_DEFAULTS = {"bwd_variant": 0, "bwd_fused": 1, "dw_variant": 0, "dw_tgs": 0, "fwd_split": 1, "bwd_fronts": 0,
                 "bwd_fused_wg_limit": 0}

FAMILIES = {"generic": "chord_dw_generic_k<f32", "win": "chord_dw_win_k", "chunk": "chord_dw_chunk_k",
            "fused": "chord_bwd_fused_k", "fused_edge": "chord_bwd_fused_edge_k", "generic_f64": "chord_dw_generic_k<f64"}

# name, shape, knobs off their defaults, explicit offsets or None, dW's shift off a 16-byte boundary in elements, the shifts of
# (W, dZ, V), V broadcast over the batch ([N, C], v_batch_stride = 0), gradients asked for ("both" or "dw"), and a substring of
# the route psf_describe_bwd names ('*' stands for any text in between; the route starts with the kernel's name)
Case = namedtuple("Case", "name B N L C knobs offsets dw_mis op_mis bcast want route")


def ceil_log2(n: int) -> int:
    return max(int(n) - 1, 0).bit_length()


def tile_rows(C: int) -> int:
    """Rows per tile of the window and fused kernels."""
    return 256 >> ceil_log2((C + 3) // 4)


def family(case: Case) -> str:
    for fam in ("generic_f64", "generic", "win", "chunk", "fused_edge", "fused"):
        if case.route.startswith(FAMILIES[fam]):
            return fam
    raise AssertionError(case.route)


def route_matches(case: Case, described: str) -> bool:
    """The parts of case.route (separated by '*') occur in `described`, in order."""
    at = 0
    for part in case.route.split("*"):
        at = described.find(part, at)
        if at < 0:
            return False
        at += len(part)
    return True


def elem_bytes(case: Case) -> int:
    return 8 if "<f64" in case.route else 4


def dtype_of(case: Case):
    return np.float64 if elem_bytes(case) == 8 else np.float32


def describable(case: Case) -> bool:
    """psf_describe_bwd plans with aligned operands and chord offsets (a broadcast V changes no route: plan_bwd only asks
    v_batch_stride to be 0 or N C)."""
    return case.offsets is None and case.dw_mis == 0 and not any(case.op_mis)


def describe_knobs(case: Case) -> dict:
    """The knobs under which psf_describe_bwd (both gradients) plans the dW kernel this case runs."""
    knobs = dict(case.knobs)
    if case.want == "dw":
        knobs["bwd_fused"] = 0
    return knobs


def chord_offsets(N: int, L: int) -> list:
    return [0] + [(1 << k) % N for k in range(L - 1)]


def reduced_offsets(case_or_N, L=None, offsets=None) -> list:
    if isinstance(case_or_N, Case):
        case_or_N, L, offsets = case_or_N.N, case_or_N.L, case_or_N.offsets
    if offsets is None:
        return chord_offsets(case_or_N, L)
    assert len(offsets) == L
    return [int(o) % case_or_N for o in offsets]


def duplicate_links(case: Case) -> list:
    """(k, j), j < k: link k reduces to the same offset as the earlier link j, so column k of dW must equal column j."""
    off, first, out = reduced_offsets(case), {}, []
    for k, o in enumerate(off):
        if o in first:
            out.append((k, first[o]))
        else:
            first[o] = k
    return out


# ------------------------------------------------------------------------------------------------------------ the table
def _c(name, B, N, L, C, route, knobs=None, offsets=None, dw_mis=0, op_mis=(0, 0, 0), bcast=False, want="both"):
    return Case(name, B, N, L, C, dict(knobs or {}), None if offsets is None else tuple(offsets), dw_mis, tuple(op_mis), bcast,
                want, route)


def _far_odd(N, L, C, shift=37):
    """Chord near links of the tile, every far link moved by `shift`: only the general instances apply."""
    KN = min(2 + ceil_log2(tile_rows(C)), L)
    return [0] + [1 << k for k in range(KN - 1)] + [(1 << k) + shift for k in range(KN - 1, L - 1)]


def _build():
    WIN, CHUNK, GEN, FUSED, EDGE = (FAMILIES[f] for f in ("win", "chunk", "generic", "fused", "fused_edge"))
    two = {"bwd_fused": 0}            # the two-kernel route
    win32 = {"bwd_fused": 0, "dw_variant": 1}  # the whole-row window dW where the chunk kernel is the default
    t = []
    # ---- window dW: C = 4 (one lane per row); exactly two tiles (the window wraps once), one row more, ragged
    t += [_c("win_c4_n512_l4", 2, 512, 4, 4, WIN, two), _c("win_c4_n513_l5", 2, 513, 5, 4, WIN, two),
          _c("win_c4_n600_l20", 1, 600, 20, 4, WIN, two), _c("win_c4_n512_l20", 1, 512, 20, 4, WIN, two)]
    t += [_c("win_c8_n256_l5", 3, 256, 5, 8, WIN, two), _c("win_c8_n257_l20", 2, 257, 20, 8, WIN, two)]
    # idle lanes (channel groups no power of two: the all-edge instance)
    t += [_c("win_c12_n128_l4", 2, 128, 4, 12, WIN), _c("win_c20_n150_l20", 2, 150, 20, 20, WIN),
          _c("win_c28_n300_l5", 3, 300, 5, 28, WIN), _c("win_c12_n150_l9", 1, 150, 9, 12, WIN),
          _c("win_c28_n128_l20", 2, 128, 20, 28, WIN), _c("win_c20_n300_l11", 2, 300, 11, 20, WIN)]
    for C, L in ((16, 4), (32, 5), (64, 20), (128, 9)):
        TR, kn = tile_rows(C), (win32 if C % 32 == 0 else two)
        t += [_c(f"win_c{C}_n{2 * TR}_l{L}", 2, 2 * TR, L, C, WIN, kn), _c(f"win_c{C}_n{2 * TR + 1}_l{L}", 2, 2 * TR + 1, L, C, WIN, kn)]
    t += [_c("win_c136_n16_l20", 2, 16, 20, 136, WIN), _c("win_c136_n37_l5", 3, 37, 5, 136, WIN)]   # 34 of 64 lanes
    t += [_c("win_c256_n8_l20", 2, 8, 20, 256, WIN, {"dw_variant": 1}), _c("win_c256_n9_l4", 1, 9, 4, 256, WIN, {"dw_variant": 1}),
          _c("win_c256_n37_l20", 2, 37, 20, 256, WIN, {"dw_variant": 1})]
    t += [_c("win_c8_n257_split0", 2, 257, 9, 8, WIN, {"bwd_fused": 0, "fwd_split": 0}),
          _c("win_c8_n257_split2", 2, 257, 9, 8, WIN, {"bwd_fused": 0, "fwd_split": 2}),
          _c("win_c16_n129_dw1", 2, 129, 10, 16, WIN, two, dw_mis=1), _c("win_c8_n300_dw3_l7", 3, 300, 7, 8, WIN, two, dw_mis=3)]
    # ---- chunk-looping dW: 1, 2, 3, 5 and 32 chunks; two tiles, one row more, ragged
    t += [_c("chunk_c32_n64_l4", 2, 64, 4, 32, CHUNK, two), _c("chunk_c64_n65_l9", 2, 65, 9, 64, CHUNK, two),  # N L % 4 != 0
          _c("chunk_c96_n100_l20", 2, 100, 20, 96, CHUNK), _c("chunk_c160_n64_l5", 3, 64, 5, 160, CHUNK),
          _c("chunk_c1024_n64_l5", 1, 64, 5, 1024, CHUNK), _c("chunk_c1024_n65_l11", 1, 65, 11, 1024, CHUNK),
          _c("chunk_c64_n48_l9_tg16auto", 2, 48, 9, 64, CHUNK + "<f32,L=9,TG=16", two),
          _c("chunk_c128_n32_l10_tgs5", 2, 32, 10, 128, CHUNK + "<f32,L=10,TG=16", {"bwd_fused": 0, "dw_tgs": 5}),
          _c("chunk_c128_n80_l10_tgs4", 2, 80, 10, 128, CHUNK + "<f32,L=10,TG=8", {"bwd_fused": 0, "dw_tgs": 4}),
          _c("chunk_c128_n80_l10_auto", 2, 80, 10, 128, CHUNK + "<f32,L=10,TG=16", two),
          _c("chunk_c32_n65_dw1", 2, 65, 8, 32, CHUNK, two, dw_mis=1), _c("chunk_c96_n64_dw2", 1, 64, 6, 96, CHUNK, dw_mis=2)]
    t += [_c(f"chunk_c96_n100_split{s}", 2, 100, 9, 96, CHUNK, {"fwd_split": s}) for s in (0, 1, 2)]
    # ---- generic dW
    t += [_c("gen_c1_n7_l3", 2, 7, 3, 1, GEN + ",VEC=1"), _c("gen_c6_n50_l21", 2, 50, 21, 6, GEN + ",VEC=1"),
          _c("gen_c260_n40_l9", 2, 40, 9, 260, GEN + ",VEC=4"), _c("gen_c8_n7_l5", 3, 7, 5, 8, GEN + ",VEC=4"),  # below two tiles
          _c("gen_c16_n64_l3", 2, 64, 3, 16, GEN + ",VEC=4"), _c("gen_c8_n300_l21", 1, 300, 21, 8, GEN + ",VEC=4"),
          _c("gen_c8_n300_dz1", 2, 300, 9, 8, GEN + ",VEC=1", op_mis=(0, 1, 0)),
          _c("gen_c32_n100_v1", 2, 100, 9, 32, GEN + ",VEC=1", op_mis=(0, 0, 1)),
          _c("gen_c8_n512_variant1", 2, 512, 10, 8, GEN + ",VEC=4", {"bwd_variant": 1}),
          _c("gen_c64_n70_variant1", 2, 70, 9, 64, GEN + ",VEC=4", {"bwd_variant": 1})]
    # f64 (gradcheck's kernel): 16 bytes are two elements, so C = 6 and C = 8 both take VEC = 2; an odd C takes VEC = 1
    t += [_c("f64_c6_n50_l9", 2, 50, 9, 6, FAMILIES["generic_f64"] + ",VEC=2"),
          _c("f64_c8_n300_l10", 2, 300, 10, 8, FAMILIES["generic_f64"] + ",VEC=2"),
          _c("f64_c7_n50_l9", 2, 50, 9, 7, FAMILIES["generic_f64"] + ",VEC=1")]
    # ---- fused step, aligned instance (default knobs, both gradients)
    for C in (4, 8, 16, 32, 64, 128):
        TR = tile_rows(C)
        t += [_c(f"fused_c{C}_n{2 * TR}_l4", 2, 2 * TR, 4, C, FUSED + "<"), _c(f"fused_c{C}_n{3 * TR}_l20", 2, 3 * TR, 20, C, FUSED + "<")]
    for C in (8, 32):
        TR = tile_rows(C)
        t += [_c(f"fused_c{C}_n{8 * TR}_fronts{f}", 2, 8 * TR, 12, C, FUSED + f"<*fronts={f}", {"bwd_fronts": f}) for f in (1, 2, 4, 8)]
        t += [_c(f"fused_c{C}_n{8 * TR}_wg3", 2, 8 * TR, 12, C, FUSED + "<", {"bwd_fused_wg_limit": 3})]
    # ---- fused step, edge instance
    t += [_c("edge_c4_n513_l5", 2, 513, 5, 4, EDGE), _c("edge_c32_n65_l20", 2, 65, 20, 32, EDGE), _c("edge_c128_n17_l9", 3, 17, 9, 128, EDGE),
          _c("edge_c8_n256_w1_dw3", 2, 256, 9, 8, EDGE, dw_mis=3, op_mis=(1, 0, 0)),
          _c("edge_c16_n129_w1_dw3", 2, 129, 20, 16, EDGE, dw_mis=3, op_mis=(1, 0, 0)),
          _c("edge_c32_n64_far_odd", 2, 64, 12, 32, EDGE, offsets=_far_odd(64, 12, 32)),
          _c("edge_c8_n512_far_odd", 2, 512, 12, 8, EDGE, offsets=_far_odd(512, 12, 8))]
    # ---- across routes: B = 1 and 3, a broadcast V, dW alone, explicit offsets (negative, >= N, duplicates)
    t += [_c("win_c8_n300_bcast", 3, 300, 10, 8, WIN, two, bcast=True), _c("chunk_c96_n70_bcast", 3, 70, 9, 96, CHUNK, bcast=True),
          _c("gen_c6_n50_bcast", 3, 50, 7, 6, GEN + ",VEC=1", bcast=True), _c("fused_c8_n256_bcast", 3, 256, 9, 8, FUSED + "<", bcast=True),
          _c("edge_c32_n65_bcast", 3, 65, 9, 32, EDGE, bcast=True), _c("fused_c16_n128_b1", 1, 128, 8, 16, FUSED + "<"),
          _c("win_c8_n256_dw_only", 2, 256, 9, 8, WIN, want="dw"), _c("chunk_c32_n64_dw_only", 3, 64, 8, 32, CHUNK, want="dw"),
          _c("win_c64_n33_dw_only", 1, 33, 6, 64, WIN, want="dw"),  # below two 32-row chunk tiles, no multiple of 16: the window dW
          _c("win_c32_n100_offsets", 2, 100, 10, 32, WIN, win32, offsets=[0, 1, 2, 4, 8, 16, 32, -3, 117, 17]),
          _c("edge_c32_n100_offsets", 2, 100, 10, 32, EDGE, offsets=[0, 1, 2, 4, 8, 16, 32, -3, 117, 17]),
          _c("chunk_c64_n70_offsets", 2, 70, 9, 64, CHUNK, two, offsets=[0, 1, 2, 4, 8, 16, 32, -5, 103]),
          _c("gen_c6_n50_offsets", 2, 50, 5, 6, GEN + ",VEC=1", offsets=[5, -1, 5, 1000, 0]),
          _c("gen_c8_n300_near_not_chord", 2, 300, 6, 8, GEN + ",VEC=4", offsets=[0, 3, -300, 299, 7, 3 - 600])]
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    for c in t:
        assert c.B * c.N * max(c.C, c.L) < 2_000_000 and set(c.knobs) <= set(KNOB_DEFAULTS), c.name
    return t


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def cases_of(fam: str) -> list:
    return [c for c in CASES if family(c) == fam]


# ------------------------------------------------------------------------------------------------------------ operands
def _rng(case: Case, tag: int):
    return np.random.default_rng([zlib.crc32(case.name.encode()), tag])


def _v_shape(case: Case):
    return (case.N, case.C) if case.bcast else (case.B, case.N, case.C)


def _ints(rng, shape):
    """Integers in [-127, 127], zero excluded, as float64."""
    return (rng.integers(1, 128, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float64)


def int_case(case: Case):
    assert 127 * 127 * case.C < LIMIT, "a row dot of integers in [-127, 127] must stay below 2^24"
    rng = _rng(case, 1)
    dt = dtype_of(case)
    return _ints(rng, (case.B, case.N, case.C)).astype(dt), _ints(rng, _v_shape(case)).astype(dt)


def scaled_int_case(case: Case):
    dZ, V = int_case(case)
    rng = _rng(case, 2)
    s = rng.integers(-40, 41, size=(case.B, case.N, 1))
    tq = rng.integers(-40, 41, size=V.shape[:-1] + (1,))
    dt = dtype_of(case)
    return np.ldexp(dZ, s).astype(dt), np.ldexp(V, tq).astype(dt)


def row_code(b, q):
    return (np.asarray(q) + CODE_BATCH * np.asarray(b)) % CODE_MOD


def row_coded_case(case: Case):
    assert case.C * (CODE_MOD - 1) < LIMIT
    dt = dtype_of(case)
    q = np.arange(case.N)
    code = row_code(0, q) if case.bcast else row_code(np.arange(case.B)[:, None], q[None, :])
    V = np.broadcast_to(code[..., None], _v_shape(case)).astype(dt)
    return np.ones((case.B, case.N, case.C), dtype=dt), np.ascontiguousarray(V)


def decode_rows(case: Case, got, where):
    """For elements `where` (index tuples (b, p, k)) of a row-coded dW: (row that should have been read, rows of that batch
    element whose code the value names, or the value itself if it is no multiple of C)."""
    out = []
    off = reduced_offsets(case)
    for b, p, k in where:
        v = float(got[b, p, k])
        want = (p + off[k]) % case.N
        named = None
        if v == np.rint(v) and v % case.C == 0:
            code = int(v) // case.C
            named = [q for q in range(case.N) if int(row_code(0 if case.bcast else b, q)) == code]
        out.append(((b, p, k), want, named if named else v))
    return out


def real_case(case: Case, cancel: bool = False):
    rng = _rng(case, 4 if cancel else 3)
    dt = dtype_of(case)
    dZ = rng.standard_normal((case.B, case.N, case.C)).astype(dt)
    V = rng.standard_normal(_v_shape(case)).astype(dt)
    if cancel:
        h = case.C // 2
        if h:
            dZ[..., h:2 * h] = dZ[..., :h]
            V[..., h:2 * h] = (-V[..., :h].astype(np.float64) + 2.0 ** -12 * rng.standard_normal(V[..., :h].shape)).astype(dt)
    return dZ, V


KINDS_EXACT = {"int": int_case, "scaled_int": scaled_int_case, "row_coded": row_coded_case}
KINDS_REAL = {"real": lambda c: real_case(c), "cancel": lambda c: real_case(c, cancel=True)}


def w_case(case: Case):
    """W of the step (needed for dV only): 0.3 N(0, 1)."""
    return (0.3 * _rng(case, 5).standard_normal((case.B, case.N, case.L))).astype(dtype_of(case))


# ------------------------------------------------------------------------------------------------------------ references
def dw_terms(dZ, V, off):
    """The products dZ[b,p,c] V[b,(p+off_k) mod N,c] as float64 [B, N, L, C] (off: reduced offsets)."""
    dZ = np.asarray(dZ, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    return np.stack([dZ * np.roll(V, -int(o), axis=-2) for o in off], axis=2)


def dw_sums(dZ, V, L, offsets=None):
    """(exact, absum), float64 [B, N, L]: sum_c dZ V and sum_c |dZ V| (|dZ V| = |dZ| |V| exactly in float64 for f32 inputs)."""
    N = np.asarray(dZ).shape[1]
    terms = dw_terms(dZ, V, reduced_offsets(N, L, offsets))
    return terms.sum(-1), np.abs(terms).sum(-1)


def exact_as(exact, dtype):
    """An exactly representable answer in `dtype`; asserts that the conversion loses nothing."""
    out = np.asarray(exact).astype(dtype)
    assert np.array_equal(out.astype(np.float64), np.asarray(exact, dtype=np.float64)), "the exact answer is not representable"
    return out


def exact_f32(exact):
    return exact_as(exact, np.float32)


def gamma(C: int) -> float:
    return C * U / (1.0 - C * U)


def envelope(absum, C):
    """Largest |got - exact| of a correct f32 dW (module docstring), float64 reference error included."""
    return (gamma(C) + C * 2.0 ** -52) * np.asarray(absum, dtype=np.float64)


def envelope_ratio(got, exact, absum, C):
    """|got - exact| / envelope per element (0 where both vanish); NaN or Inf in `got` gives inf."""
    err = np.abs(np.asarray(got, dtype=np.float64) - exact)
    env = envelope(absum, C)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / env)
    return np.where(np.isfinite(r), r, np.inf)


def rel_inf(a, b) -> float:
    """max|a-b| / max|b|: the bar test_gpu_parity.py holds dW to (<= 1e-5), for showing what it cannot see."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d = np.where(np.isnan(d), np.inf, d)
    denom = np.max(np.abs(b))
    return float(np.max(d) / (denom if denom > 0 else 1.0))


# ------------------------------------------------------------------------------------------------------------ emulated defects
# Each takes (case, dZ, V, rows) and returns the float64 dW a kernel with that one mistake would produce (summed exactly: the
# mistake, not rounding, is what differs), or None where the mistake cannot occur on the case. `rows` is an index array of the
# sequence rows the mistake touches, for the defects that are local to a tile or a row.
def _flat_rows(case, V, b, rows):
    """Rows `rows` (any int, past the end too) of batch element b of V as laid out in memory, with the batch stride that a
    full-batch V has: what lies beyond the array reads as zero."""
    V = np.asarray(V, dtype=np.float64)
    flat = V.reshape(-1, case.C)
    idx = b * case.N + np.asarray(rows)
    ok = idx < flat.shape[0]
    out = np.zeros((len(idx), case.C))
    out[ok] = flat[idx[ok]]
    return out


def defect_drop_last_group(case, dZ, V, rows):
    """The last channel group of a row (its last 1..4 channels) never enters the sum."""
    terms = dw_terms(dZ, V, reduced_offsets(case))
    g = (case.C - 1) % 4 + 1
    terms[:, rows, :, case.C - g:] = 0.0
    return terms.sum(-1)


def defect_skip_chunk(case, dZ, V, rows, chunk=-1):
    """One 32-channel chunk of the chunk loop is skipped (the last by default)."""
    if family(case) != "chunk":
        return None
    n = case.C // 32
    c0 = (chunk % n) * 32
    terms = dw_terms(dZ, V, reduced_offsets(case))
    terms[:, rows, :, c0:c0 + 32] = 0.0
    return terms.sum(-1)


def defect_stale_lane(case, dZ, V, rows, stale=2.0 ** -6):
    """An idle lane (channel groups no power of two) adds what it found in LDS: stale but small."""
    CG = (case.C + 3) // 4
    if family(case) not in ("win", "generic") or CG & (CG - 1) == 0:
        return None
    out = dw_terms(dZ, V, reduced_offsets(case)).sum(-1)
    out[:, rows, :] += stale
    return out


def defect_no_wrap(case, dZ, V, rows=None):
    """p + off is not wrapped at N: the read runs on into the next batch element's rows (zero past the array)."""
    dZ = np.asarray(dZ, dtype=np.float64)
    off = reduced_offsets(case)
    out = np.empty((case.B, case.N, case.L))
    p = np.arange(case.N)
    for b in range(case.B):
        for k, o in enumerate(off):
            out[b, :, k] = (dZ[b] * _flat_rows(case, V, 0 if case.bcast else b, p + o)).sum(-1)
    return out


def defect_ragged_row_unwritten(case, dZ, V, rows=None, fill=0.0):
    """The last row of a ragged last tile is never stored: dW keeps what the buffer held."""
    if family(case) in ("generic", "generic_f64"):  # 256 threads, up to 64 lanes per row (generic_geom)
        TR = 256 >> min(ceil_log2(case.C // 4 if case.C % 4 == 0 else case.C), 6)
    else:
        TR = 32 if family(case) == "chunk" else tile_rows(case.C)
    if case.N % TR == 0:
        return None
    out = dw_terms(dZ, V, reduced_offsets(case)).sum(-1)
    out[:, case.N - 1, :] = fill
    return out


def defect_far_link_neighbour(case, dZ, V, rows=None):
    """The last link takes the neighbouring offset (off + 1)."""
    off = reduced_offsets(case)
    off[-1] = (off[-1] + 1) % case.N
    return dw_terms(dZ, V, off).sum(-1)


def defect_bcast_stride(case, dZ, V, rows=None):
    """The batch stride N C is applied to a broadcast V: batch element b > 0 reads past the [N, C] array."""
    if not case.bcast or case.B < 2:
        return None
    dZ = np.asarray(dZ, dtype=np.float64)
    off = reduced_offsets(case)
    out = np.empty((case.B, case.N, case.L))
    p = np.arange(case.N)
    for b in range(case.B):
        for k, o in enumerate(off):
            out[b, :, k] = (dZ[b] * _flat_rows(case, V, b, (p + o) % case.N)).sum(-1)
    return out


DEFECTS = {"drop_last_group": defect_drop_last_group, "skip_chunk": defect_skip_chunk, "stale_lane": defect_stale_lane,
           "no_wrap": defect_no_wrap, "ragged_row_unwritten": defect_ragged_row_unwritten,
           "far_link_neighbour": defect_far_link_neighbour, "bcast_stride": defect_bcast_stride}
LOCAL_DEFECTS = ("drop_last_group", "skip_chunk", "stale_lane")  # take the rows they touch


def smallest_row(dZ, V=None):
    """The sequence row whose dZ is smallest in magnitude over the batch (one row, as an index array)."""
    mag = np.abs(np.asarray(dZ, dtype=np.float64)).max(axis=(0, 2))
    return np.array([int(np.argmin(mag))])


# ------------------------------------------------------------------------------------------------------------ the chain case
CHAIN = dict(B=2, N=1100, L=11, C=8, M=2)


def chain_case():
    """Operands of the per-step backward chain test: V0 and dOut integers in [-127, 127], W_m in {-1, 0, 1}.
    X_1 = W_0 (.) V0 is an integer of magnitude <= L 127, dX_1 = W_1^T (.) dOut likewise, so every row dot of dW_1 = dOut . X_1
    and dW_0 = dX_1 . V0 sums C integers of magnitude <= 127 L 127: 8 * 127 * 11 * 127 < 2^24, exact in any order.
    Returns (W [M,B,N,L], V0, dOut, X_1, dW [M,B,N,L]) as f32, the last two computed exactly."""
    B, N, L, C, M = (CHAIN[k] for k in "BNLCM")
    rng = np.random.default_rng(20240)
    W = rng.integers(-1, 2, size=(M, B, N, L)).astype(np.float64)
    V0 = _ints(rng, (B, N, C))
    dOut = _ints(rng, (B, N, C))
    off = chord_offsets(N, L)
    assert C * 127 * L * 127 < LIMIT
    X1 = sum(W[0][:, :, k:k + 1] * np.roll(V0, -o, axis=1) for k, o in enumerate(off))
    dX1 = sum(np.roll(W[1][:, :, k:k + 1] * dOut, o, axis=1) for k, o in enumerate(off))  # dV[q] = sum_k (W dZ)[q - off_k]
    dW1 = dw_terms(dOut, X1, off).sum(-1)
    dW0 = dw_terms(dX1, V0, off).sum(-1)
    f = exact_f32
    return f(W), f(V0), f(dOut), f(X1), np.stack([f(dW0), f(dW1)])
