"""CPU: the attention-map queries without a device — the identity they rest on in float64, the oracle's dV as the f32
reference of a row, and the host side of psf_chord_chain_tr_supported / _f32 / _bf16 (the shape query needs no device and
every argument check of the entries returns before anything is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attention_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ALIAS, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -4, -7
ENTRIES = ("psf_chord_chain_tr_supported", "psf_chord_chain_tr_f32", "psf_chord_chain_tr_bf16")


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


# ---- the identity, in float64 and through the oracle --------------------------------------------------------------
def _small():
    rng = np.random.default_rng(5)
    B, N, L, M = 2, 64, 7, 6
    return [rng.standard_normal((B, N, L)) / np.sqrt(L) for _ in range(M)], B, N, L, M


def test_transposed_chain_on_one_hot_vectors_is_the_rows_of_the_dense_product():
    Ws, B, N, L, M = _small()
    A = ac.dense_map_f64(Ws)
    rows = np.stack([np.arange(N), np.arange(N)[::-1]])  # every row, in two orders
    got = ac.tr_chain_f64(Ws, ac.one_hot(rows, N, np.float64))  # [B, N, R]: column j is row rows[b, j]
    want = np.stack([A[b][rows[b]].T for b in range(B)])
    assert np.max(np.abs(got - want)) <= 1e-12
    # explicit and negative offsets follow the same rule
    off = (-1, 0, 5, -37, 63, 64, 200)
    A = ac.dense_map_f64(Ws, off)
    got = ac.tr_chain_f64(Ws, ac.one_hot(rows, N, np.float64), off)
    assert np.max(np.abs(got - np.stack([A[b][rows[b]].T for b in range(B)]))) <= 1e-12


def test_oracle_dv_applied_m_times_gives_the_rows_in_f32():
    Ws, B, N, L, M = _small()
    Ws = [W.astype(np.float32) for W in Ws]
    rows = np.stack([np.arange(N), np.arange(N)[::-1]])
    got = ac.oracle_f32(Ws, ac.one_hot(rows, N))
    exact = ac.tr_chain_f64(Ws, ac.one_hot(rows, N, np.float64))
    absprod = ac.tr_chain_f64([np.abs(W) for W in Ws], ac.one_hot(rows, N, np.float64))
    assert absprod.min() >= 0 and absprod.max() > 0
    assert np.all(np.abs(got - exact) <= ac.gamma(M, L) * absprod)
    A = ac.dense_map_f64(Ws)
    assert np.max(np.abs(exact - np.stack([A[b][rows[b]].T for b in range(B)]))) <= 1e-12


def test_bf16_reference_rounds_every_step_and_keeps_the_bound():
    Ws, B, N, L, M = _small()
    Ws = [ac.rne_bf16(W) for W in Ws]
    rows = np.stack([np.arange(N), np.arange(N)[::-1]])
    got = ac.oracle_bf16(Ws, ac.one_hot(rows, N))
    assert np.array_equal(got, ac.rne_bf16(got))
    exact = ac.tr_chain_f64(Ws, ac.one_hot(rows, N, np.float64))
    absprod = ac.tr_chain_f64([np.abs(W) for W in Ws], ac.one_hot(rows, N, np.float64))
    assert np.all(np.abs(got - exact) <= ac.gamma(M, L, 2) * absprod)
    assert ac.gamma(M, L, 2) > 100 * ac.gamma(M, L)


def test_case_lists_cover_what_they_claim():
    for cases, vec in ((ac.F32_CASES, 4), (ac.BF16_CASES + [ac.BF16_ODD_W], 8)):
        assert len({c[0] for c in cases}) == len(cases)
        assert {1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097} <= {c[2] for c in cases}
        assert {2, 20} <= {c[3] for c in cases} and any(c[2] == 1024 and c[3] == 12 for c in cases)
        assert {1, 2, 11, 64} <= {c[4] for c in cases} and {1, 3} <= {c[1] for c in cases}
        assert all(c[5] % vec == 0 for c in cases)
        for name, B, N, L, M, R, off, sp in cases:
            assert ac.covered(N, L, R, M, 16 // vec) == (N <= 1024), name
    assert {4, 8, 12, 64} <= {c[5] for c in ac.F32_CASES} and {8, 16, 24} <= {c[5] for c in ac.BF16_CASES}
    assert max(c[5] for c in ac.F32_CASES + ac.BF16_CASES) == 64
    # the split of the column groups over workgroups: full ones of 1, 2, 3, 4 groups, several per sequence, and a ragged last one
    assert ac.workgroup_groups(12, 4) == (3, [3]) and ac.workgroup_groups(24, 2) == (3, [3]) and ac.workgroup_groups(64, 4) == (4, [4] * 4)
    assert ac.workgroup_groups(20, 4) == (3, [3, 2]) and ac.workgroup_groups(52, 4) == (4, [4, 4, 4, 1])
    assert ac.workgroup_groups(40, 2) == (3, [3, 2]) and ac.workgroup_groups(56, 2) == (4, [4, 3])
    for cases, eb in ((ac.F32_CASES, 4), (ac.BF16_CASES, 2)):
        splits = [ac.workgroup_groups(c[5], eb) for c in cases if c[2] <= 1024]
        assert {1, 2, 3, 4} <= {G for G, _ in splits}
        ragged = [(G, per) for G, per in splits if per[-1] < G]
        assert len(ragged) >= 2, "no case whose last workgroup holds fewer groups than the instance's G"
        assert all(sum(per) * (16 // eb) == c[5] for (G, per), c in zip(splits, [c for c in cases if c[2] <= 1024]))
    assert ("imdb", 2, 4097, 13, 12, 4, None, None) in ac.F32_CASES
    assert {c[7] for c in ac.F32_CASES} == {None, "dense", "nan", "inf"}
    assert any(c[6] and min(c[6]) < 0 for c in ac.F32_CASES) and any(c[6] and min(c[6]) >= 0 for c in ac.F32_CASES)


# ---- the library's host side ---------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound(lib):
    from sparsefactorization_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "psf_chord.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
        assert re.search(r"\bint %s\s*\(" % name, header), name
    assert len(lib.psf_chord_chain_tr_supported.argtypes) == 5
    assert len(lib.psf_chord_chain_tr_f32.argtypes) == len(lib.psf_chord_chain_tr_bf16.argtypes) == 11
    assert lib.psf_version() == 2  # additive: the ABI version stays


def test_pointer_positions_read_as_tensors_of_the_suffix_dtype():
    import ptr_audit
    from sparsefactorization_amd import _lib
    for entry, dtype in (("psf_chord_chain_tr_f32", torch.float32), ("psf_chord_chain_tr_bf16", torch.bfloat16)):
        wanted = [ptr_audit.wanted(entry, i, _lib.SIGNATURES) for i in range(11)]
        assert wanted[:4] == [(dtype,)] * 4 and all(w == () for w in wanted[4:]), entry
    assert all(ptr_audit.wanted("psf_chord_chain_tr_supported", i, _lib.SIGNATURES) == () for i in range(5))


def test_python_surface():
    import sparsefactorization_amd as sfa
    from sparsefactorization_amd import attention_map
    from sparsefactorization_amd.lra_psf import ChangedPSF
    for name in ("chain_transposed", "attention_rows", "attention_cols"):
        assert getattr(sfa, name) is getattr(attention_map, name) and name in sfa.__all__
    assert callable(ChangedPSF.attention)


def test_supported_follows_the_rule_everywhere(lib):
    q = lib.psf_chord_chain_tr_supported
    for N in (0, 1, 2, 1023, 1024, 1025, 4097):
        for L in (0, 1, 2, 3, 19, 20, 21):
            for M in (0, 1, 2, 64, 65):
                for R in (0, 1, 3, 4, 5, 7, 8, 9, 12, 16, 20, 24, 64, 4100):
                    for eb in (2, 4):
                        assert q(N, L, R, M, eb) == int(ac.covered(N, L, R, M, eb)), (N, L, R, M, eb)
    assert q(1024, 20, 64, 64, 4) == 1 and q(1024, 20, 64, 64, 2) == 1 and q(1, 2, 4, 1, 4) == 1 and q(1, 2, 8, 1, 2) == 1
    assert q(128, 8, 4, 7, 2) == 0      # half a bf16 group
    for eb in (0, 1, 3, 8, -4):
        assert q(128, 8, 8, 7, eb) == 0  # f64 and anything else: no one launch


def _table(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _call(lib, entry, M=3, W=None, Q=0x10000, out=0x20000, scratch=0x30000, B=2, N=128, L=8, R=8, offsets=None):
    """Fake (never dereferenced) device addresses: every check below returns before a launch."""
    W = _table([0x100000 + 0x10000 * m for m in range(max(M, 1))]) if W is None else W
    return getattr(lib, entry)(W, Q, out, scratch, M, B, N, L, R, offsets, None)


@pytest.mark.parametrize("entry,elem", [("psf_chord_chain_tr_f32", 4), ("psf_chord_chain_tr_bf16", 2)])
def test_entries_validate_before_they_launch(lib, entry, elem):
    vec = 16 // elem
    call = lambda **kw: _call(lib, entry, **kw)  # noqa: E731
    # on either route: one launch (N = 128) and per step (N = 2000)
    for N in (128, 2000):
        assert call(N=N, M=0) == E_SHAPE
        assert call(N=N, M=-1) == E_SHAPE
        assert call(N=N, W=ctypes.POINTER(ctypes.c_void_p)()) == E_NULL
        assert call(N=N, Q=None) == E_NULL
        assert call(N=N, out=None) == E_NULL
        assert call(N=N, B=-1) == E_SHAPE
        assert call(N=N, L=0) == E_SHAPE
        assert call(N=N, L=65) == E_SHAPE
        assert call(N=N, R=0) == E_SHAPE
        for R in (1, vec - 1, vec + 1, 3 * vec + vec // 2):
            assert call(N=N, R=R) == E_SHAPE and b"multiple" in lib.psf_last_error(), R
        assert call(N=N, B=0) == 0                                        # an empty batch is no work ...
        assert call(N=N, B=0, Q=None) == E_NULL                           # ... after the table checks
        assert call(N=N, W=_table([0x100000, None, 0x120000])) == E_NULL and b"step 1" in lib.psf_last_error()
        assert call(N=N, out=0x10000) == E_ALIAS
        assert call(N=N, scratch=0x10000) == E_ALIAS
        assert call(N=N, scratch=0x20000) == E_ALIAS
        assert call(N=N, W=_table([0x100000, 0x110000 + elem // 2, 0x120000])) == E_ALIGN and b"step 1" in lib.psf_last_error()
        assert call(N=N, Q=0x10008) == E_ALIGN
        assert call(N=N, out=0x20004) == E_ALIGN
        assert call(N=N, scratch=0x30008) == E_ALIGN
    assert call(N=0) == E_SHAPE
    # NULL scratch: fine where one launch applies or M = 1 (the checks go on to the next fault), PSF_E_UNSUPPORTED elsewhere
    assert call(N=128, scratch=None, out=0x10000) == E_ALIAS
    assert call(N=2000, M=1, scratch=None, out=0x10000) == E_ALIAS
    for kw in (dict(N=1025), dict(N=4097), dict(L=1), dict(L=21), dict(M=65)):
        assert call(scratch=None, **kw) == E_UNSUPPORTED, kw
        assert call(scratch=None, B=0, **kw) == E_UNSUPPORTED, kw        # (as psf_chord_chain_bwd_f32: before the B == 0 return)
        assert call(out=0x10000, **kw) == E_ALIAS, kw                     # with scratch the per-step route validates on
    # bf16 W rows may start at any 2-byte address, f32 rows at any 4-byte one
    assert call(W=_table([0x100000 + elem, 0x110000 + elem, 0x120000 + elem]), out=0x10000) == E_ALIAS
    # no knob selects the route: the backward chain's knob does not reach these entries
    from sparsefactorization_amd import _lib
    with _lib.tuning(chain_bwd_fused=0):
        assert lib.psf_chord_chain_tr_supported(128, 8, 8, 7, elem) == 1
        assert call(N=128, scratch=None, out=0x10000) == E_ALIAS


def test_python_boundary_raises_without_a_device():
    import sparsefactorization_amd as sfa
    W = [torch.zeros(1, 8, 4), torch.zeros(1, 8, 4)]
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.chain_transposed(W, torch.zeros(1, 8, 4))
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.attention_rows(W, [0])
    with pytest.raises(RuntimeError, match="HIP"):
        sfa.attention_cols(W, [0])
    with pytest.raises(TypeError, match="dtype"):
        sfa.chain_transposed(W, torch.zeros(1, 8, 4, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="dtype"):
        sfa.attention_rows([W[0], W[1].double()], [0])
    with pytest.raises(ValueError):
        sfa.chain_transposed([], torch.zeros(1, 8, 4))
    with pytest.raises(ValueError):
        sfa.chain_transposed(W, torch.zeros(1, 9, 4))
