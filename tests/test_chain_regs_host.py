"""CPU: the host side of psf_chord_chain_last_f32 (csrc/fwd_chain_regs.h) — where psf_chord_chain_last_supported says yes and
no, what the entry declines or refuses before any HIP call, the describe strings, the compiled instances' registers and
scratch, and chord.py's choice between the new entry and psf_chord_chain_fwd_f32 (entries spied on: nothing is launched).

No call here reaches a launch: the entry is only ever given arguments it declines or refuses, and the Python route is checked
against stand-ins."""
import contextlib
import ctypes
import os
import subprocess

import pytest
import torch

N, L, C, M, B = 16384, 15, 8, 14, 64
E_NULL, E_SHAPE, E_ALIAS, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -4, -7


def _rule_constants():
    """(kChainRegsFillPct, kChainRegsMaxRounds) of csrc/fwd_chain_regs_launch.h; a fill of 0 = never automatic."""
    import re
    from sparsefactorization_amd import build
    text = open(os.path.join(build.CSRC, "fwd_chain_regs_launch.h")).read()
    m = re.search(r"constexpr int kChainRegsFillPct = (\d+), kChainRegsMaxRounds = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


def _cus(lib):
    """CUs of the device the library would ask; 256 where none answers (as the library assumes)."""
    import re
    buf = ctypes.create_string_buffer(256)
    m = re.search(r"cus=(\d+)", buf.value.decode()) if lib.psf_device_info(buf, 256) == 0 else None
    return int(m.group(1)) if m and int(m.group(1)) > 0 else 256


def _automatic(lib, b, c):
    """The rule restated: the grid's rounds of one workgroup per CU are at least fill % full, and no more than the measured
    number of rounds."""
    fill, max_rounds = _rule_constants()
    wgs, cus = b * c // 2, _cus(lib)
    rounds = -(-wgs // cus)
    return 1 if fill > 0 and rounds <= max_rounds and wgs * 100 >= fill * rounds * cus else 0


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()
    return _lib.load()


def _supported(lib, B=B, N=N, L=L, C=C, M=M, w_align=16, res=1, stride=None, chord=1):
    return lib.psf_chord_chain_last_supported(B, N, L, C, M, w_align, res, N * C if stride is None else stride, chord)


def test_abi_version_is_unchanged(lib):
    from sparsefactorization_amd import _lib
    assert lib.psf_version() == 2 and _lib.ABI_VERSION == 2
    for name in ("psf_chord_chain_last_f32", "psf_chord_chain_last_supported", "psf_describe_chain_last"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    # same operands as psf_chord_chain_fwd_f32 with ONE output pointer where that takes a table
    last, fwd = _lib.SIGNATURES["psf_chord_chain_last_f32"][0], _lib.SIGNATURES["psf_chord_chain_fwd_f32"][0]
    assert len(last) == len(fwd) and [i for i, (a, b) in enumerate(zip(last, fwd)) if a is not b] == [2] and last[2] is ctypes.c_void_p


def test_supported_grid(lib):
    from sparsefactorization_amd import _lib
    declines = [dict(chord=0), dict(N=8192), dict(N=16385), dict(N=16384 + 512), dict(L=14), dict(L=16), dict(C=6), dict(C=2), dict(C=0),
                dict(w_align=4), dict(w_align=8), dict(res=1, stride=0), dict(M=65), dict(M=0), dict(B=0)]
    with _lib.tuning(chain_fused=2):  # the route on request: wherever the kernel fits
        assert _supported(lib) == 1
        for kw in declines:
            assert _supported(lib, **kw) == 0, kw
        assert _supported(lib, res=0, stride=0) == 1                     # a broadcast V0 that is not the residual
        assert _supported(lib, B=1, C=4, M=1) == 1 and _supported(lib, C=12, M=64, w_align=64) == 1
    with _lib.tuning(chain_fused=0):  # never
        assert _supported(lib) == 0 and _supported(lib, B=1024) == 0
    # automatic (chain_fused = 1): where the grid fills its rounds of one workgroup per CU (csrc/fwd_chain_regs_launch.h)
    assert lib.psf_get_tuning(b"chain_fused") == 1
    grid = [(64, 8), (61, 8), (60, 8), (128, 8), (122, 8), (256, 8), (128, 4), (42, 12), (41, 12), (32, 16),   # rounds (nearly) full
            (65, 8), (72, 8), (96, 8), (43, 12), (64, 12), (129, 8), (144, 8), (257, 8), (192, 8),                 # just above a round
            (63, 4), (32, 8), (16, 8), (1, 8), (320, 8), (4096, 8)]                                                 # too few, too many
    for b, c in grid:
        assert _supported(lib, B=b, C=c) == _automatic(lib, b, c), (b, c)
    if _cus(lib) == 256 and _rule_constants() == (95, 4):  # the shipped rule on the device it was measured on, spelled out
        on = {(64, 8), (61, 8), (128, 8), (122, 8), (192, 8), (256, 8), (128, 4), (42, 12), (41, 12), (32, 16)}
        for b, c in grid:
            assert _supported(lib, B=b, C=c) == (1 if (b, c) in on else 0), (b, c)
    for kw in declines:
        assert _supported(lib, **kw) == 0, kw


def test_entry_declines_or_refuses_before_any_launch(lib):
    """Fake pointers throughout: a call that got past its checks would launch on them, so every call here is one the entry
    answers first — PSF_E_UNSUPPORTED (nothing wrong, another route's) or an argument error."""
    vp = ctypes.c_void_p
    f = lib.psf_chord_chain_last_f32
    tab = (vp * 2)(4096, 8192)
    V0, out = vp(1 << 20), vp(1 << 21)

    def call(W=tab, V0=V0, out=out, M=2, res=1, B=2, N=N, L=L, C=C, stride=None, offsets=None):
        return f(W, V0, out, M, res, B, N, L, C, N * C if stride is None else stride, offsets, None)

    i64 = ctypes.c_int64
    chord = [0] + [1 << k for k in range(L - 1)]
    custom = (i64 * L)(*(chord[:-1] + [3]))
    for kw in (dict(offsets=custom), dict(N=8192), dict(N=16385), dict(L=14), dict(C=6), dict(W=(vp * 2)(4096, 8196)),
               dict(out=vp((1 << 21) + 4)), dict(V0=vp((1 << 20) + 8)), dict(res=1, stride=0, B=1), dict(res=1, stride=0, B=2),
               dict(M=65, W=(vp * 65)(*[4096] * 65))):
        assert call(**kw) == E_UNSUPPORTED, kw
    assert call(M=0) == E_SHAPE and call(M=-1) == E_SHAPE
    assert call(W=None) == E_NULL and call(V0=None) == E_NULL and call(out=None) == E_NULL
    assert call(W=(vp * 2)(4096, None)) == E_NULL and b"step 1" in lib.psf_last_error()
    assert call(N=0) == E_SHAPE and call(L=65) == E_SHAPE and call(stride=7) == E_SHAPE
    assert call(out=V0) == E_ALIAS and call(out=vp(8192)) == E_ALIAS and b"aliases W" in lib.psf_last_error()
    assert call(out=vp((1 << 21) + 2)) == E_ALIGN and call(W=(vp * 2)(4096, 8194)) == E_ALIGN


def test_describe_strings(lib):
    from sparsefactorization_amd import _lib
    s = _lib.describe_chain_last(B, N, L, C, M)
    assert s.startswith("chord_chain_regs_k<f32,L=15,T=512,J=32> one launch for all 14 steps, X in registers, W through 4 LDS slots of 32768 bytes")
    assert "4 workgroup(s) per sequence" in s and s.endswith(", automatic" if _automatic(lib, B, C) else ", on request only")
    assert _lib.describe_chain_last(65, N, L, C, M).endswith(", automatic" if _automatic(lib, 65, C) else ", on request only")
    assert _lib.describe_chain_last(1, N, L, 4, M).endswith(", on request only")
    with _lib.tuning(chain_fused=2):
        assert _lib.describe_chain_last(1, N, L, 12, 3).endswith("6 workgroup(s) per sequence, automatic")
    with _lib.tuning(chain_fused=0):
        assert _lib.describe_chain_last(B, N, L, C, M).endswith(", on request only")
    for shape in ((B, 8192, 14, C, M), (B, N, L, 6, M), (B, N, L, C, 65)):
        assert _lib.describe_chain_last(*shape).startswith("declined (PSF_E_UNSUPPORTED)"), shape
    # the per-step describe entries are what they were at this shape
    assert _lib.describe_chain_fwd(B, N, L, C, M) == _lib.describe_fwd(B, N, L, C)
    buf = ctypes.create_string_buffer(16)
    assert lib.psf_describe_chain_last(B, N, L, C, M, None, 16) == E_NULL
    assert lib.psf_describe_chain_last(B, 0, L, C, M, buf, 16) == E_SHAPE


def test_compiled_instances_use_no_scratch_and_fit_their_registers(lib, tmp_path):
    """The unit's gfx950 assembly, made here with the build's own flags, read as tests/test_build_resources_cpu.py reads one:
    two instances (residual on and off), no scratch, at most the 256 registers a 512-thread workgroup's waves can have, the
    LDS of four W slots and the five-slot exchange ring."""
    from sparsefactorization_amd import build
    unit = [u for u in build._unit_table() if os.path.basename(u[0]) == "fwd_chain_regs.o"]
    assert len(unit) == 1 and "fwd_chain_regs" in build.NO_SCRATCH_UNITS
    _, src, extra, lint = unit[0]
    assert lint
    asm = tmp_path / "fwd_chain_regs.s"
    proc = subprocess.run([build.hipcc(), *build.HIPCC_FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", str(asm)],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    res = build.check_no_scratch("fwd_chain_regs", str(asm))
    assert len(res) == 2 and all("chord_chain_regs_k" in k for k in res)
    for name, r in res.items():
        assert r["private_segment"] == 0 and r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert r["lds"] == 4 * 32768 + 5 * 512 * 8, (name, r)
    with_res = [r for k, r in res.items() if "Lb1E" in k]
    without = [r for k, r in res.items() if "Lb0E" in k]
    assert len(with_res) == 1 and len(without) == 1 and without[0]["vgpr"] < with_res[0]["vgpr"]


class _Stub:
    """Stands in for the loaded library in chord._chain_forward_raw: the host-only question goes to the real library, the two
    launching entries only record that they were asked."""

    def __init__(self, real):
        self.psf_chord_chain_last_supported = real.psf_chord_chain_last_supported
        self.calls = []
        self.decline = False  # the entry answers PSF_E_UNSUPPORTED although `supported` said yes (a knob changed in between)
        self.out_ptr = None

    def psf_chord_chain_last_f32(self, *a):
        self.calls.append("last")
        self.out_ptr = a[2]
        return E_UNSUPPORTED if self.decline else 0

    def psf_chord_chain_fwd_f32(self, *a):
        self.calls.append("fwd")
        return 0


@pytest.fixture
def routed(lib, monkeypatch):
    """chord._chain_forward_raw on CPU tensors with everything that touches a device replaced; yields (call, stub)."""
    from sparsefactorization_amd import chord
    stub = _Stub(lib)
    monkeypatch.setattr(chord._lib, "load", lambda: stub)
    monkeypatch.setattr(chord, "_require_hip", lambda *t: torch.device("cpu"))
    monkeypatch.setattr(chord, "_stream_ptr", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())

    def call(Ws, V0, offsets=None, keep_all=False, res=True):
        del stub.calls[:]
        outs = chord._chain_forward_raw(V0, res, offsets, Ws, keep_all)[2]
        return list(stub.calls), outs

    assert lib.psf_set_tuning(b"chain_fused", 2) == 0  # the route on request (_lib.tuning would ask the stand-in)
    try:
        call.stub = stub
        yield call
    finally:
        assert lib.psf_set_tuning(b"chain_fused", 1) == 0


def test_chord_py_falls_back_for_what_the_entry_does_not_take(routed):
    Bs, Cs, Ms = 1, 4, 2
    Ws = [torch.zeros(Bs, N, L) for _ in range(Ms)]
    V0 = torch.zeros(Bs, N, Cs)
    assert all(w.data_ptr() % 16 == 0 for w in Ws) and V0.data_ptr() % 16 == 0
    calls, outs = routed(Ws, V0)
    assert calls == ["last"] and len(outs) == 1 and outs[0].shape == (Bs, N, Cs)  # one output buffer, not two
    assert routed(Ws, V0, offsets=tuple([0] + [1 << k for k in range(L - 1)]))[0] == ["last"]  # the chord offsets, spelled out
    # a W one float off a 16-byte boundary (a contiguous view into a larger buffer)
    big = torch.zeros(Bs * N * L + 4)
    off1 = big[1:1 + Bs * N * L].view(Bs, N, L)
    assert off1.is_contiguous() and off1.data_ptr() % 16 == 4
    calls, outs = routed([Ws[0], off1], V0)
    assert calls == ["fwd"] and len({o.data_ptr() for o in outs}) == 2
    # a custom offset list
    assert routed(Ws, V0, offsets=tuple([0] + [1 << k for k in range(L - 2)] + [3]))[0] == ["fwd"]
    # every step kept (training), another dtype, another length
    assert routed(Ws, V0, keep_all=True)[0] == ["fwd"]
    assert routed([torch.zeros(Bs, 8192, 14) for _ in range(Ms)], torch.zeros(Bs, 8192, Cs))[0] == ["fwd"]


def test_a_declined_entry_is_counted_and_its_buffer_reused(routed):
    """psf_chord_chain_last_supported says yes, the entry then declines: the per-step route runs, chord.chain_last_declined
    counts it, and the output buffer already allocated becomes the route's first buffer instead of being thrown away."""
    from sparsefactorization_amd import chord
    Ws = [torch.zeros(1, N, L) for _ in range(3)]
    V0 = torch.zeros(1, N, 4)
    before = chord.chain_last_declined
    routed.stub.decline = True
    calls, outs = routed(Ws, V0)
    assert calls == ["last", "fwd"] and chord.chain_last_declined == before + 1
    assert len(outs) == 3 and outs[0].data_ptr() == routed.stub.out_ptr and outs[2] is outs[0] and outs[1] is not outs[0]
    routed.stub.decline = False
    assert routed(Ws, V0)[0] == ["last"] and chord.chain_last_declined == before + 1
