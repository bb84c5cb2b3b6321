"""CPU: tests/ptr_audit.py on a fake library — what it reports, what it leaves alone, that it cleans up, and that its table of
argument positions is the one include/psf_chord.h declares."""
import ctypes
import os
import re

import pytest
import torch

import ptr_audit
from conftest import ROOT
from sparsefactorization_amd import _lib

F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64


class FakeLib:
    """Entry points that only count their calls (the real names: the audit reads their signatures from ``_lib.SIGNATURES``)."""

    def __init__(self):
        self.calls = []
        for name in ("psf_linear_wgrad_strided_f32", "psf_sum_tensors_f32", "psf_sum_tensors_bf16", "psf_embed_tokens_f32",
                     "psf_embed_tokens_bwd_f32", "psf_mixer_fwd_in_f32", "psf_mlp_wide_bwd_f32", "psf_chord_spmm_fwd_f64"):
            setattr(self, name, self._entry(name))

    def _entry(self, name):
        def entry(*args):
            self.calls.append(name)
            return 0
        return entry


def _table(*tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _wgrad(lib, x, dy, dW, db, ws, stream=0):
    return lib.psf_linear_wgrad_strided_f32(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), x.shape[0], x.shape[1], dy.shape[1],
                                            dW.data_ptr(), db.data_ptr() if db is not None else None, ws.data_ptr(), ws.numel(), stream)


def _operands(dy_dtype=F32):
    return (torch.zeros(16, 4), torch.zeros(16, 3, dtype=dy_dtype), torch.zeros(3, 4), torch.zeros(3), torch.zeros(64, dtype=torch.uint8))


def test_clean_call_passes_and_the_call_goes_through(monkeypatch):
    lib = FakeLib()
    with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES) as a:
        assert _wgrad(lib, *_operands()) == 0
    assert lib.calls == ["psf_linear_wgrad_strided_f32"] and a.checked == 5 and not a.violations


def test_bf16_tensor_in_an_f32_entry_is_reported(monkeypatch):
    lib = FakeLib()
    with pytest.raises(ptr_audit.PointerAuditError) as err:
        with ptr_audit.audit(monkeypatch, lib):  # (``signatures`` left out: _lib.SIGNATURES, whatever ``lib`` is)
            _wgrad(lib, *_operands(BF16))
    assert err.value.violations == [("psf_linear_wgrad_strided_f32", 2, BF16, (F32,))]
    assert "argument 2: torch.bfloat16 (96 bytes), the entry reads torch.float32" in str(err.value)  # 16 x 3 bf16
    assert lib.calls == ["psf_linear_wgrad_strided_f32"]  # reported at the end of the block, the call itself is made


def test_refusing_form_raises_before_the_call_is_made(monkeypatch):
    """``refuse=True`` (the GPU tests): the offending call never reaches the library."""
    lib = FakeLib()
    with pytest.raises(ptr_audit.PointerAuditError) as err:
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES, refuse=True):
            _wgrad(lib, *_operands())
            _wgrad(lib, *_operands(BF16))
            pytest.fail("the call returned")
    assert err.value.violations == [("psf_linear_wgrad_strided_f32", 2, BF16, (F32,))]
    assert lib.calls == ["psf_linear_wgrad_strided_f32"]  # the clean call only


def test_bf16_tensor_in_a_pointer_table_is_reported(monkeypatch):
    lib = FakeLib()
    terms = [torch.zeros(8), torch.zeros(8, dtype=BF16), torch.zeros(8)]
    out = torch.zeros(8)
    with pytest.raises(ptr_audit.PointerAuditError) as err:
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
            lib.psf_sum_tensors_f32(_table(*terms), 3, 8, out.data_ptr(), None)
    assert err.value.violations == [("psf_sum_tensors_f32", (0, 1), BF16, (F32,))]
    # ... and the other way round: f32 terms in the bf16 entry, and an f32 tensor in an _f64 entry
    with pytest.raises(ptr_audit.PointerAuditError) as err:
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
            lib.psf_sum_tensors_bf16(_table(terms[1], terms[0]), 2, 8, terms[1].data_ptr(), None)
            lib.psf_chord_spmm_fwd_f64(out.data_ptr(), None, None, None, 1, 8, 1, 1, 8, None, None)
    assert err.value.violations == [("psf_sum_tensors_bf16", (0, 1), F32, (BF16,)), ("psf_chord_spmm_fwd_f64", 0, F32, (torch.float64,))]


def test_the_latest_record_of_an_address_wins(monkeypatch):
    """The allocator reuses addresses: an address asked as bf16 and then again as f32 is an f32 tensor for the next call."""
    lib = FakeLib()
    x, dy, dW, db, ws = _operands()
    raw = torch.zeros(16 * 3 * 2, dtype=BF16)
    with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES) as a:
        stale = raw.data_ptr()
        dy = raw.view(F32).reshape(16, 3)
        assert dy.data_ptr() == stale and a.seen[stale][0] == F32
        _wgrad(lib, x, dy, dW, db, ws)
    assert not a.violations and a.checked == 5


def test_int32_ids_at_an_index_position_are_reported(monkeypatch):
    lib = FakeLib()
    table, out, dout, ws = torch.zeros(6, 4), torch.zeros(10, 4), torch.zeros(10, 4), torch.zeros(32)
    for dtype in (torch.int32, torch.int16, torch.uint8):
        idx = torch.zeros(10, dtype=dtype)
        with pytest.raises(ptr_audit.PointerAuditError) as err:
            with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
                lib.psf_embed_tokens_f32(idx.data_ptr(), table.data_ptr(), None, out.data_ptr(), 10, 10, 6, 4, None)
                lib.psf_embed_tokens_bwd_f32(idx.data_ptr(), dout.data_ptr(), 10, 6, 4, table.data_ptr(), ws.data_ptr(), 128, None)
        assert err.value.violations == [("psf_embed_tokens_f32", 0, dtype, (I64,)), ("psf_embed_tokens_bwd_f32", 0, dtype, (I64,))]
    idx = torch.zeros(10, dtype=I64)
    with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES) as a:
        lib.psf_embed_tokens_bwd_f32(idx.data_ptr(), dout.data_ptr(), 10, 6, 4, table.data_ptr(), ws.data_ptr(), 128, None)
    assert a.checked == 4
    # an f32 tensor where ids are read is as wrong as int32 ids
    with pytest.raises(ptr_audit.PointerAuditError):
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
            lib.psf_embed_tokens_f32(table.data_ptr(), table.data_ptr(), None, out.data_ptr(), 10, 10, 6, 4, None)


def test_mixer_input_members_are_judged_by_kind(monkeypatch):
    lib = FakeLib()
    ids32, ids64, table, pos = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=I64), torch.zeros(6, 4), torch.zeros(8, 4, dtype=BF16)
    rest = (1, 8, 4, 1, None, None, None, None, None, 4, 4, 0, None, None, None, 0, None)
    with pytest.raises(ptr_audit.PointerAuditError) as err:
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
            for ids in (ids64, ids32):
                spec = _lib.MixerInput(_lib.MIXER_IN_TOKENS, 6, ids.data_ptr(), table.data_ptr(), None, pos.data_ptr())
                lib.psf_mixer_fwd_in_f32(ctypes.byref(spec), *rest)
            spec = _lib.MixerInput(_lib.MIXER_IN_DATA, 0, ids64.data_ptr(), None, None, None)  # rows must be floats
            lib.psf_mixer_fwd_in_f32(ctypes.byref(spec), *rest)
    name = "psf_mixer_fwd_in_f32"
    assert err.value.violations == [(name, (0, "pos"), BF16, (F32,)), (name, (0, "src"), torch.int32, (I64,)),
                                    (name, (0, "pos"), BF16, (F32,)), (name, (0, "src"), I64, (F32,))]


def test_scratch_positions_take_bytes_or_floats_only(monkeypatch):
    lib = FakeLib()
    for dtype, ok in ((torch.uint8, True), (F32, True), (BF16, False), (torch.int32, False)):
        saved, ws = torch.zeros(64, dtype=dtype), torch.zeros(64, dtype=torch.uint8)
        try:
            with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES) as a:
                lib.psf_mlp_wide_bwd_f32(saved.data_ptr(), 64, 1, 16, 1, None, None, None, None, None, None, None, None, None, None,
                                         ws.data_ptr(), 64, None)
            assert ok and a.checked == 2
        except ptr_audit.PointerAuditError as e:
            assert not ok and e.violations == [("psf_mlp_wide_bwd_f32", 0, dtype, ptr_audit._SCRATCH)]


def test_pointers_the_recorder_never_saw_are_ignored(monkeypatch):
    lib = FakeLib()
    x, _, dW, db, ws = _operands()
    early = torch.zeros(16, 3, dtype=BF16)
    address = early.data_ptr()  # asked before the block: no record — the audit judges what it saw, it does not guess
    with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES) as a:
        lib.psf_linear_wgrad_strided_f32(x.data_ptr(), 4, address, 3, 16, 4, 3, dW.data_ptr(), None, ws.data_ptr(), 64, 0xDEADBEEF)
        lib.psf_linear_wgrad_strided_f32(None, 4, None, 3, 16, 4, 3, None, None, None, 64, None)
        bad = torch.zeros(4, dtype=BF16)
        lib.psf_linear_wgrad_strided_f32(None, 4, None, 3, 16, 4, 3, None, None, None, 64, bad.data_ptr())  # the stream position
    assert not a.violations and a.checked == 3 and len(lib.calls) == 3


def test_data_ptr_is_restored_and_the_wrappers_go_inert(monkeypatch):
    lib = FakeLib()
    before = torch.Tensor.data_ptr
    assert "data_ptr" not in torch.Tensor.__dict__
    with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
        assert torch.Tensor.data_ptr is not before
    assert torch.Tensor.data_ptr is before and "data_ptr" not in torch.Tensor.__dict__
    with pytest.raises(KeyError):  # the body's own exception comes out as it is, not the audit's
        with ptr_audit.audit(monkeypatch, lib, _lib.SIGNATURES):
            _wgrad(lib, *_operands(BF16))
            raise KeyError("body")
    assert torch.Tensor.data_ptr is before and "data_ptr" not in torch.Tensor.__dict__
    assert _wgrad(lib, *_operands(BF16)) == 0  # outside a block the wrappers pass everything through
    monkeypatch.undo()
    assert lib.psf_linear_wgrad_strided_f32.__name__ == "entry"


# ------------------------------------------------------------------------------------------- the table against the header
def _prototypes():
    """{entry: [parameter type, ...]} of include/psf_chord.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "psf_chord.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(psf_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [p.strip() for p in m.group(2).split(",")]
        out[m.group(1)] = [] if params == ["void"] else [re.sub(r"\s*\w+$", "", p).replace(" ", "") for p in params]
    return out


def test_the_wanted_dtypes_are_what_the_header_declares():
    """Every ``c_void_p`` / ``POINTER(c_void_p)`` position of every typed entry: the header's parameter type is the dtype the audit
    asks for — float / uint16_t / double by the suffix, int64_t at the index positions, void at the scratch positions and for
    the stream, psf_mixer_input for the mixer's recipe."""
    by_c = {"constfloat*": (F32,), "float*": (F32,), "constuint16_t*": (BF16,), "uint16_t*": (BF16,), "constdouble*": (torch.float64,),
            "double*": (torch.float64,), "constint64_t*": (I64,), "void*": ptr_audit._SCRATCH, "constvoid*": ptr_audit._SCRATCH}
    protos = _prototypes()
    judged = 0
    for entry, (argtypes, _) in _lib.SIGNATURES.items():
        assert entry in protos and len(protos[entry]) == len(argtypes), entry
        if ptr_audit.element_type(entry) is None:
            assert not any(t in (ptr_audit._VP, ptr_audit._VPP) for t in argtypes), entry  # host-only entries take no device pointer
            continue
        assert argtypes[-1] is ptr_audit._VP and protos[entry][-1] == "void*", entry       # void* stream closes every typed entry
        for i, (ctype, decl) in enumerate(zip(argtypes, protos[entry])):
            want = ptr_audit.wanted(entry, i, _lib.SIGNATURES)
            if ctype is ptr_audit._VPP:    # ``const float* const*``: a host table of device pointers
                assert by_c[decl.replace("*const*", "*")] == want, (entry, i, decl)
            elif ctype is not ptr_audit._VP:
                assert want == ()
            elif i == len(argtypes) - 1:
                assert want == ()
            elif decl == "constpsf_mixer_input*":
                assert entry in ptr_audit.MIXER_INPUT and i == 0
            else:
                assert by_c[decl] == want, (entry, i, decl, want)
            judged += bool(want)
    assert judged > 150
    assert set(ptr_audit.MIXER_INPUT) == {e for e, p in protos.items() if "constpsf_mixer_input*" in p}
