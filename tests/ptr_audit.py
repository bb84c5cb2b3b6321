"""The dtype of every tensor whose address reaches an entry point of libpsf_chord.so, checked at the Python boundary.

The wrappers hand ``tensor.data_ptr()`` to C entries that are typed only by their name (``..._f32``, ``const int64_t* idx``): a
bf16 gradient in an ``_f32`` entry, or int32 ids where int64 are read, computes garbage from a read past the buffer's end and
nothing on the host notices. ``audit(monkeypatch)`` notices:

1. ``torch.Tensor.data_ptr`` is replaced by a recorder, address -> (dtype, nbytes) of the tensor asked LAST (the caching
   allocator hands a freed address to the next tensor, so the latest record is the one a following call means);
2. every entry of ``_lib.SIGNATURES`` on the loaded library is wrapped (as ``Spy`` of tests/test_gpu_model_twin.py wraps them).
   On each call every ``c_void_p`` argument, every element of every ``POINTER(c_void_p)`` table and the pointer members of a
   ``psf_mixer_input`` are looked up in the record, and a hit must have the dtype the entry reads there (``wanted``): the
   element type of the entry's suffix, int64 at the index positions, uint8 or float32 at the ``void* workspace`` / ``saved``
   positions of include/psf_chord.h. Addresses the recorder never saw (streams, NULL, host arrays) are not judged.

Violations are collected as (entry, argument position, dtype found, dtypes wanted) and raised when the block ends. Only host
pointers are looked at: nothing here reads a kernel.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools

import torch

_ELEM = {"_f32": torch.float32, "_bf16": torch.bfloat16, "_f64": torch.float64}
_SCRATCH = (torch.uint8, torch.float32)  # ``void* workspace`` / ``void* saved``: bytes, or floats where the wrapper counts in floats
_VP, _VPP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)

#: (entry, argument position) -> dtypes accepted there, where that is not the element type of the entry's suffix
#: (include/psf_chord.h: ``const int64_t* idx``, ``void* workspace``, ``void* saved`` / ``const void* saved``)
SPECIAL = {
    ("psf_embed_tokens_f32", 0): (torch.int64,),
    ("psf_embed_tokens_bwd_f32", 0): (torch.int64,),
    ("psf_embed_tokens_bwd_f32", 6): _SCRATCH,
    ("psf_linear_wgrad_f32", 7): _SCRATCH,
    ("psf_linear_wgrad_strided_f32", 9): _SCRATCH,
    ("psf_flat_head_f32", 7): _SCRATCH,
    ("psf_mlp_fwd_f32", 11): _SCRATCH,
    ("psf_mlp_fwd_bf16", 11): _SCRATCH,
    ("psf_mixer_fwd_f32", 15): _SCRATCH,
    ("psf_mixer_fwd_in_f32", 15): _SCRATCH,
    ("psf_mixer_fwd_bf16", 15): _SCRATCH,
    ("psf_mlp_bwd_f32", 15): _SCRATCH,
    ("psf_mlp_bwd_bf16", 15): _SCRATCH,
    ("psf_mlp_wide_fwd_f32", 11): _SCRATCH,
    ("psf_mlp_wide_fwd_f32", 13): _SCRATCH,
    ("psf_mlp_wide_bwd_f32", 0): _SCRATCH,
    ("psf_mlp_wide_bwd_f32", 15): _SCRATCH,
}
#: entries whose first argument is a ``const psf_mixer_input*``; ``src`` is typed by ``kind`` (index 2: int64 tokens)
MIXER_INPUT = ("psf_mixer_fwd_in_f32",)
_MIXER_SRC = {0: (torch.float32,), 1: (torch.float32,), 2: (torch.int64,)}


def element_type(entry: str):
    """The dtype an entry reads by its suffix, or None (host-only entries: describe, workspace, tuning)."""
    return next((dt for suffix, dt in _ELEM.items() if entry.endswith(suffix)), None)


def wanted(entry: str, position: int, signatures) -> tuple:
    """The dtypes a device pointer at ``position`` of ``entry`` may have; () where the position is no data pointer (sizes, host
    tables of int32 / int64, the stream: the last ``void*`` of every entry)."""
    argtypes = signatures[entry][0]
    elem = element_type(entry)
    if elem is None or argtypes[position] not in (_VP, _VPP):
        return ()
    if argtypes[position] is _VP and position == len(argtypes) - 1:
        return ()  # void* stream
    return SPECIAL.get((entry, position), (elem,))


class PointerAuditError(AssertionError):
    def __init__(self, violations, nbytes=()):
        """``nbytes``: per violation, the size of the tensor found (the message says how much of it the entry's type misreads)."""
        self.violations = list(violations)
        sizes = list(nbytes) + [None] * (len(self.violations) - len(nbytes))
        super().__init__("tensors of a dtype the entry does not read:\n" + "\n".join(
            f"  {e} argument {p}: {found}" + ("" if n is None else f" ({n} bytes)") + f", the entry reads {' or '.join(map(str, want))}"
            for (e, p, found, want), n in zip(self.violations, sizes)))


class Audit:
    def __init__(self, signatures, refuse=False):
        self.signatures = signatures
        self.refuse = refuse  # raise at the offending call, before it is made (the GPU tests: no such launch ever happens)
        self.seen = {}        # address -> (dtype, nbytes)
        self.violations = []  # (entry, position, dtype found, dtypes wanted)
        self.nbytes = []      # per violation: the size of the tensor found, for the report
        self.checked = 0     # pointers that were found in the record and judged
        self.active = False

    def record(self, real, tensor):
        p = real(tensor)
        if self.active and p:
            self.seen[p] = (tensor.dtype, tensor.numel() * tensor.element_size())
        return p

    def _judge(self, entry, position, address, want):
        if isinstance(address, ctypes.c_void_p):
            address = address.value
        if not isinstance(address, int) or not address:
            return
        hit = self.seen.get(address)
        if hit is None:
            return
        self.checked += 1
        if hit[0] not in want:
            self.violations.append((entry, position, hit[0], want))
            self.nbytes.append(hit[1])

    def call(self, entry, real, *args):
        if self.active:
            argtypes = self.signatures[entry][0]
            for i, arg in enumerate(args[:len(argtypes)]):
                if i == 0 and entry in MIXER_INPUT:
                    spec = getattr(arg, "_obj", arg)  # ctypes.byref(spec), or the structure itself
                    if hasattr(spec, "kind"):
                        self._judge(entry, (0, "src"), spec.src, _MIXER_SRC.get(spec.kind, ()))
                        for member in ("weight", "bias", "pos"):
                            self._judge(entry, (0, member), getattr(spec, member), (torch.float32,))
                    continue
                want = wanted(entry, i, self.signatures)
                if not want or arg is None:
                    continue
                if argtypes[i] is _VPP:
                    for j, address in enumerate(arg):
                        self._judge(entry, (i, j), address, want)
                else:
                    self._judge(entry, i, arg, want)
            if self.refuse and self.violations:
                raise PointerAuditError(self.violations, self.nbytes)
        return real(*args)


@contextlib.contextmanager
def audit(monkeypatch, lib=None, signatures=None, refuse=False):
    """``with audit(monkeypatch) as a:`` — record and judge for the length of the block; PointerAuditError at its end if anything
    was found (an exception of the body itself is passed on as it is). ``lib`` / ``signatures``: the loaded library and
    ``_lib.SIGNATURES`` by default. The wrappers of the entries stay in place (inert) until ``monkeypatch`` is undone, so that
    they nest with other wrappers of the same entries in either order; ``data_ptr`` is put back when the block ends.
    ``refuse``: raise at the first offending call INSTEAD of making it — what the GPU tests use, so that a wrapper that is wrong
    fails its test without the launch that would read past a buffer."""
    from sparsefactorization_amd import _lib
    lib = _lib.load() if lib is None else lib
    signatures = _lib.SIGNATURES if signatures is None else signatures
    a = Audit(signatures, refuse)
    for name in signatures:
        real = getattr(lib, name, None)
        if real is not None and element_type(name) is not None:
            monkeypatch.setattr(lib, name, functools.partial(a.call, name, real), raising=False)
    real_data_ptr = torch.Tensor.data_ptr

    def data_ptr(self):
        return a.record(real_data_ptr, self)

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "data_ptr", data_ptr)
        a.active = True
        try:
            yield a
        finally:
            a.active = False
    if a.violations:
        raise PointerAuditError(a.violations, a.nbytes)
