"""The grid of test_routes_host.py: which kernels the host dispatcher (csrc/psf_chord.hip) names for a shape, over every
branch of its planning code, and the tool that records a library's answers as tests/golden/routes_parent.json.

    python tests/route_grid.py /path/to/libpsf_chord.so <commit hash of that build> [out.json]

Per case: return code and string of psf_describe_fwd, psf_describe_bwd and psf_describe_chain_fwd_dtype, and the return values
of psf_chord_chain_bwd_supported, psf_mixer_fwd_plan and psf_mixer_fwd_workspace. First under the default knobs over the whole
grid, then with one knob off its default at a time over a thinned grid. No device is touched: none of these entries launches.

The file holds every distinct answer once (``strings``: base64 of zlib of the answers, one per line) and, per group of
cases, the indices of the answers in grid order (``groups``: base64 of zlib of little-endian uint32), so a replay can name the
very case that differs. ``load`` reads it back."""
import array
import base64
import ctypes
import itertools
import json
import os
import sys
import zlib

ELEMS = (2, 4, 8)
BS = (0, 1, 2, 16, 64)
NS = (1, 31, 64, 128, 255, 256, 511, 512, 1024, 1025, 2000, 2048, 2049, 2112, 2113, 4096, 4097, 4160, 4161, 8192, 16384)
# One more length, with rows of 8 channels. And with rows of 2^31 bytes per batch element in f32 (1024 channels) and in bf16
# (2048): with chord offsets every far offset is a multiple of a tile that divides N, so only that size limit takes a launch
# of full tiles off the aligned form ("tiles=full" without ", aligned").
N_LONG, CS_LONG = 1 << 19, (8, 1024, 2048)
LS = (1, 3, 4, 7, 11, 12, 15, 20, 21)
CS = (1, 4, 6, 8, 12, 16, 24, 32, 64, 96, 128, 136, 256, 1024)
MS = (1, 2, 14, 33)
NS_THIN, CS_THIN = (255, 1024, 2000, 4097, 16384), (8, 32, 64, 128)

# knob -> every legal value (the first is the default, which the first pass covers)
KNOBS = {
    "fwd_variant": (0, 1, 2), "bwd_variant": (0, 1), "fwd_split": (1, 0, 2), "fwd_wide": (0, 1, 2, 3, 4),
    "fwd_rows": (0, 1, 2, 3, 4), "dv_threads": (0, 1), "dw_variant": (0, 1, 2), "dw_tgs": (0, 1, 2, 3, 4, 5),
    "bwd_fused": (1, 0, 2), "bwd_fronts": (0, 1, 2, 3, 4, 5, 6, 7, 8), "chain_fused": (1, 0, 2), "chain_cc": (0, 1, 2),
    "chain_bwd_fused": (1, 0), "mixer_lds": (1, 0),
}

# What the recorded strings must contain at least once each, or the grid no longer reaches the dispatcher's branches:
# (name, substrings that one string must hold together)
FAMILIES = [(f"fwd window {ty} tiles={tiles}", (f"chord_fwd_win_k<{ty},", f"tiles={tiles}"), exact)
            for ty in ("f32", "bf16")
            for tiles, exact in (("edge", True), ("full+ragged", True), ("full", True), ("full, aligned", False))]
FAMILIES += [(name, subs, False) for name, subs in [
    ("wide rows", ("chord_fwd_win_k<f32,", "NT=1024>")), ("four rows", ("chord_fwd_win_k<f32,", "R=4,")),
    ("dV on 512 threads", ("chord_dv_win_k<f32,", "NT=512>")), ("generic forward, scalar", ("chord_fwd_generic_k<", "VEC=1>")),
    ("fused step f32", ("chord_bwd_fused_k<f32,",)), ("fused edge step", ("chord_bwd_fused_edge_k<f32,",)),
    ("fused step bf16", ("chord_bwd_fused_k<bf16,",)), ("chunk dW TG=8", ("chord_dw_chunk_k<f32,", "TG=8,")),
    ("chunk dW TG=16", ("chord_dw_chunk_k<f32,", "TG=16,")), ("window dW", ("chord_dw_win_k<",)), ("window dV", ("chord_dv_win_k<",)),
    ("generic dW", ("chord_dw_generic_k<",)), ("generic dV", ("chord_dv_generic_k<",)), ("two fronts", ("fronts=2",)),
] + [(f"chain {k} {ty}{' G=%d' % g if g else ''}", (f"chord_chain_{k}_k<{ty},",) + ((f"G={g},",) if g else ()))
     for ty in ("f32", "bf16") for k, g in (("lds", 0), ("rows", 1), ("rows", 2))]]


def missing_families(strings):
    """Names of the FAMILIES that no string of `strings` shows."""
    out = []
    for name, subs, exact_tiles in FAMILIES:
        def shows(s):
            if not all(x in s for x in subs):
                return False
            return not exact_tiles or s.endswith(subs[-1])  # "tiles=full" is not "tiles=full+ragged" / "full, aligned"
        if not any(shows(s) for s in strings):
            out.append(name)
    return out


def shapes(thin):
    """(N, C) pairs."""
    if thin:
        return list(itertools.product(NS_THIN, CS_THIN))
    return list(itertools.product(NS, CS)) + [(N_LONG, C) for C in CS_LONG]


def _mixer_cases(thin):
    ns, es, ms, cs = (NS_THIN, (8, 32), (2, 14), (8, 32)) if thin else (NS + (N_LONG,), (3, 4, 8, 32, 36), MS, (1, 4, 6, 8, 12, 16, 32, 64))
    for N, E, M, kind, C, L in itertools.product(ns, es, ms, range(2 if thin else 5), cs, LS):
        h = ([32] * (M + 1), [1] + [128] * M, [33] * (M + 1), [129] + [32] * M, None)[kind]
        yield N, E, M, h, C, L


def open_lib(path):
    from sparsefactorization_amd import _lib
    lib = ctypes.CDLL(path)
    for name, (argtypes, restype) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    return lib


def group_cases(lib, thin):
    """Yields (group, label, answer) in grid order under the knobs as they stand: label is a tuple that names the case, answer
    a string."""
    buf = ctypes.create_string_buffer(512)

    def described(fn, *args):
        buf.value = b""
        rc = fn(*args, buf, 512)
        return f"{rc}:{buf.value.decode()}"

    nc = shapes(thin)
    for e in ELEMS:
        for B, (N, C), L in itertools.product(BS, nc, LS):
            yield f"fwd/e{e}", (B, N, L, C), described(lib.psf_describe_fwd, B, N, L, C, e)
    for e in ELEMS:
        for B, (N, C), L in itertools.product(BS, nc, LS):
            yield f"bwd/e{e}", (B, N, L, C), described(lib.psf_describe_bwd, B, N, L, C, e)
    for e in (2, 4):
        for B, (N, C), L, M in itertools.product(BS, nc, LS, MS):
            yield f"chain/e{e}", (B, N, L, C, M), described(lib.psf_describe_chain_fwd_dtype, B, N, L, C, M, e)
    for (N, C), L, M in itertools.product(nc, LS, MS):
        yield "chain_bwd_supported", (N, L, C, M), str(lib.psf_chord_chain_bwd_supported(N, L, C, M))
    for N, E, M, h, C, L in _mixer_cases(thin):
        harr = (ctypes.c_int32 * len(h))(*h) if h is not None else None
        yield "mixer", (N, E, M, h, C, L), "%d,%d" % (lib.psf_mixer_fwd_plan(N, E, M, harr, C, L),
                                                      lib.psf_mixer_fwd_workspace(N, E, M, harr, C, L))
    if not thin:  # arguments the entries refuse
        for e, (B, N, L, C) in itertools.product((0, 3, 8, 16), ((2, 1024, 11, 8), (2, 0, 11, 8), (2, 1024, 65, 8), (-1, 1024, 11, 8), (2, 1024, 0, 8))):
            yield "refused", ("fwd", B, N, L, C, e), described(lib.psf_describe_fwd, B, N, L, C, e)
            yield "refused", ("bwd", B, N, L, C, e), described(lib.psf_describe_bwd, B, N, L, C, e)
            yield "refused", ("chain", B, N, L, C, e), described(lib.psf_describe_chain_fwd_dtype, B, N, L, C, 3, e)


def settings():
    """(name, knob or None, value): the defaults, then one knob off its default at a time."""
    yield "default", None, None
    for knob, values in KNOBS.items():
        for v in values[1:]:
            yield f"{knob}={v}", knob, v


def replay(lib):
    """Yields (setting/group, label, answer) over the whole grid; every knob it sets is restored, also when the consumer stops."""
    for name, knob, value in settings():
        saved = None
        if knob is not None:
            saved = lib.psf_get_tuning(knob.encode())
            assert saved == KNOBS[knob][0], f"{knob} is {saved}, not its default {KNOBS[knob][0]}: another test left it set"
            assert lib.psf_set_tuning(knob.encode(), value) == 0, (knob, value)
        try:
            for group, label, answer in group_cases(lib, knob is not None):
                yield f"{name}/{group}", label, answer
        finally:
            if knob is not None:
                lib.psf_set_tuning(knob.encode(), saved)


def pack(indices):
    return base64.b64encode(zlib.compress(array.array("I", indices).tobytes(), 9)).decode()


def unpack(text):
    a = array.array("I")
    a.frombytes(zlib.decompress(base64.b64decode(text)))
    return a


def record(lib, parent):
    assert array.array("I").itemsize == 4
    strings, index, groups = [], {}, {}
    for group, _label, answer in replay(lib):
        if answer not in index:
            index[answer] = len(strings)
            strings.append(answer)
        groups.setdefault(group, []).append(index[answer])
    assert not any("\n" in s for s in strings)
    return {"parent": parent, "cases": sum(len(g) for g in groups.values()),
            "strings": base64.b64encode(zlib.compress("\n".join(strings).encode(), 9)).decode(),
            "groups": {g: pack(ix) for g, ix in groups.items()}}


def load(path):
    """(parent hash, distinct answers, {group: indices}) of a recorded file."""
    with open(path) as fh:
        doc = json.load(fh)
    strings = zlib.decompress(base64.b64decode(doc["strings"])).decode().split("\n")
    return doc["parent"], strings, {g: unpack(t) for g, t in doc["groups"].items()}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routes_parent.json")
    doc = record(open_lib(sys.argv[1]), sys.argv[2])
    with open(out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    answers = load(out)[1]
    gone = missing_families(answers)
    assert not gone, f"the grid does not reach: {gone}"
    print(f"{out}: {doc['cases']} cases, {len(answers)} distinct answers, {os.path.getsize(out)} bytes")
