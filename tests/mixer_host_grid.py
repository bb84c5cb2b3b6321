"""The grid of test_mixer_host_parent.py: what the host side of the mixer entries (csrc/psf_chord.hip: psf_mixer_fwd_plan,
psf_mixer_fwd_workspace, their bf16 twins, and the validation of psf_mixer_fwd_f32 / psf_mixer_fwd_in_f32 / psf_mixer_fwd_bf16)
answers, and the tool that records a checkout's answers as tests/golden/mixer_host_parent.json.

    python tests/mixer_host_grid.py /path/to/checkout <commit hash of that checkout> [out.json]

Two kinds of case, each asked with the knob ``mixer_lds`` = 1 and = 0:

* shapes: "plan,workspace,bf16 plan,bf16 workspace" of (N, E, M, hidden widths, C, L). Each argument is varied alone around six base
  shapes (BASES), over lists that cross every limit of plan_mixer, plan_mixer_lds and plan_mixer_lds_bf16 from both sides; then the
  full cross of short N x C x L lists at two hidden widths.
* calls: "return code:psf_last_error()" of an entry called with FAKE pointers. Only calls that are answered before the first HIP
  call are listed (a PSF_E_* code, or PSF_OK for B = 0; ``answers`` asserts it): every NULL argument, every fault of every
  kind of psf_mixer_input, recipes where no single-launch kernel runs, B, the workspace, X / V0 / pos, table entries and step
  outputs at the first, a middle and the last place, and pairs of faults, which pin the order of the checks. A call that only
  one value of the knob rejects before the first HIP call is listed under that value alone (``lds``)."""
import ctypes
import itertools
import json
import os
import sys

i32, vp = ctypes.c_int32, ctypes.c_void_p
DATA, AFFINE, TOKENS = 0, 1, 2

# (N, E, M, hidden width, C, L): the two BASELINE synthetic shapes, Pathfinder, CIFAR-10, IMDb (LRA), and a bf16 network
BASES = ((128, 32, 7, 32, 8, 8), (16384, 32, 14, 32, 8, 15), (1024, 32, 11, 128, 32, 12), (1024, 16, 10, 16, 16, 11),
         (4097, 32, 12, 128, 32, 13), (512, 64, 7, 32, 16, 8))
FACTORS = {
    "N": (0, 31, 32, 64, 100, 127, 128, 255, 256, 257, 480, 512, 513, 544, 1000, 1024, 1056, 2048, 4097, 16384, 1 << 30, (1 << 30) + 1),
    "E": (0, 4, 8, 12, 16, 30, 32, 36, 48, 64, 72),
    "M": (0, 1, 2, 7, 31, 32),
    "h": (0, 1, 32, 33, 128, 129, "first=129", "mid=129", "last=129", "mid=0", None),
    "C": (0, 4, 8, 12, 16, 20, 32, 36, 64),
    "L": (1, 2, 3, 4, 8, 12, 13, 20, 21),
}
CROSS = dict(N=(32, 64, 128, 256, 480, 512, 544, 1024, 1056, 2048, 4097), C=(4, 8, 12, 16, 32, 36), L=FACTORS["L"], h=(32, 128))


def shape_cases():
    """[(N, E, M, h, C, L)], h as in FACTORS: a width for every MLP, "place=width" for one entry of another width, None for NULL."""
    out = []
    for base in BASES:
        for i, name in enumerate(("N", "E", "M", "h", "C", "L")):
            out += [base[:i] + (v,) + base[i + 1:] for v in FACTORS[name]]
    out += [(N, 32, 3, h, C, L) for h in CROSS["h"] for N in CROSS["N"] for C in CROSS["C"] for L in CROSS["L"]]
    return list(dict.fromkeys(out))


def h_table(M, h):
    if h is None:
        return None
    n = max(M, 0) + 1
    widths = [32] * n
    if isinstance(h, str):
        place, w = h.split("=")
        widths[{"first": 0, "mid": n // 2, "last": n - 1}[place]] = int(w)
    else:
        widths = [h] * n
    return (i32 * n)(*widths)


def shape_label(s):
    return "N={} E={} M={} h={} C={} L={}".format(*s)


# ---------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------
SHAPES = {"lds": (128, 32, 3, 8, 8), "step": (16384, 32, 3, 8, 15), "both": (512, 32, 3, 8, 8), "bf16": (128, 32, 3, 8, 8)}  # (N, E, M, C, L), h = 32
TAB = [0x100, 0x200, 0x300, 0x400]  # one fake pointer per MLP (M = 3)
DEFAULT = dict(null_in=False, kind=DATA, K=0, src=0x1000, weight=None, bias=None, pos=None, B=1, A=TAB, a=TAB, Bw=TAB, b=TAB, h=32,
               V0=0x2000, outs=[0x3000, 0x4000, 0x3000], ws=0x5000, wb=0, shape=None, lds=(1, 0))
RECIPES = {"data": {}, "affine": dict(kind=AFFINE, K=2, src=0x1004, weight=0x6004, bias=0x7004, pos=0x8000),
           "tokens": dict(kind=TOKENS, K=50, src=0x1008, weight=0x6000, pos=0x8000)}
ENTRIES = ("psf_mixer_fwd_f32", "psf_mixer_fwd_in_f32", "psf_mixer_fwd_bf16")
# the faults that are also asked two at a time: one or two per check of an entry
PAIRED = ("src=NULL", "src misaligned", "K=0", "weight=NULL", "weight misaligned", "table misaligned", "pos misaligned", "B=-1", "B=2^31",
          "N=100 (uncovered)", "a[2]=NULL", "b[3] odd", "h=NULL", "V0 misaligned", "out[0]=NULL", "out[2] misaligned", "out[2]=V0",
          "out[2]=out[1]", "ws misaligned", "ws short")


def _tab(place, value):
    return [value if k == place else p for k, p in enumerate(TAB)]


def _outs(place, value):
    return [value if m == place else p for m, p in enumerate(DEFAULT["outs"])]


def _faults(entry, recipe):
    """{name: overrides}: the single faults of an entry that are answered before the first HIP call, in the order of the argument list."""
    bf, f = entry == "psf_mixer_fwd_bf16", {}
    if entry == "psf_mixer_fwd_in_f32":
        f["in=NULL"] = dict(null_in=True)
    f["src=NULL"] = dict(src=None)
    f["src misaligned"] = dict(src={"data": 0x1008, "affine": 0x1002, "tokens": 0x1004}[recipe])
    if recipe == "data":
        f["src 4-byte"] = dict(src=0x1004)
    if recipe == "affine":
        f.update({"K=0": dict(K=0), "K=4": dict(K=4), "weight=NULL": dict(weight=None), "weight misaligned": dict(weight=0x6002),
                  "bias misaligned": dict(bias=0x7001)})
    if recipe == "tokens":
        f.update({"K=0": dict(K=0), "K=-1": dict(K=-1), "table=NULL": dict(weight=None), "table misaligned": dict(weight=0x6008)})
    if recipe != "data":
        f["pos misaligned"] = dict(pos=0x8008)
    f.update({"B=-1": dict(B=-1), "N=100 (uncovered)": dict(shape=(100, 32, 3, 8, 8)), "C=36 (uncovered)": dict(shape=(128, 32, 3, 36, 8)),
              "M=0": dict(shape=(128, 32, 0, 8, 8))})
    for name in ("A", "a", "Bw", "b"):
        f[name + "=NULL"] = {name: None}
    f["A[0]=NULL"], f["a[2]=NULL"], f["b[3]=NULL"] = dict(A=_tab(0, None)), dict(a=_tab(2, None)), dict(b=_tab(3, None))
    if bf:
        f["A[0] odd"], f["Bw[1] odd"], f["b[3] odd"] = dict(A=_tab(0, 0x101)), dict(Bw=_tab(1, 0x201)), dict(b=_tab(3, 0x401))
        f["B=2^31"] = dict(B=1 << 31)
    f["h=NULL"] = dict(h=None)
    f["h mid=129 (uncovered)"] = dict(h="mid=129")
    if not bf:
        f["V0=NULL"] = dict(V0=None)
    f["V0 misaligned"] = dict(V0=0x2008)
    f.update({"outs=NULL": dict(outs=None), "out[0]=NULL": dict(outs=_outs(0, None)), "out[2]=NULL": dict(outs=_outs(2, None)),
              "out[0] misaligned": dict(outs=_outs(0, 0x3008)), "out[2] misaligned": dict(outs=_outs(2, 0x3004)),
              "out[0]=V0": dict(outs=_outs(0, 0x2000)), "out[2]=V0": dict(outs=_outs(2, 0x2000)),
              "out[1]=out[0]": dict(outs=_outs(1, 0x3000)), "out[2]=out[1]": dict(outs=_outs(2, 0x4000)),
              "ws=NULL": dict(ws=None), "ws misaligned": dict(ws=0x5008), "ws short": dict(wb=-16), "ws none": dict(wb="zero")})
    return f


def call_cases():
    """[(label, entry, arguments)] with ``arguments`` = DEFAULT overridden; the label names entry, recipe, shape and the faults."""
    out = []

    def add(entry, recipe, shape, what, over, **more):
        args = dict(DEFAULT, **RECIPES[recipe])
        args.update(over, **more)
        if args["shape"] is None:
            args["shape"] = SHAPES[shape]
        out.append((f"{entry} {recipe} {shape}: {what}", entry, args))

    for entry in ENTRIES:
        bf = entry == "psf_mixer_fwd_bf16"
        for recipe in (RECIPES if entry == "psf_mixer_fwd_in_f32" else ("data",)):
            shapes = ("bf16",) if bf else ("lds", "both") if recipe != "data" else ("lds", "step", "both")
            # a recipe is turned away wherever the single-launch kernel does not run; there its other faults are asked with the knob on
            knob = (1,) if recipe != "data" else (1, 0)
            faults = _faults(entry, recipe)
            for shape in shapes:
                for what, over in faults.items():
                    add(entry, recipe, shape, what, over, lds=knob)
                add(entry, recipe, shape, "B=0", dict(B=0), lds=knob)
            for w1, w2 in itertools.combinations([w for w in faults if w in PAIRED], 2):  # (in the order of the checks' arguments)
                if not set(faults[w1]) & set(faults[w2]):
                    add(entry, recipe, shapes[0], w1 + " + " + w2, dict(faults[w1], **faults[w2]), lds=knob)
            if recipe != "data":
                add(entry, recipe, "step", "a recipe on a per-step shape", {})
                add(entry, recipe, "step", "a recipe on a per-step shape + ws short", dict(wb=-16))
                add(entry, recipe, "step", "a recipe on a per-step shape + B=-1", dict(B=-1))
                add(entry, recipe, "step", "a recipe on a per-step shape, B=0", dict(B=0))
                for shape in ("lds", "both"):
                    add(entry, recipe, shape, "a recipe with mixer_lds=0", {}, lds=(0,))
                    add(entry, recipe, shape, "a recipe with mixer_lds=0, B=0", dict(B=0), lds=(0,))
                    add(entry, recipe, shape, "a recipe with mixer_lds=0 + V0 misaligned", dict(V0=0x2008), lds=(0,))
                    add(entry, recipe, shape, "B=2^31", dict(B=1 << 31))
                    add(entry, recipe, shape, "B=2^31 + ws short", dict(B=1 << 31, wb=-16))
        if entry == "psf_mixer_fwd_in_f32":
            add(entry, "affine", "lds", "bias=NULL is allowed, B=0", dict(bias=None, B=0), lds=(1,))
            add(entry, "tokens", "lds", "a bias is ignored, B=0", dict(bias=0x7001, B=0), lds=(1,))
            for kind in (3, -1):
                add(entry, "data", "lds", f"unknown kind {kind}", dict(kind=kind))
                add(entry, "data", "lds", f"unknown kind {kind} + N=100", dict(kind=kind, shape=(100, 32, 3, 8, 8)))
        if bf:
            add(entry, "data", "bf16", "V0=NULL is allowed, B=0", dict(V0=None, B=0), lds=(1,))
    assert len({lab for lab, _e, _a in out}) == len(out), "two calls share a label"
    return out


def ask_call(lib, entry, c):
    """(return code, B) of one call."""
    N, E, M, C, L = c["shape"]
    bf = entry == "psf_mixer_fwd_bf16"
    h = h_table(M, c["h"])
    tabs = [None if c[k] is None else (vp * len(c[k]))(*c[k]) for k in ("A", "a", "Bw", "b")]
    outs = None if c["outs"] is None else (vp * len(c["outs"]))(*c["outs"])
    fit = (lib.psf_mixer_fwd_bf16_workspace if bf else lib.psf_mixer_fwd_workspace)(N, E, M, h, C, L)
    wb = 0 if c["wb"] == "zero" else max(fit, 0) + c["wb"]
    tail = (c["B"], N, E, M, *tabs, h, C, L, 1, c["V0"], outs, c["ws"], wb, None)
    if entry == "psf_mixer_fwd_in_f32":
        spec = MixerInput(c["kind"], c["K"], c["src"], c["weight"], c["bias"], c["pos"])
        return lib.psf_mixer_fwd_in_f32(None if c["null_in"] else ctypes.byref(spec), *tail)
    return getattr(lib, entry)(c["src"], *tail)


class MixerInput(ctypes.Structure):
    _fields_ = [("kind", i32), ("K", i32), ("src", vp), ("weight", vp), ("bias", vp), ("pos", vp)]


def answers(lib, set_knob):
    """{label: "lds=1 answer || lds=0 answer"} over both grids ("lds=1,0 answer" where the two agree, one of them where the call is
    asked under one value only); ``set_knob(value)`` sets mixer_lds. The knob is left at 1."""
    got = {}
    try:
        for knob in (1, 0):
            set_knob(knob)
            for s in shape_cases():
                N, E, M, h, C, L = s
                t = h_table(M, h)
                got.setdefault(shape_label(s), {})[knob] = "{},{},{},{}".format(
                    lib.psf_mixer_fwd_plan(N, E, M, t, C, L), lib.psf_mixer_fwd_workspace(N, E, M, t, C, L),
                    lib.psf_mixer_fwd_bf16_plan(N, E, M, t, C, L), lib.psf_mixer_fwd_bf16_workspace(N, E, M, t, C, L))
            for lab, entry, c in call_cases():
                if knob in c["lds"]:
                    rc = ask_call(lib, entry, c)
                    assert rc < 0 or (rc == 0 and c["B"] == 0), f"lds={knob} {lab}: rc {rc} — this call reached a HIP call"
                    got.setdefault(lab, {})[knob] = f"{rc}:{lib.psf_last_error().decode() if rc else ''}"
    finally:
        set_knob(1)
    order = [shape_label(s) for s in shape_cases()] + [lab for lab, _e, _c in call_cases()]
    return {lab: f"lds=1,0 {a[1]}" if a.get(1) == a.get(0) else " || ".join(f"lds={k} {v}" for k, v in a.items())
            for lab, a in ((lab, got[lab]) for lab in order)}


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from sparsefactorization_amd import _lib
    assert os.path.abspath(_lib.__file__).startswith(os.path.abspath(sys.argv[1]) + os.sep), _lib.__file__
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixer_host_parent.json")
    doc = {"parent": sys.argv[2], "answers": answers(_lib.load(), lambda v: _lib.set_tuning("mixer_lds", v))}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0)
        fh.write("\n")
    print(f"{path}: {len(doc['answers'])} answers ({len(shape_cases())} shapes, {len(call_cases())} calls), "
          f"{len(set(doc['answers'].values()))} distinct, {os.path.getsize(path)} bytes")
