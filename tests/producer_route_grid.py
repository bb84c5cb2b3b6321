"""The grid of test_producer_routes_host.py: which producer route sparsefactorization_amd.fused_mlp gives a call, over every limit
of its five predicates from both sides, and the tool that records a package's answers as tests/golden/producer_routes_parent.json.

    python tests/producer_route_grid.py /path/to/checkout <commit hash of that checkout> [out.json]

Per case: the booleans of eligible, trainable, wide_ok, bf16_eligible and stackable (PREDICATES, the order in which PSFNet tries
them) and the name of the first true one (NAMES), as "10101:narrow_forward". Only names that every tree since the bf16 producer
forward has are used, so the same file records from an older checkout. Nothing is launched: the tensors are CPU (or meta)
tensors and ``torch.Tensor.is_cuda`` says yes while the predicates are asked.

One factor is varied at a time around a base case (E = 32, h = 32, O = 8, K = 3, x [16, E], parameters of x's dtype), each under
f32 and bf16 and under four gradient modes; then the dtype mixes, the block forms, x's rank, the empty list, the 2^30 limit of
the wide kernels' lane offsets (meta tensors) and every switch."""
import contextlib
import json
import os
import sys

import torch
from torch import nn

PREDICATES = ("eligible", "trainable", "wide_ok", "bf16_eligible", "stackable")
NAMES = ("narrow_forward", "narrow_train", "wide", "bf16_forward", "stacked")
SWITCHES = ("enabled", "train_enabled", "wide_enabled", "bf16_enabled")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}
# off: under no_grad. train: trainable parameters. frozen_x: frozen parameters, x.requires_grad. frozen: nothing needs a gradient.
MODES = ("off", "train", "frozen_x", "frozen")
BASE = dict(E=32, h=32, O=8, K=3)
FACTORS = {
    "E": (2, 4, 6, 8, 12, 16, 32, 36, 64, 80, 128, 1024, 1040),
    "h": (1, 32, 128, 129),
    "O": (1, 16, 17, 32, 33, 128, 129),
    "K": (1, 2, 24, 25, 32, 33),
}


class Block(nn.Module):
    """MLPBlock's shape: ``network`` = Linear, GELU, Linear — or one of the forms the routes refuse."""

    def __init__(self, E, h, O, form="plain"):
        super().__init__()
        bias = form != "no_bias"
        layers = [nn.Linear(E, h, bias=bias), nn.GELU(approximate="tanh" if form == "tanh" else "none")]
        if form == "deep":
            layers += [nn.Linear(h, h), nn.GELU()]
        self.network = nn.Sequential(*layers, nn.Linear(h, O, bias=bias))


def _case(x="f32", mode="off", params=None, form="plain", shape=None, empty=False, off=None, odd=None, device="cpu", **sizes):
    """One case as a dict; ``params``: the parameters' dtype (x's when None); ``odd``: (block, layer, parameter name, dtype) of the
    one parameter of another dtype; ``off``: the switch that is off."""
    c = dict(BASE, x=x, mode=mode, params=params or x, form=form, shape=shape, empty=empty, off=off, odd=odd, device=device)
    c.update(sizes)
    return c


def cases():
    out = []
    for x in ("f32", "bf16"):
        for mode in MODES:
            for name, values in FACTORS.items():
                out += [_case(x, mode, **{name: v}) for v in values]
    for mode in MODES:
        out += [_case("f64", mode), _case("f64", mode, K=1), _case("bf16", mode, params="f32"), _case("f32", mode, params="bf16")]
        # one parameter of another dtype: the second layer's bias, and the first layer's weight (the one the f32 routes look at)
        for x, other in (("f32", "bf16"), ("bf16", "f32"), ("f32", "f64")):
            out += [_case(x, mode, odd=(1, 2, "bias", other)), _case(x, mode, odd=(1, 0, "weight", other)),
                    _case(x, mode, odd=(0, 0, "bias", other)), _case(x, mode, odd=(2, 2, "weight", other))]
        for x in ("f32", "bf16"):
            out += [_case(x, mode, form=f) for f in ("deep", "no_bias", "tanh", "wrong_in")]
            out += [_case(x, mode, form="deep", K=1)]
            out += [_case(x, mode, shape=(32,)), _case(x, mode, shape=(2, 8, 32)), _case(x, mode, empty=True)]
            out += [_case(x, mode, E=6, K=1), _case(x, mode, E=80, O=128, K=24), _case(x, mode, E=80, O=128, K=25)]
            out += [_case(x, mode, off=s) for s in SWITCHES]
            out += [_case(x, mode, off=s, E=80) for s in SWITCHES]
    # T * max(E, J) on both sides of 2^30 (J: the hidden widths, each rounded up to 32, summed), E the larger and J the larger
    for x in ("f32", "bf16"):
        for mode in ("off", "train"):
            out += [_case(x, mode, E=1024, h=128, K=1, shape=(T, 1024), device="meta") for T in ((1 << 20) - 1, 1 << 20)]
            out += [_case(x, mode, E=16, h=128, K=24, shape=(T, 16), device="meta") for T in (349525, 349526)]
            out += [_case(x, mode, E=16, h=97, K=24, shape=(2, T // 2, 16), device="meta") for T in (349524, 349526)]
    return list({label(c): c for c in out}.values())  # (the base case is in more than one factor's list)


def label(c):
    parts = [f"x={c['x']}", f"mode={c['mode']}"] + [f"{k}={c[k]}" for k in ("E", "h", "O", "K")]
    parts += [f"{k}={c[k]}" for k in ("params", "form", "shape", "empty", "off", "odd", "device")
              if c[k] != {"params": c["x"], "form": "plain", "empty": False, "device": "cpu"}.get(k)]
    return " ".join(parts)


def build(c):
    """(x, blocks) of a case."""
    E, dt = c["E"], DTYPES[c["params"]]
    blocks = [Block(E // 2 if c["form"] == "wrong_in" else E, c["h"], c["O"], c["form"]).to(dt) for _ in range(c["K"])]
    if c["odd"] is not None:
        k, layer, name, other = c["odd"]
        p = getattr(blocks[k].network[layer], name)
        p.data = p.data.to(DTYPES[other])
    x = torch.zeros(c["shape"] or (16, E), dtype=DTYPES[c["x"]], device=c["device"])
    if c["mode"] in ("frozen_x", "frozen"):
        for b in blocks:
            b.requires_grad_(False)
    if c["mode"] == "frozen_x":
        x.requires_grad_(True)
    return x, ([] if c["empty"] else blocks)


@contextlib.contextmanager
def asked_on_the_gpu(fm, c):
    """The state a case is asked in: its gradient mode, its switch off, and every tensor saying it is a HIP tensor."""
    real = torch.Tensor.is_cuda
    torch.Tensor.is_cuda = property(lambda self: True)
    if c["off"]:
        setattr(fm, c["off"], False)
    try:
        with torch.no_grad() if c["mode"] == "off" else torch.enable_grad():
            yield
    finally:
        if c["off"]:
            setattr(fm, c["off"], True)
        torch.Tensor.is_cuda = real


def answers(fm, also=None):
    """[(label, "bbbbb:first route", also(x, blocks))] over the grid, for the fused_mlp module ``fm``; ``also`` is asked in the
    same state as the predicates (None when not given)."""
    assert all(getattr(fm, s) is True for s in SWITCHES), "another test left a switch off"
    out = []
    for c in cases():
        x, blocks = build(c)
        with asked_on_the_gpu(fm, c):
            bits = [bool(getattr(fm, p)(x, blocks)) for p in PREDICATES]
            extra = also(x, blocks) if also is not None else None
        first = NAMES[bits.index(True)] if any(bits) else None
        out.append((label(c), "".join("01"[b] for b in bits) + f":{first}", extra))
    assert len({lab for lab, _a, _e in out}) == len(out), "two cases share a label"
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    from sparsefactorization_amd import fused_mlp
    assert os.path.abspath(fused_mlp.__file__).startswith(os.path.abspath(sys.argv[1]) + os.sep), fused_mlp.__file__
    path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "producer_routes_parent.json")
    doc = {"parent": sys.argv[2], "predicates": list(PREDICATES), "answers": {lab: a for lab, a, _e in answers(fused_mlp)}}
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0)
        fh.write("\n")
    print(f"{path}: {len(doc['answers'])} cases, {len(set(doc['answers'].values()))} distinct answers, {os.path.getsize(path)} bytes")
