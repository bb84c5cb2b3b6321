"""The stage contracts of a bf16 PSF model: what every stage between two tensors that reach memory has to return for the bf16
operands it received, in float64, with a per-element envelope. No GPU, and nothing of the library is imported: the stages are
the op sequence of ``psf_twin.forward`` (lookup + pos, init_linear, dropout1, the producer MLPs, dropout2, the chain, dropout3,
the CLS slice, the head).

A whole bf16 model against a float64 model is a weak test: ten dependent bf16 roundings cost 2-12 % (E16, ``e16_of``), and the
wiring defects of ``psf_twin.DEFECTS`` sit below 4 x that. One STAGE is sharp. Its operands are bf16 values, its products are
exact in f32, and what it returns is

    want = bf16_rne(exact)                                 one rounding of the float64 value
    envelope = ulp_bf16(want) + n 2^-24 sum|terms|          what any f32 summation order of the n terms can move, through a
                                                            flipped bf16 tie, by one ulp

(the form of ``mlp_bf16_bwd_ref.ref_bwd``). Stages made of several roundings (the producers: ``mlp_bf16_ref.ref`` and
``mlp_bf16_bwd_ref.ref_bwd`` as they are; the chain, whose g_m are rounded per step) push the envelopes of their intermediates
through the absolute values of what multiplies them. Inside the envelope is the hard bound; the sensitivity comes from the
SHARE of elements that differ from ``want`` at all: a correct evaluation differs only where an f32 sum falls within
n 2^-24 of a bf16 tie (measured below 1 % on every stage), a lost token, a lost residual term or a wrong row changes most of
the elements. ``cap(n)`` is that share's bound: ``mlp_bf16_ref.MAX_DIFFERING`` (0.01) for sums of at most 1024 terms, 0.05 for
the long reductions (over tokens, over N C).

Every contract takes float64 arrays holding bf16 values and returns ``(want, envelope)`` or a dict of such pairs. ``judge``
asserts finiteness, shape and the envelope and returns the differing share; ``report`` builds profiles/bf16_model_stages.md
from the "STAGE ..." lines the tests print.
"""
from __future__ import annotations

import re
from collections import OrderedDict

import numpy as np

import bf16_edges as be
import mlp_bf16_bwd_ref as RB
import mlp_bf16_ref as R
import psf_twin as T
from mlp_bf16_ref import bf16_rne, ulp_bf16

ACC = 2.0 ** -24          # one f32 rounding, relative
CAP_SHORT = R.MAX_DIFFERING  # sums of at most LONG terms
CAP_LONG = 0.05           # longer reductions: over the tokens, over N C
LONG = 1024
E16_MAX = 0.25            # condition on every case: the coarse bar 4 x E16 stays below 1


def cap(n_terms: int) -> float:
    """The largest share of elements that may differ from the contract, for a stage whose sums have ``n_terms`` terms."""
    return CAP_SHORT if n_terms <= LONG else CAP_LONG


def f64(a) -> np.ndarray:
    return np.asarray(a, np.float64)


def _single(exact, absum, n, carried=None):
    """(want, envelope) of a value rounded once from an f32 sum of n exact terms; ``carried``: what the envelopes of rounded
    intermediates contribute."""
    want = bf16_rne(exact)
    env = ulp_bf16(want) + n * ACC * absum
    return want, env if carried is None else env + carried


# ------------------------------------------------------------------------------------------------ single-rounding stages
def embed_fwd(table, idx, pos=None):
    """``table[idx] (+ pos)``: idx [B, N] integers, table [V, E], pos [N, E] or None."""
    rows = f64(table)[np.asarray(idx)]
    if pos is None:
        return rows, np.zeros_like(rows)  # a copy: the bits are determined
    p = f64(pos)[None]
    return _single(rows + p, np.abs(rows) + np.abs(p), 2)


def embed_bwd(dout, idx, vocab, padding_idx=None, with_pos=True, drop_token=None):
    """{"dTable": ..., "dpos": ...} for d(out) [B, N, E]: dTable[v] the sum over the positions holding v (the padding row and
    every absent id an exact zero: want = 0 and envelope = 0 there), dpos the sum over the batch. ``n`` (returned under "n") is
    the longest sum. ``drop_token``: a flat position left out of dTable (a seeded defect)."""
    dout, idx = f64(dout), np.asarray(idx)
    B, N, E = dout.shape
    flat, ids = dout.reshape(-1, E), idx.reshape(-1)
    hot = np.zeros((ids.size, vocab))
    hot[np.arange(ids.size), ids] = 1.0
    if padding_idx is not None:
        hot[:, padding_idx] = 0.0
    if drop_token is not None:
        hot[drop_token] = 0.0
    count = hot.sum(0)
    want, env = _single(hot.T @ flat, hot.T @ np.abs(flat), count[:, None])
    env = np.where(count[:, None] == 0, 0.0, env)  # nothing is summed there: an exact zero
    out = {"dTable": (want, env), "n": {"dTable": int(count.max()), "dpos": B}}
    if with_pos:
        out["dpos"] = _single(dout.sum(0), np.abs(dout).sum(0), B)
    return out


def linear_fwd(x, W, b=None):
    """``y = x W^T + b``, x [..., K], W [O, K]."""
    x, W = f64(x), f64(W)
    exact, absum = x @ W.T, np.abs(x) @ np.abs(W).T
    if b is not None:
        exact, absum = exact + f64(b), absum + np.abs(f64(b))
    return _single(exact, absum, W.shape[1] + (b is not None))


def linear_bwd(x, W, dy, bias=True, drop_token=None):
    """{"dx", "dW", "db"}: ``dx = dy W``, ``dW = dy^T x``, ``db = sum dy`` (over every leading dimension). ``drop_token``: a row
    left out of dW and db."""
    x, W, dy = f64(x), f64(W), f64(dy)
    x2, d2 = x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1])
    if drop_token is not None:
        d2 = d2.copy()
        d2[drop_token] = 0.0
    rows = x2.shape[0]
    out = {"dx": _single(dy @ W, np.abs(dy) @ np.abs(W), W.shape[0]),
           "dW": _single(d2.T @ x2, np.abs(d2).T @ np.abs(x2), rows),
           "n": {"dx": W.shape[0], "dW": rows, "db": rows}}
    if bias:
        out["db"] = _single(d2.sum(0), np.abs(d2).sum(0), rows)
    return out


def gelu_fwd(z):
    """``rne(GELU(z))``; the margin 2e-7 (|z| + 1) of mlp_bf16_ref covers the f32 evaluation of Phi."""
    z = f64(z)
    want = bf16_rne(R.gelu64(z))
    return want, ulp_bf16(want) + 2e-7 * (np.abs(z) + 1.0)


def gelu_bwd(z, g):
    """``rne(g GELU'(z))``; the margin of mlp_bf16_bwd_ref."""
    z, g = f64(z), f64(g)
    want = bf16_rne(g * RB.gelu_grad64(z))
    return want, ulp_bf16(want) + np.abs(g) * RB.GRAD_MARGIN * (np.abs(z) + 1.0)


def _roll(a, off):
    """Row p of the result is row (p + off) mod N of ``a`` ([B, N, ...])."""
    return np.roll(a, -off, axis=1)


def chain_step(W, X, V0, offsets, eX=None):
    """``X_m = sum_k W[..., k] roll(X, -off_k) (+ V0)``, one rounding. ``eX``: the envelope of ``X`` when it is itself a
    contract value and not an operand."""
    W, X = f64(W), f64(X)
    exact, absum = np.zeros_like(X), np.zeros_like(X)
    carried = None if eX is None else np.zeros_like(X)
    for k, off in enumerate(offsets):
        w = W[..., k:k + 1]
        exact += w * _roll(X, off)
        absum += np.abs(w) * np.abs(_roll(X, off))
        if eX is not None:
            carried += np.abs(w) * _roll(eX, off)
    if V0 is not None:
        exact, absum = exact + f64(V0), absum + np.abs(f64(V0))
    return _single(exact, absum, len(offsets) + (V0 is not None), carried)


def chain_forward(Ws, V0, residual, offsets):
    """[(X_1, e_1), ..., (X_M, e_M)] from V0 alone (the chain of a forward that keeps no step): the envelopes carried along."""
    out, X, eX = [], f64(V0), None
    for W in Ws:
        X, eX = chain_step(W, X, V0 if residual else None, offsets, eX)
        out.append((X, eX))
    return out


def chain_backward(Ws, Xs, dOut, residual, offsets, drop_residual_of=None):
    """{"dV0": (want, env), "dW": [(want, env)] * M, "g": [g_M, ..., g_0]} of the chain with operands W_m [B, N, L], the saved
    X_m (m = 0 .. M - 1, X_0 = V0) and the gradient of X_M: g_m rounded once per step and entering the next, dW_m rounded once,
    dV0 = g_M + ... + g_0 over the rounded g_m and rounded once (g_0 alone without the residual).
    ``drop_residual_of``: a step m whose g_m is left out of the residual sum (a seeded defect)."""
    M, C = len(Ws), np.shape(dOut)[-1]
    g, eg = f64(dOut), np.zeros(np.shape(dOut))
    gs, egs, dWs = [g], [eg], [None] * M
    for m in range(M - 1, -1, -1):
        W, X = f64(Ws[m]), f64(Xs[m])
        exact, absum, carried = (np.zeros(W.shape) for _ in range(3))
        for k, off in enumerate(offsets):
            xr = _roll(X, off)
            exact[..., k] = (g * xr).sum(-1)
            absum[..., k] = np.abs(g * xr).sum(-1)
            carried[..., k] = (eg * np.abs(xr)).sum(-1)
        dWs[m] = _single(exact, absum, C, carried)
        exact, absum, carried = (np.zeros_like(g) for _ in range(3))
        for k, off in enumerate(offsets):  # g_m[q] = sum_k W[q - off_k, k] g_{m+1}[q - off_k]
            w = W[..., k:k + 1]
            exact += _roll(w * g, -off)
            absum += _roll(np.abs(w * g), -off)
            carried += _roll(np.abs(w) * eg, -off)
        g, eg = _single(exact, absum, len(offsets), carried)
        gs.append(g)
        egs.append(eg)
    if residual:
        keep = [i for i in range(M + 1) if drop_residual_of is None or i != M - drop_residual_of]
        dV0 = _single(sum(gs[i] for i in keep), sum(np.abs(gs[i]) for i in keep), M + 1, sum(egs[i] for i in keep))
    else:
        dV0 = (g, eg)
    return {"dV0": dV0, "dW": dWs, "g": gs}


def chain_terms(M, L, C) -> dict:
    """The number of terms of the chain's sums, which is what ``cap`` is asked with: dW_m sums C products, dV0 M + 1 gradients,
    a step L products (+ V0). All are short sums: the cap is 1 %, also where the tensor is judged through rounded intermediates
    that never reach memory (dW_m and dV0 from the gradient of X_M alone; X_M from V0 alone)."""
    return {"dW": [C] * M, "dV0": M + 1, "X_M": L + 1}


# --------------------------------------------------------------------------------------------------------- the producers
def producers_fwd(X, params):
    """[(y_k, envelope)]: ``mlp_bf16_ref.ref`` per MLP (z, h, y: three roundings). params = [(A, a, B, b)]."""
    out = []
    for A, a, B, b in params:
        _z, _h, y, dy = R.ref(X, A, a, B, b)
        out.append((y, dy))
    return out


def producers_bwd(X, params, dYs):
    """``mlp_bf16_bwd_ref.ref_bwd``: ({"dX", "grads": [(dA, da, dB, db)]}, the envelope in the same layout)."""
    return RB.ref_bwd(X, params, dYs)


# ---------------------------------------------------------------------------------------------------------- exact stages
def dropout_fwd(x, mask, p):
    """``rne(x scale) mask`` with scale = 1 / (1 - p) as the f32 number the elementwise kernel multiplies by: the bits."""
    scale = np.float32(1.0 / (1.0 - p))
    return be.as_bf16(np.asarray(x, np.float32) * scale).astype(np.float64) * f64(mask)


dropout_bwd = dropout_fwd  # d(x) = rne(d(out) scale) mask


def cls_bwd(dflat, N):
    """The gradient of ``V[:, 0, :]``: d(flat) in row 0, exact zeros elsewhere."""
    dflat = f64(dflat)
    out = np.zeros((dflat.shape[0], N, dflat.shape[1]))
    out[:, 0] = dflat
    return out


def chain_backward_bits(shape, residual, Ws, Xs, dOut):
    """(dV0 bits, [dW_m bits]) of the one-launch backward chain, whose documented order
    ``chain_bwd_bf16_cases.backward_from`` reproduces bit for bit. shape = (B, N, M, L, C)."""
    import chain_bwd_bf16_cases as CB
    B, N, M, L, C = shape
    as32 = lambda a: np.ascontiguousarray(a, np.float32)
    return CB.backward_from((B, N, M, L, C, bool(residual), None), [as32(w) for w in Ws], [as32(x) for x in Xs], as32(dOut))


# ----------------------------------------------------------------------------------------------------------------- judge
def measure(got, want, envelope):
    """(differing share, worst |err| / envelope, element count). An element with envelope 0 must be equal."""
    got, want, envelope = f64(got), f64(want), np.broadcast_to(f64(envelope), np.shape(want))
    err = np.abs(got - want)
    if not err.size:
        return 0.0, 0.0, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / envelope)
    return float(np.mean(err != 0)), float(np.max(ratio)), int(err.size)


def line(tag, stage, tensor, share, worst, n, note=""):
    return f"STAGE {tag} {stage}.{tensor.replace(' ', '_')}: share {share:.3e} worst/envelope {worst:.4f} n {n}" + (f" [{note}]" if note else "")


def judge(stage, tensor, got, want, envelope, tag="-", note="", shares=None, n_terms=1, asserted=True, pool=True) -> float:
    """Asserts that ``got`` is finite, has the shape of ``want`` and lies inside the envelope everywhere; returns the share of
    elements that differ from ``want`` at all. With ``shares`` (a ``Shares``) the result is pooled there under ``n_terms`` and
    printed by ``Shares.lines``; without, the stage's line is printed here."""
    got = f64(got)
    assert got.shape == np.shape(want), f"{stage}.{tensor}: shape {got.shape} against {np.shape(want)}"
    assert np.all(np.isfinite(got)), f"{stage}.{tensor}: not finite"
    share, worst, n = measure(got, want, envelope)
    if shares is None:
        print(line(tag, stage, tensor, share, worst, n, note))
    else:
        shares.add(stage, tensor, share, n, n_terms, asserted, note, pool, worst)
    assert worst <= 1.0, f"{stage}.{tensor}: outside the envelope ({worst:.3f} of it)"
    return share


def allowed(size: int, n_terms: int, half: bool = False) -> int:
    """How many of ``size`` elements may differ: the cap (``half``: half of it, the condition on the plain evaluation) times the
    size, and never less than ONE element — a share moves in steps of 1 / size, so a tensor of fewer than 1 / cap elements (a bias
    gradient, the logits) cannot express the cap, and one flipped tie in it is what the envelope exists to allow."""
    return max(1, int(cap(n_terms) / (2 if half else 1) * size))


def rejected(stage, tensor, got, want, envelope, n_terms) -> bool:
    """Whether ``judge`` plus the cap turns ``got`` down: outside the envelope, or more elements differ than ``allowed``."""
    share, worst, size = measure(got, want, envelope)
    return worst > 1.0 or round(share * size) > allowed(size, n_terms)


class Shares:
    """The differing shares of a run, pooled over the instances of a stage tensor (``dA[0]`` ... ``dA[9]`` of the ten producer
    MLPs, the layers of the unfused blocks): differing elements over elements, against one cap."""

    def __init__(self):
        self.rows = OrderedDict()  # (stage, pooled tensor name, cap) -> [differing, size, n_terms, asserted, note, worst / envelope]

    def add(self, stage, tensor, share, size, n_terms, asserted=True, note="", pool=True, worst=0.0):
        """``pool`` False: the tensor stands alone (the chain's steps: dW_m of every m has a cap of its own, ``chain_terms``)."""
        # instances pool only within one class of the cap: the head's first layer (K = N C, long) and its second (short) do not
        row = self.rows.setdefault((stage, re.sub(r"\d+", "*", tensor) if pool else tensor, cap(n_terms)), [0, 0, 0, True, "", 0.0])
        row[0] += int(round(share * size))
        row[1] += size
        row[2] = max(row[2], n_terms)
        row[3] = row[3] and asserted
        row[4] = row[4] or note
        row[5] = max(row[5], worst)

    def over(self, half=False) -> list:
        """[(stage.tensor, differing, allowed)] of the asserted rows that are over the cap."""
        return [(f"{s}.{t}", d, allowed(size, n, half)) for (s, t, _c), (d, size, n, asserted, _note, _w) in self.rows.items()
                if asserted and d > allowed(size, n, half)]

    def lines(self, tag) -> list:
        """The run's record: one ``STAGE`` line per stage tensor in which an element differs (instances pooled, the two classes
        of the cap printed as one: the larger share; the chain's dW_m each on its own line), and one ``STAGE-SAME`` line naming
        the tensors equal to the contract in every element."""
        shown = OrderedDict()
        for (stage, tensor, _cap), (d, size, _n, _a, note, worst) in self.rows.items():
            name = tensor if re.fullmatch(r"dW\[\d+\]", tensor) else re.sub(r"[0-9]+", "*", tensor)
            row = shown.setdefault(f"{stage}.{name}", [0.0, 0.0, 0, ""])
            row[0], row[1], row[2], row[3] = max(row[0], d / size), max(row[1], worst), row[2] + size, row[3] or note
        out = [f"STAGE {tag} {name.replace(' ', '_')}: share {s:.3e} worst/envelope {w:.4f} n {n}" + (f" [{note}]" if note.startswith("recorded") else "")
               for name, (s, w, n, note) in shown.items() if s or w]
        same = [name.replace(" ", "_") for name, (s, w, _n, _note) in shown.items() if not (s or w)]
        return out + [f"STAGE-SAME {tag}: " + " ".join(same)]


# -------------------------------------------------------------------------------------------- the coarse whole-model net
def rounded_state(case):
    """``psf_twin.init_state`` rounded to bf16 (as float32 tensors): the parameters a ``.to(torch.bfloat16)`` model holds."""
    import torch
    return OrderedDict((k, v.to(torch.bfloat16).float()) for k, v in T.init_state(case).items())


def run_rounded(case, dtype, defect=None):
    """``psf_twin.run_twin`` on the bf16-rounded state and inputs, the loss taken in float32 (bf16 run) from the logits as
    psf_training does: {"loss", "grads"}."""
    import torch
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in rounded_state(case).items()}
    x, y, masks = T.make_batch(case)
    if x.is_floating_point():
        x = x.to(torch.bfloat16).to(dtype)
    if y.is_floating_point() and case.loss == "dot":
        y = y.to(torch.bfloat16).float()
    out = T.forward(case.kind, case.cfg, sd, x, masks, True, defect)
    value = T.loss_of(case.loss, out.float() if dtype == torch.bfloat16 else out, y)
    value.backward()
    return {"loss": float(value.detach()),
            "grads": {k: (None if v.grad is None else v.grad.double().numpy()) for k, v in sd.items()}}


def e16_of(case):
    """(E16, the parameter that sets it, the float64 run): the largest per-parameter rel_inf error of the twin in bf16 on the
    CPU against the twin in float64, both on the bf16-rounded state and inputs."""
    import torch
    r64, r16 = run_rounded(case, torch.float64), run_rounded(case, torch.bfloat16)
    errs = T.per_param_error(r16["grads"], r64["grads"])
    name = max(errs, key=errs.get)
    return errs[name], name, r64


# ---------------------------------------------------------------------------------------------------------------- report
_STAGE = re.compile(r"STAGE (\S+) (\S+) (\S+): share (\S+) worst/envelope (\S+) n (\d+)(?: \[(.*)\])?")
_SAME = re.compile(r"STAGE-SAME (\S+) (\S+): (.*)")
_ROUTE = re.compile(r"STAGE-ROUTES (\S+) (\S+): mlp (\[.*?\]) calls \{(.*)\}")
_E16 = re.compile(r"STAGE-E16 (\S+) (\S+): E16 (\S+) at (\S+) bar (\S+) worst (\S+) at (\S+)")
_DEFECT = re.compile(r"STAGE-DEFECT (\S+) (\S+) (\S+): instances (\d+) smallest share (\S+) largest worst/envelope (\S+)")
_EVAL = re.compile(r"STAGE-EVAL (\S+): (.*)")
_LINKS = re.compile(r"STAGE-LINKS \S+ \S+: (\d+) the same tensor, (\d+) copies")
_COLUMNS = ("cpu", "never", "driver", "all", "eval")


def _table(head, rows):
    return "\n".join(["| " + " | ".join(head) + " |", "|" + "---|" * len(head)] + ["| " + " | ".join(r) + " |" for r in rows])


def report(lines) -> str:
    """The Markdown tables of profiles/bf16_model_stages.md from the lines the CPU test and the GPU run print (a list of lines
    or one text). A line is ``STAGE <case> <set> <stage>.<tensor>: share ... worst/envelope ... n ...`` (``Shares.lines``);
    <set> is "cpu" for the plain evaluation, "eval" for the eval-mode forward."""
    text = lines if isinstance(lines, str) else "\n".join(lines)
    blocks = OrderedDict()
    blocks["routes"] = _table(("case", "route set", "`fused_mlp.route` answers", "entry points (`psf_..._bf16`): calls"),
                              [(c, s, f"`{mlp}`", calls.replace("'", "").replace("psf_", "").replace("_bf16", "")) for c, s, mlp, calls in _ROUTE.findall(text)])
    e16 = OrderedDict()
    for c, s, e, at, bar, worst, where in _E16.findall(text):
        row = e16.setdefault(c, [e, f"`{at}`", bar, {}])
        row[3][s] = f"{float(worst):.3f} (`{where}`)"
    blocks["e16"] = _table(("case", "E16", "set by", "bar = 4 x E16", *(f"worst error, {s}" for s in _COLUMNS[1:4])),
                           [(c, f"{float(e):.3f}", at, f"{float(bar):.3f}", *(by.get(s, "-") for s in _COLUMNS[1:4])) for c, (e, at, bar, by) in e16.items()])
    found = [(c, w, name, float(s), float(r), note) for c, w, name, s, r, _n, note in _STAGE.findall(text)]
    found += [(c, w, name, 0.0, 0.0, "") for c, w, names in _SAME.findall(text) for name in names.split()]
    cells, per_case, notes = OrderedDict(), OrderedDict(), OrderedDict()
    for case, which, name, share, ratio, note in found:
        old = cells.setdefault(name, {}).get(which, (-1.0, 0.0, ""))
        cells[name][which] = (max(old[0], share), max(old[1], ratio), case if share > old[0] else old[2])
        if note.startswith("recorded"):
            notes.setdefault((name, which, note), []).append(case)
        elif share > per_case.setdefault(case, {}).get(which, (-1.0, ""))[0]:
            per_case[case][which] = (share, name)
    fmt = lambda c: "-" if c is None else f"{c[0]:.1e} ({c[2]}); {c[1]:.2f}"
    equal = [name for name, by in cells.items() if not any(c[0] or c[1] for c in by.values())]
    blocks["stages"] = _table(("stage tensor", *(f"{w}: largest share (case); worst / envelope" for w in _COLUMNS)),
                              [(f"`{name}`", *(fmt(by.get(w)) for w in _COLUMNS)) for name, by in cells.items() if name not in equal])
    blocks["stages"] += "\n\nEqual to the contract in every element, in every case and set: " + ", ".join(f"`{n}`" for n in equal) + "."
    blocks["cases"] = _table(("case", *(f"{w}: largest asserted share (tensor)" for w in _COLUMNS)),
                             [(case, *("-" if w not in by else f"{by[w][0]:.1e} (`{by[w][1]}`)" for w in _COLUMNS)) for case, by in per_case.items()])
    blocks["unasserted"] = _table(("stage tensor", "set", "cases", "why the share is recorded and not asserted"),
                                  [(f"`{name}`", which, ", ".join(sorted(set(cases))), note) for (name, which, note), cases in notes.items()])
    links = _LINKS.findall(text)
    blocks["links"] = _table(("what a stage received", "count"), [("the tensor the stage before returned", str(sum(int(a) for a, _b in links))),
                                                                   ("a copy of it", str(sum(int(b) for _a, b in links)))])
    bad = OrderedDict()  # (defect, stage tensor) -> [cases, instances, smallest share, largest worst / envelope]
    for defect, case, name, k, share, ratio in _DEFECT.findall(text):
        row = bad.setdefault((defect, name), [[], 0, 1.0, 0.0])
        row[0].append(case)
        row[1] += int(k)
        row[2], row[3] = min(row[2], float(share)), max(row[3], float(ratio))
    blocks["defects"] = _table(("seeded defect", "stage tensor that turns it down", "at the shapes of", "instances", "smallest share", "largest worst / envelope"),
                               [(d, f"`{t}`", ", ".join(sorted(set(c))), str(k), f"{s:.1e}", f"{r:.2f}") for (d, t), (c, k, s, r) in bad.items()])
    blocks["eval"] = _table(("case", "eval mode"), _EVAL.findall(text))
    return "\n\n".join(f"<!-- begin {k} -->\n{v}\n<!-- end {k} -->" for k, v in blocks.items()) + "\n"


if __name__ == "__main__":  # python tests/bf16_stage_twin.py LOG [LOG ...] > tables
    import sys
    print(report("\n".join(open(p).read() for p in sys.argv[1:])))
