"""A float64 twin of every model class, in plain functional PyTorch, and the comparison of the library's models with it.

Nothing here imports the library or needs a GPU. ``forward(case, sd, x, ...)`` is the op sequence of ``SyntheticPSFNet``,
``LRAPSFNet``, ``GenomePSFNet``, ``AttentionBlockPSF`` and ``ChangedPSF`` driven by the constructor-argument dict of the class
and a state_dict, in whatever dtype the state_dict has:

* token MLPs are ``F.linear`` / ``F.gelu`` (erf), lookups ``F.embedding`` (with ``padding_idx = vocab - 2`` for imdb and listops);
* the chain is ``V <- sum_k W_m[..., k] * roll(V, -off_k, 1) (+ V0)`` with the offsets 0, 1, 2, 4, ... mod N written out here;
* dropout is a pre-drawn keep mask scaled by 1 / (1 - p) (``FixedDropout``, which is also installed on the library's network);
* the dense map of ``ChangedPSF`` is the product of the M circulant-sparse factors built densely.

``CASES`` are the networks the GPU suite runs, ``DEFECTS`` the wiring mistakes seeded INTO THE TWIN (never into the library) that
the comparator has to catch, ``compare`` the comparator and ``report`` the Markdown of profiles/model_twin_grads.md.

The bar of a case is 4 x E32, E32 being the largest per-parameter error (max|d| / max|ref|, ``conftest.rel_inf``) of the twin
run in float32 against the twin run in float64 on the CPU: what plain f32 arithmetic costs on that very network and batch. The
library sums in other orders and forms W through split-bf16 GEMMs at f32 accuracy, which moves the error by a small factor; a
wiring defect moves it by orders of magnitude.
"""
from __future__ import annotations

import functools
import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from conftest import rel_inf

FACTOR = 4.0          # library error <= FACTOR * E32
E32_MAX = 2e-5        # condition on every case: the bar never exceeds 8e-5
DEFECT_MARGIN = 100.0  # every seeded defect sits at least this far over its case's bar


# ------------------------------------------------------------------------------------------------------------ the pieces
def chord_offsets(N: int, L: int) -> list:
    """0, 1, 2, 4, ..., 2^(L-2), each mod N."""
    return [0] + [(1 << k) % N for k in range(L - 1)]


def mlp(spec, sd, prefix: str, x):
    """``MakeMLP(spec, ...)``: an int is a Linear to that width, a string a GELU, then a closing Linear; the parameter index is
    the position in the Sequential."""
    i = 0
    for item in spec:
        if isinstance(item, int):
            x = F.linear(x, sd[f"{prefix}.network.{i}.weight"], sd[f"{prefix}.network.{i}.bias"])
        else:
            x = F.gelu(x)
        i += 1
    return F.linear(x, sd[f"{prefix}.network.{i}.weight"], sd[f"{prefix}.network.{i}.bias"])


def chord_step(W, V, offsets):
    acc = W[..., 0:1] * torch.roll(V, -offsets[0], 1)
    for k in range(1, len(offsets)):
        acc = acc + W[..., k:k + 1] * torch.roll(V, -offsets[k], 1)
    return acc


def dense_factor(W, offsets):
    """[B, N, N]: row p holds W[b, p, k] in column (p + off_k) mod N (links that fall on one column add up)."""
    B, N, L = W.shape
    cols = (torch.arange(N).unsqueeze(1) + torch.tensor(offsets).unsqueeze(0)) % N
    A = torch.zeros(B, N, N, dtype=W.dtype)
    return A.scatter_add(2, cols.unsqueeze(0).expand(B, N, L), W)


class FixedDropout(nn.Dropout):
    """``nn.Dropout`` with a keep mask drawn beforehand: ``x * mask / (1 - p)`` in training, ``x`` otherwise. Keeps ``.p``."""

    def __init__(self, p: float, mask: torch.Tensor = None):
        super().__init__(p)
        self.register_buffer("mask", mask, persistent=False)

    def forward(self, x):
        if not self.training or self.p == 0:
            return x
        return x * self.mask.to(x.dtype) * (1.0 / (1.0 - self.p))


def _drop(x, masks, name, p, training):
    if not training or p == 0:
        return x
    return x * masks[name].to(x.dtype) * (1.0 / (1.0 - p))


# -------------------------------------------------------------------------------------------------------------- the twin
def forward(kind: str, cfg: dict, sd: dict, x, masks=None, training=True, defect=None, want_map=False, taps=None):
    """Logits (``attention``: the mixed sequence) of the ``kind`` network built as ``cls(**cfg)`` with parameters ``sd``.
    ``defect``: one of ``DEFECTS`` (the twin is then deliberately wrong). ``want_map``: also the dense map (ChangedPSF).
    ``taps``: a dict that receives the chain's operands and result ("W": [W_m], "V0", "Vfin"), their gradients retained."""
    if kind == "attention":
        N = cfg["max_seq_len"]
        M = math.ceil(math.log2(N))
        w_spec = v_spec = [cfg["embedding_size"], "GELU"]
        residual = cfg["use_residuals"]
    else:
        N, M, w_spec, v_spec, residual = cfg["n_vec"], cfg["n_W"], cfg["Ws"], cfg["V"], cfg["use_residuals"]
    offsets = chord_offsets(N, M + 1)
    if defect == "last_offset_plus_one":
        offsets[-1] = (offsets[-1] + 1) % N
    p1, p2, p3 = (cfg.get(f"dropout{i}_p", 0) for i in (1, 2, 3))

    def pos_rows(w):
        if defect == "dpos_first_sample_only":  # only sample 0's rows reach pos: the gradient is not summed over the batch
            return torch.cat([w.unsqueeze(0), w.detach().unsqueeze(0).expand(x.shape[0] - 1, -1, -1)], 0)
        return w.unsqueeze(0)

    if kind == "synthetic":
        data = x
        if cfg["problem"] == "order":
            data = F.embedding(x, sd["embedding.weight"]).squeeze(-2)
        if cfg["add_init_linear_layer"]:
            data = F.linear(data, sd["init_linear.weight"], sd["init_linear.bias"])
        if cfg["use_pos_embedding"]:
            data = data + pos_rows(sd["pos_embedding.weight"])
    else:
        pad = None
        if kind == "lra" and cfg["problem"] in ("imdb", "listops") and defect != "padding_row_not_zeroed":
            pad = cfg["vocab_size"] - 2
        data = F.embedding(x, sd["embedding.weight"], padding_idx=pad)
        if kind == "attention":
            data = data + pos_rows(sd["apc_embedding.weight"])
        elif cfg["use_pos_embedding"]:
            data = data + pos_rows(sd["pos_embedding.weight"])
        data = _drop(data, masks, "dropout1", p1, training)

    V0 = mlp(v_spec, sd, "g", data)
    order = list(range(M))
    if defect == "fs_swapped":
        order[0], order[1] = order[1], order[0]
    links_in = data.detach() if defect == "links_dx_dropped" else data  # the dX of one group of the MLP backward is lost
    Ws = [mlp(w_spec, sd, f"fs.{m}", links_in) for m in order]
    if defect != "dropout2_after_loop":
        V0 = _drop(V0, masks, "dropout2", p2, training)
    if defect == "dv0_last_token":
        V0 = torch.cat([V0[:, :-1], V0[:, -1:].detach()], 1)
    hit = M // 2  # the step the one-step defects damage
    if taps is not None:
        taps["W"], taps["V0"] = Ws, V0
        for t in (V0, *Ws):
            if t.requires_grad:
                t.retain_grad()
    V = V0
    for m, W in enumerate(Ws):
        if defect == "dw_last_token" and m == hit:
            W = torch.cat([W[:, :-1], W[:, -1:].detach()], 1)
        V = chord_step(W, V, offsets)
        if residual:
            V = V + (V0.detach() if defect == "residual_one_step" and m == hit else V0)
    if defect == "dropout2_after_loop":
        V = _drop(V, masks, "dropout2", p2, training)
    if taps is not None:
        taps["Vfin"] = V
    V = _drop(V, masks, "dropout3", p3, training)
    if kind == "attention":
        return V
    if cfg["pooling_type"] == "CLS":
        V = V[:, N - 1 if defect == "cls_reads_last_row" else 0, :]
    flat = V.reshape(V.shape[0], -1)
    if cfg["head"][0] == "linear":
        out = F.linear(flat, sd["final.weight"], sd["final.bias"])
    else:
        out = F.linear(F.gelu(F.linear(flat, sd["final.0.weight"], sd["final.0.bias"])), sd["final.2.weight"], sd["final.2.bias"])
    if not want_map:
        return out
    att = None
    for W in Ws:
        A = dense_factor(W, offsets)
        att = A if att is None else A @ att
    return out, att


def loss_of(case_loss: str, out, y):
    if case_loss == "mse":
        return F.mse_loss(out.squeeze(), y.to(out.dtype))
    if case_loss == "ce":
        return F.cross_entropy(out, y)
    if case_loss == "dot":   # attention block: sum(out * fixed random weights)
        return (out * y.to(out.dtype)).sum()
    if case_loss == "sum":
        return out.sum()
    raise ValueError(case_loss)


# --------------------------------------------------------------------------------------------------------------- the cases
Case = namedtuple("Case", "name kind cfg B loss seed routes note")


def _lra(problem, vocab, E, N, M, h, C, n_class, pooling, head, residual, pos, d=(0, 0, 0), hV=None):
    return dict(vocab_size=vocab, embedding_size=E, n_vec=N, n_W=M, Ws=[h, "GELU"], V=[hV or h, "GELU"], n_channels_V=C,
                n_class=n_class, pooling_type=pooling, head=head, use_cuda=True, use_residuals=residual, dropout1_p=d[0],
                dropout2_p=d[1], dropout3_p=d[2], init_embedding_weights=True, use_pos_embedding=pos, problem=problem)


def _synthetic(problem, N, M, E=32, h=32, C=8, Ws=None):
    adding = problem == "adding"
    return dict(vocab_size=1 if adding else 6, add_init_linear_layer=adding, embedding_size=E, n_vec=N, n_W=M,
                Ws=Ws or [h, "GELU"], V=Ws or [h, "GELU"], n_channels_V=C, n_class=1 if adding else 4, pooling_type="FLATTEN",
                head=["linear"], use_cuda=True, use_residuals=True, use_pos_embedding=not adding, problem=problem)


_GENOME = {k: v for k, v in _lra(None, 6, 32, 512, 9, 32, 32, 2, "FLATTEN", ["linear"], True, True).items() if k != "problem"}

#: ``routes``: what the GPU test asserts about the host's choices (tests/test_gpu_model_twin.py reads the keys):
#:   mlp       the names ``fused_mlp.route`` returns during the training forward, in order
#:   chain_bwd "one_launch" (psf_chord_chain_bwd_supported), "library_steps" (the library issues the steps and the one-pass
#:             residual sum) — both one call of psf_chord_chain_bwd_f32 —, "per_step_nodes" (one autograd node per factor)
#:   calls     entry point -> number of calls in one training forward + backward
CASES = [
    Case("adding", "synthetic", _synthetic("adding", 512, 9), 8, "mse", 1,
         dict(mlp=["narrow_train"], chain_bwd="one_launch",
              calls={"psf_affine_rows_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1, "psf_chord_chain_fwd_f32": 1,
                     "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 1, "psf_flat_head_bwd_f32": 1,
                     "psf_linear_wgrad_strided_f32": 1, "psf_chord_spmm_bwd_f32": 0}),
         "affine rows K = 2, narrow_train, one-launch chains, head J = 1"),
    Case("order_cls_len", "synthetic", _synthetic("order", 1025, 10), 4, "ce", 2,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1,
                     "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 1,
                     "psf_flat_head_bwd_f32": 1, "psf_chord_spmm_bwd_f32": 0}),
         "embed + pos pass, dTable with an absent id (5), library-issued backward steps + one-pass residual sum, odd N"),
    Case("pathfinder_like", "lra", _lra("pathfinder", 225, 32, 256, 8, 128, 32, 2, "FLATTEN", ["linear"], False, True), 16, "ce", 3,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 2,
                     "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 1,
                     "psf_flat_head_bwd_f32": 1}),
         "narrow_train backward split into a narrow launch (L = 9) and a wide one (C = 32), their dX added; no residual"),
    Case("listops_like", "lra", _lra("listops", 20, 64, 257, 9, 128, 64, 10, "CLS", ["non-linear", 32], True, True, (0.1, 0.1, 0.1)),
         16, "ce", 4,
         dict(mlp=["wide"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_wide_fwd_f32": 1, "psf_mlp_wide_bwd_f32": 1,
                     "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 0, "psf_mlp_fwd_f32": 0}),
         "wide route, padding row, three dropout masks, dropout2 between g and the loop, CLS gradient, C = 64"),
    Case("cifar_like", "lra", _lra("cifar10", 256, 16, 256, 8, 16, 16, 10, "FLATTEN", ["non-linear", 16], True, True), 16, "ce", 5,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1, "psf_flat_head_f32": 0, "psf_flat_head_bwd_f32": 1,
                     "psf_chord_chain_bwd_f32": 1}),
         "head with J = 16: GEMM forward, streaming backward"),
    Case("imdb_like", "lra", _lra("imdb", 97, 8, 1025, 10, 8, 8, 2, "CLS", ["linear"], True, False, (0.1, 0, 0)), 4, "ce", 6,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1,
                     "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 0}),
         "E = 8 narrow limits, odd N, padding, dropout1 only, no pos"),
    Case("genome", "genome", _GENOME, 8, "ce", 7,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 2, "psf_flat_head_f32": 1,
                     "psf_flat_head_bwd_f32": 1, "psf_chord_chain_bwd_f32": 1}),
         "C = 32 rows, FLATTEN"),
    Case("attention_block", "attention", dict(vocab_size=50, embedding_size=32, max_seq_len=300, use_cuda=True, use_residuals=True,
                                              dropout1_p=0, dropout2_p=0, dropout3_p=0), 14, "dot", 8,
         dict(mlp=["narrow_train"], chain_bwd="library_steps",
              calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 2,
                     "psf_chord_chain_bwd_f32": 1}),
         "apc embedding gradient, E = C = 32"),
    Case("stacked", "lra", _lra("listops", 20, 36, 257, 9, 40, 12, 10, "CLS", ["linear"], True, True), 16, "ce", 9,
         dict(mlp=["stacked"], chain_bwd="library_steps",
              calls={"psf_mlp_fwd_f32": 0, "psf_mlp_wide_fwd_f32": 0, "psf_linear_wgrad_strided_f32": 10,
                     "psf_chord_chain_bwd_f32": 1}),
         "stacked route (E = 36), second-layer wgrad on column slices with a row stride"),
    Case("deep_mlp", "synthetic", _synthetic("adding", 512, 9, Ws=[32, "GELU", 32, "GELU"]), 8, "mse", 10,
         dict(mlp=[None, None], chain_bwd="one_launch",
              calls={"psf_mlp_fwd_f32": 0, "psf_mlp_bwd_f32": 0, "psf_linear_wgrad_strided_f32": 31, "psf_chord_chain_bwd_f32": 1}),
         "no fused route: the modules' own TokenLinear layers (3 per MLP, 10 MLPs, init_linear)"),
    Case("per_step", "synthetic", _synthetic("adding", 512, 9), 8, "mse", 1,
         dict(mlp=[], chain_bwd="per_step_nodes",
              calls={"psf_chord_chain_fwd_f32": 0, "psf_chord_chain_bwd_f32": 0, "psf_chord_spmm_fwd_f32": 9,
                     "psf_chord_spmm_bwd_f32": 9}),
         "net.fused_chain = False: one autograd node per factor"),
]
CASE = {c.name: c for c in CASES}
#: ChangedPSF (forward only: logits and the dense map): N = 257 takes the identity padded to 260 columns, N = 256 the square one
CHANGED = [Case(f"changed_n{N}", "lra", _lra("pathfinder", 225, 32, N, 9, 32, 8, 2, "FLATTEN", ["linear"], False, True), 2, "ce", 20 + i,
                {}, "dense map W_M ... W_1 and logits") for i, N in enumerate((257, 256))]
VARIANT_CASES = ("adding", "order_cls_len", "listops_like")
FROZEN = ("input_layer", "g", "one_fs", "all_but_final")


def frozen_names(case: Case, which: str, names) -> set:
    """The parameter names ``requires_grad_(False)`` is applied to."""
    if which == "input_layer":   # the MLPs' need_dx is false
        return {n for n in names if n.startswith(("embedding.", "pos_embedding.", "apc_embedding.", "init_linear."))}
    # "g" and "one_fs" alone drop only that block's own parameter gradients: while the input layer trains, ``data`` needs a
    # gradient, so V0 = g(data) and every W_m = fs[m](data) still do and the chain's node is asked for all of them
    if which == "g":
        return {n for n in names if n.startswith("g.")}
    if which == "one_fs":
        return {n for n in names if n.startswith("fs.3.")}
    # ... with the input layer frozen as well (and the producers on their own layers: a fused producer's single node makes
    # every output need a gradient) the chain's node really sees them:
    if which == "one_fs_loop":   # need_w[3] false: all(need_w) fails, the Python per-step loop with dW[3] = None
        return frozen_names(case, "one_fs", names) | frozen_names(case, "input_layer", names)
    if which == "g_loop":        # need_v0 false while every W needs a gradient
        return frozen_names(case, "g", names) | frozen_names(case, "input_layer", names)
    if which == "all_but_final":  # the chain runs without an autograd node while grad is enabled
        return {n for n in names if not n.startswith("final.")}
    raise ValueError(which)


def shape_of(case: Case):
    cfg = case.cfg
    if case.kind == "attention":
        N = cfg["max_seq_len"]
        return case.B, N, cfg["embedding_size"], cfg["embedding_size"], math.ceil(math.log2(N))
    return case.B, cfg["n_vec"], cfg["embedding_size"], cfg["n_channels_V"], cfg["n_W"]


def init_state(case: Case) -> "OrderedDict[str, torch.Tensor]":
    """A float32 state_dict with the keys and shapes of the class, drawn from a seeded CPU generator: Linear layers uniform in
    +-1/sqrt(fan_in), tables uniform in +-0.5 (every row, the padding row too: the forward reads it like any other)."""
    gen = torch.Generator().manual_seed(1000 + case.seed)
    cfg, kind = case.cfg, case.kind
    _, N, E, C, M = shape_of(case)
    sd = OrderedDict()

    def table(name, rows):
        sd[name + ".weight"] = torch.rand(rows, E, generator=gen) - 0.5

    def linear(name, fan_in, fan_out):
        b = 1.0 / math.sqrt(fan_in)
        sd[name + ".weight"] = (torch.rand(fan_out, fan_in, generator=gen) * 2 - 1) * b
        sd[name + ".bias"] = (torch.rand(fan_out, generator=gen) * 2 - 1) * b

    def block(prefix, spec, out):
        width, i = E, 0
        for item in spec:
            if isinstance(item, int):
                linear(f"{prefix}.network.{i}", width, item)
                width = item
            i += 1
        linear(f"{prefix}.network.{i}", width, out)

    w_spec = [E, "GELU"] if kind == "attention" else cfg["Ws"]
    v_spec = [E, "GELU"] if kind == "attention" else cfg["V"]
    if kind != "attention":
        table("embedding", cfg["vocab_size"])
        table("pos_embedding", N)
    for m in range(M):
        block(f"fs.{m}", w_spec, M + 1)
    block("g", v_spec, C)
    if kind == "attention":
        table("embedding", cfg["vocab_size"])
        table("apc_embedding", N)
        return sd
    pooled = N * C if cfg["pooling_type"] == "FLATTEN" else C
    if cfg["head"][0] == "linear":
        linear("final", pooled, cfg["n_class"])
    else:
        linear("final.0", pooled, cfg["head"][1])
        linear("final.2", cfg["head"][1], cfg["n_class"])
    if kind == "synthetic" and cfg["add_init_linear_layer"]:
        linear("init_linear", 2, E)
    return sd


#: The f32 unit roundoff. A loss is one f32 number that follows several dependent f32 roundings (the head's sums, then the
#: softmax / mean or the sum): an f32 twin whose loss lands closer to float64 than ONE rounding error got there by roundings
#: that cancel, and 4 x that error is a bar no other order of f32 operations — not even the correctly rounded float64 value,
#: which may be 2^-24 off — can be held to. Like E32 = 0, such a batch gives a degenerate bar and is not used.
LOSS_FLOOR = 2.0 ** -24

def first_batch(case: Case, loss: str = None, start: int = 0) -> int:
    """The first batch number >= ``start`` whose f32-twin loss error on this host's CPU is at least LOSS_FLOOR."""
    sd32 = init_state(case)
    for k in range(start, start + 64):
        kw = dict(batches=(k,), loss=loss, sd32=sd32)
        if loss_error(run_twin(case, torch.float32, **kw), run_twin(case, torch.float64, **kw)) >= LOSS_FLOOR:
            return k
    raise RuntimeError("no batch found")


@functools.lru_cache(maxsize=None)
def batches_of(name: str, variant: str = None) -> tuple:
    """The batch numbers a case (variant None or a frozen one) or its "accumulate" / "sum_loss" variant runs on: the FIRST
    numbers 0, 1, 2, ... (the accumulation's second batch: after the first) that pass LOSS_FLOOR. A written rule evaluated where
    the test runs (the f32 twin's roundings depend on the host's CPU libraries); nothing of the library enters it."""
    if name not in CASE:
        return (0,)
    case = CASE["adding" if name == "per_step" else name]  # (per_step is adding's network and batches)
    if variant == "sum_loss":
        return (first_batch(case, "sum"),)
    main = first_batch(case)
    return (main, first_batch(case, None, main + 1)) if variant == "accumulate" else (main,)


def make_batch(case: Case, which: int = None):
    """(x, y, masks) of batch number ``which`` (None: the case's own, ``batches_of``): inputs, targets and the three keep masks,
    from a seeded CPU generator."""
    which = batches_of(case.name)[0] if which is None else which
    gen = torch.Generator().manual_seed(5000 + 10 * case.seed + which)
    cfg, kind = case.cfg, case.kind
    B, N, E, C, _ = shape_of(case)
    if kind == "synthetic" and cfg["problem"] == "adding":
        vals = torch.rand(B, N, generator=gen) * 2 - 1
        marks = torch.zeros(B, N)
        marks.scatter_(1, torch.stack([torch.randperm(N, generator=gen)[:2] for _ in range(B)]), 1.0)
        x = torch.stack([vals, marks], -1)
        y = 0.5 + (vals * marks).sum(1) / 4
    elif kind == "synthetic":
        x = torch.randint(0, cfg["vocab_size"] - 1, (B, N, 1), generator=gen)  # the last id never occurs: its dTable row is zero
        y = torch.randint(0, cfg["n_class"], (B,), generator=gen)
    elif kind == "attention":
        x = torch.randint(0, cfg["vocab_size"], (B, N), generator=gen)
        y = torch.randn(B, N, E, generator=gen)
    else:
        vocab = cfg["vocab_size"]
        x = torch.randint(0, vocab, (B, N), generator=gen)
        if cfg.get("problem") in ("imdb", "listops"):
            pad = vocab - 2
            x[x == pad] = 0
            for b in range(B):  # ragged tails of padding ids, as a padded batch has; row 0 (the CLS token) is never padding
                x[b, N - 1 - (7 * b) % (N // 2):] = pad
            x[:, 0] = vocab - 1
        y = torch.randint(0, cfg["n_class"], (B,), generator=gen)
    masks = {}
    for i, shape in ((1, (B, N, E)), (2, (B, N, C)), (3, (B, N, C))):
        p = cfg.get(f"dropout{i}_p", 0)
        masks[f"dropout{i}"] = (torch.rand(shape, generator=gen) >= p).to(torch.float32)
    return x, y, masks


# ---------------------------------------------------------------------------------------------------------- running it
def run_twin(case: Case, dtype, defect=None, frozen=None, batches=None, loss=None, sd32=None):
    """Gradients of the twin in ``dtype``: {"loss": float of the last batch, "grads": {name: ndarray or None}}. ``batches``: one
    backward per batch number without clearing the gradients in between."""
    sd32 = init_state(case) if sd32 is None else sd32
    fixed = frozen_names(case, frozen, sd32) if frozen else set()
    sd = {k: v.to(dtype).clone().requires_grad_(k not in fixed) for k, v in sd32.items()}
    value = None
    for which in batches or batches_of(case.name):
        x, y, masks = make_batch(case, which)
        out = forward(case.kind, case.cfg, sd, x.to(dtype) if x.is_floating_point() else x, masks, True, defect)
        value = loss_of(loss or case.loss, out, y)
        value.backward()
    return {"loss": float(value.detach()), "grads": {k: (None if v.grad is None else v.grad.numpy()) for k, v in sd.items()}}


def eval_logits(case: Case, dtype, sd32=None):
    sd32 = init_state(case) if sd32 is None else sd32
    sd = {k: v.to(dtype) for k, v in sd32.items()}
    x, _, masks = make_batch(case)
    with torch.no_grad():
        return forward(case.kind, case.cfg, sd, x.to(dtype) if x.is_floating_point() else x, masks, False).numpy()


def changed_outputs(case: Case, dtype, sd32=None):
    """(logits, map [B, N, N]) of the ChangedPSF twin in eval mode."""
    sd32 = init_state(case) if sd32 is None else sd32
    sd = {k: v.to(dtype) for k, v in sd32.items()}
    x, _, masks = make_batch(case)
    with torch.no_grad():
        out, att = forward(case.kind, case.cfg, sd, x, masks, False, want_map=True)
    return out.numpy(), att.numpy()


def per_param_error(got: dict, ref: dict) -> dict:
    """{name: rel_inf(got, ref)} over the parameters ``ref`` has a gradient for."""
    return {k: rel_inf(got[k], r) for k, r in ref.items() if r is not None and got.get(k) is not None}


def e32_of(run32: dict, run64: dict) -> float:
    return max(per_param_error(run32["grads"], run64["grads"]).values())


def loss_error(run: dict, run64: dict) -> float:
    return abs(run["loss"] - run64["loss"]) / abs(run64["loss"])


Verdict = namedtuple("Verdict", "failures worst worst_name bar errors")


def compare(got: dict, ref64: dict, e32: float, loss_e32: float = None) -> Verdict:
    """The library's (or a damaged twin's) run ``got`` against the float64 twin's ``ref64`` with the bar FACTOR * e32.
    ``failures`` is empty when: the parameters without a gradient are exactly the twin's; every element the twin has as an exact
    zero is an exact zero; every parameter's rel_inf error is within the bar; and (``loss_e32`` given) the loss is within
    FACTOR * loss_e32."""
    bar = FACTOR * e32
    failures, errors = [], {}
    for name, r in ref64["grads"].items():
        g = got["grads"].get(name)
        if r is None or g is None:
            if (r is None) != (g is None):
                failures.append(f"{name}: gradient is {'None' if g is None else 'set'}, the twin's is {'None' if r is None else 'set'}")
            continue
        g = np.asarray(g)
        if g.shape != r.shape:
            failures.append(f"{name}: shape {g.shape} against {r.shape}")
            continue
        if not np.isfinite(g).all():
            failures.append(f"{name}: not finite")
            continue
        zero = r == 0
        if zero.any() and (g[zero] != 0).any():
            failures.append(f"{name}: {int((g[zero] != 0).sum())} of the twin's {int(zero.sum())} exact zeros are not zero "
                            f"(largest {np.abs(g[zero]).max():.3e})")
        errors[name] = rel_inf(g, r)
        if not errors[name] <= bar:
            failures.append(f"{name}: error {errors[name]:.3e} > bar {bar:.3e} ({errors[name] / bar:.1f} x)")
    if set(got["grads"]) != set(ref64["grads"]):
        failures.append(f"parameter names differ: {sorted(set(got['grads']) ^ set(ref64['grads']))}")
    if loss_e32 is not None:
        le = loss_error(got, ref64)
        if not le <= FACTOR * loss_e32:
            failures.append(f"loss: error {le:.3e} > {FACTOR * loss_e32:.3e}")
    worst_name = max(errors, key=errors.get) if errors else None
    return Verdict(failures, errors.get(worst_name, 0.0), worst_name, bar, errors)


# -------------------------------------------------------------------------------------------------------------- defects
#: name -> (what is wrong in the twin, the cases it can show in)
DEFECTS = OrderedDict([
    ("dw_last_token", ("dW of the last token of one step lost", ("adding", "order_cls_len", "listops_like"))),
    ("dv0_last_token", ("dV0 of the last token lost", ("adding", "order_cls_len", "listops_like"))),
    ("residual_one_step", ("the residual's gradient of one step lost", ("adding", "order_cls_len", "listops_like"))),
    ("fs_swapped", ("fs[0] and fs[1] swapped", ("adding", "pathfinder_like", "stacked"))),
    ("last_offset_plus_one", ("the last link's offset off by one (N not a power of two)",
                              ("order_cls_len", "listops_like", "imdb_like", "attention_block"))),
    ("padding_row_not_zeroed", ("the padding row's gradient not zeroed", ("listops_like", "imdb_like"))),
    ("dropout2_after_loop", ("dropout2 applied after the loop instead of before it", ("listops_like",))),
    ("dpos_first_sample_only", ("dpos not summed over the batch", ("order_cls_len", "pathfinder_like", "attention_block"))),
    ("cls_reads_last_row", ("CLS pooling reading row N - 1", ("listops_like", "imdb_like"))),
    ("links_dx_dropped", ("the narrow / wide dX halves of the MLP backward not added (only g's kept)",
                          ("pathfinder_like", "genome", "attention_block"))),
])


def defect_ratio(case: Case, defect: str, ref64: dict, e32: float, sd32=None) -> tuple:
    """(worst error / bar, parameter) of the float32 twin with ``defect`` against the clean float64 twin. An exact zero that is
    no longer zero (the padding row) counts as an error of the size of that residue relative to the parameter's largest gradient."""
    bad = run_twin(case, torch.float32, defect=defect, sd32=sd32)
    errs = per_param_error(bad["grads"], ref64["grads"])
    name = max(errs, key=errs.get)
    return errs[name] / (FACTOR * e32), name


# --------------------------------------------------------------------------------------------------------------- report
def measure_cpu() -> dict:
    """Everything the CPU can say: per case E32 (and the parameter that sets it), the loss and eval-logit errors of the f32
    twin, and per defect the ratio over the bar."""
    out = OrderedDict()
    for case in CASES:
        sd32 = init_state(case)
        r64, r32 = run_twin(case, torch.float64, sd32=sd32), run_twin(case, torch.float32, sd32=sd32)
        errs = per_param_error(r32["grads"], r64["grads"])
        name = max(errs, key=errs.get)
        row = dict(e32=errs[name], e32_param=name, n_params=len(errs), loss_e32=loss_error(r32, r64),
                   logits_e32=rel_inf(eval_logits(case, torch.float32, sd32), eval_logits(case, torch.float64, sd32)), defects={})
        for d, (_, where) in DEFECTS.items():
            if case.name in where:
                row["defects"][d] = defect_ratio(case, d, r64, row["e32"], sd32)
        out[case.name] = row
    return out


def gpu_lines(text: str) -> dict:
    """{case or case/variant: (worst error, parameter, E32 on that host)} from the "TWIN ..." lines tests/test_gpu_model_twin.py prints."""
    import re
    pat = re.compile(r"TWIN (\S+): E32 (\S+) bar \S+ worst (\S+) \(\S+ x bar\) at (\S+);")
    return {m.group(1): (float(m.group(3)), m.group(4), float(m.group(2))) for m in pat.finditer(text)}


def _table(head, rows):
    return "\n".join(["| " + " | ".join(head) + " |", "|" + "---|" * len(head)] + ["| " + " | ".join(r) + " |" for r in rows])


def report_blocks(cpu: dict, log: str = "") -> dict:
    """{block name: Markdown} of everything measured in profiles/model_twin_grads.md. ``cpu``: ``measure_cpu()``; ``log``: the output
    of the GPU run (tests/test_gpu_model_twin.py prints "TWIN...", "ROUTES ..." lines). The CPU columns are the host's that ran
    ``measure_cpu``; the library's error is set against the bar of the host that ran the GPU test, which is what it asserts."""
    import re
    gpu = gpu_lines(log)
    rows = []
    for case in CASES:
        r, g = cpu[case.name], gpu.get(case.name)
        lib = ("-",) * 5 if g is None else (f"{g[2]:.2e}", f"{FACTOR * g[2]:.2e}", f"{g[0]:.2e}", f"{g[0] / (FACTOR * g[2]):.2f}", f"`{g[1]}`")
        rows.append((case.name, str(shape_of(case)), str(r["n_params"]), f"{r['e32']:.2e}", f"`{r['e32_param']}`", *lib))
    blocks = {"cases": _table(("case", "(B, N, E, C, M)", "parameters", "E32, CPU host", "set by", "E32, GPU host's CPU", "bar there = 4 x E32",
                               "library worst error", "error / bar", "parameter"), rows)}
    blocks["variants"] = _table(("case / variant", "E32, GPU host's CPU", "library worst error", "error / bar", "parameter"),
                                [(k, f"{v[2]:.2e}", f"{v[0]:.2e}", f"{v[0] / (FACTOR * v[2]):.2f}", f"`{v[1]}`") for k, v in gpu.items() if "/" in k])
    blocks["routes"] = _table(("case", "`fused_mlp.route` answers", "chain backward", "entry point: calls asserted", "reaches"),
                              [(c.name, ", ".join(map(str, c.routes["mlp"])) or "not asked", c.routes["chain_bwd"],
                                ", ".join(f"`{k}`: {v}" for k, v in c.routes["calls"].items()), c.note) for c in CASES])
    pat = re.compile(r"TWIN-LOSS (\S+) batches (\([^)]*\)): \S+ against \S+ error (\S+) bar (\S+) \((\S+) x\)")
    blocks["losses"] = _table(("case / variant", "batches", "library loss error", "bar = 4 x the f32 twin's", "error / bar"),
                              [(m.group(1).replace("/None", ""), m.group(2), m.group(3), m.group(4), m.group(5)) for m in pat.finditer(log)])
    pat = re.compile(r"TWIN-EVAL (\S+) route=(\S+): mixer calls (\d+) error (\S+) bar (\S+) \((\S+) x\)")
    blocks["eval"] = _table(("case", "`fused_mixer.route`", "`psf_mixer_fwd_in_f32` calls", "logit error", "bar", "error / bar"),
                            [m.groups() for m in pat.finditer(log)])
    pat = re.compile(r"TWIN-MAP (\S+): map (\S+) bar (\S+); logits (\S+) bar (\S+)")
    blocks["map"] = _table(("ChangedPSF case", "map error", "bar", "logit error", "bar"), [m.groups() for m in pat.finditer(log)])
    blocks["defects"] = _table(("defect seeded into the f32 twin", "case", "worst error / bar", "parameter"),
                               [(text, c.name, f"{cpu[c.name]['defects'][d][0]:.0f} x", f"`{cpu[c.name]['defects'][d][1]}`")
                                for d, (text, _) in DEFECTS.items() for c in CASES if d in cpu[c.name]["defects"]])
    return blocks


def report(cpu: dict, log: str = "", old: str = None) -> str:
    """profiles/model_twin_grads.md: ``old`` (the present file) with every ``<!-- begin NAME -->`` ... ``<!-- end NAME -->`` block
    replaced by what was measured now, the text around the blocks kept; without ``old``, the blocks alone."""
    import re
    blocks = report_blocks(cpu, log)
    if old is None:
        return "\n\n".join(f"<!-- begin {k} -->\n{v}\n<!-- end {k} -->" for k, v in blocks.items()) + "\n"
    for k, v in blocks.items():
        old, n = re.subn(rf"(<!-- begin {k} -->\n).*?(\n<!-- end {k} -->)", lambda m: m.group(1) + v + m.group(2), old, flags=re.S)
        assert n == 1, f"block {k} not found"
    return old


if __name__ == "__main__":  # python tests/psf_twin.py <output of `pytest tests/test_gpu_model_twin.py -m gpu -s`> [file to update]
    import sys
    log = open(sys.argv[1]).read() if len(sys.argv) > 1 else ""
    if len(sys.argv) > 2:
        text = report(measure_cpu(), log, open(sys.argv[2]).read())
        open(sys.argv[2], "w").write(text)
    else:
        print(report(measure_cpu(), log))
