"""``TokenLinear`` — ``nn.Linear`` for the token-wise MLPs that produce the chain's operands
(``MLPBlock``, SyntheticExperiments/psf.py:35-60: ``W_m = fs[m](data)``, ``V = g(data)``).

Same parameters, same state_dict keys, same forward (``addmm`` on rocBLAS/hipBLASLt). Only the weight and bias
gradients differ: for T = B*N tokens and layer widths of 2..128 they are a reduction over ~10^6 rows into a tile
of a few hundred numbers, for which library GEMMs take ~1 ms per layer (84 % of a training step at
Order/Adding N = 16384 — profiles/r01_train_step_profile.log). ``psf_linear_wgrad_f32`` (csrc/linear_wgrad.hip)
streams X and dY once through the f32 matrix core instead. Layers outside its range (wide ListOps layers,
fp64, CPU tensors) use the stock autograd formulas. bf16 layers do too, unless ``bf16_linear_route`` is "always":
then ``psf_linear_wgrad_bf16`` (csrc/linear_wgrad_bf16.hip) takes them on the bf16 matrix core.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib

MAX_WIDTH = 128   # kernel limit on in_features / out_features
MIN_TOKENS = 4096  # below this the stock path is fine


def autocast_on(t: torch.Tensor) -> bool:
    """Autocast is active for ``t``'s device. An autocast-eligible op inside a custom Function (``F.linear``) then returns
    bf16 / f16, and autograd hands the Function's backward an upstream gradient of that dtype: the kernels behind the
    Functions here are typed by their name only, so under autocast ``TokenLinear`` and the J > 8 FLATTEN head are the stock
    modules ("Autocast and index types"). No kernel here takes a CPU tensor; "cpu" is answered so that the
    host tests can drive ``TokenLinear.forward`` under ``torch.autocast("cpu")``. ``TokenLinear.forward`` asks once and
    ``wgrad_supported`` again: the second answer is for ``fused_mlp.stacked_apply``, which calls ``_TokenLinearFn`` itself."""
    kind = t.device.type
    return kind in ("cuda", "cpu") and torch.is_autocast_enabled(kind)


# "never" (default) or "always": whether the token-wise Linear layers of a bf16 model run on the library's bf16 instances — the
# weight / bias gradient on psf_linear_wgrad_bf16 (csrc/linear_wgrad_bf16.hip: bf16 matrix core, f32 sums, one rounding) and the
# rows of a 1-3-input layer on psf_affine_rows_bf16 — instead of the stock F.linear and its library GEMMs. A switch of its own,
# not a wider meaning of ``bf16_route``: models that run with that one at "always" keep their bits. Opt-in because the weight
# gradient then comes from another summation order than the library GEMM's (profiles/bf16_linear_wgrad_ab.md). At "never"
# nothing of it is reached.
bf16_linear_route = "never"


def _bf16_linear_on() -> bool:
    if bf16_linear_route not in ("never", "always"):
        raise ValueError(f'token_linear.bf16_linear_route must be "never" or "always", not {bf16_linear_route!r}')
    return bf16_linear_route == "always"


def wgrad_supported(x2d: torch.Tensor, out_features: int) -> bool:
    if x2d.dtype == torch.bfloat16:
        if not _bf16_linear_on():  # (asked first: a misspelt switch raises for every bf16 layer, wherever its operands live)
            return False
    elif x2d.dtype != torch.float32:
        return False
    return (x2d.is_cuda and x2d.shape[0] >= MIN_TOKENS and x2d.shape[1] <= MAX_WIDTH and out_features <= MAX_WIDTH
            and not autocast_on(x2d))


def _wgrad_bf16_operand(t: torch.Tensor, width: int) -> torch.Tensor:
    """``t`` as psf_linear_wgrad_bf16 takes it: unit inner stride, a row stride >= the width, and a base aligned to the vector
    the entry loads for that row stride (2 g bytes, g the largest power of two <= 8 dividing the stride). A slice that misses
    any of it is made contiguous (a fresh allocation is aligned for every stride)."""
    if t.stride(1) != 1 or t.stride(0) < width:
        return t.contiguous()
    ld = t.stride(0)
    if t.data_ptr() % (2 * (8 if ld % 8 == 0 else ld & -ld)):
        return t.contiguous()
    return t


def _linear_wgrad_bf16(x2d: torch.Tensor, dy2d: torch.Tensor, need_bias: bool):
    T, m = x2d.shape
    n = dy2d.shape[1]
    lib = _lib.load()
    ws_bytes = lib.psf_linear_wgrad_bf16_workspace(T, m, n)
    if ws_bytes < 0:
        raise ValueError(f"psf_linear_wgrad_bf16 does not support T={T}, m={m}, n={n}")
    x2d, dy2d = _wgrad_bf16_operand(x2d, m), _wgrad_bf16_operand(dy2d, n)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x2d.device)
    dW = torch.empty((n, m), dtype=torch.bfloat16, device=x2d.device)
    db = torch.empty(n, dtype=torch.bfloat16, device=x2d.device) if need_bias else None
    with torch.cuda.device(x2d.device):
        rc = lib.psf_linear_wgrad_bf16(x2d.data_ptr(), x2d.stride(0), dy2d.data_ptr(), dy2d.stride(0), T, m, n, dW.data_ptr(),
                                       db.data_ptr() if db is not None else None, ws.data_ptr(), ws_bytes,
                                       _lib.stream_ptr(x2d.device))
    _lib.check(rc, "psf_linear_wgrad_bf16")
    return dW, db


def linear_wgrad(x2d: torch.Tensor, dy2d: torch.Tensor, need_bias: bool = True):
    """(dWeight [n, m], dBias [n] or None) for X [T, m], dY [T, n] on the HIP kernel. Both float32 on one HIP device — or, with
    ``bf16_linear_route`` at "always", both bfloat16: anything else is a TypeError (the entry takes raw addresses and would read
    another dtype's bytes as its own)."""
    operands = (("x", x2d), ("dy", dy2d))
    want = torch.float32
    if isinstance(x2d, torch.Tensor) and x2d.dtype == torch.bfloat16 and _bf16_linear_on():
        want = torch.bfloat16
    takes = "float32" if want == torch.float32 else "bfloat16"
    for name, t in operands:  # the element type first, of both operands: the message names the one that is wrong and why
        if not isinstance(t, torch.Tensor) or t.dtype != want:
            raise TypeError(f"linear_wgrad takes {takes} tensors on one HIP device; {name} is {getattr(t, 'dtype', type(t))}")
    for name, t in operands:
        if not t.is_cuda or t.device != x2d.device:
            raise TypeError(f"linear_wgrad takes {takes} tensors on one HIP device; {name} is on '{t.device}'"
                            + (f", x on '{x2d.device}'" if t.is_cuda else ""))
    if want == torch.bfloat16:
        return _linear_wgrad_bf16(x2d, dy2d, need_bias)
    T, m = x2d.shape
    n = dy2d.shape[1]
    lib = _lib.load()
    ws_bytes = lib.psf_linear_wgrad_workspace(T, m, n)
    if ws_bytes < 0:
        raise ValueError(f"psf_linear_wgrad does not support T={T}, m={m}, n={n}")
    # column slices of a wider row-major array (unit inner stride) are taken as they are, with their row stride
    if x2d.stride(1) != 1 or x2d.stride(0) < m:
        x2d = x2d.contiguous()
    if dy2d.stride(1) != 1 or dy2d.stride(0) < n:
        dy2d = dy2d.contiguous()
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=x2d.device)
    dW = torch.empty((n, m), dtype=torch.float32, device=x2d.device)
    db = torch.empty(n, dtype=torch.float32, device=x2d.device) if need_bias else None
    with torch.cuda.device(x2d.device):
        rc = lib.psf_linear_wgrad_strided_f32(x2d.data_ptr(), x2d.stride(0), dy2d.data_ptr(), dy2d.stride(0), T, m, n,
                                              dW.data_ptr(), db.data_ptr() if db is not None else None, ws.data_ptr(),
                                              ws_bytes, _lib.stream_ptr(x2d.device))
    _lib.check(rc, "psf_linear_wgrad_strided_f32")
    return dW, db


def _affine_rows_bf16_supported(x: torch.Tensor, weight: torch.Tensor, bias) -> bool:
    return (_bf16_linear_on() and x.is_cuda and weight.dtype == torch.bfloat16 and x.dim() >= 2 and 1 <= x.shape[-1] <= 3
            and weight.dim() == 2 and weight.shape[1] == x.shape[-1] and weight.shape[0] % 8 == 0 and 8 <= weight.shape[0] <= 1024
            and (bias is None or bias.dtype == torch.bfloat16) and not autocast_on(x))


def affine_rows_supported(x: torch.Tensor, weight: torch.Tensor, bias) -> bool:
    """``x @ weight.T + bias`` with at most three inputs per position on the GPU in fp32: psf_affine_rows_f32 (csrc/embed.hip)
    writes the rows in one pass (init_linear of the synthetic PSFNet, SyntheticExperiments/psf.py:153-154: a library GEMM
    takes 80 us for that K = 2 product at 1 M positions, the pass 25). The bf16 case (psf_affine_rows_bf16, E a multiple of 8)
    when ``bf16_linear_route`` is "always"."""
    if x.dtype == torch.bfloat16:
        return _affine_rows_bf16_supported(x, weight, bias)
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() >= 2 and 1 <= x.shape[-1] <= 3
            and weight.dim() == 2 and weight.shape[1] == x.shape[-1] and weight.shape[0] % 4 == 0 and 4 <= weight.shape[0] <= 1024
            and (bias is None or bias.dtype == torch.float32))


def affine_rows(x: torch.Tensor, weight: torch.Tensor, bias) -> torch.Tensor:
    """The rows themselves (no autograd). Products summed in input order with fused adds, then one rounded add of the bias —
    the arithmetic of the mixer kernels' affine recipe, bit for bit. bf16 operands: the same f32 chain, rounded to bf16 once."""
    K, E = x.shape[-1], weight.shape[0]
    x2 = x.detach().reshape(-1, K).contiguous()
    w = weight.detach().contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    out = torch.empty((x2.shape[0], E), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    entry, name = ((lib.psf_affine_rows_bf16, "psf_affine_rows_bf16") if x.dtype == torch.bfloat16
                   else (lib.psf_affine_rows_f32, "psf_affine_rows_f32"))
    with torch.cuda.device(x.device):
        rc = entry(x2.data_ptr(), w.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                   x2.shape[0], K, E, _lib.stream_ptr(x.device))
    _lib.check(rc, name)
    return out.reshape(*x.shape[:-1], E)


class _TokenLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if affine_rows_supported(x, weight, bias):
            return affine_rows(x, weight, bias)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = dy.matmul(weight) if need_x else None
        dW = db = None
        if need_w or need_b:
            dW, db = linear_wgrad(x.reshape(-1, x.shape[-1]), dy.reshape(-1, dy.shape[-1]), need_b)
            if not need_w:
                dW = None
        return dx, dW, db


EMB_MAX_VOCAB, EMB_MAX_WIDTH = 512, 4096  # limits of psf_embed_tokens_bwd_f32

# "never" (default) or "always": whether bf16 token embeddings run on the library's bf16 instances — the lookup fused with the
# positional add on psf_embed_tokens_bf16 (the bits of the stock `embedding(idx) + pos` in bf16) and the table gradient on
# psf_embed_tokens_bwd_bf16 (f32 partial sums, one rounding: capturable, unlike aten::embedding_dense_backward) — instead of
# the stock nn.Embedding path. "always" is what makes a bf16 token model capturable by train.GraphedStep; opt-in like
# chord.bf16_chain_bwd_route, because the table gradient then differs from the stock operator's in its summation order
# (profiles/bf16_train_graph_ab.md). At "never" nothing here is reached.
bf16_route = "never"


def embedding_wgrad(idx: torch.Tensor, dout: torch.Tensor, vocab: int, padding_idx) -> torch.Tensor:
    """d(table) [vocab, E] of ``table[idx]`` given d(out) [..., E]: ``psf_embed_tokens_bwd_f32`` (csrc/embed.hip —
    per-slice LDS tables with single-owner accumulation, fixed-order reduction: deterministic, no host read-back, so
    a training step stays capturable in a HIP graph). Vocabularies beyond its LDS table use PyTorch's kernel — in
    eager mode only: under stream capture that case raises (the aten operator is not capturable). A bf16 ``dout`` goes to
    ``psf_embed_tokens_bwd_bf16`` (same kernels, f32 partial sums, a bf16 table gradient rounded once) when ``bf16_route`` is
    "always", and through the aten operator otherwise."""
    E = dout.shape[-1]
    d2 = dout.reshape(-1, E).contiguous()
    T = d2.shape[0]
    if idx.dtype != torch.int64:  # nn.Embedding takes int32 ids too; psf_embed_tokens_bwd_f32 reads ``const int64_t*``
        idx = idx.to(torch.int64)
    bf16 = dout.dtype == torch.bfloat16 and bf16_route == "always" and dout.is_cuda
    if vocab > EMB_MAX_VOCAB or E > EMB_MAX_WIDTH or not (dout.dtype == torch.float32 or bf16) or T == 0:
        if dout.is_cuda and torch.cuda.is_current_stream_capturing():
            # aten::embedding_dense_backward sizes a rocprim partition from a host read-back: not capturable, and a
            # replay of such a capture faulted the GPU (profiles/r01_graph_step_lab.log). Refuse instead.
            raise RuntimeError(
                f"embedding gradient for a {vocab} x {E} {dout.dtype} table cannot be captured in a HIP graph: the "
                f"capturable kernel psf_embed_tokens_bwd_f32 is limited to vocab <= {EMB_MAX_VOCAB}, width <= "
                f"{EMB_MAX_WIDTH}, float32, and the fallback aten::embedding_dense_backward reads sizes back to the host")
        pad = -1 if padding_idx is None else padding_idx
        return torch.ops.aten.embedding_dense_backward(dout.contiguous(), idx, vocab, pad, False)
    lib = _lib.load()
    idx_c = idx.reshape(-1).contiguous()
    ws_bytes = lib.psf_embed_tokens_bwd_workspace(T, vocab, E)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=d2.device)
    dW = torch.empty((vocab, E), dtype=dout.dtype, device=d2.device)
    entry, name = ((lib.psf_embed_tokens_bwd_bf16, "psf_embed_tokens_bwd_bf16") if bf16
                   else (lib.psf_embed_tokens_bwd_f32, "psf_embed_tokens_bwd_f32"))
    with torch.cuda.device(d2.device):
        rc = entry(idx_c.data_ptr(), d2.data_ptr(), T, vocab, E, dW.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(d2.device))
    _lib.check(rc, name)
    if padding_idx is not None and padding_idx >= 0:
        dW[padding_idx].zero_()
    return dW


class _TokenEmbeddingFn(torch.autograd.Function):
    """weight[idx] whose weight gradient runs on ``embedding_wgrad`` instead of PyTorch's sort-and-scatter (4.5 ms
    per step for the 6-token vocabulary of Temporal Order at T = 655 360)."""

    @staticmethod
    def forward(ctx, idx, weight, padding_idx):
        ctx.save_for_backward(idx)
        ctx.vocab, ctx.padding_idx = weight.shape[0], padding_idx
        return torch.nn.functional.embedding(idx, weight, padding_idx)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        return None, embedding_wgrad(idx, dout, ctx.vocab, ctx.padding_idx), None


class _EmbedTokensFn(torch.autograd.Function):
    """out = weight[idx] (+ pos broadcast over the batch) in one pass (csrc/embed.hip). Gradients: the table's by
    ``embedding_wgrad``; pos's is the sum of the output gradient over the batch."""

    @staticmethod
    def forward(ctx, idx, weight, pos, padding_idx):
        lib = _lib.load()
        V, E = weight.shape
        idx_c = idx.contiguous()
        T = idx_c.numel()
        N = pos.shape[0] if pos is not None else 1
        out = torch.empty(*idx.shape, E, dtype=weight.dtype, device=idx.device)
        w, p = weight.detach().contiguous(), (pos.detach().contiguous() if pos is not None else None)
        entry, name = ((lib.psf_embed_tokens_bf16, "psf_embed_tokens_bf16") if weight.dtype == torch.bfloat16
                       else (lib.psf_embed_tokens_f32, "psf_embed_tokens_f32"))
        with torch.cuda.device(idx.device):
            rc = entry(idx_c.data_ptr(), w.data_ptr(), p.data_ptr() if p is not None else None, out.data_ptr(), T, N, V, E,
                       _lib.stream_ptr(idx.device))
        _lib.check(rc, name)
        ctx.save_for_backward(idx_c)
        ctx.vocab, ctx.padding_idx, ctx.has_pos, ctx.n_pos = V, padding_idx, pos is not None, N
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        E = dout.shape[-1]
        dW = dpos = None
        if ctx.needs_input_grad[1]:
            dW = embedding_wgrad(idx, dout, ctx.vocab, ctx.padding_idx)
        if ctx.has_pos and ctx.needs_input_grad[2]:
            dpos = dout.reshape(-1, ctx.n_pos, E).sum(0)
        return None, dW, dpos, None


def _vec16(t: torch.Tensor) -> bool:
    """What psf_embed_tokens_bf16 reads as it stands (a non-contiguous operand is copied, and a copy is aligned)."""
    return not t.is_contiguous() or t.data_ptr() % 16 == 0


def embed_tokens(idx: torch.Tensor, embedding: nn.Embedding, pos: torch.Tensor = None) -> torch.Tensor:
    """``embedding(idx) + pos.unsqueeze(0)`` (``pos`` [N, E] with N = idx.shape[-1], or None) — the opening lines of
    every PSFNet.forward. One fused pass on the GPU for plain fp32 embeddings; anything else (CPU, max_norm, sparse
    gradients, E not a multiple of 4) takes the stock modules. bf16 tables take the pass too when ``bf16_route`` is "always"
    (``pos`` bf16 or None, E a multiple of 8, 16-byte aligned storage), and the stock modules otherwise."""
    w = embedding.weight
    if (bf16_route == "always" and idx.is_cuda and idx.dtype == torch.int64 and w.dtype == torch.bfloat16 and w.shape[1] % 8 == 0
            and embedding.max_norm is None and not embedding.scale_grad_by_freq and not embedding.sparse
            and _vec16(w) and (pos is None or (pos.dtype == torch.bfloat16 and pos.dim() == 2 and pos.shape[0] == idx.shape[-1]
                                               and pos.shape[1] == w.shape[1] and _vec16(pos)))):
        return _EmbedTokensFn.apply(idx, w, pos, embedding.padding_idx)
    if (idx.is_cuda and idx.dtype == torch.int64 and w.dtype == torch.float32 and w.shape[1] % 4 == 0
            and embedding.max_norm is None and not embedding.scale_grad_by_freq and not embedding.sparse
            and (pos is None or (pos.dtype == torch.float32 and pos.dim() == 2 and pos.shape[0] == idx.shape[-1]
                                 and pos.shape[1] == w.shape[1]))):
        return _EmbedTokensFn.apply(idx, w, pos, embedding.padding_idx)
    out = embedding(idx)
    return out if pos is None else out + pos.unsqueeze(0)


class TokenEmbedding(nn.Embedding):
    """Drop-in ``nn.Embedding`` (same parameters / state_dict / forward values) for small vocabularies looked up
    at ~1e6 positions; larger vocabularies, CPU tensors and exotic options use the stock path."""

    def forward(self, idx: torch.Tensor) -> torch.Tensor:
        if (torch.is_grad_enabled() and self.weight.requires_grad and idx.is_cuda
                and (self.weight.dtype == torch.float32 or (self.weight.dtype == torch.bfloat16 and bf16_route == "always"))
                and self.num_embeddings <= EMB_MAX_VOCAB and self.embedding_dim <= EMB_MAX_WIDTH
                and self.max_norm is None and not self.scale_grad_by_freq and not self.sparse):
            return _TokenEmbeddingFn.apply(idx, self.weight, self.padding_idx)
        return super().forward(idx)


class TokenLinear(nn.Linear):
    """Drop-in ``nn.Linear`` (``isinstance(layer, nn.Linear)`` holds; identical parameters and state_dict)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if autocast_on(x):  # nn.Linear itself: the dtype, values and gradients autocast gives the stock module
            return super().forward(x)
        if torch.is_grad_enabled() and (self.weight.requires_grad or (self.bias is not None and self.bias.requires_grad)) \
                and x.dim() >= 2 and wgrad_supported(x.reshape(-1, x.shape[-1]), self.out_features):
            return _TokenLinearFn.apply(x, self.weight, self.bias)
        if not torch.is_grad_enabled() and affine_rows_supported(x, self.weight, self.bias):
            return affine_rows(x, self.weight, self.bias)
        return super().forward(x)
