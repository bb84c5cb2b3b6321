"""Fused PSFNet producer MLPs (``g`` and ``fs[0..M)``) — forward and backward in one launch each.

``MLPBlock`` is ``Linear(E, h) -> GELU -> Linear(h, out)`` (SyntheticExperiments/psf.py:35-60); PSFNet applies
M+1 of them to the same ``data`` (psf.py:165,175). ``ROUTES`` is the ordered table of the ways to run them, each a predicate
and the function it guards; ``route(x, blocks)`` names the first whose predicate takes a call and ``apply(x, blocks)`` runs it.
The order is stated there and nowhere else. A call that no route takes (CPU tensors, MLPs of another form, a single fp64 MLP)
gets None and runs the stock modules. ``_walk`` is the one check of a call against a route's limits (``_Limits``).
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import List, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

enabled = True        # module-level switches (tests / A-B timing), read at every call
train_enabled = True
wide_enabled = True
bf16_enabled = True
bf16_train_route = "never"  # "always": a bf16 call that needs a gradient takes "bf16_train" (below) instead of "stacked"

#: name: (predicate, function), in the order ``route`` asks the predicates; ``apply`` calls ``function(x, blocks)`` of the first
#: that says yes. Names, not functions: both are looked up in this module when a call is routed, so a test or an A-B script
#: that replaces ``wide_apply`` is the one that runs.
ROUTES = {
    # The narrow kernels. psf_mlp_fwd_f32 (csrc/mlp_fwd.hip) evaluates all MLPs from one read of ``data`` on the f32 matrix
    # core, the hidden layer staying in registers. First: nothing needs a gradient, nothing is saved.
    "narrow_forward": ("eligible", "fused_mlp_forward"),
    # ... under autograd. psf_mlp_bwd_f32 (csrc/mlp_bwd.hip) recomputes the hidden layer, accumulates dX over all MLPs in
    # registers and reduces weight gradients in a fixed order, so the forward saves only ``data`` and the parameters (autograd
    # through the PyTorch layers keeps 2 x [T, (M+1) h] activations). Before the wide kernels, whose limits overlap these at
    # E = 16 and 32: the narrow ones never let a hidden activation reach memory.
    "narrow_train": ("trainable", "fused_mlp_apply"),
    # f32 past the narrow limits: the LRA widths, E up to 1024, outputs up to 128 (the reference ListOps network has E = 512,
    # out = 12 and 128, LRA/psf_training_config.py:2-30), with or without autograd (csrc/mlp_wide.hip). The M+1 first layers are
    # ONE stacked GEMM on the bf16 matrix pipe at f32 accuracy, forward, input gradient and weight gradient; the forward keeps
    # the hidden pre-activations for the backward instead of recomputing them.
    "wide": ("wide_ok", "wide_apply"),
    # Inference of a bf16 model (``PSFNet(...).to(torch.bfloat16)`` under ``no_grad``; csrc/mlp_fwd_bf16.hip): one launch, one
    # MFMA term per product, the three roundings of the layer-by-layer evaluation. It shares no call with the three above
    # (they want f32) and comes before the stacked route, which takes every dtype, at every T: 3.3-5.7 x faster than
    # stacked_apply at every size of profiles/bf16_mlp_ab.md (1 024 tokens: 398.9 -> 109.8 us per call; 1 048 576 tokens:
    # 1947.7 -> 342.9 us). Training in bf16 (unless "bf16_train" below is switched on) and the LRA widths in bf16 go on to
    # ``stacked_apply``. Autocast with f32 parameters does not come here: f32 ``data`` keeps the f32 routes above, which call no
    # autocast-eligible op and return f32 under autocast too; bf16 ``data`` (made by an autocast op upstream) with f32
    # parameters matches NO route — every route wants x and the first layer's weight of one dtype — and ``apply`` returns None:
    # the blocks' own layers run, which under autocast are nn.Linear (tests/test_gpu_autocast.py pins both).
    "bf16_forward": ("bf16_eligible", "fused_mlp_forward_bf16"),
    # ... under autograd, opt-in (``bf16_train_route = "always"``; the default "never" leaves training on ``stacked_apply``).
    # psf_mlp_fwd_bf16 forward, saving only ``data`` and the parameters, and psf_mlp_bwd_bf16 (csrc/mlp_bwd_bf16.hip) backward:
    # the hidden layer recomputed with the forward's bits, the roundings of PyTorch's bf16 autograd on the stacked route (one per
    # tensor it materialises), dX accumulated over all MLPs in f32 and rounded once, weight gradients reduced in a fixed order.
    # The two [T, sum h] bf16 activations of the stacked route are neither written nor read back. E <= 32, at most MAX_K MLPs.
    "bf16_train": ("bf16_trainable", "fused_mlp_apply_bf16"),
    # Last, whatever no kernel of ours took (fp64, odd widths), on library GEMMs laid out for it: the M+1 first layers share
    # their input, so they run as ONE Linear(E, sum h) — one GEMM forward, one for the input gradient (K = sum h, instead of
    # M+1 GEMMs plus M accumulations of a [T, E] tensor) and one for the weight gradient; GELU and its backward one kernel each.
    "stacked": ("stackable", "stacked_apply"),
}

#: What a kernel family takes: x and the parameters of ``dtype``, E within [e_min, e_max] and a multiple of e_mult (bf16: a
#: row of X is then a whole number of 16-byte vectors), hidden widths <= h_max, output widths <= o_max, at most k_max MLPs
#: (the narrow forward launchers split a longer call). ``all_params``: the dtype of all four parameters of a block is looked
#: at, not only the first layer's weight. ``_ANY`` is ``stackable``'s looser rule: the dtype of x, whatever it is, at any size.
_Limits = namedtuple("_Limits", "dtype e_min e_max e_mult h_max o_max k_max all_params")
MAX_K = 32            # MLPs per launch of the narrow kernels
_NARROW = _Limits(torch.float32, 4, 64, 4, 128, 32, 1 << 30, False)
_NARROW_TRAIN = _NARROW._replace(e_max=32, k_max=MAX_K)
_BF16 = _Limits(torch.bfloat16, 8, 64, 8, 128, 32, 1 << 30, True)
_BF16_TRAIN = _BF16._replace(e_max=32, k_max=MAX_K)
_WIDE = _Limits(torch.float32, 16, 1024, 16, 128, 128, 24, False)
_ANY = _Limits(None, 0, 1 << 30, 1, 1 << 30, 1 << 30, 1 << 30, False)


def _two_layer(block: nn.Module) -> Optional[tuple]:
    """(lin1, lin2) if ``block.network`` is exactly Linear, GELU(erf), Linear with biases.
    The answer is remembered on the block and re-validated by identity (six dictionary look-ups): the eligibility checks ask
    it up to four times per block and step, and indexing an nn.Sequential costs microseconds — 0.17 ms of the 1.5 ms the host
    needs to issue a CIFAR-10 training step (profiles/lra_host_profile.py)."""
    seen = block.__dict__.get("_psf_two_layer")
    if seen is not None:
        net, l1, act, l2 = seen
        mods = net._modules
        if (block._modules.get("network") is net and len(mods) == 3 and mods.get("0") is l1 and mods.get("1") is act
                and mods.get("2") is l2 and act.approximate == "none" and l1._parameters.get("bias") is not None
                and l2._parameters.get("bias") is not None):
            return l1, l2
        del block.__dict__["_psf_two_layer"]
    net = getattr(block, "network", None)
    if not isinstance(net, nn.Sequential) or len(net) != 3:
        return None
    l1, act, l2 = net[0], net[1], net[2]
    if not (isinstance(l1, nn.Linear) and isinstance(l2, nn.Linear) and isinstance(act, nn.GELU)):
        return None
    if getattr(act, "approximate", "none") != "none" or l1.bias is None or l2.bias is None:
        return None
    if type(net) is nn.Sequential and all(k in net._modules for k in ("0", "1", "2")):  # (plain containers with the default keys)
        block.__dict__["_psf_two_layer"] = (net, l1, act, l2)
    return l1, l2


def _needs_grad(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for b in blocks for p in b.parameters()))


def _walk(x: torch.Tensor, blocks: Sequence[nn.Module], lim: _Limits) -> Optional[list]:
    """The one block walk of every predicate: [(lin1, lin2), ...] when ``x`` is a HIP tensor [..., E], every block a two-layer
    erf-GELU MLP on input width E and the call is not empty and inside ``lim``; None otherwise."""
    dtype, e_min, e_max, e_mult, h_max, o_max, k_max, all_params = lim
    if not x.is_cuda or x.dim() < 2 or x.dtype != (dtype or x.dtype) or not 1 <= len(blocks) <= k_max:
        return None
    E = x.shape[-1]
    if E < e_min or E > e_max or E % e_mult:
        return None
    pairs = []
    for b in blocks:
        l1, l2 = _two_layer(b) or (None, None)
        if l1 is None or l1.in_features != E or l1.out_features > h_max or l2.out_features > o_max or l1.weight.dtype != x.dtype:
            return None
        if all_params and any(p.dtype != dtype for p in (l1.bias, l2.weight, l2.bias)):
            return None
        pairs.append((l1, l2))
    return pairs


def eligible(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """Inference: the fused forward can replace ``[b(x) for b in blocks]`` and nothing needs a gradient."""
    return enabled and not _needs_grad(x, blocks) and _walk(x, blocks, _NARROW) is not None


def trainable(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """Training: fused forward + fused backward (``fused_mlp_apply``) can replace the PyTorch layers."""
    return enabled and train_enabled and _needs_grad(x, blocks) and _walk(x, blocks, _NARROW_TRAIN) is not None


def bf16_eligible(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """Inference in bf16: ``fused_mlp_forward_bf16`` can replace ``[b(x) for b in blocks]`` — a HIP bf16 input, two-layer
    erf-GELU blocks whose four parameters all are bf16, sizes within psf_mlp_fwd_bf16's limits, nothing needing a gradient."""
    return enabled and bf16_enabled and not _needs_grad(x, blocks) and _walk(x, blocks, _BF16) is not None


def bf16_trainable(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """Training in bf16, opt-in: ``fused_mlp_apply_bf16`` (psf_mlp_fwd_bf16 + psf_mlp_bwd_bf16) can replace the stacked route."""
    return (bf16_train_route == "always" and enabled and bf16_enabled and train_enabled and _needs_grad(x, blocks)
            and _walk(x, blocks, _BF16_TRAIN) is not None)


def wide_ok(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """The wide kernels (psf_mlp_wide_*) can replace ``[b(x) for b in blocks]``, with or without autograd."""
    pairs = _walk(x, blocks, _WIDE) if enabled and wide_enabled else None
    if pairs is None:
        return False
    E = x.shape[-1]
    J = sum((l1.out_features + 31) // 32 * 32 for l1, _ in pairs)
    return x.numel() // E * max(E, J) < 2 ** 30  # 32-bit lane offsets into a bf16 plane


def stackable(x: torch.Tensor, blocks: Sequence[nn.Module]) -> bool:
    """GPU call of >= 2 two-layer MLPs that share their input and that the fused kernels do not take, of any width."""
    return enabled and len(blocks) >= 2 and _walk(x, blocks, _ANY) is not None


def route(x: torch.Tensor, blocks: Sequence[nn.Module]) -> Optional[str]:
    """The name of the first of ``ROUTES`` that takes ``[b(x) for b in blocks]``, or None."""
    here = globals()
    return next((name for name, (predicate, _fn) in ROUTES.items() if here[predicate](x, blocks)), None)


def apply(x: torch.Tensor, blocks: Sequence[nn.Module]) -> Optional[List[torch.Tensor]]:
    """``[b(x) for b in blocks]`` by that route; None when no route takes the call (the caller then runs the modules)."""
    name = route(x, blocks)
    return None if name is None else globals()[ROUTES[name][1]](x, blocks)


def _ptrs(tensors: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sizes(params: Sequence[torch.Tensor]):
    """(K, h table, O table) of params = (A0, a0, B0, b0, A1, ...)."""
    K = len(params) // 4
    return K, (ctypes.c_int32 * K)(*[A.shape[0] for A in params[0::4]]), (ctypes.c_int32 * K)(*[B.shape[0] for B in params[2::4]])


def _scratch(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)  # the caching allocator aligns to 512 bytes


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself, or a copy when its first byte is not on a 16-byte boundary (a contiguous view into a larger buffer — the
    gradients of the W_m are such views of one [M, B, N, L] tensor — keeps its storage offset through ``contiguous()``)."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _bytes(kernel: str, entry: str, *args) -> int:
    """What the library's ``entry(*args)`` asks for ``kernel``; sizes outside the kernel's limits raise."""
    nbytes = getattr(_lib.load(), entry)(*args)
    if nbytes < 0:
        raise ValueError(f"{kernel} does not support these layer sizes")
    return nbytes


def _forward_raw(x2: torch.Tensor, params: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """x2 [T, E] contiguous, f32 or bf16; params = (A0, a0, B0, b0, A1, ...) contiguous of x2's dtype. One launch per <= MAX_K
    MLPs: psf_mlp_fwd_f32 or psf_mlp_fwd_bf16, which take the same arguments."""
    T, E = x2.shape
    dev = x2.device
    kernel, entry = ("psf_mlp_fwd_bf16",) * 2 if x2.dtype == torch.bfloat16 else ("psf_mlp_fwd", "psf_mlp_fwd_f32")
    launch = getattr(_lib.load(), entry)
    outs: List[torch.Tensor] = []
    for start in range(0, len(params), 4 * MAX_K):
        grp = params[start:start + 4 * MAX_K]
        K, h, O = _sizes(grp)
        ys = [torch.empty((T, B.shape[0]), dtype=x2.dtype, device=dev) for B in grp[2::4]]
        ws = _scratch(_bytes(kernel, kernel + "_workspace", E, K, h, O), dev)  # packed weight images
        with torch.cuda.device(dev):
            rc = launch(x2.data_ptr(), T, E, K, _ptrs(grp[0::4]), _ptrs(grp[1::4]), _ptrs(grp[2::4]), _ptrs(grp[3::4]), h, O,
                        _ptrs(ys), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, entry)
        outs.extend(ys)
    return outs


def _backward_raw(x2: torch.Tensor, params: Sequence[torch.Tensor], gys: Sequence[torch.Tensor], need_dx: bool):
    T, E = x2.shape
    dev = x2.device
    K, h, O = _sizes(params)
    grads = [torch.empty_like(p) for p in params]
    dX = torch.empty_like(x2) if need_dx else None
    kernel, entry = ("psf_mlp_bwd_bf16",) * 2 if x2.dtype == torch.bfloat16 else ("psf_mlp_bwd", "psf_mlp_bwd_f32")
    ws = _scratch(_bytes(kernel, kernel + "_workspace", T, E, K, h, O), dev)  # packed weights + per-workgroup partial sums
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), entry)(x2.data_ptr(), T, E, K, _ptrs(params[0::4]), _ptrs(params[1::4]), _ptrs(params[2::4]),
                                         h, O, _ptrs(gys), dX.data_ptr() if need_dx else None, _ptrs(grads[0::4]),
                                         _ptrs(grads[1::4]), _ptrs(grads[2::4]), _ptrs(grads[3::4]), ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr(dev))  # psf_mlp_bwd_f32 and psf_mlp_bwd_bf16 take the same arguments
    _lib.check(rc, entry)
    return dX, grads


class _FusedMLPFn(torch.autograd.Function):
    """(Y_0, ..., Y_{K-1}) = MLPs(x2); saves x2 and the parameters only."""

    @staticmethod
    def forward(ctx, x2, *params):
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)  # (no graph is recorded in here: no detach)
        if x2.dtype == torch.bfloat16:  # psf_mlp_fwd_bf16 / psf_mlp_bwd_bf16 read X as 16-byte vectors
            x2 = _aligned16(x2)
        ctx.save_for_backward(x2, *params)
        return tuple(_forward_raw(x2, params))

    @staticmethod
    def backward(ctx, *gys):
        x2, *params = ctx.saved_tensors
        Bs = params[2::4]
        gys = [torch.zeros((x2.shape[0], B.shape[0]), dtype=x2.dtype, device=x2.device) if g is None else g.contiguous()
               for g, B in zip(gys, Bs)]
        if x2.dtype == torch.bfloat16:  # psf_mlp_bwd_bf16 reads a tile of dY[k] as 16-byte vectors from dY[k]'s first byte
            gys = [_aligned16(g) for g in gys]
        need_dx = ctx.needs_input_grad[0]
        # The backward kernel sizes its dY prefetch and its weight buffering for the WIDEST output of a call: one MLP
        # with more than 16 outputs (g of the LRA networks: 32 channels) would put all ~50 units of the 12 link MLPs
        # on the slower configuration. Wide and narrow MLPs therefore go in two launches and their dX are added.
        # psf_mlp_bwd_bf16 does not size itself by the widest output (its dY planes always hold 32 columns), and its contract
        # rounds dX ONCE over all MLPs: a bf16 call is never split.
        narrow = [k for k, B in enumerate(Bs) if B.shape[0] <= 16]
        wide = [k for k, B in enumerate(Bs) if B.shape[0] > 16]
        if not narrow or not wide or x2.dtype == torch.bfloat16:
            dX, grads = _backward_raw(x2, params, gys, need_dx)
            return (dX, *grads)
        grads: List[Optional[torch.Tensor]] = [None] * len(params)
        dX = None
        for group in (narrow, wide):
            sub_params = [params[4 * k + i] for k in group for i in range(4)]
            d, g_sub = _backward_raw(x2, sub_params, [gys[k] for k in group], need_dx)
            for n, k in enumerate(group):
                grads[4 * k:4 * k + 4] = g_sub[4 * n:4 * n + 4]
            if need_dx:
                dX = d if dX is None else dX.add_(d)
        return (dX, *grads)


def _params_of(blocks: Sequence[nn.Module]) -> List[torch.Tensor]:
    out: List[torch.Tensor] = []
    for b in blocks:
        l1, l2 = _two_layer(b)
        out += [l1.weight, l1.bias, l2.weight, l2.bias]
    return out


def fused_mlp_forward(x: torch.Tensor, blocks: Sequence[nn.Module]) -> List[torch.Tensor]:
    """[block(x) for block in blocks] without autograd, by the fused kernel (f32 or bf16, by x's dtype). Caller checks ``eligible`` first."""
    lead, E = x.shape[:-1], x.shape[-1]
    x2 = x.detach().reshape(-1, E).contiguous()
    params = [p.detach().contiguous() for p in _params_of(blocks)]
    return [y.reshape(*lead, y.shape[1]) for y in _forward_raw(x2, params)]


def fused_mlp_apply(x: torch.Tensor, blocks: Sequence[nn.Module]) -> List[torch.Tensor]:
    """[block(x) for block in blocks] under autograd (fused forward and backward). Caller checks ``trainable``."""
    lead, E = x.shape[:-1], x.shape[-1]
    x2 = x.reshape(-1, E).contiguous()
    ys = _FusedMLPFn.apply(x2, *_params_of(blocks))
    return [y.reshape(*lead, y.shape[1]) for y in ys]


fused_mlp_apply_bf16 = fused_mlp_apply      # of a bf16 model: psf_mlp_fwd_bf16 / psf_mlp_bwd_bf16. Caller checks ``bf16_trainable``.
fused_mlp_forward_bf16 = fused_mlp_forward  # of a bf16 model: the fused bf16 kernel. Caller checks ``bf16_eligible`` first.


def _wide_forward_raw(x2: torch.Tensor, params: Sequence[torch.Tensor], keep: bool = True):
    """(Y_0..Y_{K-1}, saved): ``saved`` holds X as bf16 term planes and the hidden pre-activations (mlp_wide.hip).
    ``keep`` False (inference): no record is kept — the library works in scratch and skips what only a backward reads."""
    T, E = x2.shape
    dev = x2.device
    K, h, O = _sizes(params)
    n_saved = _bytes("psf_mlp_wide_fwd", "psf_mlp_wide_saved_bytes", T, E, K, h, O)
    saved = _scratch(n_saved, dev) if keep else None
    ws = _scratch(_bytes("psf_mlp_wide_fwd", "psf_mlp_wide_fwd_workspace", T, E, K, h, O) + (0 if keep else n_saved + 256), dev)
    ys = [torch.empty((T, B.shape[0]), dtype=torch.float32, device=dev) for B in params[2::4]]
    with torch.cuda.device(dev):
        rc = _lib.load().psf_mlp_wide_fwd_f32(x2.data_ptr(), T, E, K, _ptrs(params[0::4]), _ptrs(params[1::4]), _ptrs(params[2::4]),
                                              _ptrs(params[3::4]), h, O, _ptrs(ys), saved.data_ptr() if keep else None,
                                              saved.numel() if keep else 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "psf_mlp_wide_fwd_f32")
    return ys, saved


def _wide_backward_raw(saved: torch.Tensor, T: int, E: int, params: Sequence[torch.Tensor], gys: Sequence[torch.Tensor], need_dx: bool):
    dev = saved.device
    K, h, O = _sizes(params)
    grads = [torch.empty_like(p) for p in params]
    dX = torch.empty((T, E), dtype=torch.float32, device=dev) if need_dx else None
    ws = _scratch(_bytes("psf_mlp_wide_bwd", "psf_mlp_wide_bwd_workspace", T, E, K, h, O), dev)
    with torch.cuda.device(dev):
        rc = _lib.load().psf_mlp_wide_bwd_f32(saved.data_ptr(), saved.numel(), T, E, K, _ptrs(params[0::4]), _ptrs(params[2::4]), h, O,
                                              _ptrs(gys), dX.data_ptr() if need_dx else None, _ptrs(grads[0::4]), _ptrs(grads[1::4]),
                                              _ptrs(grads[2::4]), _ptrs(grads[3::4]), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(dev))
    _lib.check(rc, "psf_mlp_wide_bwd_f32")
    return dX, grads


class _WideMLPFn(torch.autograd.Function):
    """(Y_0, ..., Y_{K-1}) = MLPs(x2) on the wide kernels; saves the kernels' own record of X and the hidden layer."""

    @staticmethod
    def forward(ctx, x2, *params):
        params = tuple(p if p.is_contiguous() else p.contiguous() for p in params)  # (inside Function.forward: nothing to detach from)
        ys, saved = _wide_forward_raw(x2, params)
        ctx.save_for_backward(saved, *params)
        ctx.x_shape = tuple(x2.shape)
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        saved, *params = ctx.saved_tensors
        T, E = ctx.x_shape
        gys = [torch.zeros((T, B.shape[0]), dtype=torch.float32, device=saved.device) if g is None else g.contiguous()
               for g, B in zip(gys, params[2::4])]
        dX, grads = _wide_backward_raw(saved, T, E, params, gys, ctx.needs_input_grad[0])
        return (dX, *grads)


def wide_apply(x: torch.Tensor, blocks: Sequence[nn.Module]) -> List[torch.Tensor]:
    """[block(x) for block in blocks] on the wide kernels (autograd-aware). Caller checks ``wide_ok`` first."""
    lead, E = x.shape[:-1], x.shape[-1]
    if _needs_grad(x, blocks):
        ys = _WideMLPFn.apply(x.reshape(-1, E).contiguous(), *_params_of(blocks))
    else:
        ys, _ = _wide_forward_raw(x.detach().reshape(-1, E).contiguous(), [p.detach().contiguous() for p in _params_of(blocks)], keep=False)
    return [y.reshape(*lead, y.shape[1]) for y in ys]


def stacked_apply(x: torch.Tensor, blocks: Sequence[nn.Module]) -> List[torch.Tensor]:
    """[block(x) for block in blocks] with the first layers stacked into one Linear (autograd-transparent: the
    parameters stay the modules' own tensors; ``torch.cat`` routes their gradients back)."""
    pairs = [_two_layer(b) for b in blocks]
    lead, E = x.shape[:-1], x.shape[-1]
    x2 = x.reshape(-1, E)
    hidden = F.gelu(F.linear(x2, torch.cat([l1.weight for l1, _ in pairs], 0), torch.cat([l1.bias for l1, _ in pairs], 0)))
    parts = hidden.split([l1.out_features for l1, _ in pairs], dim=-1)  # column slices: GEMM operands with lda = sum h
    from .token_linear import _TokenLinearFn, wgrad_supported  # (token_linear imports nothing from here)
    outs = []
    for p, (_, l2) in zip(parts, pairs):
        # second-layer weight gradients are [out x T] * [T x h] reductions into a tiny tile: on the tall-skinny MFMA
        # kernel (reads the slice with its row stride) where it applies — 135 us each through hipBLASLt at ListOps sizes
        if torch.is_grad_enabled() and l2.weight.requires_grad and wgrad_supported(p, l2.out_features):
            y = _TokenLinearFn.apply(p, l2.weight, l2.bias)
        else:
            y = F.linear(p, l2.weight, l2.bias)
        outs.append(y.reshape(*lead, l2.out_features))
    return outs
