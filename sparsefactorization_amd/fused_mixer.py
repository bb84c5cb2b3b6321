"""The mixer with W produced inside the chain step — ``psf_mixer_fwd_f32`` (csrc/fwd_mlp_step.h).

``V = g(data); for m: W = fs[m](data); V = spmm(idx, W, V) (+ V0)`` (SyntheticExperiments/psf.py:165-188) as M + 2
launches that never write a W_m: every step kernel computes its tile's rows of W_m on chip from the tile's rows of ``data``.
Inference only (nothing is kept for a backward); ``eligible`` says whether a call can take it, otherwise the caller
produces the W_m (fused_mlp.py) and runs the chain (chord.chord_chain).
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import torch
from torch import nn

from . import _lib
from .fused_mlp import _needs_grad, _ptrs, _two_layer

enabled = True  # module-level switch (tests / A-B timing)
#: "auto": take the fused path where it is measured faster than psf_mlp_fwd_f32 + psf_chord_chain_fwd_f32 end to end
#: (profiles/r04l_mixer_bench.log: long sequences of narrow rows with one hidden unit — the step kernel stages its MLP's
#: weight image per tile, 14 KB per 32 hidden rows, which short tiles (C = 32: 64 rows) and 128-wide hidden layers do not
#: amortise — and the short sequences that run as one LDS-resident launch); "always": wherever the shape is covered; "never".
route = "auto"
#: Hand the single-launch kernel (short sequences, csrc/mixer_lds.h) the RECIPE of ``data`` — the affine input layer or the
#: embedding lookup, include/psf_chord.h: psf_mixer_input — instead of its rows. Off: ``data`` is written once
#: (psf_affine_rows_f32 / psf_embed_tokens_f32) and passed as rows. The per-step kernels take rows only: evaluating a recipe
#: inside them measured slower than the one pass that writes the rows (712 against 609 + 28 us at Temporal Order's shape,
#: 0.97 against 0.82 ms per Adding forward; profiles/r04h_mixer_bench.log, r04w_bench_stdout.log) and round 5 removed those
#: instances (two thirds of that translation unit).
recipe_in_kernel = False
#: A bf16 model's short sequences: the whole mixer in ONE launch (psf_mixer_fwd_bf16, csrc/mixer_lds_bf16.h) instead of
#: psf_mlp_fwd_bf16 + psf_chord_chain_fwd_bf16 — the same bits. "never": the two calls, as before; "always": wherever
#: ``covered_bf16`` holds and nothing needs a gradient. The default stays "never" until the numbers of
#: profiles/bf16_mixer_ab.md are acted on.
bf16_route = "never"


class Recipe:
    """How ``data`` [B, N, E] comes about (include/psf_chord.h: psf_mixer_input): given (``data``), an affine map of a few
    inputs per position (``affine``: init_linear of the Adding network, psf.py:153-154) or an embedding lookup (``tokens``:
    psf.py:151-152), each optionally plus a positional row. The single-launch kernel evaluates the last two itself (``data``
    is then never written); for the per-step kernels ``rows()`` writes it once."""

    def __init__(self, kind, src, weight=None, bias=None, pos=None, K=0, E=None):
        self.kind, self.src, self.weight, self.bias, self.pos, self.K = kind, src, weight, bias, pos, K
        self.E = E if E is not None else (src.shape[-1] if kind == _lib.MIXER_IN_DATA else weight.shape[0 if kind == _lib.MIXER_IN_AFFINE else 1])

    @staticmethod
    def data(x):
        return Recipe(_lib.MIXER_IN_DATA, x)

    @staticmethod
    def affine(inp, linear: nn.Linear, pos=None):
        return Recipe(_lib.MIXER_IN_AFFINE, inp, linear.weight, linear.bias, pos, K=inp.shape[-1])

    @staticmethod
    def tokens(idx, table: torch.Tensor, pos=None):
        return Recipe(_lib.MIXER_IN_TOKENS, idx, table, None, pos, K=table.shape[0])

    @property
    def B(self):
        return self.src.shape[0]

    @property
    def N(self):
        return self.src.shape[1]

    def tensors(self):
        return [t for t in (self.src, self.weight, self.bias, self.pos) if t is not None]

    def rows(self) -> torch.Tensor:
        """``data`` [B, N, E] written once: psf_affine_rows_f32 / psf_embed_tokens_f32 (+ the positional rows)."""
        from .token_linear import _EmbedTokensFn, affine_rows
        if self.kind == _lib.MIXER_IN_DATA:
            return self.src
        with torch.no_grad():
            if self.kind == _lib.MIXER_IN_AFFINE:
                x = affine_rows(self.src, self.weight, self.bias)
                return x if self.pos is None else x + self.pos.unsqueeze(0)
            return _EmbedTokensFn.apply(self.src, self.weight, self.pos, None)

    def ok(self):
        """Shapes and dtypes the library takes; anything else makes the caller materialise ``data`` instead."""
        s = self.src
        if not s.is_cuda:
            return False
        if self.kind == _lib.MIXER_IN_DATA:
            return s.dim() == 3 and s.dtype == torch.float32
        if self.pos is not None and (self.pos.dtype != torch.float32 or tuple(self.pos.shape) != (self.N, self.E)):
            return False
        if self.kind == _lib.MIXER_IN_AFFINE:
            return (s.dim() == 3 and s.dtype == torch.float32 and 1 <= s.shape[-1] <= 3 and self.weight.dtype == torch.float32
                    and tuple(self.weight.shape) == (self.E, s.shape[-1]))
        return s.dim() == 2 and s.dtype == torch.int64 and self.weight.dtype == torch.float32 and self.weight.dim() == 2


def _block_pairs(E: int, g: nn.Module, fs: Sequence[nn.Module], dtype: torch.dtype = torch.float32):
    """((M, h table, C, L), [(lin1, lin2), ...]) when every block is Linear, GELU(erf), Linear of input width E in ``dtype`` and
    the link MLPs agree on L; None otherwise. (f32: the first layer's weight decides, as ever; bf16: all four parameters.)"""
    if not len(fs):
        return None
    pairs = [_two_layer(b) for b in [g, *fs]]
    if any(p is None for p in pairs):
        return None
    if any(l1.in_features != E or l1.weight.dtype != dtype for l1, _ in pairs):
        return None
    if dtype != torch.float32 and any(p.dtype != dtype for l1, l2 in pairs for p in (l1.bias, l2.weight, l2.bias)):
        return None
    L = pairs[1][1].out_features
    if any(l2.out_features != L for _, l2 in pairs[1:]):
        return None
    h = (ctypes.c_int32 * len(pairs))(*[l1.out_features for l1, _ in pairs])
    return (len(fs), h, pairs[0][1].out_features, L), pairs


def _block_sizes(E: int, g: nn.Module, fs: Sequence[nn.Module]):
    """(M, h table, C, L), or None (see _block_pairs)."""
    found = _block_pairs(E, g, fs)
    return None if found is None else found[0]


def _route_ok(N: int, E: int, M: int, C: int, L: int, h, tokens: int = 1 << 62, plan=None) -> bool:
    if route != "auto":
        return route == "always"
    if N >= 8192 and C <= 32 and max(h) <= 32:  # (32-channel rows since the step kernel's diet: genome shape 488 -> 451 us)
        return True
    # short sequences: ONE launch with V resident in LDS (csrc/mixer_lds.h) against producer + chain
    # (profiles/r04n_mixer_bench_short.log: cfg1 115 -> 89 us per forward, N = 512: 134 -> 106)
    if plan is None:  # (``_found`` passes the answer it already has)
        plan = _lib.load().psf_mixer_fwd_plan(N, E, M, h, C, L)
    if plan == 2:
        return True
    # An EAGER forward of a small network is bound by the host, and the fused route is one library call for all its M + 2
    # launches: in the no-grad forward of the LRA networks (profiles/infer_route_sweep.py, ms per forward, fused / through
    # memory) CIFAR-10's widths (hidden 16) win at every batch size — 0.227 / 0.270 at 32 k tokens, 0.319 / 0.339 at 524 k —
    # and hidden 128 wins while the GPU time of the heavier step kernels stays under the host's: Pathfinder 0.173 / 0.222 at
    # 16 k tokens, IMDb 0.247 / 0.291 at 32 k, but 0.377 / 0.280 at 65 k. Under stream capture there is no host in the replay
    # and the GPU-time rule above stands.
    if plan == 1 and not torch.cuda.is_current_stream_capturing():
        return (max(h) <= 32 and C <= 32) or tokens <= 40000
    return False


class _Found(tuple):
    """``found``: ((M, h table, C, L), [(lin1, lin2), ...]), as ever, carrying the library's two answers for the shape: ``plan``
    (psf_mixer_fwd_plan / psf_mixer_fwd_bf16_plan) and ``ws_bytes``. The forward that is handed one asks neither again."""


def _found(N: int, E: int, g: nn.Module, fs: Sequence[nn.Module], dtype: torch.dtype, tokens=None):
    """``found`` of either dtype from ONE walk of the blocks, one plan and one workspace query; None when blocks or shape are not covered
    (f32: psf_mixer_fwd_workspace < 0; bf16: psf_mixer_fwd_bf16_plan != 2) or, f32 with ``tokens`` (B N) given, ``_route_ok`` says no."""
    bp = _block_pairs(E, g, fs, dtype)
    if bp is None:
        return None
    M, h, C, L = bp[0]
    lib, bf = _lib.load(), dtype == torch.bfloat16
    plan = (lib.psf_mixer_fwd_bf16_plan if bf else lib.psf_mixer_fwd_plan)(N, E, M, h, C, L)
    if (plan != 2) if bf else (tokens is not None and not _route_ok(N, E, M, C, L, h, tokens, plan)):
        return None
    ws_bytes = (lib.psf_mixer_fwd_bf16_workspace if bf else lib.psf_mixer_fwd_workspace)(N, E, M, h, C, L)
    if ws_bytes < 0:
        return None
    found = _Found(bp)
    found.plan, found.ws_bytes = plan, ws_bytes
    return found


def _covered(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module], dtype: torch.dtype):
    """``found`` for ``data`` [B, N, E] of ``dtype`` on the GPU inside the dtype's limits, whatever the route switches say; or None."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or not x.is_cuda or x.dtype != dtype:
        return None
    return _found(x.shape[1], x.shape[-1], g, fs, dtype)


def find(r: Recipe, g: nn.Module, fs: Sequence[nn.Module]):
    """((M, h table, C, L), [(lin1, lin2), ...]) when the fused mixer can run from this recipe, nothing needs a gradient and
    ``route`` wants it; None otherwise. ``mixer_forward_in`` takes it as ``found`` and neither walks the blocks nor asks the library again."""
    if not enabled or route == "never" or not r.ok() or torch.is_grad_enabled() and (
            any(t.requires_grad for t in r.tensors() if t.is_floating_point()) or any(p.requires_grad for b in (g, *fs) for p in b.parameters())):
        return None
    return _found(r.N, r.E, g, fs, torch.float32, r.B * r.N)


def find_bf16(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module]):
    """``found`` for ``mixer_forward_bf16`` when ``bf16_route`` wants the single launch, it covers the call and nothing needs a
    gradient; None otherwise."""
    if not enabled or bf16_route != "always" or _needs_grad(x, [g, *fs]):
        return None
    return _covered(x, g, fs, torch.bfloat16)


def eligible_recipe(r: Recipe, g: nn.Module, fs: Sequence[nn.Module]) -> bool:
    """The fused mixer can run from this recipe, nothing needs a gradient, and ``route`` wants it."""
    return find(r, g, fs) is not None


def eligible(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module]) -> bool:
    return eligible_recipe(Recipe.data(x), g, fs) and not x.requires_grad


def covered(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module]) -> bool:
    """The shape is inside the fused path's limits (whatever ``route`` says about using it)."""
    return _covered(x, g, fs, torch.float32) is not None


def covered_bf16(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module]) -> bool:
    """bf16 ``data`` [B, N, E] on the GPU, every block Linear -> GELU(erf) -> Linear in bf16, the link MLPs agreeing on L, and a
    shape the single launch takes (psf_mixer_fwd_bf16_plan == 2) — whatever ``bf16_route`` says about using it."""
    return _covered(x, g, fs, torch.bfloat16) is not None


def _launch(entry: str, first, shape, found, use_residual: bool, dtype: torch.dtype, dev, with_v0: bool) -> torch.Tensor:
    """What both forwards end in: the four parameter tables, the workspace, (f32: the buffer that receives g(data);) two ping-pong
    step buffers, the output table, the call of ``entry`` with ``first`` as its first argument, the check. Returns V_M."""
    ((M, h, C, L), pairs), (B, N, E) = found, shape
    params = [p if p.is_contiguous() else p.contiguous() for l1, l2 in pairs for p in (l1.weight, l1.bias, l2.weight, l2.bias)]
    ws = torch.empty(found.ws_bytes, dtype=torch.uint8, device=dev)
    V0 = torch.empty((B, N, C), dtype=dtype, device=dev)  # (bf16, whose entry takes none: a step buffer; empty_like is the cheaper call)
    bufs = [torch.empty_like(V0) for _ in range(min(M, 2))] if with_v0 else [V0, torch.empty_like(V0)][:M]
    o_tab = (ctypes.c_void_p * M)(*[bufs[m % len(bufs)].data_ptr() for m in range(M)])
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), entry)(first, B, N, E, M, _ptrs(params[0::4]), _ptrs(params[1::4]), _ptrs(params[2::4]),
                                         _ptrs(params[3::4]), h, C, L, 1 if use_residual else 0, V0.data_ptr() if with_v0 else None,
                                         o_tab, ws.data_ptr(), found.ws_bytes, _lib.stream_ptr(dev))
    _lib.check(rc, entry)
    return bufs[(M - 1) % len(bufs)]


def _aligned(t, align):  # ``t`` detached, contiguous and ``align``-byte aligned (a copy where it is not); None stays None
    if t is not None:
        t = t.detach().contiguous()
        return t if t.data_ptr() % align == 0 else t.clone()


def mixer_forward_in(r: Recipe, g: nn.Module, fs: Sequence[nn.Module], use_residual: bool, found=None) -> torch.Tensor:
    """V_M [B, N, C] from the recipe of ``data``. ``found``: what ``find`` returned for these arguments; without it the caller
    checks ``eligible_recipe`` (or ``covered``) first."""
    if found is None:
        found = _found(r.N, r.E, g, fs, torch.float32)
        if found is None:
            raise ValueError("psf_mixer_fwd does not cover this shape" if _block_pairs(r.E, g, fs) is not None else
                             "psf_mixer_fwd does not cover these blocks: every block must be Linear(E, h) -> GELU(erf) -> "
                             "Linear(h, out) in f32 on input width E, the link MLPs agreeing on L (check eligible() / covered())")
    shape, dev = (r.B, r.N, r.E), r.src.device
    if r.kind != _lib.MIXER_IN_DATA and not (recipe_in_kernel and found.plan == 2):
        r = Recipe.data(r.rows())  # the per-step kernels take rows (psf_mixer_fwd_plan: 2 = the single-launch kernel runs)
    keep = [_aligned(r.src, 16 if r.kind == _lib.MIXER_IN_DATA else 8), _aligned(r.weight, 16), _aligned(r.bias, 4), _aligned(r.pos, 16)]
    spec = _lib.MixerInput(r.kind, int(r.K), *[t.data_ptr() if t is not None else None for t in keep])
    return _launch("psf_mixer_fwd_in_f32", ctypes.byref(spec), shape, found, use_residual, torch.float32, dev, True)


def mixer_forward(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module], use_residual: bool) -> torch.Tensor:
    """V_M [B, N, C] from ``data`` [B, N, E]. Caller checks ``eligible`` (or ``covered``) first."""
    return mixer_forward_in(Recipe.data(x), g, fs, use_residual)


def mixer_forward_bf16(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module], use_residual: bool, found=None) -> torch.Tensor:
    """V_M [B, N, C] in bf16 from bf16 ``data`` [B, N, E] in ONE launch (psf_mixer_fwd_bf16): the bits of ``fused_mlp_forward_bf16``
    + ``chord_chain``. Caller checks ``covered_bf16`` (or passes what ``find_bf16`` returned)."""
    if found is None:
        found = _covered(x, g, fs, torch.bfloat16)
        if found is None:
            raise ValueError("psf_mixer_fwd_bf16 does not cover this call: bf16 data [B, N, E] on the GPU, every block "
                             "Linear(E, h) -> GELU(erf) -> Linear(h, out) in bf16, the link MLPs agreeing on L (check covered_bf16())")
    x = _aligned(x, 16)
    return _launch("psf_mixer_fwd_bf16", x.data_ptr(), tuple(x.shape), found, use_residual, torch.bfloat16, x.device, False)


def forward_from_data(x: torch.Tensor, g: nn.Module, fs: Sequence[nn.Module], use_residual: bool):
    """V_M from ``data`` [B, N, E] by the fused mixer of its dtype — bf16: the single launch where ``bf16_route`` wants it; otherwise
    the f32 mixer unless ``data`` itself requires a gradient — or None when that mixer does not take the call."""
    if x.dtype == torch.bfloat16:
        found = find_bf16(x, g, fs)
        return None if found is None else mixer_forward_bf16(x, g, fs, use_residual, found)
    r = Recipe.data(x)
    found = None if x.requires_grad else find(r, g, fs)
    return None if found is None else mixer_forward_in(r, g, fs, use_residual, found)
