"""Selected rows and columns of the attention map ``A_b = W_{M-1} ... W_0`` without the dense [B, N, N] map.

The reference's two visualisation scripts build the whole map (``ChangedPSF.forward``: the chain on ``eye(N)``, C = N) and
then read a sliver of it: LRA/attention_maps/psf_utils_attn_IMDb.py:67 takes ``W_final[0, 0, :]`` — one row, the CLS
token's — and pathfinder_inference.py:319-321 takes ``att_map[i].T[indices_full]`` — 18 columns per image. A selected row or
column costs O(M N L) instead of O(M N^2 L):

* a COLUMN of ``A`` is the forward chain applied to a one-hot vector: ``attention_cols`` is ``chord_chain`` on a batched
  one-hot ``V0``. The forward kernels treat channels independently, so these are the dense map's columns bit for bit.
* a ROW of ``A`` is the transposed chain applied to a one-hot vector: ``attention_rows`` runs ``chain_transposed``
  (psf_chord_chain_tr_f32 / _bf16: one launch with Y and W_m resident in LDS for N <= 1024, csrc/chain_tr_lds.h; the per-step
  dV launches issued by the library beyond). Each step is the dV half of the backward step, so a row carries the bits of M
  calls of psf_chord_spmm_bwd_* with dW = NULL — the same values as the dense map's row, summed in another order.

Inference only: everything here runs under ``no_grad`` and returns detached tensors. HIP devices only, like chord.py.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib
from .chord import _norm_offsets, _require_hip, _stream_ptr, _suffix, chord_chain


def _check_links(W_list: Sequence[torch.Tensor]):
    if not len(W_list):
        raise ValueError("W_list is empty")
    W0 = W_list[0]
    if W0.dim() != 3:
        raise ValueError(f"every W_m must be [B, N, L], got {tuple(W0.shape)}")
    for w in W_list:
        if w.shape != W0.shape:
            raise ValueError(f"every W_m must be [B, N, L] = {tuple(W0.shape)}, got {tuple(w.shape)}")
        if w.dtype != W0.dtype:
            raise TypeError(f"every W_m must share a dtype (got {W0.dtype} and {w.dtype})")
    if W0.shape[2] > _lib.MAX_LINKS:
        raise ValueError(f"L={W0.shape[2]} exceeds {_lib.MAX_LINKS}")
    return W0.shape


def chain_transposed(W_list: Sequence[torch.Tensor], Y: torch.Tensor, offsets: Optional[Sequence[int]] = None) -> torch.Tensor:
    """``Y_M = Y;  Y_m = W_m^T (.) Y_{m+1}  for m = M-1 .. 0``; returns ``Y_0`` [B, N, R].

    ``Y_m[b,q,c] = sum_k W_m[b,(q-off_k) mod N,k] * Y_{m+1}[b,(q-off_k) mod N,c]``. W_m [B,N,L], Y [B,N,R] with any R >= 1
    (zero columns are appended up to the library's 16-byte column groups and cut off again). float32 and bfloat16 run
    psf_chord_chain_tr_*; float64 runs M dV steps of psf_chord_spmm_bwd_f64. No autograd: the result is detached."""
    B, N, L = _check_links(W_list)
    if Y.dtype != W_list[0].dtype:
        raise TypeError(f"W ({W_list[0].dtype}) and Y ({Y.dtype}) must share a dtype")
    suffix = _suffix(Y)
    if Y.dim() != 3 or Y.shape[0] != B or Y.shape[1] != N or Y.shape[2] < 1:
        raise ValueError(f"Y must be [{B}, {N}, R] with R >= 1, got {tuple(Y.shape)}")
    dev = _require_hip(Y, *W_list)
    offsets = _norm_offsets(offsets)
    M, R = len(W_list), Y.shape[2]
    with torch.no_grad():
        Ws = [w.detach() if w.is_contiguous() else w.detach().contiguous() for w in W_list]
        vec = 16 // Y.element_size()
        Rp = (R + vec - 1) // vec * vec
        if Rp != R:
            Q = torch.zeros((B, N, Rp), dtype=Y.dtype, device=dev)
            Q[..., :R] = Y
        else:
            Q = Y.detach().contiguous()
            if Q.data_ptr() % 16:  # (a contiguous view at an odd storage offset)
                Q = Q.clone()
        out = torch.empty_like(Q)
        lib = _lib.load()
        off = _lib.offsets_array(offsets)
        if suffix == "_f64":
            fn = lib.psf_chord_spmm_bwd_f64
            bufs = [out, torch.empty_like(Q)]
            y = Q
            with torch.cuda.device(dev):
                for m in range(M - 1, -1, -1):
                    dst = bufs[m & 1]  # step 0 writes ``out``
                    rc = fn(y.data_ptr(), Ws[m].data_ptr(), None, None, dst.data_ptr(), B, N, L, Rp, N * Rp, off, _stream_ptr(dev))
                    _lib.check(rc, "psf_chord_spmm_bwd_f64")
                    y = dst
        else:
            one_launch = bool(lib.psf_chord_chain_tr_supported(N, L, Rp, M, Y.element_size()))
            scratch = None if one_launch or M == 1 else torch.empty_like(Q)
            w_tab = (ctypes.c_void_p * M)(*[w.data_ptr() for w in Ws])
            with torch.cuda.device(dev):
                rc = getattr(lib, "psf_chord_chain_tr" + suffix)(w_tab, Q.data_ptr(), out.data_ptr(),
                                                               None if scratch is None else scratch.data_ptr(), M, B, N, L, Rp,
                                                               off, _stream_ptr(dev))
            _lib.check(rc, "psf_chord_chain_tr" + suffix)
        return out[..., :R] if Rp != R else out


def _one_hot(index, B: int, N: int, dtype: torch.dtype, dev: torch.device, what: str):
    """([B, N, Rp] with a 1 at [b, index[b, j], j], R): ``index`` an int sequence or tensor, [R] (every sample) or [B, R]; Rp is
    R rounded up to whole 16-byte column groups (zero columns), which keeps every step on the vector kernels."""
    idx = index.detach().cpu() if isinstance(index, torch.Tensor) else torch.as_tensor(index if hasattr(index, "__array__") else list(index))
    if idx.numel() == 0 or idx.dim() not in (1, 2) or idx.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"{what} must be a non-empty integer sequence [R] or [B, R], got {tuple(idx.shape)} {idx.dtype}")
    idx = idx.to(torch.int64)
    if idx.dim() == 1:
        idx = idx.unsqueeze(0).expand(B, -1).contiguous()
    if idx.shape[0] != B:
        raise ValueError(f"{what} must be [R] or [{B}, R], got {tuple(idx.shape)}")
    if int(idx.min()) < 0 or int(idx.max()) >= N:
        raise ValueError(f"{what} must lie in [0, {N}), got {int(idx.min())} .. {int(idx.max())}")
    R = idx.shape[1]
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    hot = torch.zeros((B, N, (R + vec - 1) // vec * vec), dtype=dtype, device=dev)
    hot[..., :R].scatter_(1, idx.to(dev).unsqueeze(1), 1)
    return hot, R


def attention_rows(W_list: Sequence[torch.Tensor], rows) -> torch.Tensor:
    """``result[b,i,:] = A_b[rows[b,i],:]`` for ``A_b = W_{M-1} ... W_0`` — [B, R, N]. ``rows``: [R] or [B, R] indices in [0, N)."""
    B, N, _ = _check_links(W_list)
    dev = _require_hip(*W_list)
    _suffix(W_list[0])
    Q, R = _one_hot(rows, B, N, W_list[0].dtype, dev, "rows")
    return chain_transposed(W_list, Q)[..., :R].transpose(1, 2)


def attention_cols(W_list: Sequence[torch.Tensor], cols) -> torch.Tensor:
    """``result[b,:,j] = A_b[:,cols[b,j]]`` — [B, N, R]: the forward chain on a one-hot V0, the dense map's columns bit for bit."""
    B, N, _ = _check_links(W_list)
    dev = _require_hip(*W_list)
    _suffix(W_list[0])
    with torch.no_grad():
        V0, R = _one_hot(cols, B, N, W_list[0].dtype, dev, "cols")
        return chord_chain([w.detach() for w in W_list], V0, False)[..., :R]
