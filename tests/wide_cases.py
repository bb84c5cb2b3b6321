"""Cases, a plain-Python mirror of the host plan, operands, references and canary helpers for the wide producer MLPs
(csrc/mlp_wide.hip, csrc/x3_gemm.h: psf_mlp_wide_fwd_f32 / psf_mlp_wide_bwd_f32), used by test_gpu_wide_mlp_edges.py and
checked without a GPU by test_wide_cases_cpu.py.

``plan`` restates make_wide_plan and the three size functions of mlp_wide.hip: what the caller-owned scratch areas hold and
how the weight-gradient GEMM is split over the tokens. It serves to SIZE the scratch areas exactly, to assert what a case
reaches and to pin the split-K property; it never computes an answer.

A case is (T, E, [(h, O), ...]). ``problem`` gives its operands and reference once, shared and read-only: seeded MLPBlocks
with normal X and dY against float64 copies of the same blocks (forward <= 1e-5, gradients <= 2e-5 of max|reference| per
tensor, the bounds of test_gpu_wide_mlp.py: dense operands, every split of every sum carries weight) or, with a ``kind``, a
known-answer construction of tests/x3_exact.py (the reference is then exact in f32 and the GPU test asserts equal bits).

The canary helpers place a tensor inside bands of one fixed NaN bit pattern and count what a call did to it: band words
that changed, output words that still hold the pattern. They are plain functions over tensors of any device.
"""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch

import x3_exact as xe

# ---------------------------------------------------------------- constants of the kernels
# csrc/mlp_wide.hip
MAX_MLPS = 24          # kMaxWideMlps
MAX_UNITS = 96         # kMaxWideUnits: 24 MLPs x 4 units of 32 hidden rows
PACK_BT_STEP = 1024    # kPackBtStep
SPLITS_MAX = 64        # kSplitsMax
SLOT_CLASS = 4 * 96    # kSlotClass: work-item slots per unit class of wide_mid_k
SLOT_BYTES = 3 * SLOT_CLASS * 4   # kSlotBytes
RED_SLICES = 8         # kRedSlices
MID_TILES = 8          # kMidTiles: 32-token tiles per work item of wide_mid_k
MIN_CHUNKS = 32        # make_wide_plan: at least 32 k-chunks (512 tokens) per split
WORKGROUPS = 256       # launch_gemm / make_wide_plan: one persistent workgroup per CU
E_MIN, E_MAX, H_MAX, O_MAX = 16, 1024, 128, 128   # make_wide_plan's shape check
PLANE_LIMIT = 1 << 31  # make_wide_plan: bytes of one bf16 term plane (32-bit lane offsets in the GEMM loader)
# csrc/x3_gemm.h
TILE = 256             # kTile
TILE_NARROW = 64       # kTileNarrow
OUT_TILES_MAX = 4      # kOutTilesMax
PACK2_TILE = 2048      # kPack2Tile
CHUNK = 16             # tokens (or columns) per k-chunk of x3_gemm_k

TOL_FWD, TOL_BWD = 1e-5, 2e-5   # test_gpu_wide_mlp.py


def up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def wide_class(O: int) -> int:
    return 0 if O <= 16 else 1 if O <= 32 else 2


def wide_nsub(ot: int) -> int:
    return 1 if ot <= 1 else 2 if ot == 2 else 4


def rec_size(ot: int, first: bool) -> int:
    return ot * 1024 + 32 + (ot * 32 if first else 0)


def split_rule(chunks: int, tiles: int, parent: bool = False) -> int:
    """Splits of the weight-gradient GEMM. ``parent``: the rule before the fix, which could leave the last splits empty."""
    s = WORKGROUPS // tiles
    s = min(s, chunks // MIN_CHUNKS, SPLITS_MAX)
    s = max(s, 1)
    if parent:
        return s
    per = -(-chunks // s)
    return -(-chunks // per)


def split_ranges(chunks: int, splits: int):
    """[k_begin, k_end) of every split as x3_gemm_k's ``decode`` cuts them (k_end < k_begin where the kernel's nk is negative)."""
    per = -(-chunks // splits)
    return [(sp * per, min((sp + 1) * per, chunks)) for sp in range(splits)]


def plan(T: int, E: int, layers, parent_splits: bool = False):
    """make_wide_plan + saved_bytes / fwd_ws_bytes / bwd_ws_bytes of mlp_wide.hip; None where the library answers -1."""
    K = len(layers)
    if T < 1 or E < E_MIN or E > E_MAX or E % 16 or K < 1 or K > MAX_MLPS:
        return None
    j = rec = 0
    n_slots = [0, 0, 0]
    for h, O in layers:
        if h < 1 or h > H_MAX or O < 1 or O > O_MAX:
            return None
        ot, nu = -(-O // 32), -(-h // 32)
        for u in range(nu):
            rec += wide_nsub(ot) * rec_size(ot, u == 0)
            n_slots[wide_class(O)] += wide_nsub(ot)
        j += 32 * nu
    T_pad, E_pad, J, J_pad = up(T, TILE), up(E, 256), j, up(j, 256)
    U = J_pad // 32
    xp_plane = E // 16 * T_pad * 32
    gp_plane = J // 16 * T_pad * 32
    if xp_plane >= PLANE_LIMIT or gp_plane >= PLANE_LIMIT:
        return None
    hf_bytes = T_pad // 32 * U * 4096
    w1p_plane = E // 16 * J_pad * 32
    w1tp_plane = J // 16 * E_pad * 32
    pack2_bytes = J // 32 * OUT_TILES_MAX * 3 * PACK2_TILE
    packbt_bytes = J // 32 * 8 * 3 * PACK_BT_STEP
    groups = T_pad // (32 * MID_TILES)
    narrow_e = E <= 128
    tiles_e = -(-E // TILE_NARROW) if narrow_e else E_pad // 256
    tiles = J_pad // 256 * tiles_e
    chunks = T_pad // CHUNK
    splits = split_rule(chunks, tiles, parent_splits)
    rest = 3 * w1tp_plane + packbt_bytes + SLOT_BYTES + 3 * gp_plane + up((groups + RED_SLICES) * rec * 4, 256)
    return dict(T=T, T_pad=T_pad, E=E, E_pad=E_pad, J=J, J_pad=J_pad, K=K, U=U, rec_total=rec, groups=groups, n_slots=n_slots,
                tiles_e=tiles_e, tiles=tiles, chunks=chunks, splits=splits,
                saved=3 * xp_plane + hf_bytes,
                fwd_ws=3 * w1p_plane + up(J_pad * 4, 256) + pack2_bytes + up(K * OUT_TILES_MAX * 32 * 4, 256),
                bwd_ws=rest + splits * J_pad * E_pad * 4, bwd_ws_less_splits=rest, split_slab=J_pad * E_pad * 4)


def tile_counts():
    """Every tile count of the weight-gradient GEMM the limits allow: (J_pad / 256 in 1..12) x (column tiles of E: 1, 2 on the
    256 x 64 configuration, 1..4 on the square one)."""
    return sorted({m * n for m in range(1, MAX_UNITS * 32 // 256 + 1) for n in range(1, E_MAX // 256 + 1)})


def shape_with_tiles(tiles: int):
    """(E, layers) of a shape whose weight-gradient GEMM has ``tiles`` tiles."""
    for n, E in ((1, 16), (2, 128), (3, 528), (4, 1024)):
        if tiles % n == 0 and tiles // n <= MAX_UNITS * 32 // 256:
            return E, [(128, 1)] * (2 * (tiles // n))
    raise ValueError(tiles)


# ---------------------------------------------------------------- the GPU case tables (test_gpu_wide_mlp_edges.py)
CASES = {
    "smallest": (1, 16, [(1, 1)]),                                 # one valid token in a 256-row tile
    "odd": (255, 48, [(96, 33), (33, 1), (128, 20)]),              # ragged everything
    "units": (300, 16, [(128, 128)] * 24),                         # U = 96, 384 class-2 slots
    "wrap0": (5700, 16, [(128, 12)] * 24),                         # 23 groups x 96 items of class 0: more than 2048 waves
    "widest": (257, 1024, [(128, 12)] * 24),                       # J_pad = 3072, four E tiles, 48 GEMM tiles
    "uneven": (8800, 16, [(32, 8)]),                               # 17 splits, the last one shorter
    "empty1": (25700, 16, [(32, 1)]),                              # T_pad = 25856, 1 tile: empty splits before the fix
    "empty6": (22100, 64, [(128, 12)] * 12),                       # T_pad = 22272, 6 tiles: the same
    "cap64": (33000, 64, [(128, 8)]),                              # T_pad = 33024: the parent's 64 splits, 63 with a K range
    # the small cases of the further tests
    "o4": (300, 32, [(128, 12), (64, 64)]),                        # every O a multiple of 4: the float4 side of vec_ok / row4
    "fuse4": (300, 32, [(128, 12), (100, 15), (128, 96), (97, 1)]),  # four-unit MLPs: second layers in the GEMM epilogue
    "local": (300, 32, [(100, 12), (33, 40)]),                     # padded hidden rows (100 -> 128, 33 -> 64), padded tokens
    "t257": (257, 144, [(64, 12), (127, 33)]),                     # one token past a tile
}
TABLE = ["smallest", "odd", "units", "wrap0", "widest", "uneven", "empty1", "empty6", "cap64"]
# known-answer constructions of x3_exact.make_case that the table runs besides the seeded operands (kind per case);
# test_wide_cases_cpu.py asserts their exactness
EXACT = {"smallest": "x", "odd": "w", "units": "dy", "widest": "x", "uneven": "x", "empty1": "dy", "cap64": "w"}
TABLE_RUNS = [(n, None) for n in TABLE] + [(n, EXACT[n]) for n in TABLE if n in EXACT]
ALIGN = ["odd", "o4"]
NULL_DX = ["odd", "o4"]
FUSE = ["fuse4"]
LOCAL = "local"
LOCAL_TOKENS = [0, 31, 32, 255, 256, 299]
STALE = ["smallest", "odd", "t257"]
REPEAT = ["odd", "fuse4"]
SEED = 20


def mlp_parameters(E, layers, seed):
    """(A, a, B, b) per MLP as f32 arrays, and the MLPBlocks they came from."""
    from sparsefactorization_amd.psfnet import MLPBlock
    torch.manual_seed(seed)
    blocks = [MLPBlock([h, 'GELU'], E, o) for h, o in layers]
    params = [tuple(p.detach().numpy().copy() for p in (b.network[0].weight, b.network[0].bias, b.network[2].weight, b.network[2].bias))
              for b in blocks]
    return params, blocks


def float64_reference(blocks, X, dYs):
    """Y_k, dX and (dA, da, dB, db)_k of float64 copies of the blocks."""
    refs = [copy.deepcopy(b).double() for b in blocks]
    x = torch.from_numpy(X).double().requires_grad_(True)
    ys = [b(x) for b in refs]
    torch.autograd.backward(ys, [torch.from_numpy(d).double() for d in dYs])
    grads = [tuple(p.grad.numpy() for p in (b.network[0].weight, b.network[0].bias, b.network[2].weight, b.network[2].bias)) for b in refs]
    return {"Y": [y.detach().numpy() for y in ys], "dX": x.grad.numpy(), "grads": grads}


@functools.lru_cache(maxsize=None)
def problem(name, kind=None):
    """(X, params, dYs, reference, exact) of a case: computed once, shared, never written to. ``kind`` None: seeded
    MLPBlocks and normal operands; "x", "w", "dy": that known-answer construction."""
    T, E, layers = CASES[name]
    if kind is not None:
        case = xe.make_case(kind, T, E, layers, seed=xe.seed("wide", T, E))
        X, params, dYs, ref, exact = case.X, [tuple(p) for p in case.params], case.dYs, case.reference(), True
    else:
        params, blocks = mlp_parameters(E, layers, SEED + T + E)
        rng = np.random.default_rng(SEED + T)
        X = rng.standard_normal((T, E)).astype(np.float32)
        dYs = [rng.standard_normal((T, o)).astype(np.float32) for _, o in layers]
        ref, exact = float64_reference(blocks, X, dYs), False
    for a in [X, *dYs, *[p for ps in params for p in ps]]:
        a.setflags(write=False)
    return X, params, dYs, ref, exact


# ---------------------------------------------------------------- canaries
CANARY = 0x7FC0C0DE      # as int32 / f32 bits: a quiet NaN with a payload that no arithmetic on the operands produces
BAND = 64                # floats on either side of a tensor: 256 bytes, so a shift-0 view keeps the allocation's alignment
SCRATCH_BAND = 64 * 1024  # bytes on either side of a scratch area


def _words(t):
    return t.view(torch.int32)


def banded(shape, device, shift=0):
    """(buffer, view, (lo, hi)): a tensor of ``shape`` at floats [lo, hi) of a buffer that holds CANARY everywhere;
    ``shift`` floats off the 16-byte boundary the allocation and the band give it."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * BAND + 4,), CANARY, dtype=torch.int32, device=device).view(torch.float32)
    lo = BAND + shift
    return buf, buf[lo:lo + n].view(*shape), (lo, lo + n)


def banded_input(a, device, shift=0):
    """The array inside canary bands: a kernel that reads past an operand's ends and uses what it finds shows NaN."""
    _, view, _ = banded(a.shape, device, shift)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32, copy=True)))  # (a copy: the shared operands are read-only)
    return view


def band_damage(buf, span) -> int:
    """Words of the two bands that no longer hold the canary."""
    lo, hi = span
    w = _words(buf)
    return int((w[:lo] != CANARY).sum()) + int((w[hi:] != CANARY).sum())


def unwritten(buf, span) -> int:
    """Words of the tensor that still hold the canary: elements the call never stored."""
    lo, hi = span
    return int((_words(buf)[lo:hi] == CANARY).sum())


def scratch(nbytes, device):
    """(buffer, view): ``nbytes`` bytes of 0xFF (NaN as f32 and as bf16) on a 256-byte boundary, SCRATCH_BAND bytes of 0xFF
    on either side inside the same allocation. nbytes = 0 gives an empty view."""
    buf = torch.full((nbytes + 2 * SCRATCH_BAND,), 0xFF, dtype=torch.uint8, device=device)
    return buf, buf[SCRATCH_BAND:SCRATCH_BAND + nbytes]


def scratch_damage(buf, nbytes) -> int:
    """Bytes of the two bands of a scratch area that are no longer 0xFF."""
    return int((buf[:SCRATCH_BAND] != 0xFF).sum()) + int((buf[SCRATCH_BAND + nbytes:] != 0xFF).sum())


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
