// psf_chord.hip — C ABI (include/psf_chord.h) and kernel dispatch for libpsf_chord.so. gfx950 only.
//
// Host side of the drop-in boundary that replaces torch_sparse.spmm at SyntheticExperiments/psf.py:178-184
// (and its copies) and spmul_cuda.{forward_host,backward_host} (spmul/spmul_cuda.cu:31-59,114-159).
// Stateless apart from a thread-local error string and a few process-wide tuning integers.
//
// Every step is planned once (plan_fwd / plan_bwd / plan_chain, and plan_mixer / plan_mixer_bf16 for the mixers, fill a plain
// struct) and the plan is either executed (fwd_impl / bwd_impl / chain_impl / mixer_impl / mixer_bf16_impl, from the caller's
// pointers), printed (psf_describe_*, operands taken as aligned: nullptr, which aligned_to accepts) or reported
// (psf_mixer_fwd*_plan / *_workspace). The order of the picks, the gates and the thresholds exist in the planners only.

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/psf_chord_tuning.h"
#include "bwd_kernels.h"
#include "bwd_window_launch.h"
#include "bwd_chain_lds.h"
#include "bwd_chain_lds_bf16.h"
#include "chain_tr_lds.h"
#include "fwd_chain_lds_bf16.h"
#include "fwd_chain_lds_launch.h"
#include "fwd_chain_regs_launch.h"
#include "fwd_kernels.h"
#include "fwd_mlp_step_launch.h"
#include "fwd_window_launch.h"
#include "mixer_lds_bf16_launch.h"
#include "mixer_lds_launch.h"
#include "mlp_fwd_x3.h"

using namespace psf;

namespace {

// ------------------------------------------------------------------------------------------------------
// errors, tuning
// ------------------------------------------------------------------------------------------------------
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int fail_hip(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s (hipError_t %d)", what, hipGetErrorString(e), (int)e);
  return (int)e;
}

// The knobs: include/psf_chord_tuning.h lists every key with its range, default and meaning. Each row makes an atomic and
// the row of g_knobs that psf_set_tuning / psf_get_tuning search by name. The chord part is private to this unit: g_<key>,
// a member of Tuning and its load in snapshot(). The producer part is read by the units that use it (mlp_fwd.hip,
// mlp_wide.hip declare psf_g_<key> extern) and is no member of Tuning.
#define X(key, lo, hi, def) std::atomic<int> g_##key{def};
PSF_TUNING_KNOBS_CHORD(X)
#undef X

}  // namespace
#define X(key, lo, hi, def) std::atomic<int> psf_g_##key{def};
PSF_TUNING_KNOBS_PRODUCER(X)
#undef X
namespace {

struct Knob {
  const char* key;
  std::atomic<int>* var;
  int lo, hi;
};
Knob g_knobs[] = {
#define X(key, lo, hi, def) {#key, &g_##key, lo, hi},
    PSF_TUNING_KNOBS_CHORD(X)
#undef X
#define X(key, lo, hi, def) {#key, &psf_g_##key, lo, hi},
    PSF_TUNING_KNOBS_PRODUCER(X)
#undef X
};

// One consistent view of the knobs per entry-point call: every extern "C" function takes ONE snapshot and hands it down, so
// a psf_set_tuning from another thread changes the next call, never the middle of one; `walk_backwards` (zigzag of a chain's
// odd steps) travels in it too instead of in thread-local state.
struct Tuning {
#define X(key, lo, hi, def) int key;
  PSF_TUNING_KNOBS_CHORD(X)
#undef X
  bool walk_backwards;
};

Tuning snapshot() {
  Tuning t;
#define X(key, lo, hi, def) t.key = g_##key.load();
  PSF_TUNING_KNOBS_CHORD(X)
#undef X
  t.walk_backwards = false;
  return t;
}

int ceil_log2(int64_t x) {
  int s = 0;
  while (((int64_t)1 << s) < x) ++s;
  return s;
}

// Reduce the caller's offsets (or the chord pattern) into [0, N).
void make_offsets(int64_t N, int32_t L, const int64_t* offsets, Offsets* out) {
  for (int k = 0; k < L; ++k) {
    int64_t o;
    if (offsets != nullptr) {
      o = offsets[k] % N;
      if (o < 0) o += N;
    } else if (k == 0) {
      o = 0;
    } else if (k - 1 < 62) {
      o = ((int64_t)1 << (k - 1)) % N;
    } else {  // 2^(k-1) does not fit in int64: (2^62 mod N) * 2 mod N
      int64_t t = ((int64_t)1 << 62) % N;
      for (int i = 62; i < k - 1; ++i) t = (t * 2) % N;
      o = t;
    }
    out->v[k] = (int32_t)o;
  }
  for (int k = L; k < PSF_MAX_LINKS; ++k) out->v[k] = 0;
}

int check_dims(int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride) {
  if (B < 0 || N < 1 || L < 1 || C < 1)
    return fail(PSF_E_SHAPE, "need B >= 0, N >= 1, L >= 1, C >= 1 (got B=%lld N=%lld L=%d C=%lld)", (long long)B,
                (long long)N, (int)L, (long long)C);
  if (L > PSF_MAX_LINKS) return fail(PSF_E_SHAPE, "L=%d exceeds PSF_MAX_LINKS=%d", (int)L, PSF_MAX_LINKS);
  if (N > (int64_t)1 << 30) return fail(PSF_E_SHAPE, "N=%lld exceeds 2^30", (long long)N);
  if (C > (int64_t)1 << 30 || N * C > (int64_t)1 << 40) return fail(PSF_E_SHAPE, "N*C too large");
  if (v_batch_stride != 0 && v_batch_stride != N * C)
    return fail(PSF_E_SHAPE, "v_batch_stride must be 0 (broadcast) or N*C=%lld, got %lld", (long long)(N * C),
                (long long)v_batch_stride);
  return PSF_OK;
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Geometry of a launch over row tiles [tile0, tile0 + tiles) of every batch element.
int make_geom(const Tuning& tn, int64_t B, int64_t N, int32_t L, int64_t C, int vec, int tg_shift, int TR, bool split_channels,
              int64_t v_bstride, int tile0, int tiles, Geom* gm) {
  gm->N = (int32_t)N;
  gm->L = L;
  gm->C = (int32_t)C;
  gm->CG = (int32_t)((C + vec - 1) / vec);
  gm->tg_shift = tg_shift;
  gm->TR = TR;
  gm->tiles_n = tiles;
  gm->tile0 = tile0;
  const int TG = 1 << tg_shift;
  gm->chunks_c = split_channels ? (gm->CG + TG - 1) / TG : 1;
  gm->per_b = gm->tiles_n * gm->chunks_c;
  const int64_t nb = B * (int64_t)gm->per_b;
  if (nb > (int64_t)0x7fffffff)
    return fail(PSF_E_SHAPE, "launch of %lld workgroups exceeds the grid limit", (long long)nb);
  gm->nblocks = (uint32_t)nb;
  gm->per_b_inv = udiv_inv_of((uint32_t)gm->per_b);
  gm->chunks_inv = udiv_inv_of((uint32_t)gm->chunks_c);
  gm->xq = gm->nblocks / kXcds;
  gm->xr = gm->nblocks % kXcds;
  gm->remap = tn.xcd_remap ? (tn.walk_backwards && tn.chain_zigzag ? 2 : 1) : 0;
  gm->aligned = 0;  // window_launches sets it from the pick
  gm->ileave = 0;
  gm->v_bstride = v_bstride;
  return PSF_OK;
}

int generic_geom(const Tuning& tn, int64_t B, int64_t N, int32_t L, int64_t C, int vec, bool split_channels, int64_t v_bstride,
                 Geom* gm) {
  const int64_t CG = (C + vec - 1) / vec;
  const int tgs = ceil_log2(CG) > 6 ? 6 : ceil_log2(CG);
  const int TR = kBlock >> tgs;
  return make_geom(tn, B, N, L, C, vec, tgs, TR, split_channels, v_bstride, 0, (int)((N + TR - 1) / TR), gm);
}

// ------------------------------------------------------------------------------------------------------
// element types, window-kernel selection
// ------------------------------------------------------------------------------------------------------
// What the planners need to know of an element type. f32 has every configuration; the bf16 window kernels
// (fwd_window_launch.h: kWinTgsMaxBf16) take 16-byte groups of 8 channels, TGS 0..4 on 256 threads x `rows` (forward and dV: 2,
// rows wider than 128 channels split into 128-channel chunks; dW: 1); f64 exists for gradcheck, on the generic kernels.
struct Elem {
  const char* name;
  int bytes, vec;   // element bytes; elements per 16-byte group
  bool window;      // LDS-window kernels, the fused backward step and the one-launch chain exist
  int tgs_max;      // widest window-kernel channel-group shift
  bool f32_routes;  // the wide-row, four-row and 512-thread window configurations, the chunk-looping dW and the EDGE
                    // instance of the fused step exist
};
constexpr Elem kBf16{"bf16", 2, 8, true, kWinTgsMaxBf16, false}, kF32{"f32", 4, 4, true, kWinTgsMax, true},
    kF64{"f64", 8, 2, false, 0, false};
const Elem& elem_of(int bytes) { return bytes == 2 ? kBf16 : bytes == 4 ? kF32 : kF64; }
template <typename T>
constexpr bool kIsBf16 = std::is_same<T, __bf16>::value;

struct WinPick {
  int tgs, rows, nt, TR, KN;
  int tiles_full;  // row tiles per sequence with all TR rows < N
  bool ragged;     // N % TR != 0: one more, partial, tile per sequence
  bool all_edge;   // every tile must take the EDGE kernel (channel groups not a multiple of TG, or W not chunk-clean)
  bool aligned = false;  // Geom::aligned
};

void set_pick(WinPick* pk, int tgs, int rows, int nt, int TR, int KN, int64_t N) {
  pk->tgs = tgs, pk->rows = rows, pk->nt = nt, pk->TR = TR, pk->KN = KN;
  pk->tiles_full = (int)(N / TR), pk->ragged = (N % TR) != 0;
}

// The near links of a tile of TR rows: offsets 0, 1, 2, ..., 2^(KN-2) <= TR, at most L of them. They are compile-time
// constants in the window kernels, so 0 (no kernel) unless the caller's first KN offsets are the chord pattern's.
int near_links(int TR, int32_t L, const Offsets& offs) {
  int KN = 2;
  for (int t = TR; t > 1; t >>= 1) ++KN;
  if (KN > L) KN = L;
  for (int k = 0; k < KN; ++k)
    if (offs.v[k] != chord_off(k)) return 0;
  return KN;
}

// Run-time configuration -> compiled instance, by argument type.
hipError_t launch_win(const WinPick& pk, int L, const FwdWinArgs& a) {
  if (pk.nt == kWideThreads) return pk.tgs == kWideTgs ? launch_fwd_win<kWideTgs, kWideThreads>(pk.rows, L, a) : hipErrorInvalidValue;
  return with_int<0, kWinTgsMax>(pk.tgs, [&](auto t) { return launch_fwd_win<t(), 256>(pk.rows, L, a); });
}
hipError_t launch_win(const WinPick& pk, int L, const FwdWinArgsT<__bf16>& a) {
  return with_int<0, kWinTgsMaxBf16>(pk.tgs, [&](auto t) { return launch_fwd_win_bf16<t()>(pk.rows, L, a); });
}
hipError_t launch_dv(const WinPick& pk, int L, const BwdWinArgs& a) {
  if (pk.nt == kWideThreads) return pk.tgs == kWideTgs ? launch_dv_win<kWideTgs, kWideThreads>(pk.rows, L, a) : hipErrorInvalidValue;
  if (pk.nt == kDvMidThreads)
    return with_int<0, kDvMidTgsMax>(pk.tgs, [&](auto t) { return launch_dv_win<t(), kDvMidThreads>(pk.rows, L, a); });
  return with_int<0, kWinTgsMax>(pk.tgs, [&](auto t) { return launch_dv_win<t(), 256>(pk.rows, L, a); });
}
hipError_t launch_dv(const WinPick& pk, int L, const BwdWinArgsT<__bf16>& a) {
  return with_int<0, kWinTgsMaxBf16>(pk.tgs, [&](auto t) { return launch_dv_win_bf16<t()>(L, a); });
}
hipError_t launch_dw(bool chunk, const WinPick& pk, int L, const BwdWinArgs& a) {
  if (chunk) return with_int<kDwChunkTgsMin, kDwChunkTgsMax>(pk.tgs, [&](auto t) { return launch_dw_chunk<t()>(L, a); });
  return with_int<0, kWinTgsMax>(pk.tgs, [&](auto t) { return launch_dw_win<t()>(pk.rows, L, a); });
}
hipError_t launch_dw(bool, const WinPick& pk, int L, const BwdWinArgsT<__bf16>& a) {
  return with_int<0, kWinTgsMaxBf16>(pk.tgs, [&](auto t) { return launch_dw_win_bf16<t()>(L, a); });
}
hipError_t launch_fused(bool edge, int tgs, int L, const BwdWinArgs& a) {
  if (edge) return with_int<0, kFusedTgsMax>(tgs, [&](auto t) { return launch_bwd_fused_edge<t()>(L, a); });
  return with_int<0, kFusedTgsMax>(tgs, [&](auto t) { return launch_bwd_fused<t()>(L, a); });
}
hipError_t launch_fused(bool, int tgs, int L, const BwdWinArgsT<__bf16>& a) {
  return with_int<0, kFusedBf16TgsMax>(tgs, [&](auto t) { return launch_bwd_fused_bf16<t()>(L, a); });
}

// Row widths the fused backward step takes: exactly 4 << tgs channels with a whole row inside one workgroup. Rounds 3-5: up
// to 32 channels. Round 6 (profiles/r06p_bwd_fused_wide*.log, us per step, two kernels / fused, operands rotating, dZ chained):
// 64 channels at every length — N = 1024: 11.3 / 8.9; 2000: 20.2 / 15.3; 2048: 21.6 / 17.4; 2049 (edge instance): 23.6 / 18.8;
// 4096: 42.8 / 38.3; 4097: 23.8 / 18.7; 8192: 43.7 / 42.9; 16384: 49.3 / 47.2 — and 128 channels up to N = 4096 — ListOps'
// N = 2000: 39.3 / 35.4; 2001: 40.1 / 36.9; 1024, 4096, 4097 equal — but not beyond (N = 16384: 96.3 / 102.8: tiles of 8 rows).
// bf16 (bwd_fused_bf16.h): rows of exactly 8 << tgs channels (8..128).
bool fused_step_width(const Elem& el, int64_t C, int64_t N) {
  if (!el.f32_routes) return C == 8 || C == 16 || C == 32 || C == 64 || C == 128;
  return C == 4 || C == 8 || C == 16 || C == 32 || C == 64 || (C == 128 && N <= 4096);
}

// The automatic route (bwd_fused = 1). f32: wherever the step applies. bf16 (was fused_step_auto_bf16): only the widths and
// lengths where it measured faster than the two window kernels by more than the run-to-run spread
// (profiles/bf16_bwd_fused_ab.md). Until a shape has been measured it stays on the two kernels; bwd_fused = 2 takes the fused
// step wherever it applies.
bool fused_step_auto(const Elem& el, int64_t B, int64_t N, int64_t C) {
  (void)B, (void)N, (void)C;
  return el.f32_routes;
}

// The EDGE instance of the fused step (bwd_fused.h: chord_bwd_fused_edge_k) takes what pick_fused_step turns away for its
// geometry: any N >= two tiles (N = 2^k + 1 with a CLS token), any far offsets, W / dW at any alignment. Same rows (fused_step_width), chord near offsets, 16-byte aligned row operands. Knob bwd_fused = 2 keeps its meaning (the aligned instance or
// nothing); 1 (default) lets this one in.
// There is no bf16 edge instance: ragged N, other far offsets and misaligned W / dW stay on the two window kernels.
bool pick_fused_edge_step(const Elem& el, const Tuning& tn, const void* dZ, const void* V, const void* dV, int64_t N, int32_t L,
                          int64_t C, int64_t v_bstride, const Offsets& offs, WinPick* pk) {
  if (!el.f32_routes || tn.bwd_fused != 1 || L < kWinLmin || L > kWinLmax || !fused_step_width(el, C, N)) return false;
  const int tgs = ceil_log2(C / el.vec), TR = 256 >> tgs;
  if (N < 2 * (int64_t)TR) return false;
  if (!aligned_to(dZ, 16) || !aligned_to(V, 16) || !aligned_to(dV, 16)) return false;
  if (v_bstride != 0 && v_bstride != N * C) return false;
  const int KN = near_links(TR, L, offs);
  if (!KN) return false;
  set_pick(pk, tgs, 1, 256, TR, KN, N);
  pk->all_edge = true;
  return true;
}

// The fused dV + dW step (bwd_fused.h, bwd_fused_bf16.h) applies to full tiles of rows of exactly el.vec << tgs channels
// (fused_step_width), N a multiple of the tile (256 >> tgs rows) and at least two tiles, chord near offsets, every far offset a
// multiple of the tile, all five operands 16-byte aligned and W / dW chunk-clean, a batch element's rows below 2^31 bytes.
// Knob bwd_fused: 0 never, 1 where fused_step_auto says, 2 wherever it applies. (One pick for both element types: bf16's
// was pick_fused_step_bf16.)
bool pick_fused_step(const Elem& el, const Tuning& tn, const void* dZ, const void* W, const void* V, const void* dW, const void* dV,
                     int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_bstride, const Offsets& offs, WinPick* pk) {
  const int knob = tn.bwd_fused;
  if (!knob || L < kWinLmin || L > kWinLmax || !fused_step_width(el, C, N)) return false;
  if (knob == 1 && !fused_step_auto(el, B, N, C)) return false;
  const int tgs = ceil_log2(C / el.vec), TR = 256 >> tgs;
  if (N % TR != 0 || N < 2 * (int64_t)TR) return false;
  if (!aligned_to(dZ, 16) || !aligned_to(W, 16) || !aligned_to(V, 16) || !aligned_to(dW, 16) || !aligned_to(dV, 16)) return false;
  if ((B * N * (int64_t)L) % el.vec != 0 || (v_bstride != 0 && v_bstride != N * C)) return false;
  const int KN = near_links(TR, L, offs);
  if (!KN) return false;
  for (int k = KN; k < L; ++k)
    if (offs.v[k] % TR != 0) return false;  // far row blocks are TR-aligned (scalar block addresses in the kernel)
  if (N * C * el.bytes >= ((int64_t)1 << 31)) return false;
  set_pick(pk, tgs, 1, 256, TR, KN, N);
  pk->all_edge = false;
  return true;
}

// Interleaved fronts of the fused step (Geom::ileave): the shift, 0 = one front.
// Two interleaved fronts per batch element (Geom::ileave, bwd_fused.h): tile t of the XCD's walk is row block
// (t mod 2) tiles / 2 + t / 2, so the rows N / 2 apart that the longest link joins are in flight together. Round 6,
// operands rotating as in the chain's backward (profiles/r06c_bwd_ileave2.log, us per step, one front / two): Order
// shape (N = 16384, C = 8, B = 40) 41.1 / 39.2, N = 4096 x 32 channels 22.1 / 21.6, genome (N = 16384 x 32) 46.5 / 47.0
// (noise); four and eight fronts equal two. In the training steps (r06c_step_ileave.log): Order 2.100 -> 2.074 ms,
// genome 1.764 -> 1.734, IMDb (edge kernel: not applicable) unchanged. Auto: two fronts from N = 8192 on. (The forward
// window kernel gains nothing from it at any shape — cfg2 25.8 / 26.0 us, genome 22.8 / 23.2 — and keeps one front:
// profiles/r06c_fwd_fronts.log.)
// Fronts and workgroups per CU: f32's rules (two fronts from N = 8192 on; no limit) kept unmeasured for bf16 unless the .md says otherwise
int fused_fronts_shift(const Tuning& tn, int64_t N, int tiles_full) {
  const int fronts = tn.bwd_fronts ? tn.bwd_fronts : (N >= 8192 ? 2 : 1);
  int sh = 0;
  while ((2 << sh) <= fronts) ++sh;
  return sh > 0 && tiles_full % (1 << sh) == 0 ? sh : 0;
}

// Workgroups per CU of the f32 fused step, re-measured on the round-4 kernel with rotating operands (profiles/r04am_bwd_fused_wg_sweep.log, us per
// step, what fits / three): 5120 tiles (N = 16384, C = 8, B = 40) 42.3 / 40.9; 8192 tiles (C = 32, B = 16) 51.0 / 49.6; 4096
// tiles (N = 4096, C = 16, B = 64) 26.6 / 25.4; 2048 tiles 12.6 / 13.5 and 14.7 / 15.0: three from 4096 tiles on.
// Rows of 64 / 128 channels (round 6, tiles of 16 / 8 rows; profiles/r06r_bwd_rows_wide.log, what fits / three / four):
// N = 2048 x 64, B = 32: 17.4 / 17.3 / 15.9; N = 4096 x 64, B = 16: 17.4 / 17.3 / 16.3; N = 2000 x 128: 35.5 / 35.6 / 34.8;
// N = 16384 x 64: 47.0 / 47.1 / 47.5 — four from 4096 tiles on. bf16: no limit (see fused_fronts_shift).
int fused_wg_auto(const Elem& el, int64_t tiles_total, int tgs) {
  return el.f32_routes && tiles_total >= 4096 ? (tgs >= 4 ? 4 : 3) : 0;
}

// A ragged last tile per sequence (N % TR != 0) runs on the EDGE instance. In a second launch of its own it costs a
// kernel boundary, ~2.7 us whatever the shape (r02d: IMDb N = 4097, C = 32: 15.3 us split vs 12.7 in one predicated
// launch; N = 2000, C = 16: 7.7 vs 5.0; dW at N = 2000, C = 128: 21.9 vs 16.1); predicating EVERY tile costs 0-5 % of the
// launch (r01c: cfg2 27.6 -> 28.9 us). So: one predicated launch unless the launch is long enough for 5 % to exceed the
// boundary, i.e. beyond ~300 MB of algorithmic bytes.
bool ragged_in_one_launch(const Tuning& tn, bool ragged, int64_t B, int64_t N, int32_t L, int64_t C) {
  return ragged && tn.fwd_split == 1 && 4 * B * N * (L + 3 * C) <= (int64_t)300 * 1000 * 1000;
}

// Chunk-looping dW (bwd_dw_chunk.h, f32), rows of >= 32 channels whose channel groups split into chunks of 8 (or 16) lanes:
// 256 threads x 1 row, so tiles of 32 (16) rows. Fills `pick` when the kernel applies.
bool pick_dw_chunk(const Tuning& tn, const void* dW, int64_t B, int64_t N, int32_t L, int64_t C, const Offsets& offs, bool vec_ok,
                   WinPick* pick) {
  if (!vec_ok || L < kWinLmin || L > kWinLmax) return false;
  const int64_t CG = C / 4;
  if (CG % 8 != 0 || CG / 8 > 4096) return false;
  int tgs = 3;
  const int knob = tn.dw_tgs;
  // 16 lanes per row chunk (16-row tiles) when that spares the launch its ragged last tile (ListOps: N = 2000 = 125 * 16)
  if (knob == 5 || (knob == 0 && CG % 16 == 0 && N % 32 != 0 && N % 16 == 0)) tgs = CG % 16 == 0 ? 4 : 3;
  const int TR = win_tile_rows(tgs, 1, 256);
  if (N < 2 * (int64_t)TR) return false;
  const int KN = near_links(TR, L, offs);
  if (!KN) return false;
  if (N * C >= ((int64_t)1 << 31)) return false;                 // 32-bit element offsets inside a batch element
  set_pick(pick, tgs, 1, 256, TR, KN, N);
  pick->all_edge = ragged_in_one_launch(tn, pick->ragged, B, N, L, C) || !aligned_to(dW, 16) || ((N * (int64_t)L) % 4) != 0 || !tn.fwd_split;
  return true;
}

// Decide whether a window kernel applies (vectorisable, chord-like near links); fills pick on success.
// `W` is the flat [B,N,L] array the kernel copies in 16-byte chunks (W itself, or dW for the dW kernel).
// `rows_pref`: 2 (forward, dV) or 1 (dW): the compiled rows per thread (fwd_window_launch.h).
// `chunk_channels`: the kernel may split a row's channels over several workgroups (forward, dV) — then wide f32 rows
// (C >= 64) use the wide-row configuration: 32-channel chunks, 1024 threads, 256-row tiles.
// bf16 (was pick_window_bf16): no wide-row, four-row or 512-thread configuration; the same near-offset and alignment rules
// with 8 elements per 16-byte chunk and 2-byte elements.
bool pick_window(const Elem& el, const Tuning& tn, const void* W, int64_t B, int64_t N, int32_t L, int64_t C, const Offsets& offs,
                 bool vec_ok, WinPick* pick, int rows_pref, bool chunk_channels, int nt_pref = 0, bool forward = false) {
  if (!vec_ok || L < kWinLmin || L > kWinLmax) return false;
  const int64_t CG = C / el.vec;
  int tgs = ceil_log2(CG) > el.tgs_max ? el.tgs_max : ceil_log2(CG);
  int nt = 256;
  int rows = rows_pref;
  if (el.f32_routes) {
    const int wide = tn.fwd_wide;
    // Forward, rows of 64..256 channels, sequences up to 4096: 32-channel chunks on 1024-thread workgroups (256-row tiles: two
    // far links at L = 12 instead of five to seven). With the scalar block addresses of round 4 they beat the whole-row tiles that
    // rounds 1-3 measured faster: N = 2048, B = 32: C = 64 10.7 -> 9.0 us per step, C = 96 16.7 -> 14.3, C = 128 19.5 -> 18.3,
    // C = 192 29.9 -> 25.7, C = 256 36.1 -> 33.9; N = 4096: +2..5 %; C = 512: equal; N = 16384, C = 64, B = 8: 23.7 -> 25.7 (slower)
    // (profiles/r04ak_fwd_wide_rule_sweep.log). The backward kernels keep their configuration.
    // Round 5, with operands rotating beyond the Infinity Cache as a training step has them (profiles/r05m_fwd_wide_mid.log, us per
    // step, chunks / whole rows): N = 2048, C = 64: 10.5 / 11.8; N = 2048, C = 128: 20.8 / 22.0; N = 4096, C = 64: 21.7 / 22.6; C = 256:
    // 21.2 / 21.9 — but ListOps' N = 2000, C = 128: 23.9 / 21.1: 2000 is no multiple of the 256-row chunk tile (every tile then takes the
    // per-lane request form) and a multiple of the whole-row tile. So: chunks only where their tiles divide N or the whole-row tiles do not.
    const int64_t tr_whole = win_tile_rows(tgs, rows, 256), tr_chunk = win_tile_rows(kWideTgs, rows, kWideThreads);
    const bool auto_wide = forward && wide == 0 && CG >= 16 && CG <= 64 && N <= 4096 && (N % tr_chunk == 0 || N % tr_whole != 0);
    if (chunk_channels && (wide == 1 || auto_wide) && CG >= 16 && N >= 2 * (int64_t)win_tile_rows(kWideTgs, rows, kWideThreads)) {
      tgs = kWideTgs;  // 32-channel chunks on 1024-thread workgroups
      nt = kWideThreads;
    } else if (chunk_channels && wide == 2 && CG >= 16) {
      tgs = kWideTgs;  // 32-channel chunks on 256-thread workgroups
    } else if (nt_pref == kDvMidThreads && tgs <= kDvMidTgsMax && N >= 2 * (int64_t)win_tile_rows(tgs, 1, kDvMidThreads)) {
      nt = kDvMidThreads;  // dV: 512 threads x 1 row
      rows = 1;
    }
    // Forward, rows of 16..64 channels: four rows per thread (fwd_window_launch.h: win_rows4_compiled) where the four-row tile
    // divides N, i.e. where its launches take the aligned request form; the per-lane form of other lengths (2^k + 1: LRA's
    // CLS-token column) is faster on the smaller tile (N = 4097 x 32: 11.3 / 12.1 us, N = 1025: 6.9 / 7.2, two rows / four:
    // profiles/r06k_fwd_rows_product.log). From N = 4096 on: below that the two forms are within 3 % of each other and the sign
    // depends on how the step is driven (Pathfinder's shape, N = 1024 x 32: 6.32 / 6.13 us per step inside a chain, but 5.82 /
    // 6.39 us per launch for the same step launched alone again and again under rocprofv3: r06m_fwd_rows_resident.log,
    // r06z_bwd_summary.md of both collections).
    if (forward && win_rows4_compiled(tgs, nt) && tn.fwd_rows != 2 && N >= 2 * (int64_t)win_tile_rows(tgs, 4, nt)) {
      if (tn.fwd_rows == 4 || (N >= 4096 && N % win_tile_rows(tgs, 4, nt) == 0)) rows = 4;
    }
  }
  const int TR = win_tile_rows(tgs, rows, nt);
  if (N < 2 * (int64_t)TR) return false;  // the window may wrap at most once
  const int KN = near_links(TR, L, offs);
  if (!KN) return false;
  set_pick(pick, tgs, rows, nt, TR, KN, N);
  pick->aligned = (N % TR) == 0 && N * C * el.bytes < ((int64_t)1 << 31);
  for (int k = KN; k < L; ++k)
    if (offs.v[k] % TR != 0) pick->aligned = false;
  const int TG = 1 << tgs;
  pick->all_edge = (CG % TG) != 0 || !aligned_to(W, 16) || ((B * N * (int64_t)L) % el.vec) != 0 || !tn.fwd_split ||
                   ragged_in_one_launch(tn, pick->ragged, B, N, L, C);
  return true;
}

// The dV window kernel's configuration for a shape.
// default rows per thread (r01 sweep, us at cfg2): dV R=2 31.3 vs R=1 32.7; 512 threads x 1 row per thread instead of
// 256 x 2 is the same tile at C <= 8 (r02 lab 28.65 vs 29.05 us at cfg2)
bool pick_dv(const Elem& el, const Tuning& tn, const void* W, int64_t B, int64_t N, int32_t L, int64_t C, const Offsets& offs,
             bool vec_ok, WinPick* pk) {
  const int nt_dv = (tn.dv_threads == 0 && C <= 8) ? kDvMidThreads : 0;
  return pick_window(el, tn, W, B, N, L, C, offs, vec_ok, pk, 2, true, nt_dv);
}

// ------------------------------------------------------------------------------------------------------
// one plan per step
// ------------------------------------------------------------------------------------------------------
struct FwdPlan {
  bool window;    // the LDS-window kernel of `pk`; else the generic kernel on `vec` elements per thread
  bool refused;   // fwd_variant = 2 and the window kernel does not apply: a launch is PSF_E_TUNING
  WinPick pk;
  int vec;
  int wg_per_cu;  // window kernel: FwdWinArgsT::wg_per_cu
};

FwdPlan plan_fwd(const Elem& el, const Tuning& tn, const void* W, const void* V, const void* res, const void* out, int64_t B,
                 int64_t N, int32_t L, int64_t C, const Offsets& offs) {
  FwdPlan p{};
  const bool vec_ok = (C % el.vec == 0) && aligned_to(V, 16) && aligned_to(out, 16) && (!res || aligned_to(res, 16));
  p.vec = vec_ok ? el.vec : 1;
  p.window = el.window && tn.fwd_variant != 1 && pick_window(el, tn, W, B, N, L, C, offs, vec_ok, &p.pk, 2, true, 0, true);
  p.refused = !p.window && tn.fwd_variant == 2;
  if (!p.window) return p;
  // Workgroups per CU. Measured (profiles/r01e_fwd_wg_per_cu.log, us per launch, 4 / 3 per CU): cfg2 (C = 8, 4096
  // tiles) 27.6 / 27.0; the same at B = 40 (2560 tiles) 18.9 / 18.8; C = 32, B = 16: 24.5 / 24.8; N = 4096, C = 16:
  // 8.9 / 9.2; 2 per CU: 30.0 at cfg2. Round 3, chains that keep every step's output (training; N = 16384, C = 8, no limit /
  // three per CU, profiles/r03al_fwd_wg_limit_sweep.log): B = 16 (1024 tiles) 9.4 / 9.7; B = 24 13.5 / 13.2; B = 32 16.5 /
  // 16.1; B = 40 19.9 / 19.0; B = 48 22.8 / 21.8. So: three for narrow rows on launches of >= 1536 tiles, no limit otherwise.
  // Rows of 32 channels on launches of >= 8192 tiles (round 4, profiles/r04ai_fwd_mid_sweep.log, N = 16384, B = 64): 102.9 / 97.4;
  // at B = 16 (4096 tiles) 22.6 / 22.7, N = 4096, B = 32: 11.2 / 11.6 — so three there too, from 8192 tiles on.
  // Rows of 16 channels (same sweep script, us per step, what fits / three): 8192 tiles (N = 16384, B = 64) 45.9 / 44.3; 2048
  // tiles (B = 16) 13.1 / 12.8; 1024 tiles (N = 4096, B = 32) 7.1 / 7.8: three from 2048 tiles on.
  // bf16 (was fwd_window_bf16): these thresholds, keyed on TGS and tile count, are f32 measurements applied to bf16 unchanged —
  // a bf16 channel group holds twice the channels and a bf16 tile twice the rows of the f32 configuration with the same TGS, so
  // they describe other workloads here; not re-tuned for bf16.
  const int knob = tn.fwd_wg_limit;
  const int64_t tiles_total = B * (int64_t)(p.pk.tiles_full + (p.pk.ragged ? 1 : 0));
  const bool three = p.pk.nt == 256 && ((p.pk.tgs <= 1 && tiles_total >= 1536) || (p.pk.tgs == 2 && tiles_total >= 2048) ||
                                        (p.pk.tgs == 3 && tiles_total >= 8192));
  p.wg_per_cu = knob == 0 ? (three ? 3 : 0) : (knob == 1 ? 0 : knob);
  return p;
}

enum class Route { kNone, kGeneric, kWindow, kChunk };  // kNone: not asked for, or the fused step computes it
enum class Fused { kNone, kAligned, kEdge };

struct BwdPlan {
  Fused fused;
  WinPick fpk;            // fused step: its tiles, fronts shift (Geom::ileave) and workgroups per CU
  int ileave, wg_per_cu;
  Route dw, dv;           // otherwise, per gradient: kChunk (dW, f32), kWindow or kGeneric (on dw_vec / dv_vec elements per thread)
  WinPick dwpk, dvpk;
  bool dw_all_edge;       // (dV's is dvpk.all_edge)
  int dw_vec, dv_vec;
  bool refused;           // dw_variant = 2 and the chunk-looping dW kernel does not apply: a launch is PSF_E_TUNING
};

// The kernels of one backward step. Pointers may be nullptr (describe: taken as aligned); want_dw / want_dv say which
// gradients the caller asks for.
BwdPlan plan_bwd(const Elem& el, const Tuning& tn, const void* dZ, const void* W, const void* V, const void* dW, const void* dV,
                 bool want_dw, bool want_dv, int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_bstride, const Offsets& offs) {
  BwdPlan p{};
  const bool dw_ok = (C % el.vec == 0) && aligned_to(dZ, 16) && aligned_to(V, 16);
  const bool dv_ok = (C % el.vec == 0) && aligned_to(dZ, 16) && aligned_to(dV, 16);
  p.dw_vec = dw_ok ? el.vec : 1, p.dv_vec = dv_ok ? el.vec : 1;
  p.dw = want_dw ? Route::kGeneric : Route::kNone, p.dv = want_dv ? Route::kGeneric : Route::kNone;
  // LDS-window kernels (f32 and bf16; f64 takes the generic kernels)
  if (!el.window || tn.bwd_variant == 1 || B < 1) return p;
  if (want_dw && want_dv) {  // the fused step, aligned instance first
    if (pick_fused_step(el, tn, dZ, W, V, dW, dV, B, N, L, C, v_bstride, offs, &p.fpk)) {
      p.fused = Fused::kAligned;
      p.ileave = fused_fronts_shift(tn, N, p.fpk.tiles_full);
      p.wg_per_cu = tn.bwd_fused_wg_limit ? tn.bwd_fused_wg_limit : fused_wg_auto(el, B * (int64_t)p.fpk.tiles_full, p.fpk.tgs);
    } else if (pick_fused_edge_step(el, tn, dZ, V, dV, N, L, C, v_bstride, offs, &p.fpk)) {
      p.fused = Fused::kEdge;
    }
    if (p.fused != Fused::kNone) {
      p.dw = p.dv = Route::kNone;
      return p;
    }
  }
  // dW before dV: dV's output is the next (earlier) step's dZ, read first thing by that step's kernels; writing
  // it last leaves it cache-hot (dV 27.4 -> 26.9 us, dW 20.5 -> 20.4 us in the Order training step)
  // default rows per thread (r01 sweep, us at cfg2): dV R=2 31.3 vs R=1 32.7; dW R=1 22.9 vs R=2 28.7
  if (want_dw) {
    if (el.f32_routes && tn.dw_variant != 1 && pick_dw_chunk(tn, dW, B, N, L, C, offs, dw_ok, &p.dwpk)) {
      p.dw = Route::kChunk;
      p.dw_all_edge = p.dwpk.all_edge;
    } else {
      p.refused = el.f32_routes && tn.dw_variant == 2;  // (planned on all the same: describe names what follows)
      if (C / el.vec <= (1 << el.tgs_max) && pick_window(el, tn, dW, B, N, L, C, offs, dw_ok, &p.dwpk, 1, false)) {
        p.dw = Route::kWindow;
        // the dW tile store is chunk-clean only if every sequence starts on a 16-byte boundary
        p.dw_all_edge = p.dwpk.all_edge || ((N * (int64_t)L) % el.vec) != 0;
      }
    }
  }
  if (want_dv && pick_dv(el, tn, W, B, N, L, C, offs, dv_ok, &p.dvpk)) p.dv = Route::kWindow;
  return p;
}

// ------------------------------------------------------------------------------------------------------
// typed entry points
// ------------------------------------------------------------------------------------------------------
// Issue the one to two launches of a window kernel: full tiles on the predicate-free instance, the ragged last
// tile of every sequence (if any) on the EDGE instance; everything on the EDGE instance when `all_edge`.
// `launch` reads *gm and *edge, which are filled in before each call.
// `vec`: elements per 16-byte channel group (4 for f32, 8 for bf16).
template <typename F>
int window_launches(const Tuning& tn, const WinPick& pk, bool all_edge, int64_t B, int64_t N, int32_t L, int64_t C,
                    int64_t v_bstride, bool split_channels, Geom* gm, bool* edge, F launch, const char* what, int vec = 4) {
  const int tiles_all = pk.tiles_full + (pk.ragged ? 1 : 0);
  struct Part {
    int tile0, tiles;
    bool edge;
  };
  Part parts[2];
  int np = 0;
  if (all_edge) {
    parts[np++] = {0, tiles_all, true};
  } else {
    if (pk.tiles_full > 0) parts[np++] = {0, pk.tiles_full, false};
    if (pk.ragged) parts[np++] = {pk.tiles_full, 1, true};
  }
  for (int i = 0; i < np; ++i) {
    if (int rc = make_geom(tn, B, N, L, C, vec, pk.tgs, pk.TR, split_channels, v_bstride, parts[i].tile0, parts[i].tiles, gm))
      return rc;
    gm->aligned = pk.aligned && !parts[i].edge;
    *edge = parts[i].edge;
    hipError_t e = launch();
    if (e != hipSuccess) return fail_hip(e, what);
  }
  return PSF_OK;
}

template <typename T>
int fwd_impl(const Tuning& tn, const T* W, const T* V, const T* res, T* out, int64_t B, int64_t N, int32_t L, int64_t C,
             int64_t v_batch_stride, const int64_t* offsets, void* stream) {
  if (int rc = check_dims(B, N, L, C, v_batch_stride)) return rc;
  if (B == 0) return PSF_OK;
  if (!W || !V || !out) return fail(PSF_E_NULL, "W, V and out must be non-NULL");
  if (out == V) return fail(PSF_E_ALIAS, "out must not alias V (rows are gathered from other rows)");
  if (!aligned_to(W, sizeof(T)) || !aligned_to(V, sizeof(T)) || !aligned_to(out, sizeof(T)) ||
      (res && !aligned_to(res, sizeof(T))))
    return fail(PSF_E_ALIGN, "pointers must be aligned to the element size");
  Offsets offs;
  make_offsets(N, L, offsets, &offs);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int VECW = 16 / (int)sizeof(T);

  const FwdPlan p = plan_fwd(elem_of((int)sizeof(T)), tn, W, V, res, out, B, N, L, C, offs);
  if constexpr (sizeof(T) != 8) {
    if (p.window) {
      FwdWinArgsT<T> a;
      a.W = W;
      a.V = V;
      a.res = res;
      a.out = out;
      a.offs = offs;
      a.w_total = B * N * (int64_t)L;
      a.stream = s;
      a.wg_per_cu = p.wg_per_cu;
      return window_launches(tn, p.pk, p.pk.all_edge, B, N, L, C, v_batch_stride, true, &a.gm, &a.edge,
                             [&] { return launch_win(p.pk, L, a); },
                             kIsBf16<T> ? "chord_fwd_win<bf16> launch" : "chord_fwd_win launch", VECW);
    }
  }
  if (p.refused)
    return fail(PSF_E_TUNING, "fwd_variant=2 forced but the window kernel does not apply to N=%lld L=%d C=%lld",
                (long long)N, (int)L, (long long)C);

  Geom gm;
  if (int rc = generic_geom(tn, B, N, L, C, p.vec, true, v_batch_stride, &gm)) return rc;
  if (p.vec != 1)
    hipLaunchKernelGGL((chord_fwd_generic_k<T, VECW>), dim3(gm.nblocks), dim3(kBlock), 0, s, W, V, res, out, gm, offs);
  else
    hipLaunchKernelGGL((chord_fwd_generic_k<T, 1>), dim3(gm.nblocks), dim3(kBlock), 0, s, W, V, res, out, gm, offs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "chord_fwd_generic launch");
  return PSF_OK;
}

template <typename T>
int bwd_impl(const Tuning& tn, const T* dZ, const T* W, const T* V, T* dW, T* dV, int64_t B, int64_t N, int32_t L, int64_t C,
             int64_t v_batch_stride, const int64_t* offsets, void* stream) {
  if (int rc = check_dims(B, N, L, C, v_batch_stride)) return rc;
  if (B == 0) return PSF_OK;
  if (!dZ) return fail(PSF_E_NULL, "dZ must be non-NULL");
  if (dV && !W) return fail(PSF_E_NULL, "dV requested but W is NULL");
  if (dW && !V) return fail(PSF_E_NULL, "dW requested but V is NULL");
  if (dV && dV == dZ) return fail(PSF_E_ALIAS, "dV must not alias dZ");
  if (!aligned_to(dZ, sizeof(T)) || (W && !aligned_to(W, sizeof(T))) || (V && !aligned_to(V, sizeof(T))) ||
      (dW && !aligned_to(dW, sizeof(T))) || (dV && !aligned_to(dV, sizeof(T))))
    return fail(PSF_E_ALIGN, "pointers must be aligned to the element size");
  Offsets offs;
  make_offsets(N, L, offsets, &offs);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  constexpr int VECW = 16 / (int)sizeof(T);

  const BwdPlan p = plan_bwd(elem_of((int)sizeof(T)), tn, dZ, W, V, dW, dV, dW != nullptr, dV != nullptr, B, N, L, C, v_batch_stride, offs);
  if (p.refused)
    return fail(PSF_E_TUNING, "dw_variant=2 forced but the chunk-looping dW kernel does not apply to N=%lld L=%d C=%lld",
                (long long)N, (int)L, (long long)C);
  if constexpr (sizeof(T) != 8) {
    constexpr bool bf = kIsBf16<T>;
    const int64_t w_total = B * N * (int64_t)L;
    if (p.fused != Fused::kNone) {
      const bool edge = p.fused == Fused::kEdge;
      BwdWinArgsT<T> a{dZ, W, dV, Geom{}, offs, w_total, edge, s};
      a.V2 = V;
      a.out2 = dW;
      a.wg_per_cu = p.wg_per_cu;
      if (int rc = make_geom(tn, B, N, L, C, VECW, p.fpk.tgs, p.fpk.TR, false, v_batch_stride, 0,
                             p.fpk.tiles_full + (p.fpk.ragged ? 1 : 0), &a.gm))
        return rc;
      a.gm.ileave = p.ileave;
      hipError_t e = launch_fused(edge, p.fpk.tgs, L, a);
      if (e != hipSuccess) return fail_hip(e, bf ? "chord_bwd_fused<bf16>" : edge ? "chord_bwd_fused_edge" : "chord_bwd_fused");
    }
    if (p.dw == Route::kChunk || p.dw == Route::kWindow) {
      BwdWinArgsT<T> a{dZ, V, dW, Geom{}, offs, w_total, false, s};
      int rc = window_launches(tn, p.dwpk, p.dw_all_edge, B, N, L, C, v_batch_stride, false, &a.gm, &a.edge,
                               [&] { return launch_dw(p.dw == Route::kChunk, p.dwpk, L, a); },
                               bf ? "chord_dw_win<bf16>" : p.dw == Route::kChunk ? "chord_dw_chunk" : "chord_dw_win", VECW);
      if (rc) return rc;
    }
    if (p.dv == Route::kWindow) {
      BwdWinArgsT<T> a{dZ, W, dV, Geom{}, offs, w_total, false, s};
      int rc = window_launches(tn, p.dvpk, p.dvpk.all_edge, B, N, L, C, N * C, true, &a.gm, &a.edge,
                               [&] { return launch_dv(p.dvpk, L, a); }, bf ? "chord_dv_win<bf16>" : "chord_dv_win", VECW);
      if (rc) return rc;
    }
  }

  if (p.dv == Route::kGeneric) {
    Geom gm;
    if (int rc = generic_geom(tn, B, N, L, C, p.dv_vec, true, N * C, &gm)) return rc;
    if (p.dv_vec != 1)
      hipLaunchKernelGGL((chord_dv_generic_k<T, VECW>), dim3(gm.nblocks), dim3(kBlock), 0, s, dZ, W, dV, gm, offs);
    else
      hipLaunchKernelGGL((chord_dv_generic_k<T, 1>), dim3(gm.nblocks), dim3(kBlock), 0, s, dZ, W, dV, gm, offs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "chord_dv_generic launch");
  }
  if (p.dw == Route::kGeneric) {
    Geom gm;
    if (int rc = generic_geom(tn, B, N, L, C, p.dw_vec, false, v_batch_stride, &gm)) return rc;
    if (p.dw_vec != 1)
      hipLaunchKernelGGL((chord_dw_generic_k<T, VECW>), dim3(gm.nblocks), dim3(kBlock), 0, s, dZ, V, dW, gm, offs);
    else
      hipLaunchKernelGGL((chord_dw_generic_k<T, 1>), dim3(gm.nblocks), dim3(kBlock), 0, s, dZ, V, dW, gm, offs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail_hip(e, "chord_dw_generic launch");
  }
  return PSF_OK;
}

// Bit m set: step m's result reaches memory. A buffer that a later step overwrites (inference ping-pong) need not be stored.
template <typename T>
uint64_t chain_store_mask(T* const* out_steps, int32_t M) {
  uint64_t mask = 0;
  for (int m = 0; m < M; ++m) {
    bool later = false;
    for (int q = m + 1; q < M; ++q) later = later || out_steps[q] == out_steps[m];
    if (!later) mask |= (uint64_t)1 << m;
  }
  return mask;
}

// Where the automatic route (chain_fused = 1) runs a chain in one launch; `few_kept`: at most two step results reach memory.
// f32. Every workgroup of a sequence streams the sequence's whole W: with `chunks` workgroups per sequence W crosses
// L2 -> CU `chunks` times and every output row is stored in `chunks` pieces. Past ~8 the per-step kernels win
// (profiles/r03n_chain_train_sweep.log, us per chain one launch / per step: ListOps N = 2000, C = 128, 32 chunks:
// 361 / 223; N = 2048, C = 64, 16 chunks: 184 / 119; Pathfinder C = 32, 4 chunks: 72 / 78). chain_fused = 2 forces it.
// Round 4 (the kernel built without SLP packing, profiles/r04al_chain_fused*.log, us per step, per-step / one launch):
// when only the last result is kept (inference: two alternating buffers) the one launch wins wherever it fits, wide rows
// included — N = 2000, C = 128: 18.6 / 15.1; N = 1024, C = 1024: 20.1 / 10.4; N = 2048, C = 64: 9.0 / 8.4 — and when every
// step is kept (training) it loses from 65536 elements per sequence on — N = 2048, C = 32: 6.9 / 10.3; C = 64: 10.2 / 17.2 —
// and wins below — N = 1024, C = 32: 7.1 / 5.6; N = 2048, C = 8: 6.9 / 4.3.
// Round 6: the workgroups of a sequence now share an XCD (fwd_chain_lds.h: W crosses the fabric once per sequence) — one
// launch, blockIdx order / XCD-aware, us per step-equivalent (profiles/r06u_chain_lds_xcd.log): N = 2000 x 128: 17.3 / 13.4;
// N = 2048 x 64: 9.5 / 6.8; Pathfinder 1024 x 32: 3.4 / 2.6; attention map 1024 x 1024: 9.8 / 8.9. With every step kept
// (training) it now wins up to 65 536 elements per sequence and, for N <= 1024, up to 131 072 (per step / one launch,
// r06u_chain_keep_sweep.log): 2048 x 32: 6.9 / 5.8; 1024 x 64: 6.7 / 4.0; 1024 x 128: 9.2 / 7.8; but 2048 x 64: 9.8 / 11.0;
// 2000 x 64: 10.5 / 10.8; 2000 x 128: 20.9 / 23.2.
// Later in round 6: 1057 <= N <= 2048 on launches of >= 256 workgroups run chord_chain_rows_k (two channel groups per
// workgroup: half the W streams). us per step, per-step launches / one group / two groups (profiles/r06v_chain_lds8_ab.log; lds8 = this kernel's first name):
// last kept: 2000 x 128: 19.3 / 13.5 / 8.0; 2048 x 64: 8.9 / 6.8 / 4.3; every step kept: 2000 x 128: 20.9 / 23.6 / 17.2;
// 2048 x 64: 9.7 / 11.0 / 8.9; 2000 x 64: 10.6 / 10.8 / 8.2; 2000 x 256: 37.7 / 39.5 / 32.6 - so with that instance the one
// launch also takes training chains (up to the 524 288 elements per sequence measured); ListOps training step 2.507 -> 2.476 ms.
// 2113 <= N <= 4160 (the LRA text task, N = 4097 x 32, B = 32: 256 workgroups) run the same kernel with one channel group and
// five rows per thread when only the last result is kept (profiles/r06v_chain_long_ab2.log, per-step / one launch):
// 13.0 / 7.2 us per step; 4096 x 32: 11.8 / 6.5; 3000 x 32: 9.6 / 5.4; with every step kept the per-step kernels stay
// (13.5 / 14.5), and below 256 workgroups too (B = 16: 7.4 / 6.6 last kept but 8.3 / 11.3 kept; C = 8: 6.4 / 6.6).
// bf16 (was chain_bf16_gate): bf16's own measurements, not the f32 gate
// (profiles/bf16_chain_ab.log, us per step, per-step launches / one launch, last result kept | every step kept):
//   ListOps 2000 x 128 (rows_k G = 2, 256 workgroups): 12.2 / 5.9 | 13.0 / 6.8;  2048 x 64 (lds_k CC = 1): 6.6 / 3.6 | 7.3 / 4.2;
//   Pathfinder 1024 x 32: 4.9 / 3.2 | 6.4 / 3.6;  attention map 1024 x 1024, broadcast eye: 9.8 / 6.3 | 11.0 / 6.7;
//   synthetic N = 128 / 1024 / 2048 x 8: 5.2 / 2.6, 5.1 / 2.2, 4.8 / 3.1 | 6.4 / 3.8, 6.3 / 3.6, 6.2 / 3.5.
// So, unlike f32, keeping every step costs the one launch nothing against the per-step route (its stores are the per-step
// kernels' stores), and it is taken for every instance up to the 1 048 576 elements per sequence measured, EXCEPT the
// long-row instance (rows_k G = 1, 2113 <= N <= 4160): the text task 4097 x 32 has 4 channel groups, so 128 workgroups of
// 832 threads at B = 32 — half the CUs idle: 9.3 / 9.0 | 10.0 / 9.6, inside the rounds' spread when the last result is kept;
// B = 16: 6.0 / 8.9 | 6.4 / 9.5, a loss. No bf16 launch of that instance with >= 256 workgroups has been measured, so it
// is never automatic (chain_fused = 2 with chain_cc = 2 runs it).
bool chain_gate(const Elem& el, const ChainLdsPlan& plan, int64_t N, int64_t C, bool few_kept) {
  if (el.bytes == 2) return plan.big != 2 && N * C <= 1048576;
  return few_kept || N * C <= 65536 || (N <= 1024 && N * C <= 131072) || (plan.big == 1 && N * C <= 524288);
}

struct ChainPlan {
  bool one_launch;  // short sequences: the whole chain in ONE launch with the sequence's X slice resident in LDS (`lds`)
  bool grid_ok;     // ... whose B * chunks workgroups fit a grid
  ChainLdsPlan lds;
};

// The one launch needs C a multiple of the 16-byte group, V0 and every stored result 16-byte aligned, and W rows that whole
// aligned dwords cover: a 4-byte-aligned W, or in bf16 (ceil(L / 2) dwords per row) any 2-byte-aligned W for odd L. Anything
// else takes the per-step launches. W_steps == nullptr (describe): operands taken as aligned.
template <typename T>
ChainPlan plan_chain(const Elem& el, const Tuning& tn, const T* const* W_steps, const T* V0, T* const* out_steps, int32_t M,
                     bool few_kept, int64_t B, int64_t N, int32_t L, int64_t C) {
  ChainPlan p{};
  const int cf = tn.chain_fused;
  bool ok = el.window && cf && M >= 2 && M <= kChainMaxSteps && B >= 1 && plan_chain_lds(N, C, L, M, &p.lds, tn.chain_cc, B, el.bytes) &&
            (cf == 2 || chain_gate(el, p.lds, N, C, few_kept)) && aligned_to(V0, 16);
  const size_t w_align = el.bytes == 2 && L % 2 ? 2 : 4;
  for (int m = 0; ok && W_steps && m < M; ++m) ok = aligned_to(W_steps[m], w_align) && aligned_to(out_steps[m], 16);
  p.one_launch = ok;
  p.grid_ok = ok && B * (int64_t)p.lds.chunks <= 0x7fffffff;
  return p;
}

template <typename T>
int chain_impl(Tuning tn, const T* const* W_steps, const T* V0, T* const* out_steps, int32_t M, int32_t use_residual,
               int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride, const int64_t* offsets,
               void* stream) {
  if (M < 0) return fail(PSF_E_SHAPE, "M must be >= 0");
  if (M == 0) return PSF_OK;
  if (!W_steps || !out_steps || !V0) return fail(PSF_E_NULL, "W_steps, out_steps and V0 must be non-NULL");
  if (use_residual && v0_batch_stride == 0 && B != 1)
    return fail(PSF_E_SHAPE, "a broadcast V0 cannot be the residual");
  for (int m = 0; m < M; ++m) {
    if (!W_steps[m] || !out_steps[m]) return fail(PSF_E_NULL, "step %d: NULL pointer", m);
    if (use_residual && out_steps[m] == V0) return fail(PSF_E_ALIAS, "step %d: out aliases the residual V0", m);
    if (out_steps[m] == (m == 0 ? V0 : out_steps[m - 1]))
      return fail(PSF_E_ALIAS, "step %d: out aliases the step's input", m);
  }

  if constexpr (sizeof(T) != 8) {  // the one launch: f32 (fwd_chain_lds.h) and bf16 (fwd_chain_lds_bf16.h: 8 channels per
                                   // 16-byte LDS slot, bit-identical to the per-step bf16 kernels)
    const uint64_t store_mask = M <= kChainMaxSteps ? chain_store_mask(out_steps, M) : ~(uint64_t)0;
    const ChainPlan p = plan_chain(elem_of((int)sizeof(T)), tn, W_steps, V0, out_steps, M, __builtin_popcountll(store_mask) <= 2, B, N, L, C);
    if (p.one_launch && p.grid_ok) {
      if (int rc = check_dims(B, N, L, C, v0_batch_stride)) return rc;
      std::conditional_t<kIsBf16<T>, ChainArgsBf16, ChainArgs> a;
      for (int m = 0; m < kChainMaxSteps; ++m) {
        a.W[m] = m < M ? W_steps[m] : nullptr;
        a.out[m] = m < M ? out_steps[m] : nullptr;
      }
      a.store_mask = store_mask;
      a.V0 = V0;
      a.v0_bstride = v0_batch_stride;
      a.M = M;
      a.N = (int32_t)N;
      a.C = (int32_t)C;
      a.CG = (int32_t)(C / (16 / (int)sizeof(T)));
      a.chunks = p.lds.chunks;
      a.xcd_remap = tn.xcd_remap && p.lds.chunks > 1 ? 1 : 0;  // (one workgroup per sequence shares nothing with its neighbours)
      Offsets offs;
      make_offsets(N, L, offsets, &offs);
      hipStream_t s = reinterpret_cast<hipStream_t>(stream);
      if constexpr (kIsBf16<T>) {
        hipError_t e = launch_chain_lds_bf16(p.lds, L, use_residual != 0, a, offs, (int)B, s);
        if (e != hipSuccess) return fail_hip(e, "chord_chain_lds<bf16> launch");
      } else {
        hipError_t e = launch_chain_lds(p.lds, L, use_residual != 0, a, offs, (int)B, s);
        if (e != hipSuccess) return fail_hip(e, "chord_chain_lds launch");
      }
      return PSF_OK;
    }
  }

  for (int m = 0; m < M; ++m) {
    const T* in = m == 0 ? V0 : out_steps[m - 1];
    const int64_t stride = m == 0 ? v0_batch_stride : N * C;
    // zigzag: every XCD walks its tile range forwards on even steps and backwards on odd ones, so a launch begins
    // with the tiles whose inputs the previous launch wrote LAST (still in that XCD's L2), not first
    tn.walk_backwards = (m & 1) != 0;
    int rc = fwd_impl<T>(tn, W_steps[m], in, use_residual ? V0 : nullptr, out_steps[m], B, N, L, C, stride, offsets, stream);
    if (rc) return rc;
  }
  return PSF_OK;
}

// The backward chain in one library call (K = float or __bf16). f32 runs the one-launch kernel where it fits
// (bwd_chain_lds.h; the one-launch bf16 kernel has an entry of its own, psf_chord_chain_bwd_lds_bf16 below). Otherwise the M per-step launches of psf_chord_spmm_bwd_*
// (the fused step where it applies), the gradient handed from dX_steps[m] to the next step, and ONE psf_sum_tensors_* pass over
// the residual terms at the end — ((g_M + g_{M-1}) + ... + g_1) + g_0, in bf16 summed in f32 and rounded once: what the
// caller's loop (chord.py) did, without M trips through its language's FFI.
template <typename K>
int chain_bwd_impl(const K* dOut, const K* const* W_steps, const K* V0, const K* const* X_steps, K* const* dW_steps, K* dV0,
                   K* const* dX_steps, int32_t M, int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C,
                   const int64_t* offsets, void* stream) {
  constexpr int VECW = 16 / (int)sizeof(K);
  if (M < 1) return fail(PSF_E_SHAPE, "M must be >= 1");
  if (!dOut || !W_steps || !V0 || !X_steps || !dW_steps || !dV0) return fail(PSF_E_NULL, "a required pointer is NULL");
  if (int rc = check_dims(B, N, L, C, N * C)) return rc;
  const Tuning tn = snapshot();
  if (!tn.chain_bwd_fused) return PSF_E_UNSUPPORTED;  // (knob off: the caller runs the steps itself)
  const bool one_launch = !kIsBf16<K> && chain_bwd_lds_fits(N, C, L, M);
  // the per-step path inside the library needs the M gradient buffers and, with the residual, psf_sum_tensors_*'s limits
  if (!one_launch && (!dX_steps || (use_residual && (M + 1 > 32 || (B * N * C) % VECW != 0)))) return PSF_E_UNSUPPORTED;
  if (B == 0) return PSF_OK;
  for (int m = 0; m < M; ++m) {
    const K* x = m == 0 ? V0 : X_steps[m];
    if (!W_steps[m] || !x || !dW_steps[m]) return fail(PSF_E_NULL, "step %d: NULL pointer", m);
    if (dW_steps[m] == W_steps[m]) return fail(PSF_E_ALIAS, "step %d: dW aliases W", m);
    if (!one_launch && !dX_steps[m]) return fail(PSF_E_NULL, "step %d: dX_steps[m] is NULL", m);
  }
  if constexpr (!kIsBf16<K>) {
    if (one_launch) {
      if (B > 0x7fffffff) return fail(PSF_E_SHAPE, "B too large");
      ChainBwdArgs a;
      for (int m = 0; m < M; ++m) {
        const float* x = m == 0 ? V0 : X_steps[m];
        if (!aligned_to(W_steps[m], 4) || !aligned_to(dW_steps[m], 4) || !aligned_to(x, 16))
          return fail(PSF_E_ALIGN, "step %d: W / dW must be 4-byte, X 16-byte aligned", m);
        a.W[m] = W_steps[m], a.X[m] = x, a.dW[m] = dW_steps[m];
      }
      for (int m = M; m < kChainMaxSteps; ++m) a.W[m] = nullptr, a.X[m] = nullptr, a.dW[m] = nullptr;
      if (!aligned_to(dOut, 16) || !aligned_to(dV0, 16)) return fail(PSF_E_ALIGN, "dOut and dV0 must be 16-byte aligned");
      a.dOut = dOut, a.dV0 = dV0, a.M = M, a.N = (int32_t)N, a.C = (int32_t)C;
      Offsets offs;
      make_offsets(N, L, offsets, &offs);
      hipError_t e = launch_chain_bwd_lds(L, (int)(C / 4), use_residual != 0, a, offs, (int)B, reinterpret_cast<hipStream_t>(stream));
      if (e != hipSuccess) return fail_hip(e, "chord_chain_bwd_lds launch");
      return PSF_OK;
    }
  }
  const K* g = dOut;
  const K* terms[kChainMaxSteps + 1];
  int nterms = 0;
  for (int m = M - 1; m >= 0; --m) {
    if (use_residual) terms[nterms++] = g;
    K* dx = (m == 0 && !use_residual) ? dV0 : dX_steps[m];
    if (int rc = bwd_impl<K>(tn, g, W_steps[m], m == 0 ? V0 : X_steps[m], dW_steps[m], dx, B, N, L, C, N * C, offsets, stream))
      return rc;
    g = dx;
  }
  if (use_residual) {
    terms[nterms++] = g;  // ((g_M + g_{M-1}) + ... + g_1) + g_0
    if constexpr (kIsBf16<K>)
      return psf_sum_tensors_bf16(reinterpret_cast<const uint16_t* const*>(terms), nterms, B * N * C, reinterpret_cast<uint16_t*>(dV0), stream);
    else
      return psf_sum_tensors_f32(terms, nterms, B * N * C, dV0, stream);
  }
  return PSF_OK;
}

// The transposed chain Y_m = W_m^T (.) Y_{m+1}, m = M-1 .. 0 (K = float or __bf16): rows of the attention map. One launch
// where chain_tr_lds.h covers the shape; otherwise the M per-step dV launches of psf_chord_spmm_bwd_* (dW = NULL), taking
// turns between `scratch` and `out` so that step 0 writes `out`. Same bits either way.
template <typename K>
int chain_tr_impl(const K* const* W_steps, const K* Q, K* out, K* scratch, int32_t M, int64_t B, int64_t N, int32_t L, int64_t R,
                  const int64_t* offsets, void* stream) {
  constexpr int VECW = 16 / (int)sizeof(K);
  if (M < 1) return fail(PSF_E_SHAPE, "M must be >= 1");
  if (!W_steps || !Q || !out) return fail(PSF_E_NULL, "a required pointer is NULL");
  if (int rc = check_dims(B, N, L, R, N * R)) return rc;
  if (R % VECW != 0) return fail(PSF_E_SHAPE, "R=%lld must be a multiple of %d", (long long)R, VECW);
  const bool one_launch = chain_tr_lds_fits(N, L, R, M, (int)sizeof(K)) && B * ((R / VECW + kChainTrGroups - 1) / kChainTrGroups) <= 0x7fffffff;
  if (!one_launch && M > 1 && !scratch) return PSF_E_UNSUPPORTED;  // (the per-step route needs the second buffer)
  if (B == 0) return PSF_OK;
  for (int m = 0; m < M; ++m)
    if (!W_steps[m]) return fail(PSF_E_NULL, "step %d: NULL pointer", m);
  if (out == Q || (scratch && (scratch == Q || scratch == out))) return fail(PSF_E_ALIAS, "Q, out and scratch must be distinct");
  for (int m = 0; m < M; ++m)
    if (!aligned_to(W_steps[m], sizeof(K))) return fail(PSF_E_ALIGN, "step %d: W must be %d-byte aligned", m, (int)sizeof(K));
  if (!aligned_to(Q, 16) || !aligned_to(out, 16) || (scratch && !aligned_to(scratch, 16)))
    return fail(PSF_E_ALIGN, "Q, out and scratch must be 16-byte aligned");
  if (one_launch) {
    ChainTrArgs<K> a;
    for (int m = 0; m < kChainMaxSteps; ++m) a.W[m] = m < M ? W_steps[m] : nullptr;
    a.Q = Q, a.out = out, a.M = M, a.N = (int32_t)N, a.R = (int32_t)R;
    a.CG = (int32_t)(R / VECW), a.chunks = (a.CG + kChainTrGroups - 1) / kChainTrGroups;
    Offsets offs;
    make_offsets(N, L, offsets, &offs);
    hipError_t e = launch_chain_tr_lds(L, a, offs, B, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail_hip(e, kIsBf16<K> ? "chord_chain_tr_lds<bf16> launch" : "chord_chain_tr_lds launch");
    return PSF_OK;
  }
  const Tuning tn = snapshot();
  const K* y = Q;
  for (int m = M - 1; m >= 0; --m) {
    K* dst = (m & 1) ? scratch : out;  // step 0 writes out
    if (int rc = bwd_impl<K>(tn, y, W_steps[m], nullptr, nullptr, dst, B, N, L, R, N * R, offsets, stream)) return rc;
    y = dst;
  }
  return PSF_OK;
}

// ------------------------------------------------------------------------------------------------------
// the mixer with W computed inside the step (fwd_mlp_step.h)
// ------------------------------------------------------------------------------------------------------
enum class MixerRoute { kNone, kLds, kSteps };  // kNone: only the LDS-resident kernel covers the shape and this snapshot keeps it away
struct MixerPlan {
  bool covered;      // one of the two kernel families covers the shape (psf_mixer_fwd_workspace() >= 0)
  int units;         // packed images over all M + 1 MLPs
  int64_t ws_bytes;  // ... in bytes; -1 when not covered
  MixerRoute route;  // kLds: the single-launch LDS-resident kernel (mixer_lds.h, `lds`); kSteps: the per-step kernels (fwd_mlp_step.h)
  MixerLdsPlan lds;
  WinPick pk;        // kSteps: the tiles of every launch, pk.all_edge for the M steps
  bool g_all_edge;   // ... and for the g launch
};

// The mixer of one shape under one snapshot. Mirrors the limits stated in include/psf_chord.h. B enters the route (the LDS
// kernel's grid) and the tile decision only: the queries, which have no B, plan with B = 1.
MixerPlan plan_mixer(const Tuning& tn, int64_t B, int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  MixerPlan p{};
  p.ws_bytes = -1;
  if (!h || M < 1 || M > 31 || E < 4 || E > 32 || (E & 3) || C < 4 || C > 32 || (C & 3) || L < kMlpStepLmin || L > kMlpStepLmax ||
      N < 1 || N > (int64_t)1 << 30)
    return p;
  int units = 0, nu_max = 0;
  for (int k = 0; k <= M; ++k) {
    if (h[k] < 1 || h[k] > 128) return p;
    const int nu = (h[k] + 31) / 32;
    units += nu, nu_max = nu > nu_max ? nu : nu_max;
  }
  if (units > 128) return p;
  const bool lds_ok = plan_mixer_lds(N, C, L, M, nu_max, &p.lds);
  const int tgs = ceil_log2(C / 4), TR = tgs <= kMlpStepTgsMax ? mlp_step_tile_rows(tgs) : 0;
  Offsets offs;
  make_offsets(N, L, nullptr, &offs);
  const int KN = TR && N >= 2 * (int64_t)TR ? near_links(TR, L, offs) : 0;  // (the window may wrap at most once) 0: no per-step kernel
  if (!lds_ok && !KN) return p;
  p.covered = true, p.units = units, p.ws_bytes = (int64_t)units * kX3ImageBytes;
  p.route = lds_ok && tn.mixer_lds && B <= 0x7fffffff ? MixerRoute::kLds : KN ? MixerRoute::kSteps : MixerRoute::kNone;
  if (p.route != MixerRoute::kSteps) return p;
  // the tile geometry of every per-step launch
  set_pick(&p.pk, tgs, mlp_step_rows(tgs), 256, TR, KN, N);
  const int TG = 1 << tgs;
  // The step kernel's full-tile instance takes every row block as TR-aligned (scalar block addresses, fwd_mlp_step.h): N and
  // every far offset multiples of TR, rows of exactly 4 TG channels, a batch element under 2^31 bytes; anything else runs the
  // predicated instance on every tile. (ragged_in_one_launch's E: this step moves the data row, not the W row.)
  bool blocks_aligned = (N % TR) == 0 && C == 4 * (int64_t)TG && N * C * 4 < ((int64_t)1 << 31) && N * (int64_t)E * 4 < ((int64_t)1 << 31);
  for (int k = KN; k < L; ++k) blocks_aligned = blocks_aligned && (offs.v[k] % TR) == 0;
  // (the entry plans before it has looked at B: one that it then turns away, B < 0 or B * N > 2^40, stays out of the product)
  const int64_t Bt = B < 0 || B > ((int64_t)1 << 40) / N ? 0 : B;
  p.pk.all_edge = !blocks_aligned || !tn.fwd_split || ragged_in_one_launch(tn, p.pk.ragged, Bt, N, E, C);
  p.g_all_edge = p.pk.ragged && p.pk.all_edge;  // the g kernel needs its predicate only for rows >= N
  return p;
}

// The bf16 mixer has the single launch only (mixer_lds_bf16.h): its limits (plan_mixer_lds_bf16) and the knob.
struct MixerBf16Plan {
  bool covered, run;  // inside the limits; ... and mixer_lds lets it run
  int64_t ws_bytes;   // -1 when not covered
  MixerLdsBf16Plan lds;
};

MixerBf16Plan plan_mixer_bf16(const Tuning& tn, int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  MixerBf16Plan p{};
  p.covered = plan_mixer_lds_bf16(N, E, M, h, C, L, &p.lds);
  p.run = p.covered && tn.mixer_lds;
  p.ws_bytes = p.covered ? (int64_t)p.lds.units * psf_mlp_bf16::kImgBytes : -1;
  return p;
}

// The four layer tables of mixer entry `who`: every MLP's pointers non-NULL and aligned to `align` bytes (1: not looked at).
template <typename T>
int check_layer_tables(const char* who, const T* const* A, const T* const* a, const T* const* Bw, const T* const* b, int32_t M, size_t align) {
  for (int k = 0; k <= M; ++k) {
    if (!A[k] || !a[k] || !Bw[k] || !b[k]) return fail(PSF_E_NULL, "%s: NULL layer pointer (MLP %d)", who, k);
    if (!aligned_to(A[k], align) || !aligned_to(a[k], align) || !aligned_to(Bw[k], align) || !aligned_to(b[k], align))
      return fail(PSF_E_ALIGN, "%s: weights and biases must be %d-byte aligned (MLP %d)", who, (int)align, k);
  }
  return PSF_OK;
}

// ... and its step outputs: non-NULL, 16-byte aligned, none of them V0 or its own step's input.
template <typename T>
int check_out_steps(const char* who, T* const* out_steps, const T* V0, int32_t M) {
  for (int m = 0; m < M; ++m) {
    if (!out_steps[m]) return fail(PSF_E_NULL, "%s: step %d: NULL output", who, m);
    if (!aligned_to(out_steps[m], 16)) return fail(PSF_E_ALIGN, "%s: step %d: output not 16-byte aligned", who, m);
    if (out_steps[m] == V0) return fail(PSF_E_ALIAS, "%s: step %d: out aliases V0", who, m);
    if (m > 0 && out_steps[m] == out_steps[m - 1]) return fail(PSF_E_ALIAS, "%s: step %d: out aliases the step's input", who, m);
  }
  return PSF_OK;
}

int mixer_impl(Tuning tn, const psf_mixer_input* in, int64_t B, int64_t N, int32_t E, int32_t M, const float* const* A,
               const float* const* a, const float* const* Bw, const float* const* b, const int32_t* h, int64_t C, int32_t L,
               int32_t use_residual, float* V0, float* const* out_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!in || !in->src || !A || !a || !Bw || !b || !h || !V0 || !out_steps || !workspace)
    return fail(PSF_E_NULL, "psf_mixer_fwd: NULL argument");
  MixerIn mi;
  mi.src = in->src, mi.weight = in->weight, mi.bias = in->bias, mi.pos = in->pos, mi.kind = in->kind, mi.K = in->K;
  if (in->kind == PSF_MIXER_IN_DATA) {
    mi.weight = mi.bias = mi.pos = nullptr, mi.K = 0;
    if (!aligned_to(in->src, 16)) return fail(PSF_E_ALIGN, "psf_mixer_fwd: X must be 16-byte aligned");
  } else if (in->kind == PSF_MIXER_IN_AFFINE) {
    if (in->K < 1 || in->K > 3) return fail(PSF_E_SHAPE, "psf_mixer_fwd: the affine input takes 1..3 values per position (K=%d)", (int)in->K);
    if (!in->weight) return fail(PSF_E_NULL, "psf_mixer_fwd: affine input without a weight");
    if (!aligned_to(in->src, 4) || !aligned_to(in->weight, 4) || (in->bias && !aligned_to(in->bias, 4)))
      return fail(PSF_E_ALIGN, "psf_mixer_fwd: affine input pointers must be 4-byte aligned");
  } else if (in->kind == PSF_MIXER_IN_TOKENS) {
    if (in->K < 1) return fail(PSF_E_SHAPE, "psf_mixer_fwd: empty vocabulary");
    if (!in->weight) return fail(PSF_E_NULL, "psf_mixer_fwd: token input without a table");
    if (!aligned_to(in->src, 8) || !aligned_to(in->weight, 16))
      return fail(PSF_E_ALIGN, "psf_mixer_fwd: tokens must be 8-byte, the table 16-byte aligned");
    mi.bias = nullptr;
  } else {
    return fail(PSF_E_SHAPE, "psf_mixer_fwd: unknown input kind %d", (int)in->kind);
  }
  if (mi.pos && !aligned_to(mi.pos, 16)) return fail(PSF_E_ALIGN, "psf_mixer_fwd: pos must be 16-byte aligned");
  const MixerPlan mp = plan_mixer(tn, B, N, E, M, h, C, L);
  if (!mp.covered)
    return fail(PSF_E_SHAPE, "psf_mixer_fwd: shape outside the fused path (N=%lld E=%d M=%d C=%lld L=%d; see psf_mixer_fwd_workspace)",
                (long long)N, (int)E, (int)M, (long long)C, (int)L);
  if (int rc = check_dims(B, N, L, C, N * C)) return rc;
  if (in->kind != PSF_MIXER_IN_DATA && mp.route != MixerRoute::kLds)  // (before anything is launched)
    return fail(PSF_E_SHAPE, "psf_mixer_fwd: an input recipe (kind %d) is evaluated by the single-launch kernel only (short sequences, "
                "psf_mixer_fwd_plan() == 2); for N=%lld write the rows with psf_affine_rows_f32 / psf_embed_tokens_f32 and pass them",
                (int)in->kind, (long long)N);
  if (B == 0) return PSF_OK;
  if (workspace_bytes < mp.ws_bytes || !aligned_to(workspace, 16))
    return fail(PSF_E_SHAPE, "psf_mixer_fwd: workspace too small (psf_mixer_fwd_workspace) or not 16-byte aligned");
  if (!aligned_to(V0, 16)) return fail(PSF_E_ALIGN, "psf_mixer_fwd: V0 must be 16-byte aligned");
  if (B * N > (int64_t)1 << 40) return fail(PSF_E_SHAPE, "psf_mixer_fwd: B*N too large");
  if (int rc = check_layer_tables("psf_mixer_fwd", A, a, Bw, b, M, 1)) return rc;
  if (int rc = check_out_steps<float>("psf_mixer_fwd", out_steps, V0, M)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // (1) all M + 1 weight sets -> unit images (one launch)
  int32_t O[32], first_unit[33];
  for (int k = 0; k <= M; ++k) O[k] = k ? L : (int32_t)C;
  hipError_t e = psf_x3_pack_launch(E, M + 1, A, a, Bw, b, h, O, workspace, first_unit, s);
  if (e != hipSuccess) return fail_hip(e, "psf_mixer_fwd: pack");
  Offsets offs;
  make_offsets(N, L, nullptr, &offs);
  if (mp.route == MixerRoute::kLds) {  // short sequences: the whole mixer in ONE launch, V resident in LDS
    MixerLdsArgs la;
    la.in = mi, la.images = reinterpret_cast<const unsigned char*>(workspace), la.V0 = V0;
    for (int k = 0; k <= M + 1; ++k) la.first_unit[k] = first_unit[k];
    for (int m = 0; m < kMixerLdsMaxSteps; ++m) la.out[m] = m < M ? out_steps[m] : nullptr;
    la.store_mask = (uint32_t)chain_store_mask(out_steps, M);  // a buffer that a later step overwrites (two-buffer inference) is not stored at all
    la.M = M, la.N = (int32_t)N, la.C = (int32_t)C, la.E = E, la.L = L, la.CG = (int32_t)(C / 4), la.WS = mp.lds.WS;
    la.TT = (int32_t)(N / 32), la.nu_max = mp.lds.nu_max;
    e = launch_mixer_lds(mp.lds, use_residual != 0, la, offs, (int)B, s);
    return e == hipSuccess ? PSF_OK : fail_hip(e, "chord_mixer_lds launch");
  }
  if (mp.route == MixerRoute::kNone)
    return fail(PSF_E_TUNING, "psf_mixer_fwd: mixer_lds=0 but only the LDS-resident kernel covers N=%lld C=%lld", (long long)N, (long long)C);
  const WinPick& pk = mp.pk;
  const unsigned char* images = reinterpret_cast<const unsigned char*>(workspace);
  FwdMlpArgs fa;  // (gm and edge are window_launches')
  fa.in = mi, fa.E = E, fa.offs = offs, fa.stream = s;
  // (2) V0 = g(data): the matrix phase alone, on the same tiles
  fa.V = fa.res = nullptr, fa.out = V0, fa.images = images, fa.nu = first_unit[1] - first_unit[0], fa.wg_per_cu = 0;
  if (int rc = window_launches(tn, pk, mp.g_all_edge, B, N, L, C, N * C, false, &fa.gm, &fa.edge,
                               [&] { return with_int<0, kMlpStepTgsMax>(pk.tgs, [&](auto t) { return launch_mixer_g<t()>(fa); }); }, "chord_mixer_g launch"))
    return rc;
  for (int m = 0; m < M; ++m) {  // (3) the M steps
    fa.V = m == 0 ? V0 : out_steps[m - 1], fa.res = use_residual ? V0 : nullptr, fa.out = out_steps[m];
    fa.images = images + (size_t)first_unit[m + 1] * kX3ImageBytes, fa.nu = first_unit[m + 2] - first_unit[m + 1];
    fa.wg_per_cu = tn.mixer_wg_limit;
    tn.walk_backwards = (m & 1) != 0;  // zigzag, as chain_impl
    if (int rc = window_launches(tn, pk, pk.all_edge, B, N, L, C, N * C, false, &fa.gm, &fa.edge,
                                 [&] { return with_int<0, kMlpStepTgsMax>(pk.tgs, [&](auto t) { return launch_fwd_mlp<t()>(L, fa); }); }, "chord_fwd_mlp launch"))
      return rc;
  }
  return PSF_OK;
}

int mixer_bf16_impl(const Tuning& tn, const uint16_t* X, int64_t B, int64_t N, int32_t E, int32_t M, const uint16_t* const* A,
                    const uint16_t* const* a, const uint16_t* const* Bw, const uint16_t* const* b, const int32_t* h, int64_t C, int32_t L,
                    int32_t use_residual, uint16_t* V0, uint16_t* const* out_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!X || !A || !a || !Bw || !b || !h || !out_steps || !workspace) return fail(PSF_E_NULL, "psf_mixer_fwd_bf16: NULL argument");
  if (B < 0 || B > 0x7fffffff) return fail(PSF_E_SHAPE, "psf_mixer_fwd_bf16: need 0 <= B < 2^31 (got B=%lld)", (long long)B);
  const MixerBf16Plan mp = plan_mixer_bf16(tn, N, E, M, h, C, L);
  if (!mp.covered)
    return fail(PSF_E_UNSUPPORTED, "psf_mixer_fwd_bf16: no kernel for N=%lld E=%d M=%d C=%lld L=%d (psf_mixer_fwd_bf16_plan): run "
                "psf_mlp_fwd_bf16 and psf_chord_chain_fwd_bf16", (long long)N, (int)E, (int)M, (long long)C, (int)L);
  if (!mp.run) return fail(PSF_E_UNSUPPORTED, "psf_mixer_fwd_bf16: mixer_lds=0 takes the single-launch mixer away");
  if (!aligned_to(X, 16)) return fail(PSF_E_ALIGN, "psf_mixer_fwd_bf16: X must be 16-byte aligned");
  if (V0 && !aligned_to(V0, 16)) return fail(PSF_E_ALIGN, "psf_mixer_fwd_bf16: V0 must be 16-byte aligned");
  if (workspace_bytes < mp.ws_bytes || !aligned_to(workspace, 16))
    return fail(PSF_E_SHAPE, "psf_mixer_fwd_bf16: workspace too small (psf_mixer_fwd_bf16_workspace) or not 16-byte aligned");
  if (int rc = check_layer_tables("psf_mixer_fwd_bf16", A, a, Bw, b, M, 2)) return rc;
  if (int rc = check_out_steps<uint16_t>("psf_mixer_fwd_bf16", out_steps, V0, M)) return rc;
  if (B == 0) return PSF_OK;
  int32_t O[32];
  for (int k = 0; k <= M; ++k) O[k] = k ? L : (int32_t)C;
  psf_mlp_bf16::Args pack;
  if (!psf_mlp_bf16::make_plan(E, M + 1, h, O, pack.unit, &pack.U)) return fail(PSF_E_SHAPE, "psf_mixer_fwd_bf16: unit plan");
  for (int k = 0; k < psf_mlp_bf16::kMaxK; ++k)
    pack.m[k] = k <= M ? psf_mlp_bf16::Mlp{A[k], a[k], Bw[k], b[k], nullptr, h[k], O[k]} : psf_mlp_bf16::Mlp{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  pack.X = X, pack.images = reinterpret_cast<unsigned char*>(workspace), pack.T = B * N, pack.E = E;
  MixerLdsBf16Args la;
  la.X = X, la.images = pack.images, la.V0 = V0, la.first_unit[0] = 0;
  for (int k = 0; k <= M; ++k) la.first_unit[k + 1] = la.first_unit[k] + (h[k] + 31) / 32;
  for (int m = 0; m < kMixerLdsBf16MaxSteps; ++m) la.out[m] = m < M ? out_steps[m] : nullptr;
  la.store_mask = (uint32_t)chain_store_mask(out_steps, M);  // a buffer that a later step overwrites is not stored at all
  la.M = M, la.N = (int32_t)N, la.C = (int32_t)C, la.E = E, la.L = L, la.CG = (int32_t)(C / 8), la.WS = mp.lds.WS, la.TT = (int32_t)(N / 32);
  Offsets offs;
  make_offsets(N, L, nullptr, &offs);
  const hipError_t e = launch_mixer_lds_bf16(mp.lds, use_residual != 0, pack, la, offs, (int)B, reinterpret_cast<hipStream_t>(stream));
  return e == hipSuccess ? PSF_OK : fail_hip(e, "chord_mixer_lds<bf16> launch");
}

// psf_describe_*: argument checks, and the name of a window-kernel instance
int describe_args(int64_t B, int64_t N, int32_t L, int64_t C, int32_t elem_bytes, bool f64, const char* buf, int32_t cap) {
  if (!buf || cap < 1) return fail(PSF_E_NULL, "buf is NULL");
  if (int rc = check_dims(B, N, L, C, N * C)) return rc;
  if (elem_bytes != 2 && elem_bytes != 4 && !(f64 && elem_bytes == 8))
    return fail(PSF_E_SHAPE, f64 ? "elem_bytes must be 2 (bf16), 4 or 8" : "elem_bytes must be 2 (bf16) or 4");
  return PSF_OK;
}

// The last-result chain of a long f32 sequence in one launch (fwd_chain_regs.h): what psf_chord_chain_last_f32 runs, what
// psf_chord_chain_last_supported answers and what psf_describe_chain_last prints. `fits`: the kernel covers the call (the
// entry launches it); `automatic`: the caller should prefer the entry to psf_chord_chain_fwd_f32 — knob chain_fused = 2
// wherever it fits, chain_fused = 1 where the grid fills its rounds of one workgroup per CU (chain_regs_automatic,
// fwd_chain_regs_launch.h), chain_fused = 0 never.
struct ChainLastPlan {
  bool fits, automatic;
  int cus;
};
// CUs of the calling thread's current device; the MI355X's 256 where no device answers (a host without a GPU)
int current_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    (void)hipGetLastError();  // (not this call's business: the next launch must not find it)
    return kChainRegsDefaultCus;
  }
  return cus;
}
ChainLastPlan plan_chain_last(const Tuning& tn, int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t w_align,
                              bool use_residual, int64_t v0_batch_stride, bool default_offsets) {
  ChainLastPlan p{};
  p.fits = default_offsets && chain_regs_fits(B, N, L, C, M) && w_align >= 16 && w_align % 16 == 0 &&
           (v0_batch_stride == N * C || (v0_batch_stride == 0 && !use_residual));
  p.cus = p.fits && tn.chain_fused == 1 ? current_cus() : kChainRegsDefaultCus;
  p.automatic = p.fits && (tn.chain_fused == 2 || (tn.chain_fused == 1 && chain_regs_automatic(B * (C / 2), p.cus)));
  return p;
}

void print_win(char* buf, size_t cap, const char* kernel, const Elem& el, int32_t L, const WinPick& pk) {
  snprintf(buf, cap, "%s<%s,L=%d,TG=%d,R=%d,NT=%d>", kernel, el.name, (int)L, 1 << pk.tgs, pk.rows, pk.nt);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------
// extern "C"
// ------------------------------------------------------------------------------------------------------
// Other translation units of the library report through the same thread-local string (not part of the ABI).
extern "C" int psf_internal_fail(int code, const char* message) { return fail(code, "%s", message); }

extern "C" {

int psf_version(void) { return PSF_ABI_VERSION; }

const char* psf_last_error(void) { return g_err; }

const char* psf_build_info(void) {
  return "libpsf_chord: gfx950 (CDNA4, wave64) | hipcc " __VERSION__
         " | fwd: generic<f32,f64> + LDS-window<f32, L=4..20, LDS-DMA staging> + LDS-resident chain<f32, N<=2112; whole rows per thread: 8 channels N<=2048, 4 channels N<=4160>"
         " | bwd: generic dV/dW<f32,f64> + LDS-window dV/dW<f32> + fused dV+dW step<f32, C<=64; C=128 up to N=4096>"
         " | producers: fused MLP fwd (split-bf16 MFMA at f32 accuracy, f32 MFMA) + fused MLP bwd (split-bf16 MFMA on dual-use LDS planes, f32 MFMA),"
         " tall-skinny weight gradients (f32 MFMA), token embedding + positional add"
         ", wide producer MLPs (E <= 1024: stacked first layers as split-bf16 GEMMs from bf16 term planes, LDS-DMA ring)"
         " | mixer: W_m computed inside the chain step (per-step kernels; one LDS-resident launch for short sequences)"
         " | bf16 chord path: f32 accumulation, one rounding per element; fwd: generic + LDS-window<bf16, TG<=16, NT=256, R=2>; bwd: fused dV+dW step<bf16, TG<=16, NT=256> (aligned full tiles), LDS-window dV<R=2> / dW<R=1><bf16, TG<=16> + generic;"
         " backward chain issued by the library (per-step launches)"
         " | bf16 producers: fused MLP fwd<bf16> (one MFMA term, hidden layer in registers, E <= 64) + fused MLP bwd<bf16> (one MFMA"
         " term on dual-use LDS planes, the roundings of bf16 autograd, E <= 32; training route opt-in)"
         " | bf16 mixer: one LDS-resident launch for short sequences (N <= 512, C = 8 or 16), the bits of the two-call route"
         " | arithmetic of the chord path: uncontracted mul+add (bf16: exact products fused), links ascending"
#ifdef PSF_CSRC_HASH
         " | csrc=" PSF_CSRC_HASH  // build.csrc_hash() of the sources this library was built from (_lib.load compares)
#endif
      ;
}

int psf_device_info(char* buf, int32_t len) {
  if (!buf || len < 1) return fail(PSF_E_NULL, "buf is NULL or empty");
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
  char pci[64] = "?";
  (void)hipDeviceGetPCIBusId(pci, (int)sizeof(pci), dev);
  int xcds = 0, cus = 0;
  (void)hipDeviceGetAttribute(&xcds, hipDeviceAttributeNumberOfXccs, dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  hipDeviceProp_t prop;
  const char* name = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.name : "?";
  snprintf(buf, (size_t)len, "pci=%s xcds=%d cus=%d name=%s", pci, xcds, cus, name);
  return PSF_OK;
}

int psf_chord_offsets(int64_t N, int32_t L, int64_t* offsets_out) {
  if (!offsets_out) return fail(PSF_E_NULL, "offsets_out is NULL");
  if (N < 1 || L < 1 || L > PSF_MAX_LINKS)
    return fail(PSF_E_SHAPE, "need N >= 1 and 1 <= L <= %d", PSF_MAX_LINKS);
  if (N > (int64_t)1 << 30) return fail(PSF_E_SHAPE, "N exceeds 2^30");
  Offsets o;
  make_offsets(N, L, nullptr, &o);
  for (int k = 0; k < L; ++k) offsets_out[k] = o.v[k];
  return PSF_OK;
}

int psf_chord_indices(int64_t N, int32_t L, int64_t* rows_out, int64_t* cols_out) {
  if (!rows_out || !cols_out) return fail(PSF_E_NULL, "rows_out / cols_out is NULL");
  if (N < 1 || L < 1 || L > PSF_MAX_LINKS)
    return fail(PSF_E_SHAPE, "need N >= 1 and 1 <= L <= %d", PSF_MAX_LINKS);
  if (N > (int64_t)1 << 30) return fail(PSF_E_SHAPE, "N exceeds 2^30");
  Offsets o;
  make_offsets(N, L, nullptr, &o);
  for (int64_t i = 0; i < N; ++i)
    for (int k = 0; k < L; ++k) {
      rows_out[i * L + k] = i;
      int64_t c = i + o.v[k];
      cols_out[i * L + k] = c >= N ? c - N : c;
    }
  return PSF_OK;
}

int psf_chord_spmm_fwd_f32(const float* W, const float* V, const float* res, float* out, int64_t B, int64_t N,
                           int32_t L, int64_t C, int64_t v_batch_stride, const int64_t* offsets, void* stream) {
  return fwd_impl<float>(snapshot(), W, V, res, out, B, N, L, C, v_batch_stride, offsets, stream);
}
int psf_chord_spmm_fwd_f64(const double* W, const double* V, const double* res, double* out, int64_t B,
                           int64_t N, int32_t L, int64_t C, int64_t v_batch_stride, const int64_t* offsets,
                           void* stream) {
  return fwd_impl<double>(snapshot(), W, V, res, out, B, N, L, C, v_batch_stride, offsets, stream);
}

int psf_chord_spmm_bwd_f32(const float* dZ, const float* W, const float* V, float* dW, float* dV, int64_t B,
                           int64_t N, int32_t L, int64_t C, int64_t v_batch_stride, const int64_t* offsets,
                           void* stream) {
  return bwd_impl<float>(snapshot(), dZ, W, V, dW, dV, B, N, L, C, v_batch_stride, offsets, stream);
}
int psf_chord_spmm_bwd_f64(const double* dZ, const double* W, const double* V, double* dW, double* dV,
                           int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                           const int64_t* offsets, void* stream) {
  return bwd_impl<double>(snapshot(), dZ, W, V, dW, dV, B, N, L, C, v_batch_stride, offsets, stream);
}

int psf_chord_chain_fwd_f32(const float* const* W_steps, const float* V0, float* const* out_steps, int32_t M,
                            int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C,
                            int64_t v0_batch_stride, const int64_t* offsets, void* stream) {
  return chain_impl<float>(snapshot(), W_steps, V0, out_steps, M, use_residual, B, N, L, C, v0_batch_stride, offsets, stream);
}
int psf_chord_chain_fwd_f64(const double* const* W_steps, const double* V0, double* const* out_steps, int32_t M,
                            int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C,
                            int64_t v0_batch_stride, const int64_t* offsets, void* stream) {
  return chain_impl<double>(snapshot(), W_steps, V0, out_steps, M, use_residual, B, N, L, C, v0_batch_stride, offsets, stream);
}

int psf_chord_spmm_fwd_bf16(const uint16_t* W, const uint16_t* V, const uint16_t* res, uint16_t* out, int64_t B, int64_t N,
                            int32_t L, int64_t C, int64_t v_batch_stride, const int64_t* offsets, void* stream) {
  return fwd_impl<__bf16>(snapshot(), reinterpret_cast<const __bf16*>(W), reinterpret_cast<const __bf16*>(V),
                          reinterpret_cast<const __bf16*>(res), reinterpret_cast<__bf16*>(out), B, N, L, C, v_batch_stride, offsets,
                          stream);
}

int psf_chord_spmm_bwd_bf16(const uint16_t* dZ, const uint16_t* W, const uint16_t* V, uint16_t* dW, uint16_t* dV, int64_t B,
                            int64_t N, int32_t L, int64_t C, int64_t v_batch_stride, const int64_t* offsets, void* stream) {
  return bwd_impl<__bf16>(snapshot(), reinterpret_cast<const __bf16*>(dZ), reinterpret_cast<const __bf16*>(W),
                          reinterpret_cast<const __bf16*>(V), reinterpret_cast<__bf16*>(dW), reinterpret_cast<__bf16*>(dV), B, N, L,
                          C, v_batch_stride, offsets, stream);
}

int psf_chord_chain_fwd_bf16(const uint16_t* const* W_steps, const uint16_t* V0, uint16_t* const* out_steps, int32_t M,
                             int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride,
                             const int64_t* offsets, void* stream) {
  return chain_impl<__bf16>(snapshot(), reinterpret_cast<const __bf16* const*>(W_steps), reinterpret_cast<const __bf16*>(V0),
                            reinterpret_cast<__bf16* const*>(out_steps), M, use_residual, B, N, L, C, v0_batch_stride, offsets, stream);
}

int psf_chord_chain_last_supported(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t w_align, int32_t use_residual,
                                   int64_t v0_batch_stride, int32_t default_offsets) {
  return plan_chain_last(snapshot(), B, N, L, C, M, w_align, use_residual != 0, v0_batch_stride, default_offsets != 0).automatic ? 1 : 0;
}

// X_M of the chain in exactly one launch (fwd_chain_regs.h), or PSF_E_UNSUPPORTED: no per-step fallback here
// (psf_chord_chain_fwd_f32 is that route). The entry runs wherever the kernel fits; psf_chord_chain_last_supported is the
// automatic rule on top of that.
int psf_chord_chain_last_f32(const float* const* W_steps, const float* V0, float* out, int32_t M, int32_t use_residual, int64_t B,
                             int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride, const int64_t* offsets, void* stream) {
  if (M < 1) return fail(PSF_E_SHAPE, "M must be >= 1");
  if (!W_steps || !V0 || !out) return fail(PSF_E_NULL, "W_steps, V0 and out must be non-NULL");
  if (int rc = check_dims(B, N, L, C, v0_batch_stride)) return rc;
  if (out == V0) return fail(PSF_E_ALIAS, "out aliases V0");
  // the kernel copies W in 16-byte chunks and moves V0 and out rows in 8-byte pieces (C is a multiple of 4: a 16-byte aligned
  // base makes every piece aligned); anything less aligned is the per-step route's
  bool align16 = aligned_to(V0, 16) && aligned_to(out, 16), align4 = aligned_to(V0, sizeof(float)) && aligned_to(out, sizeof(float));
  for (int m = 0; m < M; ++m) {
    if (!W_steps[m]) return fail(PSF_E_NULL, "step %d: NULL pointer", m);
    if (W_steps[m] == out) return fail(PSF_E_ALIAS, "step %d: out aliases W", m);
    align16 = align16 && aligned_to(W_steps[m], 16);
    align4 = align4 && aligned_to(W_steps[m], sizeof(float));
  }
  if (!align4) return fail(PSF_E_ALIGN, "pointers must be aligned to the element size");
  const int w_align = align16 ? 16 : 4;
  Offsets offs, chord;
  make_offsets(N, L, offsets, &offs);
  make_offsets(N, L, nullptr, &chord);
  bool default_offsets = true;
  for (int k = 0; k < L; ++k) default_offsets = default_offsets && offs.v[k] == chord.v[k];
  const Tuning tn = snapshot();
  if (!plan_chain_last(tn, B, N, L, C, M, w_align, use_residual != 0, v0_batch_stride, default_offsets).fits) return PSF_E_UNSUPPORTED;
  ChainRegsArgs a;  // (B >= 1 here: an empty batch is declined with every other shape the kernel does not cover)
  for (int m = 0; m < kChainMaxSteps; ++m) a.W[m] = m < M ? W_steps[m] : nullptr;
  a.V0 = V0;
  a.out = out;
  a.v0_bstride = v0_batch_stride;
  a.M = M;
  a.C = (int32_t)C;
  a.pairs = (int32_t)(C / 2);
  a.xcd_remap = tn.xcd_remap ? 1 : 0;
  hipError_t e = launch_chain_regs(use_residual != 0, a, (int)B, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(e, "chord_chain_regs launch");
  return PSF_OK;
}

int psf_chord_chain_bwd_supported(int64_t N, int32_t L, int64_t C, int32_t M) {
  return g_chain_bwd_fused.load() && chain_bwd_lds_fits(N, C, L, M) ? 1 : 0;
}

int psf_chord_chain_bwd_f32(const float* dOut, const float* const* W_steps, const float* V0, const float* const* X_steps,
                            float* const* dW_steps, float* dV0, float* const* dX_steps, int32_t M, int32_t use_residual,
                            int64_t B, int64_t N, int32_t L, int64_t C, const int64_t* offsets, void* stream) {
  return chain_bwd_impl<float>(dOut, W_steps, V0, X_steps, dW_steps, dV0, dX_steps, M, use_residual, B, N, L, C, offsets, stream);
}

int psf_chord_chain_bwd_bf16(const uint16_t* dOut, const uint16_t* const* W_steps, const uint16_t* V0, const uint16_t* const* X_steps,
                             uint16_t* const* dW_steps, uint16_t* dV0, uint16_t* const* dX_steps, int32_t M, int32_t use_residual,
                             int64_t B, int64_t N, int32_t L, int64_t C, const int64_t* offsets, void* stream) {
  using P = const __bf16*;
  return chain_bwd_impl<__bf16>(reinterpret_cast<P>(dOut), reinterpret_cast<const P*>(W_steps), reinterpret_cast<P>(V0),
                                reinterpret_cast<const P*>(X_steps), reinterpret_cast<__bf16* const*>(dW_steps),
                                reinterpret_cast<__bf16*>(dV0), reinterpret_cast<__bf16* const*>(dX_steps), M, use_residual, B, N, L,
                                C, offsets, stream);
}

int psf_chord_chain_bwd_lds_bf16_supported(int64_t N, int32_t L, int64_t C, int32_t M) {
  return g_chain_bwd_fused.load() && chain_bwd_lds_bf16_fits(N, C, L, M) ? 1 : 0;
}

// The bf16 backward chain in exactly one launch (bwd_chain_lds_bf16.h), or PSF_E_UNSUPPORTED: no per-step fallback here
// (psf_chord_chain_bwd_bf16 is that route). Validation in chain_bwd_impl's order.
int psf_chord_chain_bwd_lds_bf16(const uint16_t* dOut, const uint16_t* const* W_steps, const uint16_t* V0,
                                 const uint16_t* const* X_steps, uint16_t* const* dW_steps, uint16_t* dV0, int32_t M,
                                 int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C, const int64_t* offsets,
                                 void* stream) {
  if (M < 1) return fail(PSF_E_SHAPE, "M must be >= 1");
  if (!dOut || !W_steps || !V0 || !X_steps || !dW_steps || !dV0) return fail(PSF_E_NULL, "a required pointer is NULL");
  if (int rc = check_dims(B, N, L, C, N * C)) return rc;
  const Tuning tn = snapshot();
  if (!tn.chain_bwd_fused || !chain_bwd_lds_bf16_fits(N, C, L, M)) return PSF_E_UNSUPPORTED;
  if (B == 0) return PSF_OK;
  if (B > 0x7fffffff) return fail(PSF_E_SHAPE, "B too large");
  ChainBwdArgsBf16 a;
  for (int m = 0; m < M; ++m) {
    const uint16_t* x = m == 0 ? V0 : X_steps[m];
    if (!W_steps[m] || !x || !dW_steps[m]) return fail(PSF_E_NULL, "step %d: NULL pointer", m);
    if (dW_steps[m] == W_steps[m]) return fail(PSF_E_ALIAS, "step %d: dW aliases W", m);
    if (!aligned_to(W_steps[m], 2) || !aligned_to(dW_steps[m], 2) || !aligned_to(x, 16))
      return fail(PSF_E_ALIGN, "step %d: W / dW must be 2-byte, X 16-byte aligned", m);
    a.W[m] = reinterpret_cast<const __bf16*>(W_steps[m]), a.X[m] = reinterpret_cast<const __bf16*>(x);
    a.dW[m] = reinterpret_cast<__bf16*>(dW_steps[m]);
  }
  for (int m = M; m < kChainMaxSteps; ++m) a.W[m] = nullptr, a.X[m] = nullptr, a.dW[m] = nullptr;
  if (!aligned_to(dOut, 16) || !aligned_to(dV0, 16)) return fail(PSF_E_ALIGN, "dOut and dV0 must be 16-byte aligned");
  a.dOut = reinterpret_cast<const __bf16*>(dOut), a.dV0 = reinterpret_cast<__bf16*>(dV0);
  a.M = M, a.N = (int32_t)N, a.C = (int32_t)C;
  Offsets offs;
  make_offsets(N, L, offsets, &offs);
  hipError_t e = launch_chain_bwd_lds_bf16(L, (int)(C / 8), use_residual != 0, a, offs, (int)B, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(e, "chord_chain_bwd_lds<bf16> launch");
  return PSF_OK;
}

int psf_chord_chain_tr_supported(int64_t N, int32_t L, int64_t R, int32_t M, int32_t elem_bytes) {
  return chain_tr_lds_fits(N, L, R, M, elem_bytes) ? 1 : 0;
}

int psf_chord_chain_tr_f32(const float* const* W_steps, const float* Q, float* out, float* scratch, int32_t M, int64_t B,
                           int64_t N, int32_t L, int64_t R, const int64_t* offsets, void* stream) {
  return chain_tr_impl<float>(W_steps, Q, out, scratch, M, B, N, L, R, offsets, stream);
}

int psf_chord_chain_tr_bf16(const uint16_t* const* W_steps, const uint16_t* Q, uint16_t* out, uint16_t* scratch, int32_t M,
                            int64_t B, int64_t N, int32_t L, int64_t R, const int64_t* offsets, void* stream) {
  return chain_tr_impl<__bf16>(reinterpret_cast<const __bf16* const*>(W_steps), reinterpret_cast<const __bf16*>(Q),
                               reinterpret_cast<__bf16*>(out), reinterpret_cast<__bf16*>(scratch), M, B, N, L, R, offsets, stream);
}

int64_t psf_mixer_fwd_workspace(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  return plan_mixer(snapshot(), 1, N, E, M, h, C, L).ws_bytes;
}
int32_t psf_mixer_fwd_plan(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  const MixerRoute r = plan_mixer(snapshot(), 1, N, E, M, h, C, L).route;
  return r == MixerRoute::kLds ? 2 : r == MixerRoute::kSteps ? 1 : 0;
}

int psf_mixer_fwd_in_f32(const psf_mixer_input* in, int64_t B, int64_t N, int32_t E, int32_t M, const float* const* A,
                         const float* const* a, const float* const* Bw, const float* const* b, const int32_t* h, int64_t C, int32_t L,
                         int32_t use_residual, float* V0, float* const* out_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  return mixer_impl(snapshot(), in, B, N, E, M, A, a, Bw, b, h, C, L, use_residual, V0, out_steps, workspace, workspace_bytes, stream);
}
int psf_mixer_fwd_f32(const float* X, int64_t B, int64_t N, int32_t E, int32_t M, const float* const* A,
                      const float* const* a, const float* const* Bw, const float* const* b, const int32_t* h, int64_t C, int32_t L,
                      int32_t use_residual, float* V0, float* const* out_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  const psf_mixer_input in{PSF_MIXER_IN_DATA, 0, X, nullptr, nullptr, nullptr};
  return mixer_impl(snapshot(), &in, B, N, E, M, A, a, Bw, b, h, C, L, use_residual, V0, out_steps, workspace, workspace_bytes, stream);
}

int32_t psf_mixer_fwd_bf16_plan(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  return plan_mixer_bf16(snapshot(), N, E, M, h, C, L).run ? 2 : 0;
}
int64_t psf_mixer_fwd_bf16_workspace(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L) {
  return plan_mixer_bf16(snapshot(), N, E, M, h, C, L).ws_bytes;
}

int psf_mixer_fwd_bf16(const uint16_t* X, int64_t B, int64_t N, int32_t E, int32_t M, const uint16_t* const* A,
                       const uint16_t* const* a, const uint16_t* const* Bw, const uint16_t* const* b, const int32_t* h, int64_t C, int32_t L,
                       int32_t use_residual, uint16_t* V0, uint16_t* const* out_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  return mixer_bf16_impl(snapshot(), X, B, N, E, M, A, a, Bw, b, h, C, L, use_residual, V0, out_steps, workspace, workspace_bytes, stream);
}

int psf_set_tuning(const char* key, int32_t value) {
  if (!key) return fail(PSF_E_NULL, "key is NULL");
  for (auto& k : g_knobs)
    if (strcmp(k.key, key) == 0) {
      if (value < k.lo || value > k.hi)
        return fail(PSF_E_TUNING, "tuning %s: value %d outside [%d, %d]", key, (int)value, k.lo, k.hi);
      k.var->store(value);
      return PSF_OK;
    }
  return fail(PSF_E_TUNING, "unknown tuning key '%s'", key);
}

int psf_get_tuning(const char* key) {
  if (!key) return fail(PSF_E_NULL, "key is NULL");
  for (auto& k : g_knobs)
    if (strcmp(k.key, key) == 0) return k.var->load();
  return fail(PSF_E_TUNING, "unknown tuning key '%s'", key);
}

// psf_describe_*: the plan of a step or chain as the launch makes it, operands taken as 16-byte aligned (nullptr) and a
// full-batch V, formatted instead of executed.
int psf_describe_fwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t elem_bytes, char* buf, int32_t cap) {
  if (int rc = describe_args(B, N, L, C, elem_bytes, true, buf, cap)) return rc;
  Offsets offs;
  make_offsets(N, L, nullptr, &offs);
  const Elem& el = elem_of(elem_bytes);
  const FwdPlan p = plan_fwd(el, snapshot(), nullptr, nullptr, nullptr, nullptr, B, N, L, C, offs);
  // (p.refused, fwd_variant = 2 where the window kernel does not apply: a launch fails with PSF_E_TUNING, this entry has
  // always named the generic kernel. Both kept as they were.)
  if (p.window) {
    snprintf(buf, cap, "chord_fwd_win_k<%s,L=%d,TG=%d,R=%d,NT=%d> TR=%d near=%d far=%d tiles=%s", el.name, (int)L, 1 << p.pk.tgs,
             p.pk.rows, p.pk.nt, p.pk.TR, p.pk.KN, (int)L - p.pk.KN,
             p.pk.all_edge ? "edge" : (p.pk.ragged ? "full+ragged" : (p.pk.aligned ? "full, aligned (scalar block addresses)" : "full")));
  } else {
    snprintf(buf, cap, "chord_fwd_generic_k<%s,VEC=%d>", el.name, p.vec);
  }
  return PSF_OK;
}

// The kernel(s) of one backward step that wants both gradients.
int psf_describe_bwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t elem_bytes, char* buf, int32_t cap) {
  if (int rc = describe_args(B, N, L, C, elem_bytes, true, buf, cap)) return rc;
  Offsets offs;
  make_offsets(N, L, nullptr, &offs);
  const Elem& el = elem_of(elem_bytes);
  const BwdPlan p = plan_bwd(el, snapshot(), nullptr, nullptr, nullptr, nullptr, nullptr, true, true, B, N, L, C, N * C, offs);
  // (p.refused, dw_variant = 2 where the chunk-looping kernel does not apply: a launch fails with PSF_E_TUNING, this entry
  // has always named the dW kernel the automatic route takes next. Both kept as they were.)
  if (p.fused == Fused::kAligned) {
    snprintf(buf, cap, "chord_bwd_fused_k<%s,L=%d,TG=%d,NT=%d> TR=%d near=%d far=%d fronts=%d", el.name, (int)L, 1 << p.fpk.tgs, p.fpk.nt,
             p.fpk.TR, p.fpk.KN, (int)L - p.fpk.KN, 1 << p.ileave);
  } else if (p.fused == Fused::kEdge) {
    snprintf(buf, cap, "chord_bwd_fused_edge_k<%s,L=%d,TG=%d,NT=%d> TR=%d near=%d far=%d", el.name, (int)L, 1 << p.fpk.tgs, p.fpk.nt,
             p.fpk.TR, p.fpk.KN, (int)L - p.fpk.KN);
  } else {
    char dw[112], dv[112];
    if (p.dw == Route::kGeneric) snprintf(dw, sizeof(dw), "chord_dw_generic_k<%s,VEC=%d>", el.name, p.dw_vec);
    else print_win(dw, sizeof(dw), p.dw == Route::kChunk ? "chord_dw_chunk_k" : "chord_dw_win_k", el, L, p.dwpk);
    if (p.dv == Route::kGeneric) snprintf(dv, sizeof(dv), "chord_dv_generic_k<%s,VEC=%d>", el.name, p.dv_vec);
    else print_win(dv, sizeof(dv), "chord_dv_win_k", el, L, p.dvpk);
    snprintf(buf, cap, "%s + %s", dw, dv);
  }
  return PSF_OK;
}

int psf_describe_chain_fwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, char* buf, int32_t cap) {
  return psf_describe_chain_fwd_dtype(B, N, L, C, M, 4, buf, cap);
}

int psf_describe_chain_fwd_dtype(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t elem_bytes, char* buf,
                                 int32_t cap) {
  if (int rc = describe_args(B, N, L, C, elem_bytes, false, buf, cap)) return rc;
  const Elem& el = elem_of(elem_bytes);
  // (as an inference chain is run: only the last result kept; bf16 under its own gate. p.grid_ok, B * chunks workgroups
  // within the grid limit, is the launch's condition only: this entry has never looked at it. Kept.)
  const ChainPlan p = plan_chain<float>(el, snapshot(), nullptr, nullptr, nullptr, M, true, B, N, L, C);
  if (!p.one_launch) return psf_describe_fwd(B, N, L, C, elem_bytes, buf, cap);
  const ChainLdsPlan& plan = p.lds;
  if (plan.big)
    snprintf(buf, cap, "chord_chain_rows_k<%s,L=%d,G=%d,R=%d> one launch for all %d steps, %d threads x %d rows x %d channels, %d workgroup(s) per sequence",
             el.name, (int)L, plan.cc, plan.rows, (int)M, plan.threads, plan.rows, el.vec * plan.cc, plan.chunks);
  else
    snprintf(buf, cap, "chord_chain_lds_k<%s,L=%d,CC=%d,R=%d> one launch for all %d steps, %d threads, %d workgroup(s) per sequence",
             el.name, (int)L, plan.cc, plan.rows, (int)M, plan.threads, plan.chunks);
  return PSF_OK;
}

// What psf_chord_chain_last_f32 does with a chain of aligned operands, a full-batch V0 and the chord offsets.
int psf_describe_chain_last(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, char* buf, int32_t cap) {
  if (int rc = describe_args(B, N, L, C, 4, false, buf, cap)) return rc;
  const ChainLastPlan p = plan_chain_last(snapshot(), B, N, L, C, M, 16, true, N * C, true);
  if (!p.fits) {
    snprintf(buf, cap, "declined (PSF_E_UNSUPPORTED): chord_chain_regs_k covers f32, N=%d, L=%d, C a multiple of 4, M <= %d", kChainRegsN,
             kChainRegsLinks, kChainMaxSteps);
    return PSF_OK;
  }
  using Cfg = ChainRegsCfg<kChainRegsLinks, kChainRegsThreads>;
  snprintf(buf, cap, "chord_chain_regs_k<f32,L=%d,T=%d,J=%d> one launch for all %d steps, X in registers, W through %d LDS slots of %d bytes, "
           "%d workgroup(s) per sequence, %s", (int)L, kChainRegsThreads, kChainRegsBlocks, (int)M, Cfg::kSlots, Cfg::kSlotBytes, (int)(C / 2),
           p.automatic ? "automatic" : "on request only");
  return PSF_OK;
}

}  // extern "C"
