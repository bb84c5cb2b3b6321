// linear_wgrad_bf16.hip — weight / bias gradient of a token-wise Linear layer whose operands are bf16.
//
//   dWt[j,i] = sum_t dY[t,j] * X[t,i]      db[j] = sum_t dY[t,j]        t < T tokens,  i < m <= 128, j < n <= 128
//
// The job of linear_wgrad.hip (a reduction over ~1e6 rows into a tile of a few hundred numbers, memory-bound) on the bf16
// matrix pipe, v_mfma_f32_32x32x16_bf16. Arithmetic contract (include/psf_chord.h): bf16 operands, every product exact in
// f32, all accumulation in f32, ONE rounding to bf16 (nearest even) per output element at the store, no float atomics and a
// fixed order of additions — two calls on the same operands give the same bits, eagerly or from a replayed graph. The
// summation order is this kernel's own (16 tokens per MFMA, 32-token tiles, one slab per wave): it is NOT the f32 kernel's.
//
// Kernel 1 (linear_wgrad_bf16_partial_k): the T rows are cut into one contiguous slab per wave, a multiple of 32 rows. The
// MFMA's k index is the token, the slow index in memory: a lane needs 8 consecutive tokens of ONE column of both operands.
// So a wave streams 32 rows of dY and X with row-wise vector loads into wave-private LDS planes ([32 tokens][32 columns] bf16,
// mlp_planes.h) and reads both operand fragments back down the columns with ds_read_b64_tr_b16. The planes are private to the
// wave: no workgroup barrier in the loop. Operands whose row stride is a multiple of 8 elements (16-byte loads) are fetched
// one tile ahead into registers; narrower strides (the two inputs of an input layer, odd widths) load 8, 4 or 2 bytes at a
// time. A vector that would cross the end of a row's m (n) columns is loaded element by element, so no load leaves
// [X, X + (T-1) ldx + m) or [dY, dY + (T-1) ldy + n). Rows past the slab's end are staged as zeros; plane columns past m (n)
// are zeroed once and never written. The bias gradient is the f32 running sum of the staged dY fragments. The workgroup's four
// slabs are added in LDS in wave order and leave as ONE f32 partial tile per workgroup.
// Kernel 2 (linear_wgrad_bf16_reduce_k): adds the partial tiles in a fixed order and stores bf16.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psf_chord.h"
#include "mlp_planes.h"

extern "C" int psf_internal_fail(int code, const char* message);  // psf_chord.hip: sets psf_last_error()

namespace {

using psf_x3::bf16x8;
using psf_x3::kPlaneBytes;
using psf_x3::plane_off;
using psf_x3::PlaneLane;
using acc16 = __attribute__((ext_vector_type(16))) float;

constexpr int kTileRows = 32;  // tokens per LDS tile: two k-steps of the MFMA
constexpr int kMaxTiles = 4;   // per dimension: up to 128 outputs

// C/D layout of v_mfma_f32_32x32x16_bf16: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int cd_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// byte offset, within an operand's planes, of element (row, column c0) — c0's 16-byte chunk swizzled, the offset inside it kept
__device__ __forceinline__ int elem_off(int row, int c0) { return (c0 >> 5) * kPlaneBytes + plane_off(row, (c0 & 31) >> 3) + 2 * (c0 & 7); }

// `cnt` (< 8) elements p[0..cnt) as the low lanes of a 16-byte vector, the rest zero: the end of a row's columns
__device__ __forceinline__ uint4 load_elems(const uint16_t* __restrict__ p, int cnt) {
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = k < cnt ? (uint32_t)p[k] : 0u;
  return uint4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}

// ---- operands with 16-byte rows: 32 rows x (4 TILES) chunks of 8 columns, 2 TILES chunks per lane, held in registers ----
template <int TILES>
struct Stage8 {
  uint4 v[2 * TILES];
};

template <int TILES>
__device__ __forceinline__ void load8(Stage8<TILES>& s, const uint16_t* __restrict__ P, int64_t ld, int width, int64_t t0, int64_t t_end,
                                      int lane) {
  constexpr int kPerRow = 4 * TILES;
#pragma unroll
  for (int it = 0; it < 2 * TILES; ++it) {
    const int idx = it * 64 + lane, row = idx / kPerRow, c0 = 8 * (idx % kPerRow);
    const int64_t t = t0 + row;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (t < t_end && c0 < width) {
      const uint16_t* p = P + t * ld + c0;
      if (c0 + 8 <= width) v = *reinterpret_cast<const uint4*>(p);
      else v = load_elems(p, width - c0);
    }
    s.v[it] = v;
  }
}

template <int TILES>
__device__ __forceinline__ void store8(const Stage8<TILES>& s, unsigned char* planes, int width, int lane) {
  constexpr int kPerRow = 4 * TILES;
#pragma unroll
  for (int it = 0; it < 2 * TILES; ++it) {
    const int idx = it * 64 + lane, row = idx / kPerRow, c0 = 8 * (idx % kPerRow);
    if (c0 < width) *reinterpret_cast<uint4*>(planes + elem_off(row, c0)) = s.v[it];
  }
}

// ---- operands with narrower rows: G = 4, 2 or 1 elements per load (row stride a multiple of G), straight into the planes ----
template <int G>
__device__ __forceinline__ void stage_small(unsigned char* planes, const uint16_t* __restrict__ P, int64_t ld, int width, int64_t t0,
                                            int64_t t_end, int lane) {
  const int per_row = (width + G - 1) / G, total = kTileRows * per_row;
  for (int idx = lane; idx < total; idx += 64) {
    const int row = idx / per_row, c0 = G * (idx - row * per_row);
    const int64_t t = t0 + row;
    const bool ok = t < t_end;
    const uint16_t* p = P + (ok ? t : t0) * ld + c0;  // (t0 < t_end: the address is in bounds also where nothing is loaded)
    unsigned char* q = planes + elem_off(row, c0);
    if constexpr (G == 1) {
      *reinterpret_cast<uint16_t*>(q) = ok ? p[0] : (uint16_t)0;
    } else {
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (ok) {
        if (c0 + G <= width) {
          if constexpr (G == 4) {
            const uint2 w = *reinterpret_cast<const uint2*>(p);
            v.x = w.x, v.y = w.y;
          } else {
            v.x = *reinterpret_cast<const uint32_t*>(p);
          }
        } else {
          v = load_elems(p, width - c0);
        }
      }
      if constexpr (G == 4) *reinterpret_cast<uint2*>(q) = uint2{v.x, v.y};
      else *reinterpret_cast<uint32_t*>(q) = v.x;
    }
  }
}

__device__ __forceinline__ void stage_narrow(int g, unsigned char* planes, const uint16_t* __restrict__ P, int64_t ld, int width, int64_t t0,
                                             int64_t t_end, int lane) {
  if (g == 4) stage_small<4>(planes, P, ld, width, t0, t_end, lane);
  else if (g == 2) stage_small<2>(planes, P, ld, width, t0, t_end, lane);
  else stage_small<1>(planes, P, ld, width, t0, t_end, lane);
}

// The wave's own LDS stores and reads stay in program order (one wave's DS operations execute in order); this keeps the
// compiler from moving them across each other and has the stores landed before the transposed reads are issued.
__device__ __forceinline__ void lds_wave_order() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ float sum8(bf16x8 v) {
  float s = (float)v[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) s += (float)v[k];
  return s;
}

// gx / gy: elements per load of X / dY — 8, 4, 2 or 1; the host derives them from the row strides
template <int TJ, int TI>
__global__ void __launch_bounds__(256)
linear_wgrad_bf16_partial_k(const uint16_t* __restrict__ X, int64_t ldx, int gx, const uint16_t* __restrict__ dY, int64_t ldy, int gy,
                            int64_t T, int m, int n, float* __restrict__ part, float* __restrict__ bpart, int64_t rows_per_wave) {
  constexpr int kWaveBytes = (TJ + TI) * kPlaneBytes;
  constexpr int kRedBytes = 4 * 16 * 64 * 4;  // (the bias sums reuse the same bytes afterwards)
  static_assert(4 * kWaveBytes >= kRedBytes, "the cross-wave reduction reuses the planes");
  __shared__ __attribute__((aligned(16))) unsigned char lds[4 * kWaveBytes];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x * 4 + wv;
  const int c = lane & 31, kk = lane >> 5;
  int64_t t_begin = (int64_t)w * rows_per_wave;  // waves past the last slab get an empty one (they still take part in
  if (t_begin > T) t_begin = T;                  // the workgroup reduction)
  int64_t t_end = t_begin + rows_per_wave;
  if (t_end > T) t_end = T;

  unsigned char* pa = lds + wv * kWaveBytes;  // TJ planes of dY, then TI planes of X
  unsigned char* pb = pa + TJ * kPlaneBytes;
  for (int i = lane * 16; i < kWaveBytes; i += 64 * 16) *reinterpret_cast<uint4*>(pa + i) = uint4{0u, 0u, 0u, 0u};
  const PlaneLane L = psf_x3::plane_lane(lane);

  acc16 acc[TJ][TI];
  float bacc[TJ];
#pragma unroll
  for (int a = 0; a < TJ; ++a) {
    bacc[a] = 0.f;
#pragma unroll
    for (int b = 0; b < TI; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  }

  const bool vy = gy == 8, vx = gx == 8;  // wave-uniform: operands with 16-byte rows are fetched one tile ahead into registers
  Stage8<TJ> sa;
  Stage8<TI> sb;
  if (t_begin < t_end) {
    if (vy) load8<TJ>(sa, dY, ldy, n, t_begin, t_end, lane);
    if (vx) load8<TI>(sb, X, ldx, m, t_begin, t_end, lane);
  }
  for (int64_t t = t_begin; t < t_end; t += kTileRows) {
    lds_wave_order();  // the previous tile's reads are done before its planes are overwritten
    if (vy) store8<TJ>(sa, pa, n, lane);
    else stage_narrow(gy, pa, dY, ldy, n, t, t_end, lane);
    if (vx) store8<TI>(sb, pb, m, lane);
    else stage_narrow(gx, pb, X, ldx, m, t, t_end, lane);
    lds_wave_order();
    if (t + kTileRows < t_end) {  // the next tile's loads fly during this tile's MFMAs
      if (vy) load8<TJ>(sa, dY, ldy, n, t + kTileRows, t_end, lane);
      if (vx) load8<TI>(sb, X, ldx, m, t + kTileRows, t_end, lane);
    }
    // EXEC is all ones here (wave-uniform control flow): ds_read_b64_tr_b16 needs it
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 fa[TJ], fb[TI];
#pragma unroll
      for (int a = 0; a < TJ; ++a) fa[a] = psf_x3::tr_frag(pa + a * kPlaneBytes, L, s);  // dY[t + 16 s + 8 kk + 0..7][32 a + c]
#pragma unroll
      for (int b = 0; b < TI; ++b) fb[b] = psf_x3::tr_frag(pb + b * kPlaneBytes, L, s);  // X [t + 16 s + 8 kk + 0..7][32 b + c]
#pragma unroll
      for (int a = 0; a < TJ; ++a) {
        bacc[a] += sum8(fa[a]);
#pragma unroll
        for (int b = 0; b < TI; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
    }
  }

  // combine the workgroup's four slabs through LDS (fixed order: wave 0 + 1 + 2 + 3), ONE partial tile per workgroup:
  // part[wg][j][i] (TJ*32 x TI*32), bpart[wg][j]. The planes are dead: their bytes are the scratch. Every wave parks a
  // 32 x 32 tile in accumulator order; each of the 256 threads then adds and stores four of its 1024 elements.
  constexpr int MJ = TJ * 32, MI = TI * 32;
  __syncthreads();
  float(*red)[16 * 64] = reinterpret_cast<float(*)[16 * 64]>(lds);
  float* __restrict__ pw = part + (int64_t)blockIdx.x * MJ * MI;
#pragma unroll
  for (int a = 0; a < TJ; ++a) {
#pragma unroll
    for (int b = 0; b < TI; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wv][r * 64 + lane] = acc[a][b][r];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = k * 256 + (int)threadIdx.x, r = e >> 6, l = e & 63;
        pw[(a * 32 + cd_row(r, l)) * MI + b * 32 + (l & 31)] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
      }
      __syncthreads();
    }
  }
  float(*redb)[kMaxTiles * 32] = reinterpret_cast<float(*)[kMaxTiles * 32]>(lds);
#pragma unroll
  for (int a = 0; a < TJ; ++a) {
    const float bs = bacc[a] + __shfl_xor(bacc[a], 32, 64);
    if (kk == 0) redb[wv][a * 32 + c] = bs;
  }
  __syncthreads();
  if (threadIdx.x < MJ) {
    const int j = threadIdx.x;
    bpart[(int64_t)blockIdx.x * MJ + j] = ((redb[0][j] + redb[1][j]) + redb[2][j]) + redb[3][j];
  }
}

// out[j*m + i] = rne_bf16(sum_p part[p][j][i]); db[j] = rne_bf16(sum_p bpart[p][j]). Fixed order: a workgroup owns kRedOuts
// outputs; lane group g adds the partials p = g, g + kRedGroups, ... in ascending p, then the kRedGroups group sums are added
// in ascending g, in f32; the total is rounded once.
constexpr int kRedOuts = 8, kRedGroups = 32;
static_assert(kRedOuts * kRedGroups == 256, "one 256-thread workgroup");

__global__ void __launch_bounds__(256)
linear_wgrad_bf16_reduce_k(const float* __restrict__ part, const float* __restrict__ bpart, int nparts, int MJ, int MI, int m, int n,
                           __bf16* __restrict__ dWt, __bf16* __restrict__ db) {
  __shared__ float sums[kRedGroups][kRedOuts];
  const int ol = threadIdx.x & (kRedOuts - 1), grp = threadIdx.x >> 3;
  const int e = blockIdx.x * kRedOuts + ol;
  const int n_out = n * m + (db != nullptr ? n : 0);
  const float* p = part;
  int64_t stride = 0;
  if (e < n * m) {
    const int j = e / m, i = e - j * m;
    p = part + (int64_t)j * MI + i;
    stride = (int64_t)MJ * MI;
  } else if (e < n_out) {
    p = bpart + (e - n * m);
    stride = MJ;
  }
  float s = 0.f;
  if (e < n_out)
    for (int q = grp; q < nparts; q += kRedGroups) s += p[(int64_t)q * stride];
  sums[grp][ol] = s;
  __syncthreads();
  if (grp == 0 && e < n_out) {
    float tot = 0.f;
#pragma unroll
    for (int g = 0; g < kRedGroups; ++g) tot += sums[g][ol];
    if (e < n * m) dWt[e] = (__bf16)tot;
    else db[e - n * m] = (__bf16)tot;
  }
}

struct Plan {
  int tj, ti, nwaves, nparts;
  int64_t rows_per_wave, part_floats, bpart_floats;
};

bool make_plan(int64_t T, int m, int n, Plan* p) {
  if (T < 1 || m < 1 || n < 1) return false;
  p->tj = (n + 31) / 32;
  p->ti = (m + 31) / 32;
  if (p->tj > kMaxTiles || p->ti > kMaxTiles) return false;
  const int64_t tile_floats = (int64_t)p->tj * p->ti * 1024;
  int64_t nw = 8192;                               // 32 waves per CU: slabs overlap each other's load bursts
  const int64_t budget = ((int64_t)32 << 20) / 4;  // <= 32 MiB of partial tiles (one per 4 waves)
  if (nw / 4 * tile_floats > budget) nw = 4 * (budget / tile_floats);
  int64_t rpw = (T + nw - 1) / nw;
  rpw = (rpw + kTileRows - 1) / kTileRows * kTileRows;  // whole LDS tiles
  nw = (T + rpw - 1) / rpw;
  p->nwaves = (int)nw;
  p->nparts = (int)((nw + 3) / 4);  // one partial tile per 4-wave workgroup
  p->rows_per_wave = rpw;
  p->part_floats = p->nparts * tile_floats;
  p->bpart_floats = (int64_t)p->nparts * p->tj * 32;
  return true;
}

// elements per load for a row stride: the largest power of two <= 8 that divides it
int granule(int64_t ld) { return (int)(ld & 7 ? ld & -ld : 8); }

template <int TJ>
hipError_t launch_ti(const Plan& p, const uint16_t* X, int64_t ldx, const uint16_t* dY, int64_t ldy, int64_t T, int m, int n, float* part,
                     float* bpart, hipStream_t s) {
  const dim3 grid(p.nparts), block(256);
  const int gx = granule(ldx), gy = granule(ldy);
  switch (p.ti) {
    case 1: hipLaunchKernelGGL((linear_wgrad_bf16_partial_k<TJ, 1>), grid, block, 0, s, X, ldx, gx, dY, ldy, gy, T, m, n, part, bpart, p.rows_per_wave); break;
    case 2: hipLaunchKernelGGL((linear_wgrad_bf16_partial_k<TJ, 2>), grid, block, 0, s, X, ldx, gx, dY, ldy, gy, T, m, n, part, bpart, p.rows_per_wave); break;
    case 3: hipLaunchKernelGGL((linear_wgrad_bf16_partial_k<TJ, 3>), grid, block, 0, s, X, ldx, gx, dY, ldy, gy, T, m, n, part, bpart, p.rows_per_wave); break;
    case 4: hipLaunchKernelGGL((linear_wgrad_bf16_partial_k<TJ, 4>), grid, block, 0, s, X, ldx, gx, dY, ldy, gy, T, m, n, part, bpart, p.rows_per_wave); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

extern "C" {

int64_t psf_linear_wgrad_bf16_workspace(int64_t T, int32_t m, int32_t n) {
  Plan p;
  if (!make_plan(T, m, n, &p)) return -1;
  return (p.part_floats + p.bpart_floats) * (int64_t)sizeof(float);
}

int psf_linear_wgrad_bf16(const uint16_t* X, int64_t ldx, const uint16_t* dY, int64_t ldy, int64_t T, int32_t m, int32_t n, uint16_t* dWt,
                          uint16_t* db, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!X || !dY || !dWt || !workspace) return psf_internal_fail(PSF_E_NULL, "psf_linear_wgrad_bf16: X, dY, dWt and workspace must be non-NULL");
  Plan p;
  if (!make_plan(T, m, n, &p)) return psf_internal_fail(PSF_E_SHAPE, "psf_linear_wgrad_bf16: need T >= 1 and 1 <= m, n <= 128");
  if (ldx < m || ldy < n) return psf_internal_fail(PSF_E_SHAPE, "psf_linear_wgrad_bf16: row strides must be >= the row lengths");
  if ((reinterpret_cast<uintptr_t>(X) & (uintptr_t)(2 * granule(ldx) - 1)) || (reinterpret_cast<uintptr_t>(dY) & (uintptr_t)(2 * granule(ldy) - 1)) ||
      (reinterpret_cast<uintptr_t>(dWt) & 1) || (reinterpret_cast<uintptr_t>(db) & 1) || (reinterpret_cast<uintptr_t>(workspace) & 3))
    return psf_internal_fail(PSF_E_ALIGN, "psf_linear_wgrad_bf16: X (dY) must be aligned to 2 g bytes, g the largest power of two <= 8 "
                                          "dividing ldx (ldy); dWt and db to 2 bytes, workspace to 4");
  if (workspace_bytes < (p.part_floats + p.bpart_floats) * (int64_t)sizeof(float))
    return psf_internal_fail(PSF_E_SHAPE, "psf_linear_wgrad_bf16: workspace smaller than psf_linear_wgrad_bf16_workspace(T, m, n)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>(workspace);
  float* bpart = part + p.part_floats;
  hipError_t e;
  switch (p.tj) {
    case 1: e = launch_ti<1>(p, X, ldx, dY, ldy, T, m, n, part, bpart, s); break;
    case 2: e = launch_ti<2>(p, X, ldx, dY, ldy, T, m, n, part, bpart, s); break;
    case 3: e = launch_ti<3>(p, X, ldx, dY, ldy, T, m, n, part, bpart, s); break;
    case 4: e = launch_ti<4>(p, X, ldx, dY, ldy, T, m, n, part, bpart, s); break;
    default: return psf_internal_fail(PSF_E_SHAPE, "psf_linear_wgrad_bf16: unsupported tile count");
  }
  if (e != hipSuccess) return psf_internal_fail((int)e, hipGetErrorString(e));
  const int outs = n * m + n;
  hipLaunchKernelGGL(linear_wgrad_bf16_reduce_k, dim3((outs + kRedOuts - 1) / kRedOuts), dim3(256), 0, s, (const float*)part,
                     (const float*)bpart, p.nparts, p.tj * 32, p.ti * 32, (int)m, (int)n, reinterpret_cast<__bf16*>(dWt),
                     reinterpret_cast<__bf16*>(db));
  e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

}  // extern "C"
