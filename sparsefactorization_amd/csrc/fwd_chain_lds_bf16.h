// fwd_chain_lds_bf16.h — the one-launch LDS-resident forward chain (fwd_chain_lds.h) in bfloat16.
//
// Same decomposition, same XCD-aware workgroup map, same W prefetch distance as the f32 kernels; what differs:
//   * a 16-byte LDS slot holds one row x EIGHT channels, so a workgroup covers 8*CC (8*G) channels and half as many
//     workgroups stream a sequence's W. Slot counts, byte limits and the N limits are those of f32.
//   * arithmetic is the bf16 contract of the per-step kernels (psf_common.h: madd_rn<__bf16>): f32 accumulator, links
//     ascending with the fused exact product, the residual with add_rn, then ONE narrow (RNE, NaN kept). That bf16 value
//     goes to LDS (and to memory when the step is stored), so keeping X in LDS as bf16 IS the per-step arithmetic: the
//     per-step route also rounds every step's result to bf16 before the next step reads it. Bit-identical.
//   * the residual rows stay in registers PACKED (4 registers per slot, as in f32) and are widened where they are added.
//   * W rows are L bf16 values at a 2-byte-aligned address (30-byte rows at L = 15: every other row starts in the middle
//     of a dword). A row is fetched as the ND = ceil(L / 2) ALIGNED dwords that cover it — the f32 kernel's load shape
//     (dwordx4 / x2 / x1 on a 4-byte-aligned packed struct) at half the requests per row: ceil(ND / 4) instead of
//     ceil(L / 4), e.g. 2 instead of 4 at L = 12..15 — and shifted into place with one v_alignbit_b32 per dword when the
//     row is consumed (shift 0 or 16 from bit 1 of the row's address: no branch). L separate 16-bit loads would have been
//     L requests per row, and the W stream's request count is this kernel's documented bound. Covering dwords never leave
//     the dword of the row's first / last element, so nothing outside the pages of W is read. For even L all rows of a
//     4-byte-aligned W are dword-aligned and ND = L / 2 covers a row exactly; the planner sends even L with a W that is only
//     2-byte aligned to the per-step kernels (ND dwords would not cover such a row).
#pragma once

#include "fwd_chain_lds.h"

namespace psf {

struct ChainArgsBf16 {
  const __bf16* W[kChainMaxSteps];  // W_m [B, N, L]
  __bf16* out[kChainMaxSteps];      // X_{m+1} [B, N, C]; written when bit m of store_mask is set
  const __bf16* V0;                 // [B, N, C] or [N, C] (v0_bstride == 0)
  uint64_t store_mask;
  int64_t v0_bstride;
  int32_t M, N, C, CG, chunks;      // CG = C / 8 channel groups, chunks = ceil(CG / CC) workgroups per sequence
  int32_t xcd_remap;
};

using U4 = uint32_t __attribute__((ext_vector_type(4)));  // one LDS slot: 8 bf16

template <int L>
struct __attribute__((packed, aligned(4))) WRowBf16 {
  static constexpr int ND = (L + 1) / 2;
  uint32_t d[ND];
};

// The covering dwords of row `row` of Wm, as loaded (not yet shifted), and the shift that aligns them: 16 * (bit 1 of the
// row's address).
template <int L>
__device__ __forceinline__ WRowBf16<L> ld_wrow(const __bf16* Wm, int64_t row, uint32_t& shift) {
  const char* p = reinterpret_cast<const char*>(Wm + row * L);
  if constexpr (L % 2 != 0) {
    // (pointer arithmetic, not an integer round trip: the load stays a global_load, not a flat one)
    const uint32_t odd = (uint32_t)reinterpret_cast<uintptr_t>(p) & 2u;
    shift = odd << 3;
    p -= odd;
  } else {
    shift = 0;
  }
  return *reinterpret_cast<const WRowBf16<L>*>(p);
}
// element k of the row then sits in half k & 1 of dword k >> 1
template <int L>
__device__ __forceinline__ WRowBf16<L> align_wrow(const WRowBf16<L>& r, uint32_t shift) {
  if constexpr (L % 2 == 0) return r;
  WRowBf16<L> o;
#pragma unroll
  for (int i = 0; i < WRowBf16<L>::ND; ++i)
    o.d[i] = __builtin_amdgcn_alignbit(i + 1 < WRowBf16<L>::ND ? r.d[i + 1] : 0u, r.d[i], shift);
  return o;
}

__device__ __forceinline__ __bf16 bf16_half(uint32_t d, int h) {
  return __builtin_bit_cast(__bf16, (uint16_t)(h ? d >> 16 : d));
}
__device__ __forceinline__ Vec<__bf16, 8> slot_vec(const U4 x) {
  Vec<__bf16, 8> v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v.e[i] = bf16_half(x[i >> 1], i & 1);
  return v;
}
__device__ __forceinline__ U4 vec_slot(const Vec<__bf16, 8>& v) {
  U4 x;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    x[i] = (uint32_t)__builtin_bit_cast(uint16_t, v.e[2 * i]) | ((uint32_t)__builtin_bit_cast(uint16_t, v.e[2 * i + 1]) << 16);
  return x;
}
// acc (+ residual), rounded once: the slot that goes to LDS and to memory
template <bool RES>
__device__ __forceinline__ U4 finish_slot(Vec<float, 8> acc, const U4 res) {
  if constexpr (RES) {
    const Vec<float, 8> r = widen<__bf16, 8>(slot_vec(res));
#pragma unroll
    for (int i = 0; i < 8; ++i) acc.e[i] = add_rn(acc.e[i], r.e[i]);
  }
  return vec_slot(narrow<__bf16, 8>(acc));
}

// chord_chain_lds_k in bf16 (T is __bf16: the overload on a leading type parameter keeps the f32 kernel's name and symbol
// as they are). Thread (rs, g): channel group g < CC (8 channels) of rows rs + j*RSN, j < R.
template <typename T, int L, int CC, int R, bool RES, int NTMAX>
__global__ void __launch_bounds__(NTMAX)
chord_chain_lds_k(const ChainArgsBf16 a, const Offsets offs) {
  static_assert(__is_same(T, __bf16), "the f32 kernel has no type parameter");
  using A8 = Vec<float, 8>;
  extern __shared__ __attribute__((aligned(16))) U4 xlds_h[];
  const int N = a.N, C = a.C;
  const int slots = N * CC;
  int cur = 0;  // buffer holding X_m; the other one receives X_{m+1}

  const int tid = threadIdx.x;
  const int g = tid & (CC - 1);
  const int rs = tid / CC;
  const int RSN = blockDim.x / CC;
  uint32_t lb = blockIdx.x;
  if (a.xcd_remap) {  // (fwd_chain_lds.h: the workgroups of a sequence on one XCD)
    const uint32_t nb = gridDim.x, xq = nb / kXcds, xr = nb % kXcds, xcd = lb % kXcds, idx = lb / kXcds;
    lb = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx;
  }
  const int b = (int)(lb / (uint32_t)a.chunks);
  const int chunk = (int)(lb - (uint32_t)b * (uint32_t)a.chunks);
  const int cg = chunk * CC + g;
  const bool cg_ok = cg < a.CG;
  const int cgc = cg_ok ? cg : a.CG - 1;

  int prow[R];
  bool pok[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int p = rs + j * RSN;
    pok[j] = p < N;
    prow[j] = pok[j] ? p : N - 1;
  }

  // X_0 slice -> LDS (and the residual rows -> registers, packed)
  const __bf16* __restrict__ V0b = a.V0 + (int64_t)b * a.v0_bstride + (int64_t)cgc * 8;
  U4 resv[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const U4 v = vec_slot(ld<__bf16, 8>(V0b + (int64_t)prow[j] * C));
    if (pok[j]) xlds_h[prow[j] * CC + g] = v;
    resv[j] = v;
  }

  // W rows a step ahead, as in f32 (2*R*ND registers: half of f32's)
  WRowBf16<L> w[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    uint32_t sh;
    const WRowBf16<L> r = ld_wrow<L>(a.W[0], (int64_t)b * N + prow[j], sh);
    w[j] = align_wrow<L>(r, sh);
  }
  __syncthreads();

  for (int m = 0; m < a.M; ++m) {
    const __bf16* __restrict__ Wn = a.W[m + 1 < a.M ? m + 1 : m];
    WRowBf16<L> wn[R];
    uint32_t shn[R];
#pragma unroll
    for (int j = 0; j < R; ++j) wn[j] = ld_wrow<L>(Wn, (int64_t)b * N + prow[j], shn[j]);

    const bool store = (a.store_mask >> m) & 1;
    __bf16* __restrict__ om = a.out[m];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int p = prow[j];
      A8 acc;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc.e[i] = 0.f;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        int src = p + offs.v[k];
        if (src >= N) src -= N;
        const U4 x = xlds_h[cur + src * CC + g];
        axpy_rn<__bf16, 8>(acc, bf16_half(w[j].d[k >> 1], k & 1), slot_vec(x));
      }
      const U4 y = finish_slot<RES>(acc, resv[j]);
      if (pok[j]) {
        xlds_h[(slots - cur) + p * CC + g] = y;
        if (store && cg_ok) *reinterpret_cast<U4*>(om + ((int64_t)b * N + p) * C + (int64_t)cg * 8) = y;
      }
    }
    __syncthreads();
    cur = slots - cur;
#pragma unroll
    for (int j = 0; j < R; ++j) w[j] = align_wrow<L>(wn[j], shn[j]);
  }
}

// chord_chain_rows_k in bf16: a thread owns G channel groups (8 channels each) of each of its R rows; W rows one ROW ahead.
//   G = 2, R = 2, 1057 <= N <= 2048: sixteen channels per workgroup.   G = 1, long rows, 2113 <= N <= 4160: eight.
template <typename T, int L, int G, int R, int CAP, bool RES>
__global__ void __launch_bounds__(1024)
chord_chain_rows_k(const ChainArgsBf16 a, const Offsets offs) {
  static_assert(__is_same(T, __bf16), "the f32 kernel has no type parameter");
  static_assert(G == 1 || G == 2, "channel groups per thread");
  using A8 = Vec<float, 8>;
  extern __shared__ __attribute__((aligned(16))) U4 xlds_h[];
  const int N = a.N, C = a.C;
  constexpr int GS = CAP;  // group stride in slots: a constant, so the second group is an immediate offset
  constexpr int slots = G * GS;
  int cur = 0;
  const int tid = threadIdx.x;
  const int RSN = blockDim.x;
  uint32_t lb = blockIdx.x;
  if (a.xcd_remap) {
    const uint32_t nb = gridDim.x, xq = nb / kXcds, xr = nb % kXcds, xcd = lb % kXcds, idx = lb / kXcds;
    lb = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx;
  }
  const int b = (int)(lb / (uint32_t)a.chunks);
  const int chunk = (int)(lb - (uint32_t)b * (uint32_t)a.chunks);
  const int cg0 = chunk * G;
  const bool g1_ok = G == 2 && cg0 + 1 < a.CG;  // (an odd number of channel groups: the last workgroup owns one)
  const int cg1 = g1_ok ? cg0 + 1 : cg0;

  int prow[R];
  bool pok[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const int p = tid + j * RSN;
    pok[j] = p < N;
    prow[j] = pok[j] ? p : N - 1;
  }

  const __bf16* __restrict__ V0b = a.V0 + (int64_t)b * a.v0_bstride;
  U4 resv[R][G];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const U4 v0 = vec_slot(ld<__bf16, 8>(V0b + (int64_t)prow[j] * C + (int64_t)cg0 * 8));
    resv[j][0] = v0;
    if (pok[j]) xlds_h[prow[j]] = v0;
    if constexpr (G == 2) {
      const U4 v1 = vec_slot(ld<__bf16, 8>(V0b + (int64_t)prow[j] * C + (int64_t)cg1 * 8));
      resv[j][1] = v1;
      if (pok[j]) xlds_h[GS + prow[j]] = v1;
    }
  }

  uint32_t shc;
  WRowBf16<L> wc = ld_wrow<L>(a.W[0], (int64_t)b * N + prow[0], shc);
  wc = align_wrow<L>(wc, shc);
  __syncthreads();
  for (int m = 0; m < a.M; ++m) {
    const bool store = (a.store_mask >> m) & 1;
    __bf16* __restrict__ om = a.out[m];
    const int mn = m + 1 < a.M ? m + 1 : m;  // (the last step re-requests one of its own rows: no branch in the pipeline)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      uint32_t shn;
      const WRowBf16<L> wnx = j + 1 < R ? ld_wrow<L>(a.W[m], (int64_t)b * N + prow[j + 1 < R ? j + 1 : 0], shn)
                                        : ld_wrow<L>(a.W[mn], (int64_t)b * N + prow[0], shn);
      int p = prow[j];
      if constexpr (R > 2) asm volatile("" : "+v"(p));  // (R x L hoisted link addresses would not fit: recomputed per step)
      A8 acc0, acc1;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc0.e[i] = acc1.e[i] = 0.f;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        int src = p + offs.v[k];
        if (src >= N) src -= N;
        const __bf16 wk = bf16_half(wc.d[k >> 1], k & 1);
        axpy_rn<__bf16, 8>(acc0, wk, slot_vec(xlds_h[cur + src]));
        if constexpr (G == 2) axpy_rn<__bf16, 8>(acc1, wk, slot_vec(xlds_h[cur + GS + src]));
      }
      const U4 y0 = finish_slot<RES>(acc0, resv[j][0]);
      U4 y1 = y0;
      if constexpr (G == 2) y1 = finish_slot<RES>(acc1, resv[j][1]);
      if (pok[j]) {
        xlds_h[(slots - cur) + p] = y0;
        if constexpr (G == 2) xlds_h[(slots - cur) + GS + p] = y1;
        if (store) {
          *reinterpret_cast<U4*>(om + ((int64_t)b * N + p) * C + (int64_t)cg0 * 8) = y0;
          if constexpr (G == 2) {
            if (g1_ok) *reinterpret_cast<U4*>(om + ((int64_t)b * N + p) * C + (int64_t)cg1 * 8) = y1;
          }
        }
      }
      wc = align_wrow<L>(wnx, shn);
    }
    __syncthreads();
    cur = slots - cur;
  }
}

}  // namespace psf
