// mixer_lds_bf16.h — the whole mixer of a short sequence in one launch (mixer_lds.h) for a bf16 model: V0 = g(data), then M
// steps V <- W_m V (+ V0) with every W_m = fs[m](data) computed on chip and the sequence's V resident in LDS as bf16.
// Its two halves exist and are pinned bit for bit; this kernel joins them and adds no arithmetic of its own:
//   * an MLP tile is mlp_fwd_bf16_k's unit loop (mlp_bf16_tile.h: mlp_unit — GEMM1 from the bias, the GELU on the
//     accumulator registers, GEMM2 over the MLP's units in unit order, ONE rounding to bf16), on the images of
//     mlp_bf16_image.h, which the producer's pack kernel writes for all M + 1 MLPs;
//   * a step is fwd_chain_lds_bf16.h's: f32 accumulator, links ascending with the fused exact product (madd_rn<__bf16>), the
//     residual with add_rn from packed registers, one narrow (finish_slot), the bf16 slot to the other X buffer and, where
//     the store mask says so, to memory.
// W_m is ROUNDED TO bf16 before the step reads it, as the producer rounds it before it writes it: the result is the bits of
// psf_mlp_fwd_bf16 followed by psf_chord_chain_fwd_bf16.
//
// One workgroup = one sequence with all its C channels (CG = C / 8 slots of 16 bytes per row). A wave owns the token tiles
// t = wave, wave + nwaves (32 tokens each, at most two): their data rows are loaded once as B-operand fragments (the 16-byte
// loads of mlp_fwd_bf16_k, ceil(E / 16) k-steps, the half-step beyond E zero) and stay in registers for all M + 1 MLPs. Per
// step each wave writes its tiles' W rows to the LDS W tile (row stride WS = 12 or 20 entries); after a barrier every thread
// accumulates its slots (at most two) from the LDS-resident X_m; the NEXT MLP's units stream into LDS by LDS-DMA meanwhile.
// HBM traffic of the whole mixer: the data rows, the weight images and whatever results the caller wants.
//
// Two rules of this code base (psf_common.h "LDS results in kernels that also issue MFMAs", psf_common.h: dma_wait_all):
//   * every LDS operand of a link group, and of an MLP unit, is in registers and waited for IN FULL before its first consumer;
//   * the LDS-DMA of an image is counted by vmcnt only, so every wave drains it explicitly (s_waitcnt vmcnt(0)) before the
//     barrier that publishes the image. Nothing here relies on the compiler doing so.
//
// Limits (plan_mixer_lds_bf16, mixer_lds_bf16_inst.hip): N a multiple of 32, 32 <= N <= 512; C = 8 or 16; E a multiple of 8,
// 8 <= E <= 64; h <= 128; 4 <= L <= 20; 1 <= M <= 31. No recipe input, no per-step form for longer sequences.
#pragma once

#include "fwd_chain_lds_bf16.h"
#include "mixer_lds_bf16_launch.h"
#include "mlp_bf16_tile.h"

namespace psf {

__device__ __forceinline__ void behind_wait(U4& r) { asm volatile("" : "+v"(r)); }
__device__ __forceinline__ void behind_wait(uint32_t& r) { asm volatile("" : "+v"(r)); }

using U2 = uint32_t __attribute__((ext_vector_type(2)));  // half a slot: 4 bf16

__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) {
  return (uint32_t)psf_mlp_bf16::bf16_rne_bits(lo) | ((uint32_t)psf_mlp_bf16::bf16_rne_bits(hi) << 16);
}

// (T is __bf16: the overload on a leading type parameter keeps the f32 kernel's name, as chord_chain_lds_k<bf16> does.)
// KS = ceil(E / 16) k-steps of the first GEMM.
template <typename T, int KS, bool RES>
__global__ void __launch_bounds__(512)
chord_mixer_lds_k(const MixerLdsBf16Args a, const Offsets offs) {
  static_assert(__is_same(T, __bf16), "the f32 kernel has no type parameter");
  namespace mb = psf_mlp_bf16;
  using psf_x3::bf16x8;
  using psf_x3::f32x16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_h[];
  const int N = a.N, CG = a.CG, WS = a.WS, L = a.L, slots = N * CG;
  U4* __restrict__ xb = reinterpret_cast<U4*>(smem_h);             // two X buffers of `slots` slots
  unsigned char* __restrict__ sW = smem_h + 2 * slots * 16;        // N rows of WS bf16
  unsigned char* __restrict__ sImg = sW + N * WS * 2;              // the units of one MLP

  const int tid = threadIdx.x, lane = tid & 63, wave64 = tid & ~63, nthreads = blockDim.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthreads >> 6;
  const int c = lane & 31, half = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * N;  // the sequence's first token

  auto stage_image = [&](int k) {  // the units of MLP k -> sImg (LDS-DMA; the caller orders it against the readers)
    const unsigned char* src = a.images + (size_t)a.first_unit[k] * mb::kImgBytes;
    const int vecs = (a.first_unit[k + 1] - a.first_unit[k]) * mb::kImgVecs;
    for (int v0 = 0; v0 < vecs; v0 += nthreads) {
      const int v = v0 + tid;
      if (v < vecs)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 16 * (size_t)v),
                                         (__attribute__((address_space(3))) void*)(sImg + 16 * (v0 + wave64)), 16, 0, 0);
    }
  };
  // MLP k on one tile: the unit loop of mlp_fwd_bf16_k; register r of lane (tok, half) is Y^T[o = cd_row(r, half)][tok]
  auto mlp_tile = [&](int k, const bf16x8(&x)[KS]) {
    const int nu = a.first_unit[k + 1] - a.first_unit[k];
    f32x16 acc2 = {};
    for (int u = 0; u < nu; ++u) mb::mlp_unit<KS, true>(sImg + u * mb::kImgBytes, x, u == 0, acc2, c, half);
    return acc2;
  };

  stage_image(0);
  // this wave's token tiles t = wv, wv + nwaves (at most two): their data rows, kept for all M + 1 MLPs
  bf16x8 xf[2][KS];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = wv + i * nwaves;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (t < a.TT && 16 * s + 8 * half < a.E) v = *reinterpret_cast<const uint4*>(a.X + (row0 + 32 * t + c) * a.E + 16 * s + 8 * half);
      xf[i][s] = __builtin_bit_cast(bf16x8, v);
    }
  }
  dma_wait_all();
  __syncthreads();  // the image of g has landed in every wave's view

  // V0 = g(data): registers 4 q .. 4 q + 3 of lane (tok, half) are channels 8 q + 4 half .. + 3 of its token — half a slot
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int t = wv + i * nwaves;
    if (t >= a.TT) break;  // wave-uniform
    const f32x16 y = mlp_tile(0, xf[i]);
    unsigned char* dst = smem_h + (size_t)(32 * t + c) * CG * 16 + 8 * half;
    for (int q = 0; q < CG; ++q)
      *reinterpret_cast<U2*>(dst + 16 * q) = q == 0 ? U2{bf16_pair(y[0], y[1]), bf16_pair(y[2], y[3])}
                                                     : U2{bf16_pair(y[4], y[5]), bf16_pair(y[6], y[7])};
  }
  __syncthreads();  // X_0 complete; every wave is done with g's image
  stage_image(1);
  // accumulate phase: thread tid owns slots tid and tid + nthreads (row = slot / CG, channel group = slot % CG)
  U4 resv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int sl = tid + j * nthreads;
    resv[j] = sl < slots ? xb[sl] : U4{0u, 0u, 0u, 0u};
    if (sl < slots && a.V0 != nullptr) *reinterpret_cast<U4*>(a.V0 + (row0 * CG + sl) * 8) = resv[j];
  }
  dma_wait_all();
  __syncthreads();  // the image of fs[0] has landed

  int cur = 0;
  for (int m = 0; m < a.M; ++m) {
    // (1) W_m rows of this wave's tiles, rounded to bf16 -> sW
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = wv + i * nwaves;
      if (t >= a.TT) break;
      const f32x16 y = mlp_tile(m + 1, xf[i]);
      unsigned char* dst = sW + (size_t)(32 * t + c) * WS * 2 + 8 * half;
#pragma unroll
      for (int q = 0; q < 3; ++q)  // entries 8 q + 4 half .. + 3: inside the row's WS entries whenever the first is a link
        if (8 * q + 4 * half < L)
          *reinterpret_cast<U2*>(dst + 16 * q) = U2{bf16_pair(y[4 * q], y[4 * q + 1]), bf16_pair(y[4 * q + 2], y[4 * q + 3])};
    }
    __syncthreads();  // W_m complete; every wave is done with this step's image
    if (m + 1 < a.M) stage_image(m + 2);  // lands during the accumulate phase

    // (2) X_{m+1}[p] = bf16( sum_k W_m[p,k] X_m[(p + off_k) mod N] (+ V0[p]) ), links ascending. Links are taken four at a
    //     time and every LDS operand of a group is waited for in full before its arithmetic.
    const bool store = (a.store_mask >> m) & 1;
    uint16_t* __restrict__ om = a.out[m];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int sl = tid + j * nthreads;
      if (sl < slots) {
        const int p = CG == 2 ? sl >> 1 : sl, g = sl - p * CG;
        Vec<float, 8> acc;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc.e[i] = 0.f;
        const unsigned char* __restrict__ wrow = sW + (size_t)p * WS * 2;
        for (int k0 = 0; k0 < L; k0 += 4) {
          U4 x[4];
          const U2 wd = *reinterpret_cast<const U2*>(wrow + 2 * k0);  // entries k0 .. k0 + 3 (WS is a multiple of 4)
          uint32_t w0 = wd.x, w1 = wd.y;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k = k0 + i < L ? k0 + i : L - 1;
            int src = p + offs.v[k];
            if (src >= N) src -= N;
            x[i] = xb[cur + src * CG + g];
          }
          lds_wait_all();
#pragma unroll
          for (int i = 0; i < 4; ++i) behind_wait(x[i]);
          behind_wait(w0), behind_wait(w1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (k0 + i < L) axpy_rn<__bf16, 8>(acc, bf16_half(i < 2 ? w0 : w1, i & 1), slot_vec(x[i]));
        }
        const U4 r = finish_slot<RES>(acc, resv[j]);
        xb[(slots - cur) + sl] = r;
        if (store) *reinterpret_cast<U4*>(om + (row0 * CG + sl) * 8) = r;
      }
    }
    dma_wait_all();
    __syncthreads();  // X_{m+1} complete, the next image landed, sW free
    cur = slots - cur;
  }
}

}  // namespace psf
