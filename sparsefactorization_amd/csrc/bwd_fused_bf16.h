// bwd_fused_bf16.h — the fused backward step of bwd_fused.h (dV and dW of one chord step in ONE kernel) for bf16 rows of
// 8, 16, 32, 64 or 128 channels:
//
//   dV[b,q,:] = sum_k W[b,(q-off_k) mod N,k] * dZ[b,(q-off_k) mod N,:]          spmul/spmul_cuda.cu:75-84
//   dW[b,p,k] = sum_c dZ[b,p,c] * V[b,(p+off_k) mod N,c]                         spmul/spmul_cuda.cu:102-111
//
// Structure of chord_bwd_fused_k: 256 threads, one row per thread, a 16-byte group is 8 channels (TG = C / 8, tile
// TR = 256 / TG rows: 256 at C = 8 down to 16 at C = 128). Staged by LDS-DMA, all before ONE barrier: the dZ window
// [q0 - TR, q0 + TR), the V window [q0, q0 + 2 TR) and the two W tiles under the dZ window as one flat image of 16-byte
// chunks (a tile is TR L / 8 chunks exactly). Far dZ / V rows and the far W elements (2-byte loads at a 2 L-byte stride) go
// to registers. dV is stored plainly; the dW tile is assembled in LDS as bf16 and leaves flat in 16-byte chunks.
//
// Arithmetic is that of the two bf16 window kernels (bwd_window.h), so the route is invisible in the results:
//   dV  f32 accumulator, links ascending, axpy_rn<__bf16, 8> (exact products fused), one narrow to bf16 — the bits of
//       chord_dv_win_k<bf16>, i.e. bf16_rne of the f32 oracle;
//   dW  per lane a running madd_rn<__bf16> over its 8 channels (c ascending, from 0), row_group_sum<TG>, one rounding to bf16 —
//       the order of chord_dw_win_k<bf16>, NOT the packed pairwise form of the f32 fused kernel: bit-identical to that kernel.
// Full tiles only: N a multiple of TR and at least 2 TR, every far offset a multiple of TR, C = 8 TG exactly, chunk-clean W / dW;
// the host (psf_chord.hip: pick_fused_step_bf16) sends anything else to the two window kernels.
#pragma once

#include "bwd_window.h"

namespace psf {

constexpr int kFusedBf16Threads = 256;

// W image in LDS as in BwdFusedCfg: the tile under the window's lower half, then the one under its upper half, as ONE flat
// array of 2 TR rows (row wr of the window, link k at element wr L + k), then a pad for the surplus lanes of the last pass.
template <int L, int TGS, int NT = kFusedBf16Threads>
struct BwdFusedBf16Cfg {
  using B = BwdWinCfg<__bf16, L, TGS, 1, NT>;
  static constexpr int tile_vecs = B::TR * L / 8;
  static constexpr int passes = (tile_vecs + NT - 1) / NT;
  static constexpr int full = tile_vecs / NT;            // passes with every lane inside the tile
  static constexpr int rem = tile_vecs - full * NT;      // lanes of the last pass inside it (0: no partial pass)
  static constexpr int w_img_bytes = (tile_vecs + passes * NT) * 16;
  static constexpr int lds_bytes = 2 * B::win_bytes + w_img_bytes;
  static_assert(B::TR % 8 == 0, "tiles start on 16-byte boundaries");
};

template <int L, int TGS, int NT>
__global__ void __launch_bounds__(NT)
chord_bwd_fused_bf16_k(const __bf16* __restrict__ dZ, const __bf16* __restrict__ W, const __bf16* __restrict__ V,
                       __bf16* __restrict__ dW, __bf16* __restrict__ dV, const Geom gm, const Offsets offs, const int64_t w_total) {
  using T = __bf16;
  using Cfg = BwdWinCfg<T, L, TGS, 1, NT>;
  constexpr int VEC = Cfg::VEC, TG = Cfg::TG, TR = Cfg::TR, KN = Cfg::KN, NF = Cfg::NF;
  using V8 = Vec<T, VEC>;
  using FC = BwdFusedBf16Cfg<L, TGS, NT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  V8* __restrict__ sZ = reinterpret_cast<V8*>(smem);
  V8* __restrict__ sV = reinterpret_cast<V8*>(smem + Cfg::win_bytes);
  V8* __restrict__ sWV = reinterpret_cast<V8*>(smem + 2 * Cfg::win_bytes);
  const T* __restrict__ sWF = reinterpret_cast<const T*>(sWV);
  T* __restrict__ sOutF = reinterpret_cast<T*>(sWV);  // the dW tile image: written after the last read of the W tiles

  int b, tile, chunk;
  decode_block(gm, b, tile, chunk);  // chunks_c == 1
  const int tid = threadIdx.x, wave64 = tid & ~63;
  const int g = tid & (TG - 1), pl = tid >> TGS;  // one row per thread: row slot = local row
  const int q0 = tile * TR, N = gm.N, C = gm.C;
  const T* __restrict__ Zb = dZ + (int64_t)b * N * C;
  const T* __restrict__ Wb = W + (int64_t)b * N * L;
  const T* __restrict__ Vb = V + (int64_t)b * gm.v_bstride;

  // Every row block this workgroup touches is TR-aligned and never wraps inside (host-checked), so every address is a
  // wave-uniform base plus one per-lane byte offset (bwd_fused.h).
  constexpr uint32_t rowB = TG * 16u;          // C = 8 TG exactly (host-checked)
  const uint32_t voff = (uint32_t)tid * 16u;  // lane's row pl of a block, channel group g: pl rowB + 16 g
  const char* __restrict__ Zbb = reinterpret_cast<const char*>(Zb);
  const char* __restrict__ Vbb = reinterpret_cast<const char*>(Vb);
  int prev0 = q0 - TR;
  if (prev0 < 0) prev0 += N;
  int next0 = q0 + TR;
  if (next0 >= N) next0 -= N;
  // (1) dZ window: slot wr <-> row (q0 - TR + wr) mod N;  V window: slot wr <-> row (q0 + wr) mod N  (one pass per block)
  static_assert(Cfg::win_vecs / NT == 2, "one row per thread: a window is two passes of TR rows");
  stage16g<0>(sbase(Zbb + (uint32_t)prev0 * rowB) + voff, sZ + wave64);
  stage16g<0>(sbase(Vbb + (uint32_t)q0 * rowB) + voff, sV + wave64);
  stage16g<0>(sbase(Zbb + (uint32_t)q0 * rowB) + voff, sZ + NT + wave64);
  stage16g<0>(sbase(Vbb + (uint32_t)next0 * rowB) + voff, sV + NT + wave64);
  // (2) far links -> registers
  V8 farZ[NF > 0 ? NF : 1], farV[NF > 0 ? NF : 1];
  T farW[NF > 0 ? NF : 1];
  int src0[NF > 0 ? NF : 1];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    src0[f] = q0 - offs.v[KN + f];
    if (src0[f] < 0) src0[f] += N;
    int dst0 = q0 + offs.v[KN + f];
    if (dst0 >= N) dst0 -= N;
    farZ[f] = ldg<T, VEC>(sbase(Zbb + (uint32_t)src0[f] * rowB) + voff);
    farV[f] = ldg<T, VEC>(sbase(Vbb + (uint32_t)dst0 * rowB) + voff);
  }
  // (3) the two W tiles under the backward window, flat 16-byte chunks. The upper tile's last pass clamps (its surplus lanes
  //     land in the pad); the lower tile's would land on the upper tile's first chunks, so it is lane-masked and comes LAST
  //     of all requests (3c).
  auto w_tile = [&](int row0) { return reinterpret_cast<const char*>(W + ((int64_t)b * N + row0) * L); };
  {
    const char* __restrict__ wp = w_tile(prev0);
    const char* __restrict__ wc = w_tile(q0);
#pragma unroll
    for (int n = 0; n < FC::full; ++n) {
      stage16g<0>(sbase(wp + (size_t)n * NT * 16) + voff, sWV + n * NT + wave64);
      stage16g<0>(sbase(wc + (size_t)n * NT * 16) + voff, sWV + FC::tile_vecs + n * NT + wave64);
    }
    if constexpr (FC::rem > 0) {
      const uint32_t i = (uint32_t)imin_rt(tid, FC::rem - 1);
      stage16g<0>(sbase(wc + (size_t)FC::full * NT * 16) + i * 16u, sWV + FC::tile_vecs + FC::full * NT + wave64);
    }
  }
  // (3b) far-link W elements: element (src0 + pl) of the link's column of row-major W — 2-byte loads at a 2 L-byte stride
#pragma unroll
  for (int f = 0; f < NF; ++f)
    farW[f] = *reinterpret_cast<const PSF_GLOBAL T*>(sbase(reinterpret_cast<const char*>(Wb + (int64_t)src0[f] * L + (KN + f))) +
                                                     (uint32_t)pl * (uint32_t)(L * sizeof(T)));
  // (3c) the lower W tile's partial pass
  if constexpr (FC::rem > 0) {
    if (tid < FC::rem)
      stage16g<0>(sbase(w_tile(prev0) + (size_t)FC::full * NT * 16) + voff, sWV + FC::full * NT + wave64);
  }
  __syncthreads();

  // (4) dV, links ascending, f32 accumulator, one rounding
  {
    Vec<float, VEC> acc;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc.e[i] = 0.0f;
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      const int wr = TR + pl - chord_off(k);  // in [0, 2 TR)
      axpy_rn<T, VEC>(acc, sWF[wr * L + k], sZ[(wr << TGS) + g]);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) axpy_rn<T, VEC>(acc, farW[f], farZ[f]);
    // dV is a plain store: the next (earlier) step reads it at once
    stg<T, VEC>(sbase(reinterpret_cast<char*>(dV + ((int64_t)b * N + q0) * C)) + lane_off(voff), narrow<T, VEC>(acc));
  }
  // (5) dW row dots (the tile's dZ rows are the upper half of the dZ window): chord_dw_win_k<bf16>'s order
  float dots[L];
  {
    const V8 dz = sZ[((TR + pl) << TGS) + g];
#pragma unroll
    for (int k = 0; k < L; ++k) {
      V8 x;
      if (k < KN) x = sV[((pl + chord_off(k)) << TGS) + g];
      else x = farV[k - KN < NF ? k - KN : 0];
      float part = 0.0f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) part = madd_rn<T>(part, dz.e[i], x.e[i]);
      dots[k] = row_group_sum<TG>(part);
    }
  }
  __syncthreads();  // every thread is done with the W tiles: their first image becomes the dW tile
  if (g == 0) {
#pragma unroll
    for (int k = 0; k < L; ++k) sOutF[pl * L + k] = (T)dots[k];  // the one rounding of the element
  }
  __syncthreads();
  // (6) flat store of the dW tile: TR L / 8 whole chunks (full tiles of chunk-clean buffers: host-checked), non-temporal as in
  //     the f32 kernel (nothing reads dW before the end of the chain)
  PSF_GLOBAL char* ob = sbase(reinterpret_cast<char*>(dW + ((int64_t)b * N + q0) * L));
  const uint32_t vo = lane_off(voff);
  const V8* __restrict__ sOutV = reinterpret_cast<const V8*>(sOutF);
#pragma unroll
  for (int n = 0; n < FC::passes; ++n) {
    const int i = n * NT + tid;
    if (n < FC::full || i < FC::tile_vecs) {
      using F4 = float __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(*reinterpret_cast<const F4*>(&sOutV[i]), reinterpret_cast<PSF_GLOBAL F4*>(ob + ((uint32_t)(n * NT) * 16u + vo)));
    }
  }
  (void)w_total;
}

}  // namespace psf
