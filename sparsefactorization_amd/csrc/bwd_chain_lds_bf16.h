// bwd_chain_lds_bf16.h — the one-launch LDS-resident backward chain (bwd_chain_lds.h) in bfloat16: N <= 1024, C = 8 or 16.
//
// Same decomposition as the f32 kernel: one workgroup per sequence, one thread per row (rounded up to whole waves, idle lanes
// clamped to row N-1), the gradient entering the step, X_m and W_m staged in LDS per step, two barriers per step, dW_m written
// per step, dV0 once at the end; no g_m ever reaches memory. What differs:
//   * a 16-byte LDS slot holds one row x EIGHT bf16 channels, so G = C / 8 slot groups (1 or 2) cover C = 8 or 16. W_m is
//     widened to f32 when it is staged (exact) and kept at the f32 kernel's odd stride L | 1, so the column reads
//     ws[src * LP + k] are conflict-free and the LDS footprint is that of the f32 C = 4 / 8 instances at the same G:
//     2 G 1024 16 + N (L | 1) 4 bytes.
//   * W_m and dW_m rows are L bf16 values at ANY 2-byte alignment (for odd L every other row starts mid-dword anyway): they
//     are read and written with plain 2-byte accesses, element by element, so nothing outside [W_m, W_m + B N L) is read and
//     nothing outside [dW_m, dW_m + B N L) is written — no covering dwords. dOut, dV0 and every X_m are 16-byte aligned (one
//     16-byte access per slot).
//
// Arithmetic contract: the BITS of the per-step bf16 route (psf_chord_chain_bwd_bf16) at 16-byte-aligned operands.
//   g_m (dV)   per output element an f32 accumulator from +0, links ascending, each term ONE fused multiply-add
//              (madd_rn<__bf16>: the product of two bf16 values is exact in f32); rounded to bf16 ONCE with the plain cast
//              (round to nearest even, a NaN stays a NaN). The rounded value is what goes to LDS and into the next step, as
//              dX_steps[m] is a bf16 tensor on the per-step route.
//   dW_m[p,k]  per 8-channel group a running madd_rn over the channels ascending from +0. C = 8 rounds that partial;
//              C = 16 rounds add_rn(partial(channels 0..7), partial(channels 8..15)) — what chord_dw_win_k<bf16>
//              (row_group_sum<2>) and chord_dw_generic_k<bf16, 8> (two lanes per row) compute; a two-term sum has no order.
//   residual   dV0 = ((g_M + g_{M-1}) + ... + g_1) + g_0 over the bf16-ROUNDED g_m, summed left to right in an f32 register
//              and rounded once: psf_sum_tensors_bf16. Without the residual dV0 = g_0.
// Nothing is contracted beyond the explicit fused multiply-adds.
#pragma once

#include "bwd_chain_lds.h"       // kChainBwdRows, chain_bwd_wstride
#include "fwd_chain_lds_bf16.h"  // U4, slot_vec, vec_slot

namespace psf {

struct ChainBwdArgsBf16 {
  const __bf16* W[kChainMaxSteps];  // W_m [B, N, L], 2-byte aligned
  const __bf16* X[kChainMaxSteps];  // X_m [B, N, C]: X[0] = V0, X[m] = the forward's result of step m-1
  __bf16* dW[kChainMaxSteps];       // dW_m [B, N, L], 2-byte aligned
  const __bf16* dOut;               // [B, N, C]
  __bf16* dV0;                      // [B, N, C]
  int32_t M, N, C;
};

// (T is __bf16: the overload on a leading type parameter keeps the f32 kernel's name and symbol as they are)
template <typename T, int L, int G, bool RES>
__global__ void __launch_bounds__(1024)
chord_chain_bwd_lds_k(const ChainBwdArgsBf16 a, const Offsets offs) {
  static_assert(__is_same(T, __bf16), "the f32 kernel has no type parameter");
  static_assert(G == 1 || G == 2, "C = 8 or 16");
  using B8 = Vec<__bf16, 8>;
  using A8 = Vec<float, 8>;
  constexpr int GS = kChainBwdRows, LP = chain_bwd_wstride<L>();
  extern __shared__ __attribute__((aligned(16))) U4 blds_h[];
  U4* const gs = blds_h;                                            // [G][GS] the gradient entering the step (bf16)
  U4* const xs = blds_h + G * GS;                                   // [G][GS] X_m (bf16)
  float* const ws = reinterpret_cast<float*>(blds_h + 2 * G * GS);  // [N][LP] W_m, widened
  const int N = a.N, C = a.C;
  const int tid = threadIdx.x, b = blockIdx.x;
  const bool pok = tid < N;
  const int p = pok ? tid : N - 1;
  const int64_t row = (int64_t)b * N + p;

  U4 g[G];      // the row of the running gradient, bf16
  A8 racc[G];   // the residual sum, f32
#pragma unroll
  for (int gi = 0; gi < G; ++gi) {
    const B8 v = ld<__bf16, 8>(a.dOut + row * C + gi * 8);
    g[gi] = vec_slot(v);
    racc[gi] = widen<__bf16, 8>(v);
  }

  for (int m = a.M - 1; m >= 0; --m) {
    // stage: this row of the gradient, of X_m and of W_m (element loads: any 2-byte alignment, nothing read beyond the row)
    const __bf16* __restrict__ wrow = a.W[m] + row * L;
    float w[L];
#pragma unroll
    for (int k = 0; k < L; ++k) w[k] = (float)wrow[k];
    if (pok) {
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        xs[gi * GS + p] = vec_slot(ld<__bf16, 8>(a.X[m] + row * C + gi * 8));
        gs[gi * GS + p] = g[gi];
      }
#pragma unroll
      for (int k = 0; k < L; ++k) ws[p * LP + k] = w[k];
    }
    __syncthreads();

    // dW_m[p, :]: per 8-channel group a running sum over the channels; two groups are added, then one rounding
    B8 gv[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi) gv[gi] = slot_vec(g[gi]);
    __bf16 dw[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
      int src = p + offs.v[k];
      if (src >= N) src -= N;
      float part[G];
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        const B8 x = slot_vec(xs[gi * GS + src]);
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = madd_rn<__bf16>(acc, gv[gi].e[i], x.e[i]);
        part[gi] = acc;
      }
      float s = part[0];
      if constexpr (G == 2) s = add_rn(part[0], part[1]);
      dw[k] = (__bf16)s;
    }
    if (pok) {
      __bf16* __restrict__ dwrow = a.dW[m] + row * L;
#pragma unroll
      for (int k = 0; k < L; ++k) dwrow[k] = dw[k];
    }

    // g_m[p, :]: the transposed links, ascending
    A8 acc[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[gi].e[i] = 0.f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      int src = p - offs.v[k];
      if (src < 0) src += N;
      const float wk = ws[src * LP + k];
#pragma unroll
      for (int gi = 0; gi < G; ++gi) {
        const A8 z = widen<__bf16, 8>(slot_vec(gs[gi * GS + src]));
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[gi].e[i] = __builtin_fmaf(wk, z.e[i], acc[gi].e[i]);  // madd_rn<__bf16> on the widened W
      }
    }
    __syncthreads();  // everyone has read this step's gs / xs / ws
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      const B8 r = narrow<__bf16, 8>(acc[gi]);  // the one rounding of g_m
      g[gi] = vec_slot(r);
      if constexpr (RES) {
        const A8 rw = widen<__bf16, 8>(r);
#pragma unroll
        for (int i = 0; i < 8; ++i) racc[gi].e[i] = add_rn(racc[gi].e[i], rw.e[i]);
      }
    }
  }
  if (pok) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
      U4 y = g[gi];
      if constexpr (RES) y = vec_slot(narrow<__bf16, 8>(racc[gi]));
      *reinterpret_cast<U4*>(a.dV0 + row * C + gi * 8) = y;
    }
  }
}

// Host side (bwd_chain_lds_bf16_inst.hip)
bool chain_bwd_lds_bf16_fits(int64_t N, int64_t C, int32_t L, int32_t M);
hipError_t launch_chain_bwd_lds_bf16(int L, int G, bool res, const ChainBwdArgsBf16& a, const Offsets& offs, int B, hipStream_t stream);

}  // namespace psf
