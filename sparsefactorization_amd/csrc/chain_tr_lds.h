// chain_tr_lds.h — the TRANSPOSED chain in one launch for short sequences (N <= 1024): rows of the attention map
// A_b = W_{M-1} ... W_0 without the dense map (psf_chord_chain_tr_f32 / _bf16).
//
//     Y_M = Q;   for m = M-1 .. 0:   Y_m[q,:] = sum_k W_m[(q-off_k) mod N, k] * Y_{m+1}[(q-off_k) mod N, :];   out = Y_0
//
// A one-hot column c of Q (a 1 at row r) comes out as row r of A_b in column c of `out`. Each step is the dV half of the
// backward step (spmul/spmul_cuda.cu:75-84), and the kernel is the dV loop of chord_chain_bwd_lds_k (bwd_chain_lds.h,
// bwd_chain_lds_bf16.h) with the X staging and the dW half removed: a thread owns one row (rounded up to whole waves, idle
// lanes clamped to row N-1), the running Y and W_m stay in LDS (W_m widened to f32 for bf16, rows at the odd stride L | 1 so
// the column reads ws[src * LP + k] are conflict-free), two barriers per step, nothing but `out` is written and no Y_m ever
// reaches memory. The next step's W row is requested before the links of this step are summed.
//
// Columns are independent, so a sequence's columns are dealt over several workgroups: the grid is B x chunks, a workgroup
// takes up to kChainTrGroups 16-byte slot groups (4 f32 or 8 bf16 columns each). kChainTrGroups = 4 is the LDS fit at the
// largest covered shape: 4 groups x 1024 rows x 16 bytes = 64 KB of Y beside 1024 x 21 x 4 = 84 KB of W_m at L = 20 is
// 148 KB of the CU's 160 KB; a fifth group (164 KB) does not fit. (The backward chain spends the same bytes on two groups of
// the gradient and two of X_m.) The Y area is G x 1024 x 16 bytes whatever N is, as in the backward chains: the group
// stride is a compile-time constant. That costs a short sequence with many columns occupancy — 64 KB at N = 128 with four
// groups where 8 KB would hold the rows, two workgroups per CU — and that shape was not timed. A stride taken from the launch's
// row count was tried and makes the f32 instances at L >= 15 with three or four groups spill (12 - 144 bytes of scratch), so
// it was not kept.
// The groups are spread evenly: chunks = ceil(CG / 4) workgroups of ceil(CG / chunks) groups (five groups: 3 + 2; thirteen:
// 4 + 4 + 4 + 1); a last workgroup with fewer groups repeats its last group in the idle slots (no predicate in the loop) and
// does not store it.
//
// Measured against the M per-step dV launches, both replayed from a graph (profiles/attention_queries_ab.md): 20.0 vs 41.7 us
// per chain at B = 64, N = 1024, L = 12, M = 11, R = 4, 53.1 vs 110.1 at R = 64, 9.5 vs 23.2 at B = 40, N = 128, L = 8, M = 7;
// bf16 27.0 vs 46.1, 72.2 vs 81.1, 12.0 vs 22.8. Ahead at every measured shape: chain_tr_lds_fits covers the compiled range.
//
// Arithmetic: the bits of M calls of psf_chord_spmm_bwd_{f32,bf16} with dW = NULL.
//   f32   links ascending from +0, product and sum rounded separately: the CPU oracle's dV.
//   bf16  f32 accumulator from +0, links ascending, one fused multiply-add per link (the bf16 product is exact in f32), ONE
//         rounding to bf16 per step (nearest even, a NaN stays a NaN); the rounded value is what enters the next step.
// W_m rows are read as the backward chains read them: f32 at any 4-byte alignment, bf16 element by element at any 2-byte
// alignment, nothing outside [W_m, W_m + B*N*L). Q and out are 16-byte aligned (one 16-byte access per slot).
#pragma once

#include "bwd_chain_lds.h"       // kChainBwdRows, chain_bwd_wstride; fwd_chain_lds.h: kChainMaxSteps, WRow
#include "fwd_chain_lds_bf16.h"  // U4, slot_vec, vec_slot
#include "fwd_chain_lds_launch.h"  // kChainLdsLmin, kChainLdsLmax: compiled for the forward chain's link counts

namespace psf {

constexpr int kChainTrGroups = 4;  // 16-byte slot groups a workgroup holds (the LDS fit at N = 1024, L = 20: above)

template <typename T>
struct ChainTrArgs {
  const T* W[kChainMaxSteps];  // W_m [B, N, L]
  const T* Q;                  // [B, N, R]
  T* out;                      // [B, N, R]
  int32_t M, N, R;
  int32_t CG, chunks;          // CG = R / (4 or 8) slot groups per row, chunks = workgroups per sequence
};

// One 16-byte slot of a row: its LDS / register form, the f32 accumulator beside it, and the three things a step does with it.
template <typename T>
struct TrSlot;
template <>
struct TrSlot<float> {
  static constexpr int kVec = 4;
  using Slot = float __attribute__((ext_vector_type(4)));
  using AccV = Vec<float, 4>;
  static __device__ __forceinline__ Slot load(const float* p) {
    const Vec<float, 4> v = ld<float, 4>(p);
    return Slot{v.e[0], v.e[1], v.e[2], v.e[3]};
  }
  static __device__ __forceinline__ void store(float* p, const Slot s) { st<float, 4>(p, Vec<float, 4>{{s.x, s.y, s.z, s.w}}); }
  static __device__ __forceinline__ void link(AccV& acc, float w, const Slot z) {
    axpy_rn<float, 4>(acc, w, Vec<float, 4>{{z.x, z.y, z.z, z.w}});
  }
  static __device__ __forceinline__ Slot finish(const AccV& acc) { return Slot{acc.e[0], acc.e[1], acc.e[2], acc.e[3]}; }
};
template <>
struct TrSlot<__bf16> {
  static constexpr int kVec = 8;
  using Slot = U4;
  using AccV = Vec<float, 8>;
  static __device__ __forceinline__ Slot load(const __bf16* p) { return *reinterpret_cast<const U4*>(p); }
  static __device__ __forceinline__ void store(__bf16* p, const Slot s) { *reinterpret_cast<U4*>(p) = s; }
  static __device__ __forceinline__ void link(AccV& acc, float w, const Slot z) {
    const AccV zw = widen<__bf16, 8>(slot_vec(z));
#pragma unroll
    for (int i = 0; i < 8; ++i) acc.e[i] = __builtin_fmaf(w, zw.e[i], acc.e[i]);  // madd_rn<__bf16> on the widened W
  }
  static __device__ __forceinline__ Slot finish(const AccV& acc) { return vec_slot(narrow<__bf16, 8>(acc)); }  // the one rounding
};

// A row of W_m, widened: f32 as one packed 4-byte-aligned struct, bf16 element by element (any 2-byte alignment)
template <int L>
__device__ __forceinline__ void ld_tr_wrow(const float* p, float (&w)[L]) {
  const WRow<L> r = *reinterpret_cast<const WRow<L>*>(p);
#pragma unroll
  for (int k = 0; k < L; ++k) w[k] = r.e[k];
}
template <int L>
__device__ __forceinline__ void ld_tr_wrow(const __bf16* __restrict__ p, float (&w)[L]) {
#pragma unroll
  for (int k = 0; k < L; ++k) w[k] = (float)p[k];
}

template <typename T, int L, int G>
__global__ void __launch_bounds__(1024)
chord_chain_tr_lds_k(const ChainTrArgs<T> a, const Offsets offs) {
  using S = TrSlot<T>;
  using Slot = typename S::Slot;
  constexpr int GS = kChainBwdRows, LP = chain_bwd_wstride<L>(), VEC = S::kVec;
  extern __shared__ __attribute__((aligned(16))) U4 trlds[];
  Slot* const ys = reinterpret_cast<Slot*>(trlds);            // [G][GS] Y_{m+1}, the vector entering the step
  float* const ws = reinterpret_cast<float*>(trlds + G * GS);  // [N][LP] W_m, widened
  const int N = a.N, R = a.R;
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (uint32_t)a.chunks), chunk = (int)(blockIdx.x - (uint32_t)b * (uint32_t)a.chunks);
  const int cg0 = chunk * G, ng = imin_rt(G, a.CG - cg0);  // this workgroup's slot groups [cg0, cg0 + ng), ng >= 1
  const bool pok = tid < N;
  const int p = pok ? tid : N - 1;
  const int64_t row = (int64_t)b * N + p;

  Slot y[G];
#pragma unroll
  for (int gi = 0; gi < G; ++gi) y[gi] = S::load(a.Q + row * R + (cg0 + imin_rt(gi, ng - 1)) * VEC);
  float w[L];
  ld_tr_wrow<L>(a.W[a.M - 1] + row * L, w);

  for (int m = a.M - 1; m >= 0; --m) {
    if (pok) {
#pragma unroll
      for (int gi = 0; gi < G; ++gi) ys[gi * GS + p] = y[gi];
#pragma unroll
      for (int k = 0; k < L; ++k) ws[p * LP + k] = w[k];
    }
    __syncthreads();
    ld_tr_wrow<L>(a.W[m > 0 ? m - 1 : 0] + row * L, w);  // (the last step re-requests its own row: no branch)

    // Y_m[p, :]: the transposed links, ascending
    typename S::AccV acc[G];
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[gi].e[i] = 0.f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      int src = p - offs.v[k];
      if (src < 0) src += N;
      const float wk = ws[src * LP + k];
#pragma unroll
      for (int gi = 0; gi < G; ++gi) S::link(acc[gi], wk, ys[gi * GS + src]);
    }
    __syncthreads();  // everyone has read this step's ys / ws
#pragma unroll
    for (int gi = 0; gi < G; ++gi) y[gi] = S::finish(acc[gi]);
  }
  if (pok) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi)
      if (gi < ng) S::store(a.out + row * R + (cg0 + gi) * VEC, y[gi]);
  }
}

// The shapes the one launch covers (psf_chord_chain_tr_supported). elem_bytes: 4 (f32) or 2 (bf16).
inline bool chain_tr_lds_fits(int64_t N, int32_t L, int64_t R, int32_t M, int32_t elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 2) return false;
  return N >= 1 && N <= kChainBwdRows && L >= kChainLdsLmin && L <= kChainLdsLmax && M >= 1 && M <= kChainMaxSteps && R >= 1 &&
         R % (16 / elem_bytes) == 0;
}

// Host side (chain_tr_lds_inst.hip, compiled once per element type). G = a.CG spread over a.chunks workgroups.
hipError_t launch_chain_tr_lds(int L, const ChainTrArgs<float>& a, const Offsets& offs, int64_t B, hipStream_t stream);
hipError_t launch_chain_tr_lds(int L, const ChainTrArgs<__bf16>& a, const Offsets& offs, int64_t B, hipStream_t stream);

}  // namespace psf
