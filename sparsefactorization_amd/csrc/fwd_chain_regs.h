// fwd_chain_regs.h — the WHOLE forward chain of a LONG sequence in one launch: X in registers, W streamed through LDS.
//
//     X_0 = V0;  X_{m+1}[p,:] = sum_k W_m[p,k] * X_m[(p+off_k) mod N,:]  (+ V0[p,:])     m = 0 .. M-1;   only X_M is stored
//
// The per-step kernels move 156 B per row-step at C = 8, of which only the 60 B of W are needed when nothing but the last X
// is returned. The LDS-resident chains (fwd_chain_lds.h) remove the rest up to N = 4160; beyond that a channel pair of a
// sequence no longer leaves LDS room to stage W. Here X does not live in LDS at all:
//
//   ownership   a workgroup of T threads owns one sequence and one channel PAIR (8 bytes per row), N = T * J rows; thread t
//               owns rows t + T j, j < J, of X_m, X_{m+1} (and V0 with the residual) in registers. The j loop is fully unrolled:
//               every register-array index is a constant.
//   links       default chord offsets only. An offset that is a multiple of T reads the thread's OWN registers,
//               x[(j + off / T) mod J]: link 0 and, at T = 512, the five links 512 .. 8192. The near links (offset < T) need
//               other threads' rows, and only of the block in hand and the next one: the X exchange ring, 4 slots of T * 8 bytes,
//               position = row mod 4T (4T divides N: the wrap mod N is free). In phase j every thread writes its row of block
//               j + 2; that slot was last read two phases (two barriers) ago. A fifth slot behind slot 3 mirrors slot 0, so a
//               read that runs from slot 3 into the next block needs no wrap: every ring address is a per-slot base register
//               plus an immediate.
//   W           staged exactly as chord_fwd_win_k stages it: the row block's T * L floats are contiguous in memory, copied
//               flat by 16-byte LDS-DMA chunks (coalesced), read back as per-row LDS words (row stride L = 15 dwords: odd,
//               conflict-free). kSlots = 4 slots of one row block each. Behind a phase's barrier the fill of block
//               g + kSlots - 1 is issued into the slot the previous phase read, so while block g is read and accumulated
//               THREE blocks (90 KB per CU) are in flight; at the next phase's counted vmcnt the oldest of them has to have
//               landed and two (60 KB) may stay outstanding across the barrier. Default cache policy, not nt: the
//               other workgroups of the sequence (one per channel pair, consecutive logical ids = one XCD) re-read W from L2.
//               The DMAs are inline assembly (x3_gemm.h: glds16): hipcc's alias rule for the builtin would make every LDS read
//               wait for vmcnt(0); the source counts them itself, and the kernel has NO other vector-memory operation between
//               the V0 loads (waited for before the first DMA) and the final stores (behind vmcnt(0)).
//   barriers    one per phase, J per step, none between steps. No communication between workgroups of any kind.
//
// Arithmetic: links ascending, a rounded product then a rounded sum, then the residual — the per-step kernels' order, so the
// results are bit-identical.
#pragma once

#include <utility>

#include "fwd_chain_lds.h"  // kChainMaxSteps
#include "psf_common.h"

namespace psf {

struct ChainRegsArgs {
  const float* W[kChainMaxSteps];  // W_m [B, N, L], 16-byte aligned
  const float* V0;                 // [B, N, C] or [N, C] (v0_bstride == 0: RES = false only)
  float* out;                      // X_M [B, N, C]
  int64_t v0_bstride;
  int32_t M, C, pairs;             // pairs = C / 2 workgroups per sequence
  int32_t xcd_remap;               // 1: consecutive logical workgroups share an XCD (knob "xcd_remap")
};

template <int L, int T>
struct ChainRegsCfg {
  static constexpr int kChunks = T * L / 4;           // 16-byte chunks of a row block's W
  static constexpr int kFull = kChunks / T;           // passes in which every thread copies a chunk
  static constexpr int kRem = kChunks - kFull * T;    // chunks of the last, partial pass (its surplus lanes re-read the last one)
  static constexpr int kPasses = kFull + (kRem > 0);  // DMA instructions per wave and block
  static constexpr int kSlotBytes = kPasses * T * 16;
  static constexpr int kRingBytes = 5 * T * 8;        // X exchange ring: four slots and a mirror of slot 0 behind slot 3
  static constexpr int kSlots = imin(4, (kLdsPerCu - kRingBytes) / kSlotBytes);
  static constexpr int kLdsBytes = kSlots * kSlotBytes + kRingBytes;
  static_assert(T % 64 == 0 && (T * L) % 4 == 0 && kSlots >= 2, "whole waves, whole chunks, a slot to read and one to fill");
};

// 16 bytes per lane global -> LDS; the wave's 64 lanes fill 1 KB at the LDS address in M0 (x3_gemm.h: glds16)
__device__ __forceinline__ void chain_regs_dma16(uint32_t lds_at, uint32_t voff, const unsigned char* base) {
  uint32_t m0_saved;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
      : "=&s"(m0_saved)
      : "s"(lds_at), "v"(voff), "s"(base)
      : "memory");
}

template <int... Js, class F>
__device__ __forceinline__ void chain_regs_each(std::integer_sequence<int, Js...>, F&& f) {
  (f(std::integral_constant<int, Js>{}), ...);
}

template <int L, int T, int J, bool RES>
__global__ void __launch_bounds__(T)
chord_chain_regs_k(const ChainRegsArgs a) {
  using Cfg = ChainRegsCfg<L, T>;
  using V2 = Vec<float, 2>;
  using F2 = float __attribute__((ext_vector_type(2)));
  constexpr int N = T * J, S = Cfg::kSlots, P = Cfg::kPasses;
  static_assert(J % 4 == 0 && J % S == 0, "ring positions are row mod 4T; a step begins at W slot 0");
  static_assert(L >= 2 && chord_off(L - 1) < N, "every offset below N");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[Cfg::kLdsBytes];

  const int tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6);
  uint32_t lb = blockIdx.x;
  if (a.xcd_remap) {  // (as in chord_chain_lds_k: the workgroups of a sequence on one XCD)
    const uint32_t nb = gridDim.x, xq = nb / kXcds, xr = nb % kXcds, xcd = lb % kXcds, idx = lb / kXcds;
    lb = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + idx;
  }
  const int b = (int)(lb / (uint32_t)a.pairs);
  const int q = (int)(lb - (uint32_t)b * (uint32_t)a.pairs);
  const int C = a.C;

  // ---- X_0 (and the residual rows) -> registers; every load has landed, and the compiler knows it, before the first DMA
  const float* __restrict__ V0b = a.V0 + (int64_t)b * a.v0_bstride + (int64_t)q * 2;
  V2 xa[J], xb[J], v0[RES ? J : 1];
  (void)v0;
  chain_regs_each(std::make_integer_sequence<int, J>{}, [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    xa[j] = ld<float, 2>(V0b + (int64_t)(tid + T * j) * C);
  });
  chain_regs_each(std::make_integer_sequence<int, J>{}, [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    behind_wait(xa[j]);
    if constexpr (RES) v0[j] = xa[j];
  });
  dma_wait_all();

  // ---- the W ring. Block g = m J + j of the chain goes to slot g mod S = j mod S.
  const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)lds);
  const uint32_t lds_wave = lds0 + wave * 1024u;
  const uint32_t voff = (uint32_t)tid * 16u;
  const uint32_t voff_last = (uint32_t)imin_rt(tid, Cfg::kRem > 0 ? Cfg::kRem - 1 : 0) * 16u;
  const int64_t seq_bytes = (int64_t)b * N * L * 4;
  auto fill = [&](const unsigned char* wseq, int jb, int slot) {  // (jb, slot: constants after unrolling)
    const unsigned char* base = wseq + (int64_t)jb * (T * L * 4);
    const uint32_t at = lds_wave + (uint32_t)slot * Cfg::kSlotBytes;
#pragma unroll
    for (int n = 0; n < Cfg::kFull; ++n) chain_regs_dma16(at + n * T * 16, voff, base + n * T * 16);
    if constexpr (Cfg::kRem > 0) chain_regs_dma16(at + Cfg::kFull * T * 16, voff_last, base + Cfg::kFull * T * 16);
  };
  // Per-thread LDS byte addresses, one per W slot and per ring slot, opaque to the optimiser: every read of a phase is then
  // this register plus an immediate that fits the two-address forms (ds_read2_b32, ds_read2_b64); folded into one base, hipcc
  // rebuilds eight to ten of them per phase, which the residual instance has no registers for.
  uint32_t wat[S], xat[4];
#pragma unroll
  for (int s = 0; s < S; ++s) wat[s] = lane_off((uint32_t)(s * Cfg::kSlotBytes + tid * (L * 4)));
#pragma unroll
  for (int s = 0; s < 4; ++s) xat[s] = lane_off((uint32_t)(S * Cfg::kSlotBytes + (s * T + tid) * 8));
  auto ring = [&](int s, int entry) -> F2& { return *reinterpret_cast<F2*>(lds + xat[s] + entry * 8); };

  const int M = a.M;
  const unsigned char* wcur = reinterpret_cast<const unsigned char*>(a.W[0]) + seq_bytes;
#pragma unroll
  for (int g = 0; g < S - 1; ++g) fill(wcur, g, g);

  for (int m = 0; m < M; ++m) {
    // the blocks requested during this step's last S - 1 phases belong to the next step; behind the last step they re-read
    // blocks of W_{M-1} into slots nobody reads again, so that every phase of the chain counts the same DMAs
    const unsigned char* wnext = reinterpret_cast<const unsigned char*>(a.W[m + 1 < M ? m + 1 : m]) + seq_bytes;
    // blocks 0 and 1 of X_m -> ring slots 0 and 1 (nobody reads those any more: below); phase 0's barrier publishes them
    ring(0, 0) = F2{xa[0].e[0], xa[0].e[1]};
    ring(1, 0) = F2{xa[1].e[0], xa[1].e[1]};

    chain_regs_each(std::make_integer_sequence<int, J>{}, [&](auto jc) {
      constexpr int j = decltype(jc)::value;
      // this wave's DMAs of block j have landed (the S - 2 blocks requested after it may stay in flight), its LDS writes and
      // reads are complete; behind the barrier that holds for every wave
      dma_wait_all_but<(S - 2) * P>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      fill(j + S - 1 < J ? wcur : wnext, (j + S - 1) % J, (j + S - 1) % S);
      if constexpr (j + 2 <= J) {  // block j + 2 of X_m (block J is block 0 again); a block of slot 0 goes to the mirror too
        const F2 own{xa[(j + 2) % J].e[0], xa[(j + 2) % J].e[1]};
        ring((j + 2) & 3, 0) = own;
        if constexpr (((j + 2) & 3) == 0) ring(3, T) = own;
      }

      const float* __restrict__ wrow = reinterpret_cast<const float*>(lds + wat[j % S]);
      V2 acc;
      acc.e[0] = acc.e[1] = 0.f;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        const int off = chord_off(k);
        V2 x;
        if (off % T == 0) {
          x = xa[(j + off / T) % J];
        } else {  // (slot 3's next block is the mirror of slot 0 behind it: no wrap)
          const F2 r = ring(j & 3, off);
          x.e[0] = r.x, x.e[1] = r.y;
        }
        axpy_rn<float, 2>(acc, wrow[k], x);
      }
      if constexpr (RES) {
        acc.e[0] = add_rn(acc.e[0], v0[j].e[0]);
        acc.e[1] = add_rn(acc.e[1], v0[j].e[1]);
      }
      xb[j] = acc;
    });

    // No barrier between steps. Phase J - 1 reads ring slot 3 and the mirror only; the next step's first writes go to slots 0
    // and 1 (last read in phases J - 4 and J - 3, two barriers back), then behind phase 0's barrier to slot 2 (phase J - 2)
    // and behind phase 1's to slot 3, and phase 0's DMA refills the W slot of phase J - 1 behind phase 0's barrier as well.
    chain_regs_each(std::make_integer_sequence<int, J>{}, [&](auto jc) { xa[decltype(jc)::value] = xb[decltype(jc)::value]; });
    wcur = wnext;
  }

  dma_wait_all();  // (the surplus blocks behind the last step)
  // (the row offsets are those of the V0 loads: recomputed from a laundered copy of the thread index, or hipcc keeps the J
  // 64-bit offsets of the prologue alive across the whole chain, in scratch memory)
  const int tid_out = (int)lane_off((uint32_t)tid);
  float* __restrict__ ob = a.out + (int64_t)b * N * C + (int64_t)q * 2;
  chain_regs_each(std::make_integer_sequence<int, J>{}, [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    st<float, 2>(ob + (int64_t)(tid_out + T * j) * C, xa[j]);
  });
}

}  // namespace psf
