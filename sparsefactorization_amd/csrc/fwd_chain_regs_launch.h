// fwd_chain_regs_launch.h — host-side interface of the register-resident one-launch chain (fwd_chain_regs.h).
#pragma once

#include "fwd_chain_regs.h"

namespace psf {

// the compiled instance: T threads x J row blocks (N = T * J exactly), L links, f32, default chord offsets
constexpr int kChainRegsThreads = 512, kChainRegsBlocks = 32, kChainRegsLinks = 15;
constexpr int kChainRegsN = kChainRegsThreads * kChainRegsBlocks;  // 16384

// The automatic rule (psf_chord_chain_last_supported), for chains of which only the last result is kept. A workgroup
// occupies a whole CU (512 threads x 241 registers, 148 KB of LDS) and takes the same time whatever runs beside it (its own
// phases bound it, not the memory system), so a grid of `wgs` = B * C / 2 workgroups runs in rounds = ceil(wgs / CUs) rounds
// of one workgroup's time, while the per-step route's time grows with wgs. The one launch therefore wins only where its
// rounds are nearly full, and loses just above every multiple of the CU count. Rule: automatic where
//     wgs * 100 >= kChainRegsFillPct * rounds * CUs   and   rounds <= kChainRegsMaxRounds,
// CUs read from the device. Measured at M = 14, residual on (profiles/chain_regs_ab.md: per-step route against one launch on
// grids of 32 to 1024 workgroups at C = 8, and at C = 4 and 12 around one round): the one launch wins from about 0.8 of a
// round's CUs on; 95 % keeps a margin for the channel counts and chain lengths that were not swept, four rounds is the
// largest grid measured. kChainRegsFillPct = 0 would mean never automatic (chain_fused = 2 takes it wherever it fits).
constexpr int kChainRegsFillPct = 95, kChainRegsMaxRounds = 4;
constexpr int kChainRegsDefaultCus = 256;  // MI355X; used where no device can be asked (a host without a GPU)

inline bool chain_regs_automatic(int64_t wgs, int cus) {
  if (kChainRegsFillPct <= 0 || cus < 1 || wgs < 1) return false;
  const int64_t rounds = (wgs + cus - 1) / cus;
  return rounds <= kChainRegsMaxRounds && wgs * 100 >= (int64_t)kChainRegsFillPct * rounds * cus;
}

// what the kernel covers, the operands' alignment apart: the compiled N and L, C a multiple of 4, 1 <= M <= kChainMaxSteps,
// B * C / 2 workgroups within a grid
bool chain_regs_fits(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M);

hipError_t launch_chain_regs(bool res, const ChainRegsArgs& args, int B, hipStream_t stream);

}  // namespace psf
