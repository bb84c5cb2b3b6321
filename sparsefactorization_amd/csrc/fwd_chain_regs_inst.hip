// fwd_chain_regs_inst.hip — instances and launcher of the register-resident one-launch chain (fwd_chain_regs.h).
#include "fwd_chain_regs.h"
#include "fwd_chain_regs_launch.h"

namespace psf {
namespace {

template <bool RES>
hipError_t launch_one(const ChainRegsArgs& a, int B, hipStream_t s) {
  // (the LDS is static: nothing to allow before the launch)
  auto kern = chord_chain_regs_k<kChainRegsLinks, kChainRegsThreads, kChainRegsBlocks, RES>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * a.pairs)), dim3(kChainRegsThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace

bool chain_regs_fits(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M) {
  return N == kChainRegsN && L == kChainRegsLinks && C >= 4 && C % 4 == 0 && M >= 1 && M <= kChainMaxSteps && B >= 1 &&
         C <= ((int64_t)1 << 30) && B * (C / 2) <= 0x7fffffff;
}

hipError_t launch_chain_regs(bool res, const ChainRegsArgs& a, int B, hipStream_t s) {
  return res ? launch_one<true>(a, B, s) : launch_one<false>(a, B, s);
}

}  // namespace psf
