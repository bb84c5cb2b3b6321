// bwd_chain_lds_bf16_inst.hip — instances and launcher of the bf16 LDS-resident backward chain (bwd_chain_lds_bf16.h).
// A unit of its own: the f32 unit's device code (bwd_chain_lds_inst.hip) is what it was.
#include <atomic>

#include "bwd_chain_lds_bf16.h"
#include "fwd_chain_lds_launch.h"  // kChainLdsLmin, kChainLdsLmax: compiled for the forward chain's link counts

namespace psf {
namespace {

template <int L, int G, bool RES>
hipError_t launch_one(const ChainBwdArgsBf16& a, const Offsets& offs, int B, hipStream_t s) {
  auto kern = chord_chain_bwd_lds_k<__bf16, L, G, RES>;
  const int lds_bytes = 2 * G * kChainBwdRows * 16 + a.N * chain_bwd_wstride<L>() * 4;
  // the first launch beyond 48 KB allows the instance's maximum (N = kChainBwdRows), so no later one has to raise again
  const int cap = 2 * G * kChainBwdRows * 16 + kChainBwdRows * chain_bwd_wstride<L>() * 4;
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds_bytes > 48 * 1024 ? cap : 0, seen); e != hipSuccess) return e;
  const int threads = (a.N + 63) / 64 * 64;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(threads), lds_bytes, s, a, offs);
  return hipGetLastError();
}

template <int L>
hipError_t launch_G(int G, bool res, const ChainBwdArgsBf16& a, const Offsets& offs, int B, hipStream_t s) {
  if (G == 1) return res ? launch_one<L, 1, true>(a, offs, B, s) : launch_one<L, 1, false>(a, offs, B, s);
  if (G == 2) return res ? launch_one<L, 2, true>(a, offs, B, s) : launch_one<L, 2, false>(a, offs, B, s);
  return hipErrorInvalidValue;
}

}  // namespace

bool chain_bwd_lds_bf16_fits(int64_t N, int64_t C, int32_t L, int32_t M) {
  return N >= 1 && N <= kChainBwdRows && (C == 8 || C == 16) && L >= kChainLdsLmin && L <= kChainLdsLmax && M >= 1 && M <= kChainMaxSteps;
}

hipError_t launch_chain_bwd_lds_bf16(int L, int G, bool res, const ChainBwdArgsBf16& a, const Offsets& offs, int B, hipStream_t s) {
  return with_int<kChainLdsLmin, kChainLdsLmax>(L, [&](auto l) { return launch_G<l()>(G, res, a, offs, B, s); });
}

}  // namespace psf
