// chain_tr_lds_inst.hip — instances and launcher of the one-launch transposed chain (chain_tr_lds.h). Compiled once per
// element type (-DPSF_BF16: the bf16 instances), so neither build waits for the other's 76 kernels.
#include <atomic>

#include "chain_tr_lds.h"

namespace psf {
namespace {

#ifdef PSF_BF16
using Elem = __bf16;
#else
using Elem = float;
#endif

template <int L, int G>
hipError_t launch_one(const ChainTrArgs<Elem>& a, const Offsets& offs, int64_t B, hipStream_t s) {
  auto kern = chord_chain_tr_lds_k<Elem, L, G>;
  const int lds_bytes = G * kChainBwdRows * 16 + a.N * chain_bwd_wstride<L>() * 4;
  // the first launch beyond 48 KB allows the instance's maximum (N = kChainBwdRows), so no later one has to raise again
  const int cap = G * kChainBwdRows * 16 + kChainBwdRows * chain_bwd_wstride<L>() * 4;
  static_assert(kChainTrGroups * kChainBwdRows * 16 + kChainBwdRows * chain_bwd_wstride<kChainLdsLmax>() * 4 <= kLdsPerCu,
                "kChainTrGroups groups beside W_m at the largest covered shape must fit a CU's LDS");
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds_bytes > 48 * 1024 ? cap : 0, seen); e != hipSuccess) return e;
  const int threads = (a.N + 63) / 64 * 64;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * a.chunks)), dim3(threads), lds_bytes, s, a, offs);
  return hipGetLastError();
}

template <int L>
hipError_t launch_G(int G, const ChainTrArgs<Elem>& a, const Offsets& offs, int64_t B, hipStream_t s) {
  return with_int<1, kChainTrGroups>(G, [&](auto g) { return launch_one<L, g()>(a, offs, B, s); });
}

}  // namespace

hipError_t launch_chain_tr_lds(int L, const ChainTrArgs<Elem>& a, const Offsets& offs, int64_t B, hipStream_t s) {
  if (a.N < 1 || a.N > kChainBwdRows || a.chunks < 1 || B * a.chunks > (int64_t)0x7fffffff) return hipErrorInvalidValue;
  const int G = (a.CG + a.chunks - 1) / a.chunks;  // groups per workgroup; the last workgroup may hold fewer
  if ((int64_t)G * a.chunks - a.CG >= G) return hipErrorInvalidValue;  // (every workgroup owns at least one group)
  return with_int<kChainLdsLmin, kChainLdsLmax>(L, [&](auto l) { return launch_G<l()>(G, a, offs, B, s); });
}

}  // namespace psf
