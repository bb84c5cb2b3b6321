// fwd_chain_lds_bf16_inst.hip — instances and launcher of the bf16 LDS-resident fused chain kernels (fwd_chain_lds_bf16.h).
// A unit of its own: the f32 unit (fwd_chain_lds_inst.hip) compiles exactly what it compiled before. The instance set is
// the f32 one (L = 2..20; plan_chain_lds selects among them with elem_bytes = 2).
#include <atomic>

#include "fwd_chain_lds_bf16.h"
#include "fwd_chain_lds_launch.h"

namespace psf {
namespace {

template <int L, int CC, int R, bool RES, int NTMAX>
hipError_t launch_one(const ChainArgsBf16& a, const Offsets& offs, int B, int threads, int lds_bytes, hipStream_t s) {
  auto kern = chord_chain_lds_k<__bf16, L, CC, R, RES, NTMAX>;
  // the first launch beyond 48 KB allows the family's maximum, so no later one has to raise again
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds_bytes > 48 * 1024 ? kChainLdsMaxBytes : 0, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * a.chunks)), dim3(threads), lds_bytes, s, a, offs);
  return hipGetLastError();
}

template <int L, int G, int R, int CAP, bool RES>
hipError_t launch_rows(const ChainArgsBf16& a, const Offsets& offs, int B, int threads, int lds_bytes, hipStream_t s) {
  auto kern = chord_chain_rows_k<__bf16, L, G, R, CAP, RES>;
  static_assert(2 * G * CAP * 16 > 48 * 1024, "both instances hold more than the default limit: the first launch raises it");
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, 2 * G * CAP * 16, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(B * a.chunks)), dim3(threads), lds_bytes, s, a, offs);
  return hipGetLastError();
}

template <int L, int CC, bool RES>
hipError_t launch_R(const ChainLdsPlan& p, const ChainArgsBf16& a, const Offsets& offs, int B, hipStream_t s) {
  if constexpr (CC == 2) {
    if (p.big == 1) return launch_rows<L, 2, 2, kChainBigRows, RES>(a, offs, B, p.threads, p.lds_bytes, s);
  } else {
    if (p.big == 2) return launch_rows<L, 1, kChainLongRowsPerThread, kChainLongRows, RES>(a, offs, B, p.threads, p.lds_bytes, s);
  }
  if (p.big) return hipErrorInvalidValue;
  if (p.rows == 1) return launch_one<L, CC, 1, RES, 512>(a, offs, B, p.threads, p.lds_bytes, s);
  if (p.rows == 2 && p.threads <= 512) return launch_one<L, CC, 2, RES, 512>(a, offs, B, p.threads, p.lds_bytes, s);
  if (p.rows == 2) return launch_one<L, CC, 2, RES, 1024>(a, offs, B, p.threads, p.lds_bytes, s);
  if constexpr (L <= kChainLdsRows3LmaxBf16) {  // (beyond: the instance would spill; not compiled, and the planner declines)
    if (p.rows == 3 && p.threads <= 768) return launch_one<L, CC, 3, RES, 768>(a, offs, B, p.threads, p.lds_bytes, s);
  }
  return hipErrorInvalidValue;
}

template <int CC>
hipError_t launch_L(int L, bool res, const ChainLdsPlan& p, const ChainArgsBf16& a, const Offsets& offs, int B, hipStream_t s) {
  return with_int<kChainLdsLmin, kChainLdsLmax>(L, [&](auto l) {
    return res ? launch_R<l(), CC, true>(p, a, offs, B, s) : launch_R<l(), CC, false>(p, a, offs, B, s);
  });
}

}  // namespace

hipError_t launch_chain_lds_bf16(const ChainLdsPlan& p, int L, bool res, const ChainArgsBf16& a, const Offsets& offs, int B,
                                 hipStream_t s) {
  if (p.cc == 2) return launch_L<2>(L, res, p, a, offs, B, s);
  return launch_L<1>(L, res, p, a, offs, B, s);
}

}  // namespace psf
