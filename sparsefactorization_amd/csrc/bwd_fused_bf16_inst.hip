// bwd_fused_bf16_inst.hip — instantiates the bf16 fused backward step (bwd_fused_bf16.h) for ONE channel-group shift.
// Built once per shift (-DPSF_TGS=0..4: rows of 8 << TGS channels); see build.py. Units of their own, so the f32 backward
// units' device code is what it was.
#ifndef PSF_TGS
#error "compile with -DPSF_TGS=<0..4>"
#endif

#include <atomic>

#include "bwd_fused_bf16.h"
#include "bwd_window_launch.h"

namespace psf {
namespace {

template <int L, int TGS, int NT>
hipError_t launch_fused_bf16(const BwdWinArgsT<__bf16>& a) {
  using Cfg = BwdFusedBf16Cfg<L, TGS, NT>;
  auto kern = chord_bwd_fused_bf16_k<L, TGS, NT>;
  int lds = Cfg::lds_bytes;
  if (a.wg_per_cu > 0) {  // occupancy limiter as in the f32 launcher (bwd_window_inst.hip)
    const int floor_bytes = kLdsPerCu / (a.wg_per_cu + 1) + 256;
    if (floor_bytes > lds && floor_bytes <= 64 * 1024) lds = floor_bytes;
  }
  static std::atomic<int> done{0};
  if (lds > 48 * 1024 && done.load() < lds) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    done.store(lds);
  }
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), lds, a.stream, a.dZ, a.WV, a.V2, a.out2, a.out, a.gm, a.offs, a.w_total);
  return hipGetLastError();
}

}  // namespace

static_assert(PSF_TGS >= 0 && PSF_TGS <= kFusedBf16TgsMax, "bf16 fused backward step: TGS 0..kFusedBf16TgsMax");
template <int TGS>
hipError_t launch_bwd_fused_bf16(int L, const BwdWinArgsT<__bf16>& a) {
  switch (L) {
#define PSF_CASE(LL) \
  case LL:           \
    return launch_fused_bf16<LL, TGS, kFusedBf16Threads>(a);
    PSF_CASE(4) PSF_CASE(5) PSF_CASE(6) PSF_CASE(7) PSF_CASE(8) PSF_CASE(9) PSF_CASE(10) PSF_CASE(11)
    PSF_CASE(12) PSF_CASE(13) PSF_CASE(14) PSF_CASE(15) PSF_CASE(16) PSF_CASE(17) PSF_CASE(18)
    PSF_CASE(19) PSF_CASE(20)
#undef PSF_CASE
    default:
      return hipErrorInvalidValue;
  }
}
template hipError_t launch_bwd_fused_bf16<PSF_TGS>(int L, const BwdWinArgsT<__bf16>& a);

}  // namespace psf
