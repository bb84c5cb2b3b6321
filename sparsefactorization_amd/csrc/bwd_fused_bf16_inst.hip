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
  const int lds = lds_for_wg_limit(Cfg::lds_bytes, a.wg_per_cu);
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), lds, a.stream, a.dZ, a.WV, a.V2, a.out2, a.out, a.gm, a.offs, a.w_total);
  return hipGetLastError();
}

template <int TGS>
hipError_t launch_L(int L, const BwdWinArgsT<__bf16>& a) {
  return with_int<kFusedLmin, kFusedLmax>(L, [&](auto l) { return launch_fused_bf16<l(), TGS, kFusedBf16Threads>(a); });
}

}  // namespace

static_assert(PSF_TGS >= 0 && PSF_TGS <= kFusedBf16TgsMax, "bf16 fused backward step: TGS 0..kFusedBf16TgsMax");
template <int TGS>
hipError_t launch_bwd_fused_bf16(int L, const BwdWinArgsT<__bf16>& a) {
  return launch_L<TGS>(L, a);  // (a lambda in a function with external linkage would export its instances)
}
template hipError_t launch_bwd_fused_bf16<PSF_TGS>(int L, const BwdWinArgsT<__bf16>& a);

}  // namespace psf
