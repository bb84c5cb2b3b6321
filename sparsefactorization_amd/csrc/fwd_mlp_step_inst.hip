// fwd_mlp_step_inst.hip — instantiates the forward step that computes its own W tile (fwd_mlp_step.h) for ONE
// channel-group shift. Built once per -DPSF_TGS=0..3 so the instances compile in parallel; see build.py.
#ifndef PSF_TGS
#error "compile with -DPSF_TGS=<0..3>"
#endif

#include <atomic>

#include "fwd_mlp_step.h"

namespace psf {
namespace {

constexpr int kLdsPerCuBytes = 160 * 1024;

template <int L, int TGS, bool RES, bool EDGE>
hipError_t launch_one(const FwdMlpArgs& a) {
  if (a.in.kind != 0) return hipErrorInvalidValue;  // rows of `data` only (recipes: mixer_lds.h)
  using Cfg = MlpStepCfg<L, TGS>;
  auto kern = chord_fwd_mlp_k<L, TGS, RES, EDGE>;
  int lds = Cfg::img_off + a.nu * kImgBytes;
  if (a.wg_per_cu > 0) {  // occupancy limiter: asking for just over 160 KB / (n + 1) caps a CU at n workgroups
    const int floor_bytes = kLdsPerCuBytes / (a.wg_per_cu + 1) + 256;
    if (floor_bytes > lds) lds = floor_bytes;
  }
  if (lds > kLdsPerCuBytes) return hipErrorInvalidValue;
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(256), lds, a.stream, a.in, a.V, a.res, a.out, a.images, a.nu, a.E, a.gm,
                     a.offs);
  return hipGetLastError();
}

template <int L, int TGS>
hipError_t launch_flags(const FwdMlpArgs& a) {
  if (a.res != nullptr) return a.edge ? launch_one<L, TGS, true, true>(a) : launch_one<L, TGS, true, false>(a);
  return a.edge ? launch_one<L, TGS, false, true>(a) : launch_one<L, TGS, false, false>(a);
}

template <int TGS>
hipError_t launch_L(int L, const FwdMlpArgs& a) {
  return with_int<kMlpStepLmin, kMlpStepLmax>(L, [&](auto l) { return launch_flags<l(), TGS>(a); });
}

}  // namespace

template <int TGS>
hipError_t launch_fwd_mlp(int L, const FwdMlpArgs& a) {
  return launch_L<TGS>(L, a);  // (a lambda in a function with external linkage would export its instances)
}

template hipError_t launch_fwd_mlp<PSF_TGS>(int L, const FwdMlpArgs& a);

template <int TGS>
hipError_t launch_mixer_g(const FwdMlpArgs& a) {
  if (a.in.kind != 0) return hipErrorInvalidValue;
  const int lds = a.nu * kImgBytes;
  auto launch = [&](auto kern) {
    if (lds > 48 * 1024) {  // (every call, not once per kernel: kept as it is, allow_dynamic_lds would skip the repeats)
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(256), lds, a.stream, a.in, a.out, a.images, a.nu, a.E, a.gm);
    return hipGetLastError();
  };
  return a.edge ? launch(chord_mixer_g_k<TGS, true>) : launch(chord_mixer_g_k<TGS, false>);
}

template hipError_t launch_mixer_g<PSF_TGS>(const FwdMlpArgs& a);

}  // namespace psf
