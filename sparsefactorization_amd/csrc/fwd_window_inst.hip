// fwd_window_inst.hip — instantiates the LDS-window forward kernels for ONE (channel-group shift, workgroup
// size) pair. Built once per compiled pair (-DPSF_TGS=0..6 [-DPSF_NT=1024]) so the instances compile in
// parallel; see build.py. With -DPSF_BF16 the unit holds the bf16 instances of that TGS instead (NT 256, R 2 only).
#ifndef PSF_TGS
#error "compile with -DPSF_TGS=<0..6>"
#endif
#ifndef PSF_NT
#define PSF_NT 256
#endif

#include <atomic>

#include "fwd_window.h"
#include "fwd_window_launch.h"

namespace psf {
namespace {

template <typename T, int L, int TGS, int R, int NT, bool RES, int MODE>
hipError_t launch_one(const FwdWinArgsT<T>& a) {
  using Cfg = FwdWinCfg<T, L, TGS, R, NT>;
  auto kern = chord_fwd_win_k<T, L, TGS, R, NT, /*DMA=*/true, RES, MODE>;
  const int lds = lds_for_wg_limit(Cfg::lds_bytes, a.wg_per_cu);
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), lds, a.stream, a.W, a.V, a.res, a.out, a.gm,
                     a.offs, a.w_total);
  return hipGetLastError();
}

template <typename T, int L, int TGS, int R, int NT>
hipError_t launch_flags(const FwdWinArgsT<T>& a) {
  if (a.res != nullptr)
    return a.edge ? launch_one<T, L, TGS, R, NT, true, 1>(a)
                  : (a.gm.aligned ? launch_one<T, L, TGS, R, NT, true, 2>(a) : launch_one<T, L, TGS, R, NT, true, 0>(a));
  return a.edge ? launch_one<T, L, TGS, R, NT, false, 1>(a)
                : (a.gm.aligned ? launch_one<T, L, TGS, R, NT, false, 2>(a) : launch_one<T, L, TGS, R, NT, false, 0>(a));
}

template <typename T, int TGS, int R, int NT>
hipError_t launch_L(int L, const FwdWinArgsT<T>& a) {
  return with_int<kWinLmin, kWinLmax>(L, [&](auto l) { return launch_flags<T, l(), TGS, R, NT>(a); });
}

}  // namespace

#ifdef PSF_BF16
template <int TGS>
hipError_t launch_fwd_win_bf16(int rows, int L, const FwdWinArgsT<__bf16>& a) {
  static_assert(TGS >= 0 && TGS <= kWinTgsMaxBf16 && PSF_NT == 256, "not a compiled bf16 configuration");
  if (rows == 2) return launch_L<__bf16, TGS, 2, 256>(L, a);
  return hipErrorInvalidValue;
}

template hipError_t launch_fwd_win_bf16<PSF_TGS>(int rows, int L, const FwdWinArgsT<__bf16>& a);
#else
template <int TGS, int NT>
hipError_t launch_fwd_win(int rows, int L, const FwdWinArgs& a) {
  static_assert(win_pair_compiled(TGS, NT), "not a compiled (TGS, NT) pair");
  if (rows == 2) return launch_L<float, TGS, 2, NT>(L, a);  // (the only compiled rows per thread: fwd_window_launch.h)
  if constexpr (win_rows4_compiled(TGS, NT)) {
    if (rows == 4) return launch_L<float, TGS, 4, NT>(L, a);
  }
  return hipErrorInvalidValue;
}

template hipError_t launch_fwd_win<PSF_TGS, PSF_NT>(int rows, int L, const FwdWinArgs& a);
#endif

}  // namespace psf
