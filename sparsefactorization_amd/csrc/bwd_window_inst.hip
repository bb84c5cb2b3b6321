// bwd_window_inst.hip — instantiates the LDS-window backward kernels for ONE (channel-group shift, workgroup
// size) pair. Built once per compiled pair (-DPSF_TGS=0..6 [-DPSF_NT=1024]); see build.py. With -DPSF_BF16 the unit holds
// the bf16 dV / dW instances of that TGS instead (NT 256: dW R 1, dV R 2).
#ifndef PSF_TGS
#error "compile with -DPSF_TGS=<0..6>"
#endif
#ifndef PSF_NT
#define PSF_NT 256
#endif

#include <atomic>

#include "bwd_dw_chunk.h"
#include "bwd_fused.h"
#include "bwd_window.h"
#include "bwd_window_launch.h"

namespace psf {
namespace {

// dV, dW and chunk dW take the same arguments; `seen` is the calling instance's own (allow_dynamic_lds, psf_common.h)
template <int NT, typename K, typename T>
hipError_t launch_win(K kern, int lds, std::atomic<int>& seen, const BwdWinArgsT<T>& a) {
  if (hipError_t e = allow_dynamic_lds(kern, lds, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), lds, a.stream, a.dZ, a.WV, a.out, a.gm, a.offs, a.w_total);
  return hipGetLastError();
}

template <typename T, int L, int TGS, int R, int NT, bool EDGE>
hipError_t launch_dw(const BwdWinArgsT<T>& a) {
  static std::atomic<int> seen{0};
  return launch_win<NT>(chord_dw_win_k<T, L, TGS, R, NT, EDGE>, BwdWinCfg<T, L, TGS, R, NT>::lds_dw, seen, a);
}

template <typename T, int L, int TGS, int R, int NT, bool EDGE>
hipError_t launch_dv(const BwdWinArgsT<T>& a) {
  static std::atomic<int> seen{0};
  return launch_win<NT>(chord_dv_win_k<T, L, TGS, R, NT, EDGE>, BwdWinCfg<T, L, TGS, R, NT>::lds_dv, seen, a);
}

template <int L, int TGS, int R, int NT, bool EDGE>
hipError_t launch_dwc(const BwdWinArgs& a) {
  static std::atomic<int> seen{0};
  return launch_win<NT>(chord_dw_chunk_k<L, TGS, R, NT, EDGE>, DwChunkCfg<L, TGS, R, NT>::lds_bytes, seen, a);
}

template <int TGS, int R, int NT>
hipError_t launch_dwc_L(int L, const BwdWinArgs& a) {
  return with_int<kDwChunkLmin, kDwChunkLmax>(L, [&](auto l) {
    return a.edge ? launch_dwc<l(), TGS, R, NT, true>(a) : launch_dwc<l(), TGS, R, NT, false>(a);
  });
}

template <int TGS, int R, int NT, bool DW, typename T = float>
hipError_t launch_L(int L, const BwdWinArgsT<T>& a) {
  return with_int<kWinLmin, kWinLmax>(L, [&](auto l) {
    if constexpr (DW) return a.edge ? launch_dw<T, l(), TGS, R, NT, true>(a) : launch_dw<T, l(), TGS, R, NT, false>(a);
    else return a.edge ? launch_dv<T, l(), TGS, R, NT, true>(a) : launch_dv<T, l(), TGS, R, NT, false>(a);
  });
}

}  // namespace

#ifdef PSF_BF16
static_assert(PSF_NT == 256 && PSF_TGS <= kWinTgsMaxBf16, "bf16 backward instances: NT 256, TGS 0..kWinTgsMaxBf16");
template <int TGS>
hipError_t launch_dw_win_bf16(int L, const BwdWinArgsT<__bf16>& a) {
  return launch_L<TGS, 1, 256, true, __bf16>(L, a);
}
template <int TGS>
hipError_t launch_dv_win_bf16(int L, const BwdWinArgsT<__bf16>& a) {
  return launch_L<TGS, 2, 256, false, __bf16>(L, a);
}
template hipError_t launch_dw_win_bf16<PSF_TGS>(int L, const BwdWinArgsT<__bf16>& a);
template hipError_t launch_dv_win_bf16<PSF_TGS>(int L, const BwdWinArgsT<__bf16>& a);
#else
#if PSF_NT == 256
template <int TGS>
hipError_t launch_dw_win(int rows, int L, const BwdWinArgs& a) {
  if (rows == 1) return launch_L<TGS, 1, 256, true>(L, a);  // (dW: one row per thread only)
  return hipErrorInvalidValue;
}
template hipError_t launch_dw_win<PSF_TGS>(int rows, int L, const BwdWinArgs& a);

#if PSF_TGS >= 3 && PSF_TGS <= 4
template <int TGS>
hipError_t launch_dw_chunk(int L, const BwdWinArgs& a) {
  static_assert(TGS >= kDwChunkTgsMin && TGS <= kDwChunkTgsMax, "chunk lanes per row");
  return launch_dwc_L<TGS, 1, 256>(L, a);
}
template hipError_t launch_dw_chunk<PSF_TGS>(int L, const BwdWinArgs& a);
#endif
#endif

#if PSF_NT != 512 || PSF_TGS <= 1  // (dV on 512 threads x 1 row is compiled for rows of <= 8 channels: bwd_window_launch.h)
template <int TGS, int NT>
hipError_t launch_dv_win(int rows, int L, const BwdWinArgs& a) {
  static_assert(dv_pair_compiled(TGS, NT), "not a compiled (TGS, NT) pair");
  if constexpr (NT == kDvMidThreads) {  // 512 threads x 1 row, or two rows per thread
    if (rows == 1) return launch_L<TGS, 1, NT, false>(L, a);
  } else {
    if (rows == 2) return launch_L<TGS, 2, NT, false>(L, a);
  }
  return hipErrorInvalidValue;
}
template hipError_t launch_dv_win<PSF_TGS, PSF_NT>(int rows, int L, const BwdWinArgs& a);
#endif

#if PSF_NT == 512
namespace {
template <int L, int TGS, int NT>
hipError_t launch_fused(const BwdWinArgs& a) {
  using Cfg = BwdFusedCfg<L, TGS, NT>;
  auto kern = chord_bwd_fused_k<L, TGS, NT>;
  const int own = Cfg::lds_bytes;
  const int lds = lds_for_wg_limit(own, a.wg_per_cu);
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, lds, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), lds, a.stream, a.dZ, a.WV, a.V2, a.out2, a.out,
                     a.gm, a.offs, a.w_total);
  return hipGetLastError();
}
template <int TGS>
hipError_t launch_fused_L(int L, const BwdWinArgs& a) {
  return with_int<kFusedLmin, kFusedLmax>(L, [&](auto l) { return launch_fused<l(), TGS, 256>(a); });
}
}  // namespace
template <int TGS>
hipError_t launch_bwd_fused(int L, const BwdWinArgs& a) {
  return launch_fused_L<TGS>(L, a);  // (a lambda in a function with external linkage would export its instances)
}
template hipError_t launch_bwd_fused<PSF_TGS>(int L, const BwdWinArgs& a);

namespace {
template <int L, int TGS, int NT>
hipError_t launch_fused_edge(const BwdWinArgs& a) {
  using Cfg = BwdFusedEdgeCfg<L, TGS, NT>;
  auto kern = chord_bwd_fused_edge_k<L, TGS, NT>;
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, Cfg::lds_bytes, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(a.gm.nblocks), dim3(NT), Cfg::lds_bytes, a.stream, a.dZ, a.WV, a.V2, a.out2, a.out, a.gm, a.offs,
                     a.w_total);
  return hipGetLastError();
}
template <int TGS>
hipError_t launch_fused_edge_L(int L, const BwdWinArgs& a) {
  return with_int<kFusedLmin, kFusedLmax>(L, [&](auto l) { return launch_fused_edge<l(), TGS, 256>(a); });
}
}  // namespace
template <int TGS>
hipError_t launch_bwd_fused_edge(int L, const BwdWinArgs& a) {
  return launch_fused_edge_L<TGS>(L, a);
}
template hipError_t launch_bwd_fused_edge<PSF_TGS>(int L, const BwdWinArgs& a);
#endif
#endif  // PSF_BF16

}  // namespace psf
