// mixer_lds_bf16_inst.hip — plan, instances and launcher of the single-launch bf16 mixer for short sequences (mixer_lds_bf16.h).
#include <atomic>

#include "mixer_lds_bf16.h"

namespace psf {

// N <= 512: with two token tiles per wave that is eight waves, the workgroup size every instance is compiled for
// (__launch_bounds__(512): 103-135 VGPRs by k-step count, no scratch). N = 1024 would fit the LDS (64 KB of X at C = 16, 40 KB of W, 27 KB of
// images) but needs sixteen waves or four tiles of data rows per wave, i.e. another set of instances; not built.
bool plan_mixer_lds_bf16(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L, MixerLdsBf16Plan* p) {
  namespace mb = psf_mlp_bf16;
  if (!h || N < 32 || N > kMixerLdsBf16MaxN || N % 32 != 0 || (C != 8 && C != 16) || E < 8 || E > mb::kMaxE || (E & 7) || L < 4 ||
      L > 20 || M < 1 || M > kMixerLdsBf16MaxSteps)
    return false;
  int units = 0, nu_max = 0;
  for (int k = 0; k <= M; ++k) {
    if (h[k] < 1 || h[k] > mb::kMaxH) return false;
    const int nu = (h[k] + 31) / 32;
    units += nu;
    nu_max = nu > nu_max ? nu : nu_max;
  }
  const int TT = (int)(N / 32), nwaves = TT < 8 ? TT : 8;  // at most two token tiles per wave
  const int64_t slots = N * (C / 8);                        // at most two slots per thread: slots <= 2 N = 64 TT
  p->threads = 64 * nwaves;
  p->WS = L <= 12 ? 12 : 20;
  p->nu_max = nu_max;
  p->units = units;
  p->lds_bytes = (int)(2 * slots * 16 + N * p->WS * 2 + (int64_t)nu_max * mb::kImgBytes);
  return slots <= 2 * (int64_t)p->threads && p->lds_bytes <= kLdsPerCu;
}

namespace {

template <int KS, bool RES>
hipError_t launch_one(const MixerLdsBf16Plan& p, const MixerLdsBf16Args& a, const Offsets& offs, int B, hipStream_t s) {
  auto kern = chord_mixer_lds_k<__bf16, KS, RES>;
  static std::atomic<int> seen{0};
  if (hipError_t e = allow_dynamic_lds(kern, p.lds_bytes, seen); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(p.threads), p.lds_bytes, s, a, offs);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_mixer_lds_bf16(const MixerLdsBf16Plan& p, bool res, const psf_mlp_bf16::Args& pack, const MixerLdsBf16Args& a,
                                 const Offsets& offs, int B, hipStream_t s) {
  if (hipError_t e = psf_mlp_bf16::pack_launch(pack, s); e != hipSuccess) return e;
  return with_int<1, 4>((a.E + 15) / 16, [&](auto ks) {
    return res ? launch_one<ks(), true>(p, a, offs, B, s) : launch_one<ks(), false>(p, a, offs, B, s);
  });
}

}  // namespace psf
