// mixer_lds_bf16_launch.h — host-side interface of the single-launch bf16 mixer for short sequences (mixer_lds_bf16.h), for
// psf_chord.hip.
#pragma once

#include "mlp_bf16_image.h"
#include "psf_common.h"

namespace psf {

constexpr int kMixerLdsBf16MaxSteps = 31;
constexpr int kMixerLdsBf16MaxN = 512;  // (plan_mixer_lds_bf16 says why not 1024)

struct MixerLdsBf16Args {
  const uint16_t* X;                              // data rows [B,N,E]
  const unsigned char* images;                    // unit images of all M + 1 MLPs (g first), mlp_bf16_image.h
  int32_t first_unit[kMixerLdsBf16MaxSteps + 2];  // first unit of MLP k; [M + 1] = total
  uint16_t* V0;                                   // [B,N,C] receives g(data), or nullptr
  uint16_t* out[kMixerLdsBf16MaxSteps];           // step results; written where bit m of store_mask is set
  uint32_t store_mask;
  int32_t M, N, C, E, L, CG, WS, TT;              // CG = C / 8 slots per row, WS = W-tile row stride (entries), TT = N / 32
};

struct MixerLdsBf16Plan {
  int threads, lds_bytes, WS, nu_max, units;
};

// The one place that states the kernel's limits: false when the shape is outside them; fills *p otherwise.
bool plan_mixer_lds_bf16(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L, MixerLdsBf16Plan* p);
// packs the weights of pack.m[] into pack.images (= a.images), then runs the mixer: two launches on `s`
hipError_t launch_mixer_lds_bf16(const MixerLdsBf16Plan& p, bool res, const psf_mlp_bf16::Args& pack, const MixerLdsBf16Args& a,
                                 const Offsets& offs, int B, hipStream_t s);

}  // namespace psf
