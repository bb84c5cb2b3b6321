// mlp_bf16_tile.h — what the kernels that evaluate a bf16 token-wise MLP on the matrix pipe share: the rounding, the GELU on
// the accumulator registers and the evaluation of ONE 32-row hidden unit on one tile of 32
// tokens. Used by mlp_fwd_bf16.hip (the producer forward) and mixer_lds_bf16.h (the single-launch mixer): one body, so the two
// give the same bits. The image is mlp_bf16_image.h's; the kernel that writes it lives in mlp_fwd_bf16.hip
// (psf_mlp_bf16::pack_launch).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mlp_bf16_image.h"
#include "mlp_x3_common.h"
#include "mlp_x3_image.h"  // gelu2
#include "psf_common.h"    // lds_wait_all

namespace psf_mlp_bf16 {

using psf_x3::bf16x8;
using psf_x3::cd_row;
using psf_x3::f32x16;

// the kernel that writes the images of a.unit[0 .. a.U) into a.images (mlp_fwd_bf16.hip; Y of a.m[] is not read)
hipError_t pack_launch(const Args& a, hipStream_t s);

// f32 -> bf16, round to nearest even, a NaN stays a NaN (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint16_t bf16_rne_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

// registers 8 s .. 8 s + 7 of GEMM1's accumulator -> the B fragment of GEMM2's k-step s: round, widen, GELU, round
__device__ __forceinline__ bf16x8 gelu_frag(const f32x16& acc1, int s) {
  bf16x8 f;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const float z0 = (float)(__bf16)acc1[8 * s + i], z1 = (float)(__bf16)acc1[8 * s + i + 1];
    const f32x2 y = gelu2(f32x2{z0, z1});
    f[i] = (__bf16)y.x;
    f[i + 1] = (__bf16)y.y;
  }
  return f;
}

// an operand fragment re-defined behind a wait (psf_common.h: behind_wait), through a type an asm operand can have
__device__ __forceinline__ void frag_behind_wait(bf16x8& f) {
  using U4 = uint32_t __attribute__((ext_vector_type(4)));
  U4 r = __builtin_bit_cast(U4, f);
  asm volatile("" : "+v"(r));
  f = __builtin_bit_cast(bf16x8, r);
}

// One unit of an MLP on one tile: GEMM1 from the bias `sa`, k-steps ascending; the GELU on its accumulator; GEMM2 into acc2,
// which starts from the bias `sb` at the MLP's first unit. `img`: the unit's image in LDS; xf[s]: the lane's B fragment of
// k-step s of its token's data row (lane = (tok = c, half)).
// FULL_WAIT: every LDS operand is in registers and waited for in full before the first instruction that consumes one
// (psf_common.h, "LDS results in kernels that also issue MFMAs") — for a caller that mixes these MFMA phases with LDS-fed f32
// arithmetic. The arithmetic is the same either way.
template <int KS, bool FULL_WAIT>
__device__ __forceinline__ void mlp_unit(const unsigned char* img, const bf16x8 (&xf)[KS], bool first, f32x16& acc2, int c, int half) {
  const float* sa = reinterpret_cast<const float*>(img + kOffSa);
  const float* sb = reinterpret_cast<const float*>(img + kOffSb);
  bf16x8 wa[KS], wb[2];
#pragma unroll
  for (int s = 0; s < KS; ++s) wa[s] = *reinterpret_cast<const bf16x8*>(img + c * kARow + 32 * s + 16 * half);
#pragma unroll
  for (int s = 0; s < 2; ++s) wb[s] = *reinterpret_cast<const bf16x8*>(img + kOffB + ((s * 2 + half) * 32 + c) * 16);
  f32x16 acc1;
  if constexpr (FULL_WAIT) {
    float ba[16], bb[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ba[r] = sa[cd_row(r, half)], bb[r] = first ? sb[cd_row(r, half)] : 0.f;
    psf::lds_wait_all();
#pragma unroll
    for (int s = 0; s < KS; ++s) frag_behind_wait(wa[s]);
    frag_behind_wait(wb[0]), frag_behind_wait(wb[1]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      asm volatile("" : "+v"(ba[r]));
      asm volatile("" : "+v"(bb[r]));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = ba[r];
    if (first) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = bb[r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = sa[cd_row(r, half)];
    if (first) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[r] = sb[cd_row(r, half)];
    }
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[s], xf[s], acc1, 0, 0, 0);
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[0], gelu_frag(acc1, 0), acc2, 0, 0, 0);
  acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[1], gelu_frag(acc1, 1), acc2, 0, 0, 0);
}

}  // namespace psf_mlp_bf16
