// mlp_bf16_image.h — the packed weight image of one 32-row hidden unit of a bf16 token-wise MLP Linear(E,h) -> GELU ->
// Linear(h,O), and the unit table of a call, for mlp_fwd_bf16.hip. The one-term twin of mlp_x3_image.h: the operands already
// are bf16, so an image holds one term where the split-bf16 kernels hold three, and the orientation is the same (GEMM1
// H^T[j][tok] = A_u X^T, GEMM2 Y^T[o][tok] += B_u[o][rho] H^T, the accumulator of GEMM1 as the B operand of GEMM2).
#pragma once

#include <stdint.h>

namespace psf_mlp_bf16 {

// unit image (bytes): A [32 j][144 B: 64 bf16 + pad] | sa 32 f32 | B' [2 s][2 half][32 o][8 bf16] | sb 32 f32
constexpr int kARow = 144;               // bytes; 36-dword stride: ds_read_b128 conflict-free over 16 lanes
constexpr int kOffSa = 32 * kARow;       // 4608
constexpr int kOffB = kOffSa + 128;      // 4736
constexpr int kBBytes = 2 * 2 * 32 * 16; // 2048
constexpr int kOffSb = kOffB + kBBytes;  // 6784
constexpr int kImgBytes = kOffSb + 128;  // 6912
constexpr int kImgVecs = kImgBytes / 16; // 432
constexpr int kTileBytes = 32 * 32 * 2;  // per-wave output tile: 32 tokens x up to 32 bf16 outputs

constexpr int kMaxE = 64, kMaxH = 128, kMaxO = 32, kMaxK = 32;

struct Mlp {
  const uint16_t* A;
  const uint16_t* a;
  const uint16_t* B;
  const uint16_t* b;
  uint16_t* Y;
  int32_t h, O;
};

struct Args {
  Mlp m[kMaxK];
  uint32_t unit[128];  // unit -> MLP | hidden block << 8 | (last unit of its MLP) << 16 (dwords: one s_load_dword per unit)
  const uint16_t* X;
  unsigned char* images;
  int64_t T;
  int32_t E, U;
};

// every MLP is cut into ceil(h/32) units of 32 hidden rows, MLP by MLP. false: the sizes are outside the kernel's limits
inline bool make_plan(int32_t E, int32_t K, const int32_t* h, const int32_t* O, uint32_t* unit, int32_t* U) {
  if (E < 8 || E > kMaxE || (E & 7) || K < 1 || K > kMaxK || !h || !O) return false;
  int n = 0;
  for (int k = 0; k < K; ++k) {
    if (h[k] < 1 || h[k] > kMaxH || O[k] < 1 || O[k] > kMaxO) return false;
    const int nb = (h[k] + 31) / 32;
    for (int hb = 0; hb < nb; ++hb) unit[n++] = (uint32_t)k | ((uint32_t)hb << 8) | ((uint32_t)(hb == nb - 1) << 16);
  }
  for (int u = n; u < 128; ++u) unit[u] = 0;
  *U = n;
  return true;
}

}  // namespace psf_mlp_bf16
