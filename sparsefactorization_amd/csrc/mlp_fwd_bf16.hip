// mlp_fwd_bf16.hip — the fused producer-MLP forward for bf16 models: K two-layer MLPs sharing one input in one launch,
// the hidden layer never leaving the registers (psf_mlp_fwd_bf16, include/psf_chord.h).
//
// The structure is x3_fwd_k's (mlp_fwd_x3.hip) without what f32 accuracy costs there: the operands already are bf16, so a
// product is ONE v_mfma_f32_32x32x16_bf16 term where the split kernel issues six, nothing is split, and an image holds one
// term instead of three (mlp_bf16_image.h).
//   X      no LDS staging: lane (tok = lane & 31, half = lane >> 5) loads its B-operand fragment of k-step s as one 16-byte
//          load, X[t, 16 s + 8 half .. +7]; ceil(E / 16) k-steps (the kernel is compiled per k-step count); the half-step
//          beyond E of E % 16 == 8 is zero and is not loaded
//   GEMM1  H^T[j][tok] = A_u X^T + a, accumulated in f32 from the bias
//   GELU   on the accumulator registers: z = bf16(acc), h = bf16(gelu2(f32(z))). Registers 8 s .. 8 s + 7 of lane (tok, half)
//          are hidden rows rho(r, half) — packed as they stand they ARE the lane's B fragment of GEMM2's k-step s
//   GEMM2  Y^T[o][tok] += B_u[o][rho] H^T over the MLP's units, in f32 from the bias b; rounded to bf16 once, at the store
//   Store  a Y row is 2 O bytes, so odd O leaves rows 2-byte aligned — but the tile's 32 rows are 64 O contiguous bytes
//          starting at a multiple of 64 bytes of Y. The wave transposes the tile into its own LDS and writes it as a flat
//          burst of 16-byte vectors; the ragged last tile ends at (T - t0) 2 O bytes with a tail of 2-byte stores.
// Weights: packed once per call into per-unit images, streamed through two LDS buffers by LDS-DMA, one barrier per unit.
// Limits: E a multiple of 8, 8 <= E <= 64; h <= 128; O <= 32; K <= 32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psf_chord.h"
#include "mlp_bf16_tile.h"

extern "C" int psf_internal_fail(int code, const char* message);

namespace {

namespace mb = psf_mlp_bf16;  // (qualified: mlp_x3_image.h has constants of the same names in this unnamed namespace)
using mb::bf16_rne_bits;
using psf_x3::bf16x8;
using psf_x3::cd_row;
using psf_x3::f32x16;

__device__ __forceinline__ float widen_bits(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// One workgroup per unit: the weights in operand order, the biases widened to f32.
__global__ void __launch_bounds__(256) mlp_bf16_pack_k(const mb::Args a) {
  const int u = blockIdx.x;
  const mb::Mlp d = a.m[a.unit[u] & 0xff];
  const int ht = 32 * (int)((a.unit[u] >> 8) & 0xff), E = a.E;
  unsigned char* img = a.images + (size_t)u * mb::kImgBytes;
  uint16_t* img16 = reinterpret_cast<uint16_t*>(img);
  float* img32 = reinterpret_cast<float*>(img);
  // A: [j][e], zero beyond E and beyond h (the pad included)
  for (int i = threadIdx.x; i < 32 * (mb::kARow / 2); i += 256) {
    const int j = i / (mb::kARow / 2), e = i - j * (mb::kARow / 2);
    img16[i] = (e < E && ht + j < d.h) ? d.A[(ht + j) * E + e] : (uint16_t)0;
  }
  for (int j = threadIdx.x; j < 32; j += 256) {
    img32[mb::kOffSa / 4 + j] = ht + j < d.h ? widen_bits(d.a[ht + j]) : 0.f;
    img32[mb::kOffSb / 4 + j] = j < d.O ? widen_bits(d.b[j]) : 0.f;
  }
  // B': [s][half][o][i] = B[o][ht + rho], rho = (i&3) + 16 s + 8 (i>>2) + 4 half
  for (int q = threadIdx.x; q < 2 * 2 * 32 * 8; q += 256) {
    const int i = q & 7, o = (q >> 3) & 31, hf = (q >> 8) & 1, s = q >> 9;
    const int rho = (i & 3) + 16 * s + 8 * (i >> 2) + 4 * hf;
    img16[mb::kOffB / 2 + q] = (o < d.O && ht + rho < d.h) ? d.B[o * d.h + ht + rho] : (uint16_t)0;
  }
}

// The LDS-DMA of an image is counted by vmcnt and by nothing else: hipcc puts no vmcnt wait in front of a workgroup barrier
// (the waves of a workgroup share a CU) nor in front of the ds_reads of the image. Every wave drains its own pieces before
// the barrier; behind the barrier all pieces have landed.
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// KS = ceil(E / 16) k-steps of the first GEMM. One tile of 32 tokens per wave, four waves, grid-strided.
template <int KS>
__global__ void __launch_bounds__(256, 4) mlp_fwd_bf16_k(const mb::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 31, half = lane >> 5;
  unsigned char* tile = lds_raw + 2 * mb::kImgBytes + wv * mb::kTileBytes;  // the wave's output tile [tok][O] bf16
  uint16_t* tile16 = reinterpret_cast<uint16_t*>(tile);
  const int E = a.E, U = a.U;
  const int64_t tiles = (a.T + 31) / 32;

  auto stage = [&](int u) {
    const unsigned char* src = a.images + (size_t)u * mb::kImgBytes;
    unsigned char* dst = lds_raw + (u & 1) * mb::kImgBytes;
    for (int v0 = 0; v0 < mb::kImgVecs; v0 += 256) {
      const int v = v0 + tid;
      if (v < mb::kImgVecs)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 16 * v),
                                         (__attribute__((address_space(3))) void*)(dst + 16 * (v0 + (tid & ~63))), 16, 0, 0);
    }
  };

  for (int64_t blk = blockIdx.x; blk * 4 < tiles; blk += gridDim.x) {
    const int64_t t0 = (blk * 4 + wv) * 32;
    const int64_t left = a.T - t0;
    const int rows = (int)(left >= 32 ? 32 : (left > 0 ? left : 0));  // wave-uniform; 0: the wave only keeps the barriers
    bf16x8 xf[KS];  // k-step s covers e = 16 s + 8 half + (0..7) of the lane's token
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (c < rows && 16 * s + 8 * half < E) v = *reinterpret_cast<const uint4*>(a.X + (t0 + c) * E + 16 * s + 8 * half);
      xf[s] = __builtin_bit_cast(bf16x8, v);
    }
    __syncthreads();  // the previous block's last unit is done with both image buffers
    stage(0);

    f32x16 acc2 = {};
    for (int u = 0; u < U; ++u) {
      dma_wait();
      __syncthreads();  // image u has landed in every wave's view; unit u-1 is finished
      if (u + 1 < U) stage(u + 1);
      const unsigned char* img = lds_raw + (u & 1) * mb::kImgBytes;
      const uint32_t ut = a.unit[u];
      const bool first = ((ut >> 8) & 0xff) == 0, last = (ut >> 16) != 0;
      mb::mlp_unit<KS, false>(img, xf, first, acc2, c, half);

      if (last && rows > 0) {
        const mb::Mlp& dp = a.m[ut & 0xff];
        const int O = dp.O;
        // register r of lane (tok, half) is Y^T[o = rho(r, half)][tok]: into the wave's tile, row-major as Y is
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = cd_row(r, half);
          if (o < O) tile16[c * O + o] = bf16_rne_bits(acc2[r]);
        }
        __builtin_amdgcn_wave_barrier();  // (a wave's LDS operations execute in order: the reads below see the writes above)
        // the tile's rows are contiguous in Y from byte t0 2 O = 64 O (t0 / 32): 16-byte aligned whenever Y is
        const int nbytes = rows * 2 * O;  // <= 2048; nothing at or beyond this byte is written
        unsigned char* yb = reinterpret_cast<unsigned char*>(dp.Y + t0 * O);
        for (int v = lane; 16 * v + 16 <= nbytes; v += 64)
          *reinterpret_cast<uint4*>(yb + 16 * v) = *reinterpret_cast<const uint4*>(tile + 16 * v);
        const int done = (nbytes & ~15) >> 1, tail = (nbytes & 15) >> 1;  // in elements; tail < 8 (ragged tiles only)
        if (lane < tail) reinterpret_cast<uint16_t*>(yb)[done + lane] = tile16[done + lane];
        __builtin_amdgcn_wave_barrier();  // the next MLP's tile is written behind these reads
      }
    }
  }
}

constexpr size_t kLdsBytes = 2 * (size_t)mb::kImgBytes + 4 * (size_t)mb::kTileBytes;
static_assert(kLdsBytes <= 48 * 1024, "no dynamic-LDS attribute needed");

void fill_args(const uint32_t* unit, int32_t U, const uint16_t* X, int64_t T, int32_t E, int32_t K, const uint16_t* const* A,
               const uint16_t* const* a, const uint16_t* const* B, const uint16_t* const* b, const int32_t* h, const int32_t* O,
               uint16_t* const* Y, void* workspace, mb::Args* args) {
  for (int k = 0; k < mb::kMaxK; ++k) args->m[k] = mb::Mlp{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  for (int k = 0; k < K; ++k) args->m[k] = mb::Mlp{A[k], a[k], B[k], b[k], Y[k], h[k], O[k]};
  for (int u = 0; u < 128; ++u) args->unit[u] = unit[u];
  args->X = X;
  args->images = reinterpret_cast<unsigned char*>(workspace);
  args->T = T;
  args->E = E;
  args->U = U;
}

}  // namespace

// the pack kernel for the other unit that evaluates these images (mixer_lds_bf16_inst.hip): Y of args.m[] is not read
hipError_t psf_mlp_bf16::pack_launch(const psf_mlp_bf16::Args& args, hipStream_t s) {
  hipLaunchKernelGGL(mlp_bf16_pack_k, dim3(args.U), dim3(256), 0, s, args);
  return hipGetLastError();
}

extern "C" {

int64_t psf_mlp_fwd_bf16_workspace(int32_t E, int32_t K, const int32_t* h, const int32_t* O) {
  uint32_t unit[128];
  int32_t U = 0;
  if (!mb::make_plan(E, K, h, O, unit, &U)) return -1;
  return (int64_t)U * mb::kImgBytes;
}

int psf_mlp_fwd_bf16(const uint16_t* X, int64_t T, int32_t E, int32_t K, const uint16_t* const* A, const uint16_t* const* a,
                     const uint16_t* const* B, const uint16_t* const* b, const int32_t* h, const int32_t* O,
                     uint16_t* const* Y, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!X || !A || !a || !B || !b || !h || !O || !Y || !workspace)
    return psf_internal_fail(PSF_E_NULL, "psf_mlp_fwd_bf16: NULL argument");
  uint32_t unit[128];
  int32_t U = 0;
  if (T < 1 || !mb::make_plan(E, K, h, O, unit, &U))
    return psf_internal_fail(PSF_E_SHAPE, "psf_mlp_fwd_bf16: need T >= 1, E in {8,16,...,64}, 1 <= K <= 32, 1 <= h <= 128, 1 <= O <= 32");
  if ((reinterpret_cast<uintptr_t>(X) & 15) != 0)
    return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_fwd_bf16: X must be 16-byte aligned");
  if (workspace_bytes < (int64_t)U * mb::kImgBytes || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return psf_internal_fail(PSF_E_SHAPE, "psf_mlp_fwd_bf16: workspace too small (psf_mlp_fwd_bf16_workspace) or not 16-byte aligned");
  for (int k = 0; k < K; ++k) {
    if (!A[k] || !a[k] || !B[k] || !b[k] || !Y[k]) return psf_internal_fail(PSF_E_NULL, "psf_mlp_fwd_bf16: NULL layer pointer");
    if ((reinterpret_cast<uintptr_t>(Y[k]) & 15) != 0)
      return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_fwd_bf16: every Y[k] must be 16-byte aligned");
    if (((reinterpret_cast<uintptr_t>(A[k]) | reinterpret_cast<uintptr_t>(a[k]) | reinterpret_cast<uintptr_t>(B[k]) |
          reinterpret_cast<uintptr_t>(b[k])) & 1) != 0)
      return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_fwd_bf16: weights and biases must be 2-byte aligned");
  }
  mb::Args args;
  fill_args(unit, U, X, T, E, K, A, a, B, b, h, O, Y, workspace, &args);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mlp_bf16_pack_k, dim3(U), dim3(256), 0, s, args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return psf_internal_fail((int)e, hipGetErrorString(e));
  const int64_t tiles = (T + 31) / 32;
  const int64_t blocks_needed = (tiles + 3) / 4;  // four waves, one tile each
  const int grid = (int)(blocks_needed < 4096 ? blocks_needed : 4096);
  switch ((E + 15) / 16) {
    case 1: hipLaunchKernelGGL(mlp_fwd_bf16_k<1>, dim3(grid), dim3(256), kLdsBytes, s, args); break;
    case 2: hipLaunchKernelGGL(mlp_fwd_bf16_k<2>, dim3(grid), dim3(256), kLdsBytes, s, args); break;
    case 3: hipLaunchKernelGGL(mlp_fwd_bf16_k<3>, dim3(grid), dim3(256), kLdsBytes, s, args); break;
    default: hipLaunchKernelGGL(mlp_fwd_bf16_k<4>, dim3(grid), dim3(256), kLdsBytes, s, args); break;
  }
  e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

}  // extern "C"
