// mlp_bwd_bf16.hip — the fused backward of the producer MLPs of a bf16 model (psf_mlp_bwd_bf16, include/psf_chord.h): the
// training twin of mlp_fwd_bf16.hip and the one-term twin of mlp_bwd_x3p_k (mlp_bwd.hip).
//
// The structure is mlp_bwd_x3p_k's without what f32 accuracy costs there: the operands already are bf16, so nothing is split,
// a product is ONE v_mfma_f32_32x32x16_bf16 where the split kernel issues six, and an image holds one plane instead of three.
// What the contract adds is the roundings of PyTorch's bf16 autograd: z, hh, g and d are rounded to bf16 on the accumulator
// registers before anything consumes them. Per 32-row hidden unit u = (k, ht) and 32-token tile, per wave:
//   1. H^T [j x tok] = A_u X^T + a_u      k-steps ascending from the bias (the forward's order: the forward's bits), then
//                                          z = bf16(acc), (y, y') = GELU, GELU'(f32(z)), hh = bf16(y)
//   2. g^T [j x tok] = B_u^T dY^T         two k-steps over o (outputs >= O are zero columns), g = bf16(acc)
//   3. d = bf16(f32(g) y')                packed as they stand, registers 8 s .. 8 s + 7 ARE the B fragment of step 6
//   4. dB_u^T [j x o] += hh^T dY          hh^T through the wave's scratch plane (accumulator-order store, transposed read)
//   5. dA_u [j x e]   += d X,  da_u += d 1   d through the same plane; da on the matrix pipe against a fragment of ones
//   6. dX^T [e x tok] += A_u^T d          A^T by transposed reads of the image in accumulator order; the accumulator persists
//                                          over ALL units of all MLPs and is rounded once, at the store
//   db_k: per-lane sums of the dY values, DPP-reduced over the token lanes, in the ht = 0 unit only.
// X and dY tiles are staged once as [tok][.] planes (mlp_planes.h) that serve both orientations. A dY row is 2 O bytes, so odd
// O leaves rows 2-byte aligned — but a tile's 32 rows are 64 O contiguous bytes from a 16-byte multiple of dY: the wave reads
// them as a flat burst of 16-byte vectors into its scratch, the ragged last tile ending in 2-byte loads (nothing at or beyond
// T O is read), and re-lays them into the plane with zeros beyond O and beyond the tile's rows (the forward's store, reversed).
// Weights: packed once per call into per-unit images, streamed through two LDS buffers by LDS-DMA, one barrier per unit.
// Weight gradients: the eight waves' sums are combined through LDS in a fixed order and flushed to the workgroup's slot of
// the partial buffer; mlp_bwd.hip's two-stage fixed-order reduction finishes them (no float atomics: bit-reproducible), with
// the one bf16 rounding at the final scatter. (The two reduction kernels are restated here, not shared: mlp_bwd.hip's unit
// keeps its instruction stream.)
// Limits: E a multiple of 8, 8 <= E <= 32; h <= 128; O <= 32; K <= 32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psf_chord.h"
#include "mlp_planes.h"
#include "psf_common.h"

extern "C" int psf_internal_fail(int code, const char* message);

namespace {

using psf_x3::bf16x8;
using psf_x3::cd_row;
using psf_x3::f32x16;
using psf_x3::kPlaneBytes;

constexpr int kBwMaxMlps = 32;
constexpr int kBwMaxUnits = 128;
constexpr int kBwPart = 1024 + 1024 + 64 + 64;  // per (slot, unit), f32: dA [j][e] | dB^T [j][o] | da [2][32] | db [2][32]
constexpr int kBwSlices = 64;                   // stage-1 reduction slices at most
static_assert(kBwPart % 4 == 0, "the stage-1 reduction reads the partial sums as float4");

// unit image (bytes): A plane [32 j][32 e] swizzled (mlp_planes.h) | sa [2 half][16 r] f32 | B^T [2 s][2 half][32 j][8 bf16]
//   A plane   row read = step-1 A operand, transposed read in accumulator order = step-6 A operand
//   sa        a[ht + cd_row(r, half)]: the lane's sixteen accumulator registers as four float4
//   B^T       step-2 A operand: B[o = 16 s + 8 half + i][ht + j]
constexpr int kBwOffSa = kPlaneBytes;             // 2048
constexpr int kBwOffBT = kBwOffSa + 128;          // 2176
constexpr int kBwImgBytes = kBwOffBT + 2048;      // 4224
constexpr int kBwImgVecs = kBwImgBytes / 16;      // 264
constexpr int kBwScrBytes = 2 * kPlaneBytes + 512;  // scratch plane / flat dY tile; as f32: combine tile [32][32] | da | db
constexpr int kBwWaves = 8;

struct BwMlp {
  const uint16_t* A;   // [h, E]
  const uint16_t* a;   // [h]
  const uint16_t* B;   // [O, h]
  const uint16_t* dY;  // [T, O]
  uint16_t* dA;
  uint16_t* da;
  uint16_t* dB;
  uint16_t* db;
  int32_t h, O;
};

struct BwArgs {
  BwMlp m[kBwMaxMlps];
  uint32_t unit[kBwMaxUnits];  // unit -> MLP | hidden block << 8 (dwords: one s_load_dword per unit)
  const uint16_t* X;
  uint16_t* dX;            // [T, E] or nullptr
  unsigned char* images;   // U images of kBwImgBytes
  float* partials;         // [G][U][kBwPart], one slot per workgroup
  float* stage1;           // [slices][U * kBwPart]
  int32_t slices;
  int64_t T;
  int64_t G;
  int32_t E, U;
};

// f32 -> bf16, round to nearest even, a NaN stays a NaN (v_cvt_pk_bf16_f32): mlp_bf16_tile.h's bf16_rne_bits, restated because
// that header brings mlp_x3_image.h's pack kernel into every unit that includes it
__device__ __forceinline__ uint16_t bf16_rne_bits(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
__device__ __forceinline__ float widen_bits(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// y = GELU(x) and dy/dx = Phi + x phi: gelu_and_grad1's arithmetic (mlp_bwd.hip), whose y is gelu2's operation for operation
// (mlp_x3_image.h: the forward's GELU), so hh has the forward's bits.
__device__ __forceinline__ void gelu_and_grad_bf16(float x, float& y, float& dydx) {
  const float t = __builtin_amdgcn_rcpf(fmaf(fabsf(x), 0.2316419f, 1.0f));
  float p = fmaf(0.53070271f, t, -0.72657602f);
  p = fmaf(p, t, 0.71070687f);
  p = fmaf(p, t, -0.14224837f);
  p = fmaf(p, t, 0.12741479f);
  p = p * t;
  const float E = __builtin_amdgcn_exp2f((x * x) * -0.72134752044448170368f);
  const float dlt = copysignf(0.5f - p * E, x);  // 0.5 - q >= 0
  const float Phi = 0.5f + dlt;
  y = x * Phi;
  dydx = fmaf(x * 0.39894228040143267794f, E, Phi);
}

__global__ void __launch_bounds__(256) mlp_bwd_bf16_pack_k(const BwArgs a) {
  using psf_x3::plane_off;
  const int u = blockIdx.x;
  const BwMlp d = a.m[a.unit[u] & 0xff];
  const int ht = 32 * (int)(a.unit[u] >> 8), E = a.E;
  unsigned char* img = a.images + (size_t)u * kBwImgBytes;
  uint16_t* img16 = reinterpret_cast<uint16_t*>(img);
  float* img32 = reinterpret_cast<float*>(img);
  for (int i = threadIdx.x; i < 32 * 32; i += 256) {  // A plane [j][e], swizzled; zero beyond E and beyond h
    const int j = i >> 5, e = i & 31;
    img16[(plane_off(j, e >> 3) >> 1) + (e & 7)] = (e < E && ht + j < d.h) ? d.A[(ht + j) * E + e] : (uint16_t)0;
  }
  for (int q = threadIdx.x; q < 32; q += 256) {  // sa[half][r] = a[ht + cd_row(r, half)]
    const int j = ht + cd_row(q & 15, q >> 4);
    img32[kBwOffSa / 4 + q] = j < d.h ? widen_bits(d.a[j]) : 0.f;
  }
  for (int q = threadIdx.x; q < 2 * 2 * 32 * 8; q += 256) {  // B^T: [s][half][j = col][i] = B[o = 16 s + 8 half + i][ht + j]
    const int i = q & 7, col = (q >> 3) & 31, hf = (q >> 8) & 1, s = q >> 9;
    const int o = 16 * s + 8 * hf + i;
    img16[kBwOffBT / 2 + q] = (o < d.O && ht + col < d.h) ? d.B[o * d.h + ht + col] : (uint16_t)0;
  }
}

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 32 lanes of the lane's half of the wave; every lane ends up with the total
__device__ __forceinline__ float half_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  return v + __shfl_xor(v, 16, 64);
}

// sixteen accumulator registers as eight packed dwords (register 2 m low, 2 m + 1 high) -> plane[c][row]: chunk g holds the
// four consecutive rows 8 g + 4 half .. + 3 (store_acc_plane's layout, one term)
__device__ __forceinline__ void store_acc_bf16(unsigned char* plane, const psf_x3::PlaneLane& L, const uint32_t (&d)[8]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) *reinterpret_cast<uint2*>(plane + L.acc_st + 16 * (g ^ L.acc_sw)) = uint2{d[2 * g], d[2 * g + 1]};
}
__device__ __forceinline__ bf16x8 acc_frag_bf16(const uint32_t (&d)[8], int s) {
  return __builtin_bit_cast(bf16x8, uint4{d[4 * s], d[4 * s + 1], d[4 * s + 2], d[4 * s + 3]});
}
__device__ __forceinline__ f32x16 mfma1(bf16x8 w, bf16x8 x, f32x16 acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, x, acc, 0, 0, 0);
}

// 512 threads, one workgroup per CU and per partial slot; every wave owns TPW tiles of 32 tokens.
template <int TPW>
__global__ void __launch_bounds__(512, 1) mlp_bwd_bf16_k(const BwArgs a) {
  using namespace psf_x3;
  constexpr int NW = kBwWaves;
  constexpr int kWaveBytes = 2 * TPW * kPlaneBytes + kBwScrBytes;  // X planes | dY planes | scratch
  // static LDS: 2 images + 8 waves x (TPW X planes + TPW dY planes + scratch) = 110 848 bytes at TPW = 2, 78 080 at TPW = 1
  __shared__ __attribute__((aligned(16))) unsigned char img_lds[2 * kBwImgBytes];
  __shared__ __attribute__((aligned(16))) unsigned char wave_lds[NW * kWaveBytes];
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, half = lane >> 5;
  unsigned char* XP = wave_lds + wv * kWaveBytes;  // [tile] planes [tok][e]
  unsigned char* YP = XP + TPW * kPlaneBytes;      // [tile] planes [tok][o] of the current MLP's dY
  unsigned char* HP = YP + TPW * kPlaneBytes;      // scratch: the flat dY tile, then hh^T, then d
  uint16_t* HP16 = reinterpret_cast<uint16_t*>(HP);
  float* SCR = reinterpret_cast<float*>(HP);       // the same bytes for the cross-wave combine
  const PlaneLane L = plane_lane(lane);
  const int E = a.E, U = a.U;
  const int64_t blk = blockIdx.x;

  auto stage = [&](int u) {  // image u by LDS-DMA: 16 bytes per lane, the wave's 1 KB destination is wave-uniform
    const unsigned char* src = a.images + (size_t)u * kBwImgBytes;
    unsigned char* dst = img_lds + (u & 1) * kBwImgBytes;
    if (tid < kBwImgVecs)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 16 * tid),
                                       (__attribute__((address_space(3))) void*)(dst + 16 * (tid & ~63)), 16, 0, 0);
  };

  f32x16 dxa[TPW];
  int64_t t0[TPW];
  int rows[TPW];  // wave-uniform; 0: the tile lies past T and the wave only keeps the barriers
#pragma unroll
  for (int tp = 0; tp < TPW; ++tp) {
    t0[tp] = ((blk * NW + wv) * TPW + tp) * 32;
    const int64_t left = a.T - t0[tp];
    rows[tp] = (int)(left >= 32 ? 32 : (left > 0 ? left : 0));
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int e0 = 16 * s + 8 * half;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (c < rows[tp] && e0 < E) v = *reinterpret_cast<const uint4*>(a.X + (t0[tp] + c) * E + e0);
      *reinterpret_cast<uint4*>(XP + tp * kPlaneBytes + L.row[s]) = v;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) dxa[tp][r] = 0.f;
  }
  stage(0);

  const bf16x8 ones = __builtin_bit_cast(bf16x8, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));
  for (int u = 0; u < U; ++u) {
    psf::dma_wait_all();  // this wave's part of image u has landed (hipcc puts no vmcnt wait in front of the barrier)
    __syncthreads();      // image u is complete in every wave's view; unit u-1's combine is finished
    if (u + 1 < U) stage(u + 1);
    const unsigned char* img = img_lds + (u & 1) * kBwImgBytes;
    const uint32_t ut = a.unit[u];
    const BwMlp& m = a.m[ut & 0xff];
    const bool first = (ut >> 8) == 0;  // the MLP's ht = 0 unit: stages dY, sums db
    const int O = m.O;

    f32x16 dA, dBT, dav;  // dav[r] = sum over tokens of d[cd_row(r, half)][tok], the same in every column
    float dbp[16];        // the lane's token, outputs 16 s + 8 half + i
#pragma unroll
    for (int r = 0; r < 16; ++r) dA[r] = dBT[r] = dav[r] = 0.f, dbp[r] = 0.f;
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      if (rows[tp] <= 0) continue;  // wave-uniform
      const unsigned char* xp = XP + tp * kPlaneBytes;
      unsigned char* yp = YP + tp * kPlaneBytes;
      if (first) {
        // the tile's rows are contiguous in dY from byte t0 2 O = 64 O (t0 / 32): 16-byte aligned whenever dY is
        const int nbytes = rows[tp] * 2 * O;  // <= 2048; nothing at or beyond this byte is read
        const unsigned char* yb = reinterpret_cast<const unsigned char*>(m.dY + t0[tp] * O);
        for (int v = lane; 16 * v + 16 <= nbytes; v += 64)
          *reinterpret_cast<uint4*>(HP + 16 * v) = *reinterpret_cast<const uint4*>(yb + 16 * v);
        const int done = (nbytes & ~15) >> 1, tail = (nbytes & 15) >> 1;  // in elements; tail < 8 (ragged tiles only)
        if (lane < tail) HP16[done + lane] = reinterpret_cast<const uint16_t*>(yb)[done + lane];
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();  // (a wave's LDS operations execute in order: the reads below see the writes above)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          uint32_t w[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int o = 16 * s + 8 * half + i;
            const bool ok = c < rows[tp] && o < O;
            const uint32_t v = HP16[ok ? c * O + o : 0];
            w[i] = ok ? v : 0u;
            dbp[8 * s + i] += __uint_as_float(w[i] << 16);
          }
          *reinterpret_cast<uint4*>(yp + L.row[s]) =
              make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();  // the scratch is rewritten behind these reads
      }
      // 1. H^T = A_u X^T + a_u, from the bias, k-steps ascending
      f32x16 acc1;
      {
        const float4* sa4 = reinterpret_cast<const float4*>(img + kBwOffSa + 64 * half);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = sa4[q];
          acc1[4 * q] = v.x, acc1[4 * q + 1] = v.y, acc1[4 * q + 2] = v.z, acc1[4 * q + 3] = v.w;
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) acc1 = mfma1(row_frag(img, L, s), row_frag(xp, L, s), acc1);
      // 2. g^T = B_u^T dY^T
      f32x16 acc3;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s)
        acc3 = mfma1(*reinterpret_cast<const bf16x8*>(img + kBwOffBT + ((s * 2 + half) * 32 + c) * 16), row_frag(yp, L, s), acc3);
      // 3. the roundings of the contract, on the accumulator registers
      uint32_t hp[8], dp[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        uint32_t hb[2], db2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const float z = (float)(__bf16)acc1[2 * q + i];
          float y, dd;
          gelu_and_grad_bf16(z, y, dd);
          const float g = (float)(__bf16)acc3[2 * q + i];
          hb[i] = bf16_rne_bits(y);
          db2[i] = bf16_rne_bits(g * dd);
        }
        hp[q] = hb[0] | (hb[1] << 16);
        dp[q] = db2[0] | (db2[1] << 16);
      }
      // hh^T and d through the scratch plane, back transposed: the A operands of the contractions over tokens
      bf16x8 ha[2], ga[2];
      store_acc_bf16(HP, L, hp);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int s = 0; s < 2; ++s) ha[s] = tr_frag(HP, L, s);
      asm volatile("" ::: "memory");
      store_acc_bf16(HP, L, dp);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int s = 0; s < 2; ++s) ga[s] = tr_frag(HP, L, s);
      asm volatile("" ::: "memory");
      // 6. dX^T += A_u^T d
      if (a.dX) {
#pragma unroll
        for (int s = 0; s < 2; ++s) dxa[tp] = mfma1(tr_frag_acc(img, L, s), acc_frag_bf16(dp, s), dxa[tp]);
      }
      // 4. dB_u^T += hh^T dY;  5. dA_u += d X, da_u += d 1
#pragma unroll
      for (int s = 0; s < 2; ++s) dBT = mfma1(ha[s], tr_frag(yp, L, s), dBT);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        dA = mfma1(ga[s], tr_frag(xp, L, s), dA);
        dav = mfma1(ga[s], ones, dav);
      }
    }
    if (first) {
#pragma unroll
      for (int i = 0; i < 16; ++i) dbp[i] = half_sum(dbp[i]);
    }
    // Combine the eight waves' sums through LDS (fixed order w = 0..7) and flush once per workgroup.
    float* pu = a.partials + (blk * (int64_t)U + u) * kBwPart;
    const float* wave0 = reinterpret_cast<const float*>(wave_lds + 2 * TPW * kPlaneBytes);  // wave 0's SCR
    auto sum8 = [&](int off) {  // off: float offset into a wave's SCR, 16-byte aligned
      float4 acc = *reinterpret_cast<const float4*>(wave0 + off);
#pragma unroll
      for (int w = 1; w < NW; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(wave0 + w * (kWaveBytes / 4) + off);
        acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
      }
      return acc;
    };
    asm volatile("" ::: "memory");
#pragma unroll
    for (int r = 0; r < 16; ++r) SCR[cd_row(r, half) * 32 + c] = dA[r];
    SCR[1024 + lane] = 0.f;  // da [2][32]: the whole sum goes to row 0
    SCR[1088 + lane] = 0.f;  // db [2][32]
    if (c == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) SCR[1024 + cd_row(r, half)] = dav[r];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) SCR[1088 + 16 * s + 8 * half + i] = dbp[8 * s + i];
    }
    __syncthreads();
    if (wv < 4) *reinterpret_cast<float4*>(pu + wv * 256 + 4 * lane) = sum8(wv * 256 + 4 * lane);
    if (wv == 4 && lane < 32) *reinterpret_cast<float4*>(pu + 2048 + 4 * lane) = sum8(1024 + 4 * lane);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) SCR[cd_row(r, half) * 32 + c] = dBT[r];
    __syncthreads();
    if (wv < 4) *reinterpret_cast<float4*>(pu + 1024 + wv * 256 + 4 * lane) = sum8(wv * 256 + 4 * lane);
  }

  if (a.dX) {  // the lane holds dX^T[e = 8 g + 4 half + (0..3)][tok = c] in registers 4 g .. 4 g + 3: the ONE rounding of dX
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      if (c < rows[tp]) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int e0 = 8 * gq + 4 * half;
          if (e0 < E) {
            uint2 v;
            v.x = (uint32_t)bf16_rne_bits(dxa[tp][4 * gq]) | ((uint32_t)bf16_rne_bits(dxa[tp][4 * gq + 1]) << 16);
            v.y = (uint32_t)bf16_rne_bits(dxa[tp][4 * gq + 2]) | ((uint32_t)bf16_rne_bits(dxa[tp][4 * gq + 3]) << 16);
            *reinterpret_cast<uint2*>(a.dX + (t0[tp] + c) * E + e0) = v;
          }
        }
      }
    }
  }
}

// stage 1: R1[s][i] = sum over the slots of slice s of P[g][i]   (mlp_bwd_reduce1_k's fixed order: four interleaved running
// sums g = g0 + 0, 1, 2, 3 (mod 4), then ((s0 + s1) + s2) + s3)
__global__ void __launch_bounds__(256) mlp_bwd_bf16_reduce1_k(const BwArgs a) {
  const int64_t n4 = (int64_t)a.U * kBwPart / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int s = blockIdx.y;
  const int64_t per = (a.G + a.slices - 1) / a.slices;
  const int64_t g0 = s * per, g1 = g0 + per < a.G ? g0 + per : a.G;
  const float4* __restrict__ P = reinterpret_cast<const float4*>(a.partials);
  float4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  int64_t g = g0;
  for (; g + 4 <= g1; g += 4) {
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = P[(g + q) * n4 + i];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q].x += v[q].x, acc[q].y += v[q].y, acc[q].z += v[q].z, acc[q].w += v[q].w;
  }
  // the up to three slots left over, into running sums 0, 1, 2 as the loop above would: statically indexed (a run-time index
  // into acc[] makes hipcc move the array to LDS)
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (g + q < g1) {
      const float4 v = P[(g + q) * n4 + i];
      acc[q].x += v.x, acc[q].y += v.y, acc[q].z += v.z, acc[q].w += v.w;
    }
  }
  float4 r;
  r.x = ((acc[0].x + acc[1].x) + acc[2].x) + acc[3].x;
  r.y = ((acc[0].y + acc[1].y) + acc[2].y) + acc[3].y;
  r.z = ((acc[0].z + acc[1].z) + acc[2].z) + acc[3].z;
  r.w = ((acc[0].w + acc[1].w) + acc[2].w) + acc[3].w;
  reinterpret_cast<float4*>(a.stage1)[s * n4 + i] = r;
}

// stage 2: sum the slices, round ONCE to bf16 and scatter into the unpadded gradient tensors
__global__ void __launch_bounds__(256) mlp_bwd_bf16_reduce2_k(const BwArgs a) {
  const int64_t n = (int64_t)a.U * kBwPart;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int u = (int)(idx / kBwPart), i = (int)(idx - (int64_t)u * kBwPart);
  const BwMlp& d = a.m[a.unit[u] & 0xff];
  const int ht = 32 * (int)(a.unit[u] >> 8), E = a.E;
  auto total = [&](int64_t at) {
    float acc = 0.f;
    for (int s = 0; s < a.slices; ++s) acc += a.stage1[s * n + at];
    return acc;
  };
  if (i < 1024) {
    const int j = i >> 5, e = i & 31;
    if (ht + j < d.h && e < E) d.dA[(ht + j) * E + e] = bf16_rne_bits(total(idx));
  } else if (i < 2048) {
    const int j = (i - 1024) >> 5, o = i & 31;
    if (ht + j < d.h && o < d.O) d.dB[o * d.h + ht + j] = bf16_rne_bits(total(idx));
  } else if (i < 2048 + 32) {
    const int j = i - 2048;
    if (ht + j < d.h) d.da[ht + j] = bf16_rne_bits(total(idx) + total(idx + 32));
  } else if (i >= 2112 && i < 2112 + 32) {
    const int o = i - 2112;
    if (ht == 0 && o < d.O) d.db[o] = bf16_rne_bits(total(idx) + total(idx + 32));
  }
}

struct BwPlan {
  int U;
  int tpw;  // tiles per wave: 2, or 1 for inputs under 512 workgroups' worth of tokens (more workgroups in flight)
  int64_t G;  // workgroups = partial slots
  int slices;
  uint32_t unit[kBwMaxUnits];
};

bool make_plan(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O, BwPlan* p) {
  if (T < 1 || E < 8 || E > 32 || (E & 7) || K < 1 || K > kBwMaxMlps || !h || !O) return false;
  p->U = 0;
  for (int u = 0; u < kBwMaxUnits; ++u) p->unit[u] = 0;
  for (int k = 0; k < K; ++k) {
    if (h[k] < 1 || h[k] > 128 || O[k] < 1 || O[k] > 32) return false;
    for (int hb = 0; hb * 32 < h[k]; ++hb) p->unit[p->U++] = (uint32_t)k | ((uint32_t)hb << 8);
  }
  const int64_t tiles = (T + 31) / 32;
  p->tpw = (tiles + kBwWaves - 1) / kBwWaves >= 512 ? 2 : 1;
  p->G = (tiles + kBwWaves * p->tpw - 1) / (kBwWaves * p->tpw);
  // stage-1 slices: about sixteen partial slots each, at most kBwSlices (mlp_bwd.hip)
  const int64_t sl = (p->G + 15) / 16;
  p->slices = (int)(sl < 1 ? 1 : (sl > kBwSlices ? kBwSlices : sl));
  return p->G <= 0x7fffffff;
}

int64_t workspace_bytes_of(const BwPlan& p) {
  return (int64_t)p.U * kBwImgBytes + (p.G + p.slices) * (int64_t)p.U * kBwPart * (int64_t)sizeof(float);
}

}  // namespace

extern "C" {

int64_t psf_mlp_bwd_bf16_workspace(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O) {
  BwPlan p;
  if (!make_plan(T, E, K, h, O, &p)) return -1;
  return workspace_bytes_of(p);
}

int psf_mlp_bwd_bf16(const uint16_t* X, int64_t T, int32_t E, int32_t K, const uint16_t* const* A, const uint16_t* const* a,
                     const uint16_t* const* B, const int32_t* h, const int32_t* O, const uint16_t* const* dY, uint16_t* dX,
                     uint16_t* const* dA, uint16_t* const* da, uint16_t* const* dB, uint16_t* const* db, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (!X || !A || !a || !B || !h || !O || !dY || !dA || !da || !dB || !db || !workspace)
    return psf_internal_fail(PSF_E_NULL, "psf_mlp_bwd_bf16: NULL argument");
  BwPlan p;
  if (!make_plan(T, E, K, h, O, &p))
    return psf_internal_fail(PSF_E_SHAPE, "psf_mlp_bwd_bf16: need T >= 1, E in {8,16,24,32}, 1 <= K <= 32, 1 <= h <= 128, 1 <= O <= 32");
  if ((reinterpret_cast<uintptr_t>(X) & 15) != 0 || (reinterpret_cast<uintptr_t>(dX) & 15) != 0)
    return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_bwd_bf16: X and dX must be 16-byte aligned");
  for (int k = 0; k < K; ++k)
    if ((reinterpret_cast<uintptr_t>(dY[k]) & 15) != 0)
      return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_bwd_bf16: every dY[k] must be 16-byte aligned");
  if (workspace_bytes < workspace_bytes_of(p) || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return psf_internal_fail(PSF_E_SHAPE, "psf_mlp_bwd_bf16: workspace too small (psf_mlp_bwd_bf16_workspace) or not 16-byte aligned");
  BwArgs args;
  for (int k = 0; k < kBwMaxMlps; ++k) args.m[k] = BwMlp{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  for (int k = 0; k < K; ++k) {
    if (!A[k] || !a[k] || !B[k] || !dY[k] || !dA[k] || !da[k] || !dB[k] || !db[k])
      return psf_internal_fail(PSF_E_NULL, "psf_mlp_bwd_bf16: NULL layer pointer");
    if (((reinterpret_cast<uintptr_t>(A[k]) | reinterpret_cast<uintptr_t>(a[k]) | reinterpret_cast<uintptr_t>(B[k]) |
          reinterpret_cast<uintptr_t>(dA[k]) | reinterpret_cast<uintptr_t>(da[k]) | reinterpret_cast<uintptr_t>(dB[k]) |
          reinterpret_cast<uintptr_t>(db[k])) & 1) != 0)
      return psf_internal_fail(PSF_E_ALIGN, "psf_mlp_bwd_bf16: weights, biases and their gradients must be 2-byte aligned");
    args.m[k] = BwMlp{A[k], a[k], B[k], dY[k], dA[k], da[k], dB[k], db[k], h[k], O[k]};
  }
  for (int u = 0; u < kBwMaxUnits; ++u) args.unit[u] = p.unit[u];
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  args.X = X;
  args.dX = dX;
  args.images = ws;
  args.partials = reinterpret_cast<float*>(ws + (int64_t)p.U * kBwImgBytes);  // kBwImgBytes is a multiple of 16
  args.stage1 = args.partials + p.G * p.U * kBwPart;
  args.slices = p.slices;
  args.T = T;
  args.G = p.G;
  args.E = E;
  args.U = p.U;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mlp_bwd_bf16_pack_k, dim3(p.U), dim3(256), 0, s, args);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return psf_internal_fail((int)e, hipGetErrorString(e));
  // every slot of the partial buffer is written exactly once: one workgroup per 8 waves x TPW tiles
  if (p.tpw == 2)
    hipLaunchKernelGGL(mlp_bwd_bf16_k<2>, dim3((unsigned)p.G), dim3(64 * kBwWaves), 0, s, args);
  else
    hipLaunchKernelGGL(mlp_bwd_bf16_k<1>, dim3((unsigned)p.G), dim3(64 * kBwWaves), 0, s, args);
  e = hipGetLastError();
  if (e != hipSuccess) return psf_internal_fail((int)e, hipGetErrorString(e));
  const int64_t n = (int64_t)p.U * kBwPart;
  hipLaunchKernelGGL(mlp_bwd_bf16_reduce1_k, dim3((unsigned)((n / 4 + 255) / 256), (unsigned)p.slices), dim3(256), 0, s, args);
  hipLaunchKernelGGL(mlp_bwd_bf16_reduce2_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, args);
  e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

}  // extern "C"
