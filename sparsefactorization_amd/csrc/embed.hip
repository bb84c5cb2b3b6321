// embed.hip — token embedding lookup fused with the positional-embedding add.
//
//   out[t, :] = table[idx[t], :] (+ pos[t mod N, :])            t < T = B*N tokens
//
// PSFNet's first two lines (SyntheticExperiments/psf.py:152-163 `embedding(data)` ... `+ pos_embedding(positions)`,
// LRA/psf.py:203-214): through PyTorch a gather kernel (142 us for the 84 MB of Temporal Order at N = 16384,
// B = 64: a 6-row table looked up a million times) followed by a broadcast add that re-reads and re-writes the
// same 84 MB. Here one pass: 16 bytes per thread, the index and table row come from cache, the output is written
// once. HBM-bound on the output (4*E bytes per token).
//
// Both the pass and the table gradient below have a bf16 instance (psf_embed_tokens_bf16, psf_embed_tokens_bwd_bf16): bf16
// storage, f32 arithmetic, one rounding per element.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/psf_chord.h"

extern "C" int psf_internal_fail(int code, const char* message);

namespace {

__global__ void __launch_bounds__(256)
embed_tokens_k(const int64_t* __restrict__ idx, const float* __restrict__ table, const float* __restrict__ pos,
               float* __restrict__ out, int64_t T, int64_t N, int32_t V, int32_t E4) {
  const int64_t total = T * E4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / E4;
    const int e4 = (int)(i - t * E4);
    int64_t v = idx[t];
    v = v < 0 ? 0 : (v >= V ? V - 1 : v);  // out-of-range ids are the caller's error (checked on the host side of the
                                           // Python wrapper in debug runs); never read outside the table
    float4 r = reinterpret_cast<const float4*>(table)[v * E4 + e4];
    if (pos) {
      const float4 p = reinterpret_cast<const float4*>(pos)[(t % N) * E4 + e4];
      r.x += p.x;
      r.y += p.y;
      r.z += p.z;
      r.w += p.w;
    }
    reinterpret_cast<float4*>(out)[i] = r;
  }
}

}  // namespace

extern "C" int psf_embed_tokens_f32(const int64_t* idx, const float* table, const float* pos, float* out, int64_t T,
                                    int64_t N, int32_t V, int32_t E, void* stream) {
  if (!idx || !table || !out) return psf_internal_fail(PSF_E_NULL, "psf_embed_tokens: idx, table and out must be non-NULL");
  if (T < 0 || N < 1 || V < 1 || E < 4 || (E & 3)) return psf_internal_fail(PSF_E_SHAPE, "psf_embed_tokens: need T >= 0, N >= 1, V >= 1, E a positive multiple of 4");
  if ((reinterpret_cast<uintptr_t>(table) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) ||
      (pos && (reinterpret_cast<uintptr_t>(pos) & 15)) || (reinterpret_cast<uintptr_t>(idx) & 7))
    return psf_internal_fail(PSF_E_ALIGN, "psf_embed_tokens: table, pos and out must be 16-byte aligned, idx 8-byte aligned");
  if (T == 0) return PSF_OK;
  const int64_t total = T * (E / 4);
  const int64_t blocks = (total + 255) / 256;
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  hipLaunchKernelGGL(embed_tokens_k, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), idx, table, pos, out, T, N,
                     V, E / 4);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

// bf16 table, pos and out: 8 channels per 16-byte vector; table + pos is one f32 add rounded to nearest even once, which are
// the bits of the stock bf16 `embedding(idx) + pos.unsqueeze(0)` (a bf16 add there is the f32 sum, rounded).
namespace {

using Bf16x8 = __bf16 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(256)
embed_tokens_bf16_k(const int64_t* __restrict__ idx, const __bf16* __restrict__ table, const __bf16* __restrict__ pos,
                    __bf16* __restrict__ out, int64_t T, int64_t N, int32_t V, int32_t E8) {
  const int64_t total = T * E8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / E8;
    const int e8 = (int)(i - t * E8);
    int64_t v = idx[t];
    v = v < 0 ? 0 : (v >= V ? V - 1 : v);  // as embed_tokens_k: never a read outside the table
    Bf16x8 r = reinterpret_cast<const Bf16x8*>(table)[v * E8 + e8];
    if (pos) {
      const Bf16x8 p = reinterpret_cast<const Bf16x8*>(pos)[(t % N) * E8 + e8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (__bf16)__fadd_rn((float)r[e], (float)p[e]);
    }
    reinterpret_cast<Bf16x8*>(out)[i] = r;
  }
}

}  // namespace

extern "C" int psf_embed_tokens_bf16(const int64_t* idx, const uint16_t* table, const uint16_t* pos, uint16_t* out, int64_t T,
                                     int64_t N, int32_t V, int32_t E, void* stream) {
  if (!idx || !table || !out) return psf_internal_fail(PSF_E_NULL, "psf_embed_tokens_bf16: idx, table and out must be non-NULL");
  if (T < 0 || N < 1 || V < 1 || E < 8 || (E & 7)) return psf_internal_fail(PSF_E_SHAPE, "psf_embed_tokens_bf16: need T >= 0, N >= 1, V >= 1, E a positive multiple of 8");
  if ((reinterpret_cast<uintptr_t>(table) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) ||
      (pos && (reinterpret_cast<uintptr_t>(pos) & 15)) || (reinterpret_cast<uintptr_t>(idx) & 7))
    return psf_internal_fail(PSF_E_ALIGN, "psf_embed_tokens_bf16: table, pos and out must be 16-byte aligned, idx 8-byte aligned");
  if (T == 0) return PSF_OK;
  const int64_t total = T * (E / 8);
  const int64_t blocks = (total + 255) / 256;
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  hipLaunchKernelGGL(embed_tokens_bf16_k, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), idx,
                     reinterpret_cast<const __bf16*>(table), reinterpret_cast<const __bf16*>(pos), reinterpret_cast<__bf16*>(out), T, N,
                     V, E / 8);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------------
// Rows of a narrow affine input layer: out[t, :] = x[t, 0..K) W^T + b, K <= 3 inputs per position
// (init_linear of the synthetic PSFNet, SyntheticExperiments/psf.py:153-154: Linear(2, 32) on [value, marker]).
// ------------------------------------------------------------------------------------------------------
// As a library GEMM the K = 2 product takes 80 us for 1 M positions; it is a 134 MB write. A thread computes four features of
// one position: x_0 w_e0, then fused adds of x_1 w_e1 and x_2 w_e2, then one rounded add of the bias — the arithmetic of the
// mixer kernels' AFFINE recipe (csrc/fwd_mlp_step.h: data_row8), so the two agree bit for bit.
namespace {

__global__ void __launch_bounds__(256)
affine_rows_k(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ out,
              int64_t T, int32_t K, int32_t E4) {
  // a thread keeps ONE group of four features (its weights and biases in registers) and walks the positions
  const int per = 256 / E4;  // positions per workgroup per pass (E4 <= 256: host-checked)
  const int tid = threadIdx.x, e4 = tid % E4, tl = tid / E4;
  if (tl >= per) return;
  float w0[4], w1[4], w2[4], bb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float* w = W + (int64_t)(4 * e4 + j) * K;
    w0[j] = w[0], w1[j] = K > 1 ? w[1] : 0.f, w2[j] = K > 2 ? w[2] : 0.f;
    bb[j] = bias ? bias[4 * e4 + j] : 0.f;
  }
  for (int64_t t = (int64_t)blockIdx.x * per + tl; t < T; t += (int64_t)gridDim.x * per) {
    const float x0 = x[t * K], x1 = K > 1 ? x[t * K + 1] : 0.f, x2 = K > 2 ? x[t * K + 2] : 0.f;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __fadd_rn(fmaf(x2, w2[j], fmaf(x1, w1[j], __fmul_rn(x0, w0[j]))), bb[j]);
    reinterpret_cast<float4*>(out)[t * E4 + e4] = make_float4(r[0], r[1], r[2], r[3]);
  }
}

}  // namespace

extern "C" int psf_affine_rows_f32(const float* x, const float* W, const float* bias, float* out, int64_t T, int32_t K, int32_t E,
                                   void* stream) {
  if (!x || !W || !out) return psf_internal_fail(PSF_E_NULL, "psf_affine_rows: x, W and out must be non-NULL");
  if (T < 0 || K < 1 || K > 3 || E < 4 || (E & 3) || E > 1024)
    return psf_internal_fail(PSF_E_SHAPE, "psf_affine_rows: need T >= 0, 1 <= K <= 3, E a multiple of 4 in 4..1024");
  if (reinterpret_cast<uintptr_t>(out) & 15) return psf_internal_fail(PSF_E_ALIGN, "psf_affine_rows: out must be 16-byte aligned");
  if (T == 0) return PSF_OK;
  const int per = 256 / (E / 4);
  const int64_t blocks = (T + per - 1) / per;
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  hipLaunchKernelGGL(affine_rows_k, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, W, bias, out, T, K, E / 4);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

// bf16 x, W, bias and out: a thread keeps EIGHT features (one 16-byte vector of the output). The same f32 chain on the widened
// operands (the products of bf16 values are exact in f32), the bias added in f32, one rounding to bf16 at the store.
namespace {

__global__ void __launch_bounds__(256)
affine_rows_bf16_k(const __bf16* __restrict__ x, const __bf16* __restrict__ W, const __bf16* __restrict__ bias, __bf16* __restrict__ out,
                   int64_t T, int32_t K, int32_t E8) {
  const int per = 256 / E8;  // positions per workgroup per pass (E8 <= 128: host-checked)
  const int tid = threadIdx.x, e8 = tid % E8, tl = tid / E8;
  if (tl >= per) return;
  float w0[8], w1[8], w2[8], bb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16* w = W + (int64_t)(8 * e8 + j) * K;
    w0[j] = (float)w[0], w1[j] = K > 1 ? (float)w[1] : 0.f, w2[j] = K > 2 ? (float)w[2] : 0.f;
    bb[j] = bias ? (float)bias[8 * e8 + j] : 0.f;
  }
  for (int64_t t = (int64_t)blockIdx.x * per + tl; t < T; t += (int64_t)gridDim.x * per) {
    const float x0 = (float)x[t * K], x1 = K > 1 ? (float)x[t * K + 1] : 0.f, x2 = K > 2 ? (float)x[t * K + 2] : 0.f;
    Bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (__bf16)__fadd_rn(fmaf(x2, w2[j], fmaf(x1, w1[j], __fmul_rn(x0, w0[j]))), bb[j]);
    reinterpret_cast<Bf16x8*>(out)[t * E8 + e8] = r;
  }
}

}  // namespace

extern "C" int psf_affine_rows_bf16(const uint16_t* x, const uint16_t* W, const uint16_t* bias, uint16_t* out, int64_t T, int32_t K,
                                    int32_t E, void* stream) {
  if (!x || !W || !out) return psf_internal_fail(PSF_E_NULL, "psf_affine_rows_bf16: x, W and out must be non-NULL");
  if (T < 0 || K < 1 || K > 3 || E < 8 || (E & 7) || E > 1024)
    return psf_internal_fail(PSF_E_SHAPE, "psf_affine_rows_bf16: need T >= 0, 1 <= K <= 3, E a multiple of 8 in 8..1024");
  if ((reinterpret_cast<uintptr_t>(out) & 15) || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(bias)) & 1))
    return psf_internal_fail(PSF_E_ALIGN, "psf_affine_rows_bf16: out must be 16-byte aligned, x, W and bias 2-byte aligned");
  if (T == 0) return PSF_OK;
  const int per = 256 / (E / 8);
  const int64_t blocks = (T + per - 1) / per;
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  hipLaunchKernelGGL(affine_rows_bf16_k, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const __bf16*>(x), reinterpret_cast<const __bf16*>(W), reinterpret_cast<const __bf16*>(bias),
                     reinterpret_cast<__bf16*>(out), T, K, E / 8);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------------
// Gradient of the table:  dTable[v, :] = sum over the tokens t with idx[t] == v of dOut[t, :]
// ------------------------------------------------------------------------------------------------------
// PyTorch's embedding_dense_backward sorts the indices and partitions them (rocprim) with sizes read back to the
// host: 0.1-0.26 ms per step on the LRA models, and not capturable in a HIP graph (a replay faulted in round 1,
// profiles/r01_graph_step_lab.log). Here ONE WAVE per (token slice, 64-column chunk) walks its tokens in order and
// accumulates into a private LDS table [V][64]: every table element has a single owner lane, so the sum over a
// slice is a fixed sequence of additions — no atomics, no sort, deterministic — and the slices are summed in a fixed
// order by a second kernel. Rows narrower than 64 floats put 64/E' tokens side by side in sub-tables (E' = E
// rounded up to a power of two), combined at the end.
namespace {

constexpr int kEmbSlicesMax = 2048;
constexpr int kEmbTokensPerSlice = 128;

// One body for both element types of dOut (float, __bf16): a bf16 gradient is widened at the load (exact), everything behind
// the load — the walk, the LDS tables, the slice rule, the f32 partial sums — is the same code.
template <typename TIn>
__device__ __forceinline__ void embed_bwd_partial_body(const int64_t* __restrict__ idx, const TIn* __restrict__ dOut, int64_t T,
                                                       int32_t V, int32_t E, int32_t ep_log2, int64_t tokens_per_slice,
                                                       float* __restrict__ part) {
  extern __shared__ float tab[];  // [subs][V][ep], subs * ep == 64
  const int lane = threadIdx.x;
  const int ep = 1 << ep_log2, subs = 64 >> ep_log2;
  const int sub = lane >> ep_log2, col = lane & (ep - 1);
  const int c = blockIdx.y * 64 + col;
  const bool active = c < E;
  for (int i = lane; i < V * 64; i += 64) tab[i] = 0.f;
  const int64_t t0 = (int64_t)blockIdx.x * tokens_per_slice;
  const int64_t t1 = t0 + tokens_per_slice < T ? t0 + tokens_per_slice : T;
  float* mine = tab + (size_t)sub * V * ep + col;
  constexpr int U = 8;  // tokens in flight per sub-table (one wave per workgroup: loads in flight hide the latency)
  for (int64_t t = t0 + sub; t < t1; t += (int64_t)U * subs) {
    int v[U];
    float g[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t tu = t + (int64_t)u * subs;
      const bool ok = tu < t1;
      int64_t vv = ok ? idx[tu] : 0;
      vv = vv < 0 ? 0 : (vv >= V ? V - 1 : vv);
      v[u] = (int)vv;
      g[u] = (ok && active) ? (float)dOut[tu * E + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) mine[v[u] * ep] += g[u];  // in token order; a single wave's LDS accesses stay ordered
    // (ds_add_f32 without return instead of this read-add-write — same order, same bits — is SLOWER: 32 -> 110 us at the
    //  Temporal-Order vocabulary of 6, where consecutive adds hit the same addresses; 35 -> 38 us at 225 rows)
  }
  // sub-tables -> one table, in sub order; this slice's partial result
  float* out = part + (size_t)blockIdx.x * V * E;
  for (int i = lane; i < V * ep; i += 64) {
    const int vrow = i >> ep_log2, cc = i & (ep - 1);
    float s = tab[vrow * ep + cc];
    for (int q = 1; q < subs; ++q) s += tab[((size_t)q * V + vrow) * ep + cc];
    const int cg = blockIdx.y * 64 + cc;
    if (cg < E) out[(size_t)vrow * E + cg] = s;
  }
}

__global__ void __launch_bounds__(64)
embed_bwd_partial_k(const int64_t* __restrict__ idx, const float* __restrict__ dOut, int64_t T, int32_t V, int32_t E,
                    int32_t ep_log2, int64_t tokens_per_slice, float* __restrict__ part) {
  embed_bwd_partial_body<float>(idx, dOut, T, V, E, ep_log2, tokens_per_slice, part);
}

__global__ void __launch_bounds__(64)
embed_bwd_partial_bf16_k(const int64_t* __restrict__ idx, const __bf16* __restrict__ dOut, int64_t T, int32_t V, int32_t E,
                         int32_t ep_log2, int64_t tokens_per_slice, float* __restrict__ part) {
  embed_bwd_partial_body<__bf16>(idx, dOut, T, V, E, ep_log2, tokens_per_slice, part);
}

// dTable[i] = sum over the slices of part[q][i]. A workgroup owns 32 consecutive elements; its 32 slice lanes each add
// every 32nd slice in ascending order, then the 32 sub-sums are added in lane order: a fixed association. (With one
// thread per element the 192 outputs of Temporal Order took 235 us for 1024 dependent loads each.) TOut = __bf16 rounds
// the f32 total once, at the store.
constexpr int kEmbRedLanes = 32;
template <typename TOut>
__device__ __forceinline__ void embed_bwd_reduce_body(const float* __restrict__ part, int32_t slices, int64_t n,
                                                      TOut* __restrict__ dTable) {
  __shared__ float sub[kEmbRedLanes][32];
  const int e = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t i = (int64_t)blockIdx.x * 32 + e;
  float s = 0.f;
  if (i < n)
    for (int q = sl; q < slices; q += kEmbRedLanes) s += part[(size_t)q * n + i];
  sub[sl][e] = s;
  __syncthreads();
  if (sl == 0 && i < n) {
    float tot = sub[0][e];
#pragma unroll
    for (int q = 1; q < kEmbRedLanes; ++q) tot += sub[q][e];
    dTable[i] = (TOut)tot;
  }
}

__global__ void __launch_bounds__(32 * kEmbRedLanes)
embed_bwd_reduce_k(const float* __restrict__ part, int32_t slices, int64_t n, float* __restrict__ dTable) {
  embed_bwd_reduce_body<float>(part, slices, n, dTable);
}

__global__ void __launch_bounds__(32 * kEmbRedLanes)
embed_bwd_reduce_bf16_k(const float* __restrict__ part, int32_t slices, int64_t n, __bf16* __restrict__ dTable) {
  embed_bwd_reduce_body<__bf16>(part, slices, n, dTable);
}

int emb_slices(int64_t T) {
  const int64_t s = (T + kEmbTokensPerSlice - 1) / kEmbTokensPerSlice;
  return (int)(s < 1 ? 1 : (s > kEmbSlicesMax ? kEmbSlicesMax : s));
}

}  // namespace

extern "C" int64_t psf_embed_tokens_bwd_workspace(int64_t T, int32_t V, int32_t E) {
  if (T < 1 || V < 1 || V > 512 || E < 1 || E > 4096) return -1;
  return (int64_t)emb_slices(T) * V * E * (int64_t)sizeof(float);
}

namespace {

// The host side of both entries: PK / RK are the partial and reduce kernels of the element types.
template <typename TIn, typename TOut, typename PK, typename RK>
int embed_bwd_launch(PK partial_k, RK reduce_k, const int64_t* idx, const TIn* dOut, int64_t T, int32_t V, int32_t E, TOut* dTable,
                     void* workspace, int64_t workspace_bytes, void* stream) {
  if (!idx || !dOut || !dTable || !workspace) return psf_internal_fail(PSF_E_NULL, "psf_embed_tokens_bwd: NULL argument");
  const int64_t need = psf_embed_tokens_bwd_workspace(T, V, E);
  if (need < 0) return psf_internal_fail(PSF_E_SHAPE, "psf_embed_tokens_bwd: need T >= 1, 1 <= V <= 512, 1 <= E <= 4096");
  if (workspace_bytes < need) return psf_internal_fail(PSF_E_SHAPE, "psf_embed_tokens_bwd: workspace smaller than psf_embed_tokens_bwd_workspace(T, V, E)");
  if constexpr (sizeof(TIn) == 2) {  // (the f32 entry checks what it always checked)
    if ((reinterpret_cast<uintptr_t>(dOut) | reinterpret_cast<uintptr_t>(dTable)) & 1)
      return psf_internal_fail(PSF_E_ALIGN, "psf_embed_tokens_bwd_bf16: dOut and dTable must be 2-byte aligned");
  }
  const int slices = emb_slices(T);
  const int64_t tps = (T + slices - 1) / slices;
  int ep_log2 = 6;  // columns per sub-table: E rounded up to a power of two, at most 64
  while (ep_log2 > 0 && (1 << (ep_log2 - 1)) >= E) --ep_log2;
  const int chunks = (E + 63) / 64;
  const size_t lds = (size_t)V * 64 * sizeof(float);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)partial_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return psf_internal_fail((int)e, hipGetErrorString(e));
  float* part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(partial_k, dim3(slices, chunks), dim3(64), lds, s, idx, dOut, T, V, E, ep_log2, tps, part);
  const int64_t n = (int64_t)V * E;
  hipLaunchKernelGGL(reduce_k, dim3((unsigned)((n + 31) / 32)), dim3(32 * kEmbRedLanes), 0, s, (const float*)part, slices, n, dTable);
  e = hipGetLastError();
  return e == hipSuccess ? PSF_OK : psf_internal_fail((int)e, hipGetErrorString(e));
}

}  // namespace

extern "C" int psf_embed_tokens_bwd_f32(const int64_t* idx, const float* dOut, int64_t T, int32_t V, int32_t E,
                                        float* dTable, void* workspace, int64_t workspace_bytes, void* stream) {
  return embed_bwd_launch(embed_bwd_partial_k, embed_bwd_reduce_k, idx, dOut, T, V, E, dTable, workspace, workspace_bytes, stream);
}

extern "C" int psf_embed_tokens_bwd_bf16(const int64_t* idx, const uint16_t* dOut, int64_t T, int32_t V, int32_t E,
                                         uint16_t* dTable, void* workspace, int64_t workspace_bytes, void* stream) {
  return embed_bwd_launch(embed_bwd_partial_bf16_k, embed_bwd_reduce_bf16_k, idx, reinterpret_cast<const __bf16*>(dOut), T, V, E,
                          reinterpret_cast<__bf16*>(dTable), workspace, workspace_bytes, stream);
}
