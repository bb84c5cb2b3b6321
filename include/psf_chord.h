/*
 * psf_chord.h — C ABI of libpsf_chord.so: PSF-Attn's chord-sparse batched matmul on MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE path of RuslanKhalitov/SparseFactorization: the call
 *
 *     V = spmm(chord_indicies, W.reshape(B, N*L), N, N, V)          (+ V = V + res_conn)
 *
 * that PSFNet.forward executes n_W times per forward
 *   (SyntheticExperiments/psf.py:172-188, LRA/psf.py:224-240, Genome_Clf/psf.py:214-230,
 *    attention_block.py:158-174, LRA/attention_maps/pathfinder_inference.py:66-81, imdb_inference.py:45-59),
 * and the reference's own optional native statement of the same operator and its gradients
 *   (spmul/spmul_cuda.cu:31-59 forward_host, :114-159 backward_host; spmul/spmul.py:12-31 SparseMultiply).
 *
 * Operator.  With link offsets off[0..L) (chord pattern: off[0]=0, off[k]=2^(k-1); taken mod N):
 *
 *   fwd : out[b,p,c] = sum_{k<L} W[b,p,k] * V[b,(p+off[k]) mod N, c]   (+ res[b,p,c])        spmul_cuda.cu:24
 *   dV  : dV [b,q,c] = sum_{k<L} W[b,(q-off[k]) mod N,k] * dZ[b,(q-off[k]) mod N, c]         spmul_cuda.cu:79-80
 *   dW  : dW [b,p,k] = sum_{c<C} dZ[b,p,c] * V[b,(p+off[k]) mod N, c]                        spmul_cuda.cu:105-108
 *
 * Sums run k (resp. c) ascending from 0 with a rounded product followed by a rounded add (no FMA
 * contraction), i.e. the order a CPU scatter_add over the reference's row-major (i,k) index list produces
 * (SyntheticExperiments/psf.py:7-32), so fp32 results are reproducible bit for bit against the oracle.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer to a contiguous row-major array; `offsets` and the step
 *     pointer tables are HOST pointers, read before the call returns;
 *   - the caller owns every buffer; the library allocates nothing on the device, keeps no pointer and
 *     holds no state besides a thread-local error string and process-wide tuning knobs;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*, NULL = default stream)
 *     of the calling thread's current device; no call synchronises;
 *   - outputs are fully overwritten (no pre-zero needed) and must not alias the gathered input
 *     (out != V, dV != dZ): rows are gathered from other rows of the same array;
 *   - return value: 0 = success; < 0 = invalid argument (PSF_E_*); > 0 = hipError_t of the failed HIP call.
 *     No C++ exception crosses this boundary. psf_last_error() describes the last failure on this thread.
 *
 * Threads.  Every entry point may be called from several host threads at once, on the same or on different streams
 * and devices: a call reads its arguments, takes ONE snapshot of the tuning knobs at entry (a psf_set_tuning from another
 * thread changes the next call, never the middle of one), enqueues its kernels and returns; the error string is
 * thread-local; nothing else is written. What the library does NOT do for the caller: order two calls that touch the same
 * buffers (that is the streams' job), or make psf_set_tuning atomic across several knobs (set them before starting the
 * worker threads). The first launch of a kernel instance that needs more than 48 KB of LDS raises that function's limit
 * (hipFuncSetAttribute, idempotent; two threads racing there both succeed).
 *
 * Streams.  Calls on different streams of one device may run at the same time and share compute units; no entry point
 * needs the device, a CU or a cache to itself, and no kernel's result depends on what runs beside it. This is tested, not
 * assumed: the forward chain at BASELINE configs[1]'s full size and the fused backward step are bit-identical to their solo
 * runs (and the chain to the CPU oracle) while the producer MLP kernels — MFMA phases, the one kind of neighbour the round-4
 * investigation ever suspected (profiles/r04b_mixer_lds_wait.md) — run on a second stream over the same CUs, and the other way
 * round (tests/test_gpu_coresidence.py). Two streams buy no time here (both kernel families are bound by the CUs' issue
 * slots and L2 ports: the two take the sum of their times, profiles/r05y_concurrent_streams_lab.log); the point is that
 * a caller who does it gets the same bits.
 *
 * Reference binding this replaces: pybind11 module `spmul_cuda` {forward_host, backward_host}
 * (spmul/spmul_cuda.cu:163-166) and the Python call torch_sparse.spmm (SyntheticExperiments/psf.py:5,178).
 * See INTEGRATION.md for the ctypes stub a maintainer of the reference would add.
 */
#ifndef PSF_CHORD_H
#define PSF_CHORD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSF_ABI_VERSION 2 /* 2 (round 5): the three "far" training entries are gone, psf_device_info is new, per-step mixer kernels take rows only.
                             The bf16 entry points (..._bf16) were added later without a version change: the change is additive.
                             So were psf_chord_chain_last_f32, psf_chord_chain_last_supported and psf_describe_chain_last. */

#define PSF_MAX_LINKS 64 /* L <= 64: N = 2^63 would need 64 links */

enum {
  PSF_OK = 0,
  PSF_E_NULL = -1,     /* a required pointer is NULL */
  PSF_E_SHAPE = -2,    /* B, N, L or C out of range */
  PSF_E_ALIAS = -3,    /* output aliases a gathered input */
  PSF_E_ALIGN = -4,    /* pointer not aligned to its element size */
  PSF_E_OFFSET = -5,   /* an explicit offset is not representable */
  PSF_E_TUNING = -6,   /* unknown tuning key / value */
  PSF_E_UNSUPPORTED = -7 /* this entry point has no kernel for the shape (psf_chord_chain_bwd_f32): not an error */
};

/* ABI version of the loaded library (== PSF_ABI_VERSION it was built with). */
int psf_version(void);

/* Human-readable description of the last failure on the calling thread ("" if none). Never NULL. */
const char* psf_last_error(void);

/* Build description: target arch, compiler, kernel variants compiled in. Never NULL. */
const char* psf_build_info(void);

/*
 * The calling thread's current HIP device, as the library sees it: "pci=<domain:bus:device.function> xcds=<n> cus=<n>
 * name=<marketing name>" into buf (NUL-terminated, truncated to len). One rank per GPU prints this into its benchmark line
 * so that a multi-GPU record shows N distinct devices (bench.py: "devices"). Touches the GPU (hipGetDevice).
 */
int psf_device_info(char* buf, int32_t len);

/*
 * Chord link offsets — the integer pattern of get_chord_indices_assym (SyntheticExperiments/psf.py:7-32):
 * offsets_out[0] = 0, offsets_out[k] = 2^(k-1) mod N for 1 <= k < L. Host-only, no GPU needed.
 */
int psf_chord_offsets(int64_t N, int32_t L, int64_t* offsets_out);

/*
 * The full COO index list of get_chord_indices_assym(n_vec=N, n_link=L): rows_out[i*L+k] = i,
 * cols_out[i*L+k] = (i + off[k]) mod N. Both arrays hold N*L entries. Host-only. Duplicate links
 * (off[k] == off[j] mod N) are kept, as in the reference.
 */
int psf_chord_indices(int64_t N, int32_t L, int64_t* rows_out, int64_t* cols_out);

/*
 * Forward step  out = W (.) V  [+ res].
 *   W   [B,N,L]   link weights (the reference's `value` reshaped, spmm arg 2 / `F` of spmul_cuda.cu:32)
 *   V   [B,N,C]   or [N,C] broadcast over the batch when v_batch_stride == 0 (the unbatched
 *                 eye(N) first operand of pathfinder_inference.py:57,75-81); otherwise
 *                 v_batch_stride must be N*C (elements)
 *   res [B,N,C]   or NULL; fused `V = V + res_conn` of SyntheticExperiments/psf.py:187-188
 *   out [B,N,C]
 *   offsets       host array of L link offsets (any int64, reduced mod N here), or NULL for the
 *                 chord pattern of psf_chord_offsets (what every PSFNet call site uses);
 *                 an explicit array is the `offsets` argument of spmul/spmul.py:8-9,15
 */
int psf_chord_spmm_fwd_f32(const float* W, const float* V, const float* res, float* out,
                           int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                           const int64_t* offsets, void* stream);
int psf_chord_spmm_fwd_f64(const double* W, const double* V, const double* res, double* out,
                           int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                           const int64_t* offsets, void* stream);

/*
 * bfloat16.  psf_chord_spmm_fwd_bf16, psf_chord_spmm_bwd_bf16, psf_chord_chain_fwd_bf16 and psf_sum_tensors_bf16 take the
 * arguments of their _f32 twins, in the same order, with the same validation. Every operand and result is bf16, passed as
 * raw bits (uint16_t: C99 has no bf16 type).
 *   Storage       W, V, res, out, dZ, dV, dW: bf16.
 *   Accumulation  each output element is accumulated in f32, in the order of the f32 kernels (links ascending for out and
 *                 dV, then the residual), and rounded to bf16 exactly once (round to nearest even; a NaN stays a NaN).
 *                 The product of two bf16 values is exact in f32 whenever it lies in f32's normal range, so the bf16
 *                 kernels fuse it into the add (one FMA gives the bits of a rounded product followed by a rounded sum);
 *                 the f32 and f64 kernels never contract. out and dV are therefore bf16_rne(f32 result of the upcast
 *                 inputs), bit for bit, as long as every nonzero product |W * V| (|W * dZ| for dV) lies in
 *                 [2^-126, FLT_MAX]. Outside that range the separately rounded product would overflow to infinity or
 *                 round to the subnormal grid while the fused form keeps it exact, and the result may differ from the
 *                 f32 reference. dW sums its channels in a per-lane order and is within one bf16 ulp of that.
 *   Alignment     pointers 2-byte aligned; the 16-byte vector kernels need C % 8 == 0 and 16-byte aligned row operands,
 *                 anything else runs the generic one-element-per-lane kernel.
 *   Kernels       forward step and dV: LDS-window kernels (rows of up to 128 channels per chunk), dW: LDS-window
 *                 kernel (rows of up to 128 channels), the generic kernels otherwise. A backward step that wants both
 *                 gradients runs ONE fused kernel (chord_bwd_fused_k<bf16>: dV and dW from one staging of the dZ rows)
 *                 for rows of 8, 16, 32, 64 or 128 channels when 4 <= L <= 20, N is a multiple of the tile (2048 / C rows)
 *                 and at least two tiles, the offsets are the chord pattern's near links with every far offset a multiple
 *                 of the tile, all five operands are 16-byte aligned, B*N*L % 8 == 0, a batch element's rows span less
 *                 than 2^31 bytes and the measured gate (knob "bwd_fused": 0 never, 1 automatic, 2 wherever it applies)
 *                 takes it; dV and dW are bit-identical to the two-kernel route. psf_describe_bwd names the route.
 *                 Forward chain: ONE launch with the
 *                 sequence's X slice resident in LDS as bf16 (chord_chain_lds_k<bf16> for N * cc <= 2112 with cc = 1 or 2
 *                 groups of 8 channels per workgroup; chord_chain_rows_k<bf16> with 16 channels per workgroup for
 *                 1057 <= N <= 2048 and with 8 for 2113 <= N <= 4160), bit-identical to the per-step launches, when
 *                 2 <= M <= 64, 2 <= L <= 20 (L <= 18 where three rows per thread are needed: 2048 < N * cc <= 2112),
 *                 C % 8 == 0, V0 and every out_steps[m] 16-byte aligned, every W_steps[m] 2-byte aligned for odd L and
 *                 4-byte aligned for even L, and the measured gate (knobs "chain_fused", "chain_cc") takes it;
 *                 otherwise M per-step launches. psf_describe_chain_fwd_dtype names the route.
 *                 Backward chain: psf_chord_chain_bwd_bf16 issues the per-step launches and the one residual sum inside
 *                 the library; psf_chord_chain_bwd_lds_bf16 is the whole chain in ONE launch for N <= 1024, C = 8 or 16,
 *                 bit-identical to it (both below).
 *                 Producer MLPs, forward (inference): psf_mlp_fwd_bf16 (below, next to psf_mlp_fwd_f32).
 *                 Mixer of a short sequence in one launch (inference): psf_mixer_fwd_bf16 (below, next to psf_mixer_fwd_f32).
 * Not covered: float16, mixed dtypes, the bf16 mixer with W computed inside per-step kernels (long sequences) or from an
 *                 input recipe, the bf16 flat-head entry, the bf16 producer backward, and
 *                 an edge instance of the bf16 fused backward step (ragged N, other far offsets, W / dW off their 16-byte
 *                 boundary: those steps run the dW and dV window kernels).
 */
int psf_chord_spmm_fwd_bf16(const uint16_t* W, const uint16_t* V, const uint16_t* res, uint16_t* out,
                            int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                            const int64_t* offsets, void* stream);

/*
 * Backward step (spmul_cuda.cu:114-159 backward_host). Either output may be NULL to skip it.
 *   dZ [B,N,C]  gradient w.r.t. the step's output (also the gradient w.r.t. `res`, which is the identity)
 *   W  [B,N,L]  needed for dV;   V [B,N,C] or [N,C] (v_batch_stride == 0) needed for dW
 *   dW [B,N,L]
 *   dV [B,N,C]  always per batch element; when V was broadcast the caller sums dV over b
 * What f32 dW is (dV is the oracle's bits, links ascending): each element is an f32 sum of the C products dZ[b,p,c] *
 * V[b,(p+off_k) mod N,c], every product and every addition rounded to nearest, in an order that belongs to the kernel
 * (channels split over lanes and chunks, combined by a tree) and so may differ between kernels, knobs "bwd_variant",
 * "bwd_fused", "dw_variant" and "dw_tgs", and from the oracle's left-to-right sum. Therefore
 *     |dW - exact| <= gamma_C * sum_c |dZ * V|,   gamma_C = C u / (1 - C u),  u = 2^-24,
 * per element; dW is exact, bit for bit on every route, whenever every partial sum of the row dot is representable
 * (integer data below 2^24, say); links that reduce to the same offset mod N give the same bits; the launch-shape knobs
 * ("fwd_split", "bwd_fronts", "bwd_fused_wg_limit") change no bit. It is not bit-identical to the oracle.
 * tests/test_gpu_dw_f32_exact.py holds every dW kernel to this.
 */
int psf_chord_spmm_bwd_f32(const float* dZ, const float* W, const float* V, float* dW, float* dV,
                           int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                           const int64_t* offsets, void* stream);
int psf_chord_spmm_bwd_f64(const double* dZ, const double* W, const double* V, double* dW, double* dV,
                           int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                           const int64_t* offsets, void* stream);
int psf_chord_spmm_bwd_bf16(const uint16_t* dZ, const uint16_t* W, const uint16_t* V, uint16_t* dW, uint16_t* dV,
                            int64_t B, int64_t N, int32_t L, int64_t C, int64_t v_batch_stride,
                            const int64_t* offsets, void* stream);

/*
 * Whole forward chain of PSFNet.forward's hot loop (SyntheticExperiments/psf.py:172-188):
 *     X_0 = V0;   X_{m+1} = W_m (.) X_m  [+ V0 if use_residual]      m = 0 .. M-1
 *   W_steps   host table of M device pointers, W_steps[m] -> [B,N,L]
 *   out_steps host table of M device pointers, out_steps[m] -> [B,N,C] receives X_{m+1}.
 *             Training keeps all M (they are the saved inputs of the backward steps); inference may
 *             alternate two buffers. out_steps[m] must differ from the step's input
 *             (V0 for m = 0, out_steps[m-1] after) and, with use_residual, from V0.
 *   V0 [B,N,C] or [N,C] with v0_batch_stride == 0 (then use_residual must be 0)
 * Launches M dependent kernels on `stream` — or, for short sequences, a single kernel that keeps each
 * sequence's X in LDS across all M steps (a step buffer that a later step overwrites, as in two-buffer
 * inference, is then not written at all). The result is out_steps[M-1].
 */
int psf_chord_chain_fwd_f32(const float* const* W_steps, const float* V0, float* const* out_steps,
                            int32_t M, int32_t use_residual,
                            int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride,
                            const int64_t* offsets, void* stream);
int psf_chord_chain_fwd_f64(const double* const* W_steps, const double* V0, double* const* out_steps,
                            int32_t M, int32_t use_residual,
                            int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride,
                            const int64_t* offsets, void* stream);
int psf_chord_chain_fwd_bf16(const uint16_t* const* W_steps, const uint16_t* V0, uint16_t* const* out_steps,
                             int32_t M, int32_t use_residual,
                             int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride,
                             const int64_t* offsets, void* stream);

/*
 * The same chain when only its LAST result is wanted, for long f32 sequences, in exactly ONE launch: out [B,N,C] receives
 * X_M and no other X_m reaches memory (csrc/fwd_chain_regs.h: a workgroup owns one sequence and one channel pair, X lives in
 * registers, W is streamed through LDS). The bits are those of psf_chord_chain_fwd_f32's out_steps[M-1].
 *   Covers N = 16384, L = 15, C a multiple of 4, 1 <= M <= 64, the chord offsets (offsets NULL or equal to them), every
 *   W_steps[m], V0 and out 16-byte aligned, and a V0 that is not broadcast when it is also the residual. Anything else returns
 *   PSF_E_UNSUPPORTED (not an error, nothing launched): the caller runs psf_chord_chain_fwd_f32. There is no fallback here.
 *   Errors, before that: M < 1 (PSF_E_SHAPE), a NULL pointer (PSF_E_NULL), the dimensions' limits (PSF_E_SHAPE), out == V0 or
 *   out == W_steps[m] (PSF_E_ALIAS), a pointer off its element size (PSF_E_ALIGN).
 * psf_chord_chain_last_supported answers 1 where a caller should PREFER this entry: the shape is covered (w_align: the
 * alignment in bytes that every W_steps[m], V0 and out is known to have; default_offsets: 1 for the chord pattern) and knob
 * "chain_fused" is 2, or 1 with a grid that fills its rounds: a workgroup takes a whole CU, so B * C / 2 workgroups run in
 * ceil(workgroups / CUs) rounds of one workgroup's time, and the one launch wins only where the workgroups are at least
 * 95 % of rounds * CUs, up to the four rounds measured (csrc/fwd_chain_regs_launch.h: chain_regs_automatic; the CU count is
 * the current device's, 256 where no device answers). Just above a multiple of the CU count it answers 0. The entry itself
 * runs wherever it fits.
 */
int psf_chord_chain_last_f32(const float* const* W_steps, const float* V0, float* out, int32_t M, int32_t use_residual,
                             int64_t B, int64_t N, int32_t L, int64_t C, int64_t v0_batch_stride,
                             const int64_t* offsets, void* stream);
int psf_chord_chain_last_supported(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t w_align,
                                   int32_t use_residual, int64_t v0_batch_stride, int32_t default_offsets);

/*
 * Whole backward chain of the same loop in one call (SyntheticExperiments/psf.py:172-188 differentiated;
 * spmul/spmul_cuda.cu:75-84,102-111 per step):
 *   - ONE launch for short sequences of narrow rows (N <= 1024, C = 4 or 8, 2 <= L <= 20, M <= 64: the synthetic tasks up to
 *     N = 1024); psf_chord_chain_bwd_supported says whether the shape is covered (1 / 0); dX_steps may be NULL then;
 *   - otherwise the M per-step launches of psf_chord_spmm_bwd_f32 and one psf_sum_tensors_f32 pass, issued by the library
 *     (no trip through the caller's FFI per step): needs dX_steps, a host table of M device buffers [B,N,C] that receive
 *     the gradient after each step (dX_steps[m] = gradient of X_m; dX_steps[0] is unused without the residual);
 *   - PSF_E_UNSUPPORTED (not an error) when neither applies — dX_steps NULL for an uncovered shape, a residual chain of more
 *     than 31 steps or B*N*C not a multiple of 4, knob "chain_bwd_fused" = 0 — and the caller runs the steps itself.
 *   dOut [B,N,C]  gradient of the chain's result X_M
 *   W_steps[m] -> W_m [B,N,L];   X_steps[m] -> X_m [B,N,C], the forward's input of step m: X_steps[0] is ignored (V0 is
 *   used), X_steps[m] = psf_chord_chain_fwd_f32's out_steps[m-1];   dW_steps[m] -> dW_m [B,N,L] (written)
 *   dV0 [B,N,C] (written): gradient of V0 through the chain and, with use_residual, through every step's "+ V0" as well,
 *   summed in the per-step path's order ((g_M + g_{M-1}) + ... + g_1) + g_0.
 * The one launch's dV0 and dW are bit-identical to the CPU oracle (products and sums rounded separately, links / channels
 * ascending); the per-step path's are those of psf_chord_spmm_bwd_f32.
 */
int psf_chord_chain_bwd_supported(int64_t N, int32_t L, int64_t C, int32_t M);
int psf_chord_chain_bwd_f32(const float* dOut, const float* const* W_steps, const float* V0, const float* const* X_steps,
                            float* const* dW_steps, float* dV0, float* const* dX_steps, int32_t M, int32_t use_residual,
                            int64_t B, int64_t N, int32_t L, int64_t C, const int64_t* offsets, void* stream);
/*
 * The same for bf16 (raw bits), arguments and validation as above. There is no one-launch kernel behind it and
 * psf_chord_chain_bwd_supported is not consulted: it always issues the M per-step launches of psf_chord_spmm_bwd_bf16 (the
 * fused step where that applies), handing the gradient from dX_steps[m] to the next step, and one psf_sum_tensors_bf16 pass
 * for the residual — ((g_M + g_{M-1}) + ... + g_1) + g_0 summed in f32 and rounded once. Every dW_m and dV0 is bit-identical
 * to M calls of psf_chord_spmm_bwd_bf16 followed by that sum. PSF_E_UNSUPPORTED (the caller runs the steps itself): dX_steps
 * NULL, a residual chain with M + 1 > 32 or B*N*C % 8 != 0, knob "chain_bwd_fused" = 0.
 */
int psf_chord_chain_bwd_bf16(const uint16_t* dOut, const uint16_t* const* W_steps, const uint16_t* V0,
                             const uint16_t* const* X_steps, uint16_t* const* dW_steps, uint16_t* dV0,
                             uint16_t* const* dX_steps, int32_t M, int32_t use_residual,
                             int64_t B, int64_t N, int32_t L, int64_t C, const int64_t* offsets, void* stream);
/*
 * The bf16 backward chain of a short sequence in exactly ONE kernel launch (chord_chain_bwd_lds_k<bf16>,
 * csrc/bwd_chain_lds_bf16.h): one workgroup per sequence, the running gradient, X_m and W_m in LDS, dW_m written per step,
 * dV0 once at the end; no g_m reaches memory, so there is no dX_steps argument and no scratch gradient buffer. The entry does
 * not allocate and does not synchronise.
 *   Covered: 1 <= N <= 1024, C = 8 or 16, 2 <= L <= 20, 1 <= M <= 64, B <= 2^31 - 1, any offsets (NULL = the chord pattern).
 *   psf_chord_chain_bwd_lds_bf16_supported answers 1 / 0 for a shape (0 as well under knob "chain_bwd_fused" = 0).
 *   Arguments and validation as psf_chord_chain_bwd_bf16: X_steps[0] is ignored (V0 is used), NULL and alias checks, B == 0
 *   returns PSF_OK. PSF_E_UNSUPPORTED — never a per-step fallback — for a shape that is not covered or under knob
 *   "chain_bwd_fused" = 0: the caller uses psf_chord_chain_bwd_bf16 then.
 *   Alignment: dOut, dV0 and every X_m 16 bytes (PSF_E_ALIGN otherwise); W_m and dW_m ANY 2-byte alignment — they are read
 *   and written element by element, nothing outside [W_m, W_m + B*N*L) is read, nothing outside [dW_m, dW_m + B*N*L) or
 *   [dV0, dV0 + B*N*C) is written.
 *   Arithmetic: the bits of psf_chord_chain_bwd_bf16 at 16-byte-aligned operands. g_m: f32 accumulator from +0, links
 *   ascending, one fused multiply-add per term (the bf16 product is exact in f32), rounded to bf16 once (nearest even, NaN
 *   kept), and that rounded value enters the next step. dW_m[p,k]: per 8-channel group a running fused multiply-add over the
 *   channels ascending from +0; C = 8 rounds that partial, C = 16 rounds the f32 sum of the two partials. Residual:
 *   dV0 = ((g_M + g_{M-1}) + ... + g_1) + g_0 over the rounded g_m, summed left to right in f32, rounded once; without it
 *   dV0 = g_0.
 */
int psf_chord_chain_bwd_lds_bf16_supported(int64_t N, int32_t L, int64_t C, int32_t M);
int psf_chord_chain_bwd_lds_bf16(const uint16_t* dOut, const uint16_t* const* W_steps, const uint16_t* V0,
                                 const uint16_t* const* X_steps, uint16_t* const* dW_steps, uint16_t* dV0,
                                 int32_t M, int32_t use_residual, int64_t B, int64_t N, int32_t L, int64_t C,
                                 const int64_t* offsets, void* stream);

/*
 * The TRANSPOSED chain: selected rows of the attention map A_b = W_{M-1} ... W_0 (W_final of the LRA/attention_maps scripts) without the
 * dense [B,N,N] map.
 *     Y_M = Q;   Y_m = W_m^T (.) Y_{m+1}   for m = M-1 .. 0;   out = Y_0
 *     Y_m[b,q,c] = sum_k W_m[b,(q-off_k) mod N,k] * Y_{m+1}[b,(q-off_k) mod N,c]
 * A column c of Q that is one-hot at row r comes back as out[b,:,c] = A_b[r,:]. (A COLUMN of A_b is the forward chain on a
 * one-hot V0: psf_chord_chain_fwd_*.) Each step is the dV half of psf_chord_spmm_bwd_* (spmul/spmul_cuda.cu:75-84).
 *   W_steps    host table of M device pointers, W_steps[m] -> W_m [B,N,L]; f32 4-byte, bf16 2-byte aligned
 *   Q, out, scratch  [B,N,R], 16-byte aligned, pairwise distinct; R a multiple of 4 (f32) or 8 (bf16). Q is never written.
 *   offsets    as everywhere: NULL = the chord pattern; explicit and negative offsets are reduced mod N
 * Routes. psf_chord_chain_tr_supported(N, L, R, M, elem_bytes) answers 1 where the entry runs ONE launch
 * (chord_chain_tr_lds_k, csrc/chain_tr_lds.h): 1 <= N <= 1024, 2 <= L <= 20, 1 <= M <= 64, R as above, elem_bytes 4 or 2. One
 * thread owns a row, Y and W_m stay in LDS, a workgroup holds up to four 16-byte column groups and a sequence with more
 * columns spreads over ceil(R / 16) (f32; bf16: ceil(R / 32)) workgroups; `scratch` is not touched and may be NULL. (The
 * query has no B: a batch whose B * workgroups per sequence exceeds the grid limit of 2^31 - 1 takes the per-step route too.) Elsewhere
 * (0) the library issues the M per-step dV launches of psf_chord_spmm_bwd_* itself, taking turns between `scratch` and `out`
 * so that the last one writes `out`; `scratch` may be NULL for M = 1, otherwise a NULL `scratch` returns PSF_E_UNSUPPORTED (not
 * an error, as a NULL dX_steps of psf_chord_chain_bwd_f32). No knob selects between the two.
 * Arithmetic, on either route: the bits of M calls of psf_chord_spmm_bwd_{f32,bf16} with dW = NULL, W_{M-1} first, each
 * result fed to the next. f32: links ascending from +0, product and sum rounded separately (the CPU oracle's dV). bf16: f32
 * accumulator, one fused multiply-add per link, one rounding to bf16 per step; the rounded value enters the next step.
 * Validation, before any launch: M < 1, a bad B / N / L / R (PSF_E_SHAPE); NULL W_steps, Q or out (PSF_E_NULL); the NULL
 * scratch above (PSF_E_UNSUPPORTED); B == 0 returns PSF_OK; then a NULL W_steps[m] (PSF_E_NULL), Q, out, scratch not
 * distinct (PSF_E_ALIAS), alignment (PSF_E_ALIGN). No allocation, no synchronisation: the entries can be captured in a HIP
 * graph ("Streams" above). Added without a version change.
 */
int psf_chord_chain_tr_supported(int64_t N, int32_t L, int64_t R, int32_t M, int32_t elem_bytes);
int psf_chord_chain_tr_f32(const float* const* W_steps, const float* Q, float* out, float* scratch, int32_t M,
                           int64_t B, int64_t N, int32_t L, int64_t R, const int64_t* offsets, void* stream);
int psf_chord_chain_tr_bf16(const uint16_t* const* W_steps, const uint16_t* Q, uint16_t* out, uint16_t* scratch, int32_t M,
                            int64_t B, int64_t N, int32_t L, int64_t R, const int64_t* offsets, void* stream);

/*
 * (Rounds 2-4 also exported training variants that kept a link-major side copy of W's far columns for the dV kernel —
 * "..._chain_fwd_far_f32", "..._spmm_bwd_far_f32", "..._bwd_far_first_link". A wash end to end
 * (profiles/r02n_far_copy.log, r03aj_farcopy_in_step_ab.log), off by default since round 2, removed in round 5.)
 */

/*
 * Producer side: weight / bias gradient of the token-wise Linear layers of MLPBlock
 * (SyntheticExperiments/psf.py:35-60) that produce W_m = fs[m](data) and V = g(data) — a reduction over
 * T = B*N tokens into an n x m tile, done on the f32 matrix core (exact f32) with a fixed-order reduction:
 *     dWt[j,i] = sum_t dY[t,j] * X[t,i]     (nn.Linear.weight.grad layout, [n = out_features, m = in_features])
 *     db[j]    = sum_t dY[t,j]              (db may be NULL)
 *   X [T,m], dY [T,n] contiguous; 1 <= m, n <= 128. `workspace` is caller-owned device scratch of at least
 *   psf_linear_wgrad_workspace(T, m, n) bytes (that function returns -1 for unsupported sizes).
 */
int64_t psf_linear_wgrad_workspace(int64_t T, int32_t m, int32_t n);
int psf_linear_wgrad_f32(const float* X, const float* dY, int64_t T, int32_t m, int32_t n, float* dWt, float* db,
                         void* workspace, int64_t workspace_bytes, void* stream);
/* Same with row strides (in floats; ldx >= m, ldy >= n): X and dY may be column slices of wider row-major arrays,
 * e.g. one MLP's hidden block inside the stacked hidden layer of all MLPs. */
int psf_linear_wgrad_strided_f32(const float* X, int64_t ldx, const float* dY, int64_t ldy, int64_t T, int32_t m, int32_t n,
                                 float* dWt, float* db, void* workspace, int64_t workspace_bytes, void* stream);
/*
 * The same gradients for a layer whose operands are bf16 (raw bits), on the bf16 matrix core (csrc/linear_wgrad_bf16.hip):
 *     dWt[j*m + i] = rne_bf16(sum_t dY[t*ldy + j] * X[t*ldx + i])     db[j] = rne_bf16(sum_t dY[t*ldy + j])   (db may be NULL)
 *   T >= 1, 1 <= m, n <= 128, ldx >= m, ldy >= n (row strides in elements: column slices of wider arrays are taken as they
 *   are). Arithmetic contract: the operands are bf16; every product is exact in f32; all accumulation is in f32; each output
 *   element is rounded to bf16 ONCE, to nearest even, at the store; there are no float atomics and the partial sums are
 *   combined in a fixed order, so two calls on the same operands give the same bits, eagerly and from a replayed graph. The
 *   summation order is this kernel's own (16 tokens per matrix instruction, one slab of rows per wave, slabs combined in a
 *   fixed tree): it is NOT the order of psf_linear_wgrad_f32, and the two entries' f32 sums may differ in their last bits.
 *   No load leaves [X, X + (T-1) ldx + m) or [dY, dY + (T-1) ldy + n).
 *   Alignment: with g(ld) the largest power of two <= 8 that divides ld (the elements one vector load takes), X must be
 *   aligned to 2 g(ldx) bytes and dY to 2 g(ldy) bytes — 16 bytes for a row stride that is a multiple of 8, 2 bytes for an odd
 *   one; dWt and db to 2 bytes, workspace to 4: PSF_E_ALIGN otherwise, before any launch. NULL X, dY, dWt or workspace:
 *   PSF_E_NULL; sizes or strides out of range, or fewer than psf_linear_wgrad_bf16_workspace(T, m, n) workspace bytes (-1
 *   for unsupported sizes): PSF_E_SHAPE — the f32 entry's codes.
 */
int64_t psf_linear_wgrad_bf16_workspace(int64_t T, int32_t m, int32_t n);
int psf_linear_wgrad_bf16(const uint16_t* X, int64_t ldx, const uint16_t* dY, int64_t ldy, int64_t T, int32_t m, int32_t n,
                          uint16_t* dWt, uint16_t* db, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * out[i] = ((srcs[0][i] + srcs[1][i]) + srcs[2][i]) + ...   i < n, in that order (separately rounded additions).
 * The gradient of the chain's residual: dV_0 = dX_0 + sum over the steps of dX_m (V = V + res_conn,
 * SyntheticExperiments/psf.py:187-188, reaches V_0 from every step), summed once instead of accumulated per step.
 *   1 <= count <= 32; n a multiple of 4; every pointer 16-byte aligned; `out` may alias none of the sources.
 */
int psf_sum_tensors_f32(const float* const* srcs, int32_t count, int64_t n, float* out, void* stream);
/* bf16 terms, summed left to right in f32 and rounded to bf16 once; n a multiple of 8, other limits as above. */
int psf_sum_tensors_bf16(const uint16_t* const* srcs, int32_t count, int64_t n, uint16_t* out, void* stream);

/*
 * One Adam step over `count` tensors (the optimizer of the reference's training loop, optim.Adam(net.parameters(), lr),
 * SyntheticExperiments/psf_training.py:50-53; no weight decay, no amsgrad):
 *     m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   host tables of `count` device pointers (params, grads, exp_avg, exp_avg_sq) and element counts; every pointer 4-byte
 *   aligned (16-byte alignment and counts that are multiples of 4 take the vector path). `step` = t >= 1 from the host,
 *   or, when `step_dev` is non-NULL, t is read from that device float (a captured step must see it advance). 4096
 *   elements per workgroup: the two 524 288-element tensors of a PSFNet at N = 16384 spread over 256 workgroups.
 *   One launch takes up to 40 tensors, so a longer list is several launches. The call is validated in full before the
 *   first launch: on an error nothing is updated. PSF_E_SHAPE: count < 0, or step_dev NULL and not step >= 1 (NaN
 *   included), or more than 2^31 - 1 workgroups in one launch; PSF_E_NULL: a NULL table, a NULL tensor pointer or a negative
 *   element count at any index; PSF_E_ALIGN: a tensor pointer that is not 4-byte aligned. count = 0 returns PSF_OK before
 *   anything else is looked at; tensors of 0 elements are skipped.
 */
int psf_adam_step_f32(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      const int64_t* numels, int32_t count, float lr, float beta1, float beta2, float eps, float step,
                      const float* step_dev, void* stream);
/*
 * The same step for bf16 parameters with f32 master weights (the name carries no element-type suffix: the entry takes both).
 * Per element, with g the bf16 gradient widened to f32 (exact):
 *     (master, exp_avg, exp_avg_sq) <- the update above on (master, g, exp_avg, exp_avg_sq), in f32 — the f32 kernel's
 *     arithmetic, one template body;   params_bf16 <- master rounded to nearest even (NaN stays NaN)
 *   so the bf16 parameter is always the rounded master and never feeds back into the update: at lr = 1e-3 a step moves a
 *   weight near 1 by a quarter of half a bf16 ulp, which an Adam on the bf16 parameter alone rounds away every time.
 *   host tables of `count` device pointers: master, exp_avg, exp_avg_sq f32 (4-byte aligned), params_bf16 and grads_bf16
 *   bf16 as raw bits (2-byte aligned); PSF_E_ALIGN otherwise. The vector path takes a tensor whose f32 arrays are 16-byte
 *   and whose bf16 arrays are 8-byte aligned with a count that is a multiple of 4; any other tensor takes the scalar path.
 *   `step` / `step_dev`, the 4096-element chunks, the 40 tensors per launch, the validation in full before the first
 *   launch and every return code are those of the f32 entry above.
 */
int psf_adam_step_master(float* const* master, uint16_t* const* params_bf16, const uint16_t* const* grads_bf16,
                         float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numels, int32_t count, float lr,
                         float beta1, float beta2, float eps, float step, const float* step_dev, void* stream);

/*
 * Token embedding fused with the positional-embedding add — the first two lines of PSFNet.forward
 * (SyntheticExperiments/psf.py:152-163, LRA/psf.py:203-214):
 *     out[t,:] = table[idx[t],:] (+ pos[t mod N,:])        t < T = B*N
 *   idx [T] int64 token ids (ids outside [0,V) are clamped: never an out-of-bounds read), table [V,E],
 *   pos [N,E] or NULL, out [T,E]; E a multiple of 4; table, pos, out 16-byte aligned. One pass over the output.
 */
int psf_embed_tokens_f32(const int64_t* idx, const float* table, const float* pos, float* out, int64_t T, int64_t N,
                         int32_t V, int32_t E, void* stream);
/*
 * The same pass on bf16 (raw bits): table [V,E], pos [N,E] or NULL, out [T,E] bf16.
 *     out[t,:] = rne_bf16(f32(table[idx[t],:]) + f32(pos[t mod N,:]))
 *   — the bits of the stock `embedding(idx) + pos.unsqueeze(0)` on bf16 tensors. A 16-byte vector holds 8 channels: E a
 *   positive multiple of 8 (PSF_E_SHAPE); table, pos, out 16-byte aligned (PSF_E_ALIGN). Ids are clamped as above.
 */
int psf_embed_tokens_bf16(const int64_t* idx, const uint16_t* table, const uint16_t* pos, uint16_t* out, int64_t T, int64_t N,
                          int32_t V, int32_t E, void* stream);
/*
 * Rows of a narrow affine input layer — `init_linear` of the synthetic PSFNet (SyntheticExperiments/psf.py:153-154:
 * Linear(2, embedding_size) on [value, marker]):
 *     out[t,:] = x[t,0..K) W^T + bias          t < T
 *   x [T,K] with 1 <= K <= 3, W [E,K], bias [E] or NULL, out [T,E] 16-byte aligned, E a multiple of 4, at most 1024. One pass over the
 *   output (the K = 2 product is a 134 MB write at 1 M positions, not a GEMM). Arithmetic: x_0 w_e0, fused adds of x_1 w_e1
 *   and x_2 w_e2, one rounded add of the bias — the same as the mixer entry's PSF_MIXER_IN_AFFINE recipe, bit for bit.
 */
int psf_affine_rows_f32(const float* x, const float* W, const float* bias, float* out, int64_t T, int32_t K, int32_t E,
                        void* stream);
/*
 * The same rows on bf16 (raw bits): x [T,K], W [E,K], bias [E] or NULL, out [T,E] bf16, 1 <= K <= 3, E a multiple of 8 in
 * 8..1024 (PSF_E_SHAPE), out 16-byte aligned, x, W and bias 2-byte aligned (PSF_E_ALIGN). Per element: the f32 chain
 * x_0 w_e0, fused adds of x_1 w_e1 and x_2 w_e2 (the products of bf16 values are exact in f32), the bias added in f32, and one
 * rounding to bf16, to nearest even.
 */
int psf_affine_rows_bf16(const uint16_t* x, const uint16_t* W, const uint16_t* bias, uint16_t* out, int64_t T, int32_t K,
                         int32_t E, void* stream);
/*
 * Its gradient with respect to the table:  dTable[v,:] = sum over {t : idx[t] == v} of dOut[t,:]   (fully written;
 * the caller zeroes a padding row). No sort, no atomics, no host read-back: deterministic (a fixed order of
 * additions) and capturable in a HIP graph, unlike the sort-and-partition backward of nn.Embedding.
 *   1 <= V <= 512, 1 <= E <= 4096; `workspace`: at least psf_embed_tokens_bwd_workspace(T, V, E) bytes (-1 for
 *   unsupported sizes).
 */
int64_t psf_embed_tokens_bwd_workspace(int64_t T, int32_t V, int32_t E);
int psf_embed_tokens_bwd_f32(const int64_t* idx, const float* dOut, int64_t T, int32_t V, int32_t E, float* dTable,
                             void* workspace, int64_t workspace_bytes, void* stream);
/*
 * bf16 dOut [T,E] and bf16 dTable [V,E] (raw bits, 2-byte aligned: PSF_E_ALIGN otherwise). dOut is widened at the load, the
 * partial sums and the workspace (the same psf_embed_tokens_bwd_workspace bytes) stay f32, and the total is rounded to
 * nearest even once at the store — the same kernels instantiated for the element type, so
 *     dTable == rne_bf16(what psf_embed_tokens_bwd_f32 returns for the widened dOut),   bit for bit.
 * Same limits, deterministic, no atomics, no host read-back, capturable.
 */
int psf_embed_tokens_bwd_bf16(const int64_t* idx, const uint16_t* dOut, int64_t T, int32_t V, int32_t E, uint16_t* dTable,
                              void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The FLATTEN head of PSFNet, `final = nn.Linear(n_vec * n_channels_V, n_class)` on V.view(B, -1)
 * (SyntheticExperiments/psf.py:129-134,189-190):  out[b,j] = bias[j] + sum_i X[b,i] * W[j,i]
 *   X [B,K] (K = N*C, a multiple of 4), W [J,K] (nn.Linear.weight), bias [J] or NULL, out [B,J]; 1 <= J <= 8;
 *   X and W 16-byte aligned. `workspace`: at least psf_flat_head_workspace(B, K, J) bytes (-1 for unsupported
 *   sizes). One read of X; per-chunk partial sums are added in a fixed order: bit-reproducible run to run FOR A GIVEN
 *   (B, K). The chunk length (4096 floats, or 1024 when 4096 would leave fewer than 1024 workgroups) depends on B and K, so
 *   the logits of one sample differ in their last bits between batch sizes that fall on different sides of that rule
 *   (evaluation at another batch size than training agrees to ~1e-6 relative, not to the bit).
 */
int64_t psf_flat_head_workspace(int32_t B, int64_t K, int32_t J);
/*
 * Its backward (what autograd computes for that nn.Linear):  dW[j,i] = sum_b dY[b,j] * X[b,i],  dX[b,i] = sum_j dY[b,j] * W[j,i]
 *   dY [B,J] contiguous; dX [B,K] and / or dW [J,K] (NULL = not wanted; dW needs X, dX needs W); 1 <= B <= 1024,
 *   1 <= J <= 16 (the first layer of CIFAR-10's non-linear head has 16), K a positive multiple of 4; X, W, dX, dW 16-byte aligned. One read of X, sums over b in ascending order
 *   (bit-reproducible). The bias gradient (the column sums of dY) is left to the caller.
 */
int psf_flat_head_bwd_f32(const float* dY, const float* X, const float* W, float* dX, float* dW, int32_t B, int64_t K, int32_t J,
                          void* stream);
int psf_flat_head_f32(const float* X, const float* W, const float* bias, float* out, int32_t B, int64_t K, int32_t J,
                      void* workspace, int64_t workspace_bytes, void* stream);
/*
 * The head and its backward on bf16 (raw bits): X, W, bias, out, dY, dX, dW are bf16 arrays of the shapes above. The contract
 * is the one of psf_embed_tokens_bwd_bf16: operands are widened at the load (exact), everything in between is the f32 kernel's
 * arithmetic in the f32 kernel's order — the same kernels instantiated for the element type: a thread owns the same four
 * consecutive K elements (one 8-byte load), the same chunk rule, the same f32 partial sums in the same workspace
 * (psf_flat_head_workspace bytes, unchanged), the same fixed-order combines, the bias widened and added in f32; the backward
 * keeps dY widened in LDS, sums dW in f32 over b ascending and dX as the f32 FMA chain over j ascending — and each result
 * element is rounded to bf16 once, at the store (a plain cast: round to nearest even, a NaN stays a NaN). The product of two
 * bf16 values is exact in f32, so bit for bit
 *     out == rne_bf16(what psf_flat_head_f32     returns for the widened X, W, bias)
 *     dX  == rne_bf16(what psf_flat_head_bwd_f32 returns for the widened dY, X, W)
 *     dW  == rne_bf16(what psf_flat_head_bwd_f32 returns for the widened dY, X, W)
 * Limits as in f32: forward 1 <= J <= 8; backward 1 <= J <= 16 and 1 <= B <= 1024; K a positive multiple of 4. X, W, dX, dW
 * 8-byte aligned (PSF_E_ALIGN otherwise); NULL and shape errors as the f32 entries report them; everything is validated before
 * the first HIP call. The bias gradient stays with the caller. No atomics, no host read-back: deterministic and capturable.
 */
int psf_flat_head_bf16(const uint16_t* X, const uint16_t* W, const uint16_t* bias, uint16_t* out, int32_t B, int64_t K, int32_t J,
                       void* workspace, int64_t workspace_bytes, void* stream);
int psf_flat_head_bwd_bf16(const uint16_t* dY, const uint16_t* X, const uint16_t* W, uint16_t* dX, uint16_t* dW, int32_t B, int64_t K,
                           int32_t J, void* stream);

/*
 * Producer side, forward (inference): K two-layer token-wise MLPs sharing one input, fused in one launch —
 * g and fs[0..M) of PSFNet (MLPBlock = Linear, GELU, Linear; SyntheticExperiments/psf.py:35-60,110-126,165,175):
 *     Y[k][t,:] = GELU(X[t,:] * A[k]^T + a[k]) * B[k]^T + b[k]          (erf GELU as torch.nn.GELU(); erf is
 *                                                                          evaluated to 1.5e-7 absolute)
 *   X [T,E]; A[k] [h[k],E], a[k] [h[k]], B[k] [O[k],h[k]], b[k] [O[k]] (nn.Linear layouts); Y[k] [T,O[k]].
 *   A, a, B, b, Y, h, O are HOST tables of K entries (device pointers / sizes).
 *   Limits: E a multiple of 4, 4 <= E <= 64; 1 <= h[k] <= 128; 1 <= O[k] <= 32; 1 <= K <= 32; X 16-byte aligned.
 *   `workspace`: caller-owned, 16-byte-aligned device scratch of at least psf_mlp_fwd_workspace(E, K, h, O)
 *   bytes (the packed weight images; that function returns -1 for unsupported sizes).
 * X is read once, the hidden activations never reach memory; f32 throughout (f32 matrix core).
 */
int64_t psf_mlp_fwd_workspace(int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int psf_mlp_fwd_f32(const float* X, int64_t T, int32_t E, int32_t K, const float* const* A, const float* const* a,
                    const float* const* B, const float* const* b, const int32_t* h, const int32_t* O,
                    float* const* Y, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The same for a bf16 model (raw bits), in one launch plus the packing of the weights: table conventions, validation order
 * and error codes as psf_mlp_fwd_f32. Added without a version change (PSF_ABI_VERSION: the bf16 entries are additive).
 * Arithmetic, for k < K — every operand and result is bf16, exactly the three roundings of nn.Linear -> nn.GELU() ->
 * nn.Linear on bf16 tensors:
 *     z[t,j]    = bf16_rne( f32( sum_e X[t,e] * A[k][j,e] + a[k][j] ) )
 *     h[t,j]    = bf16_rne( GELU_f32( z[t,j] ) )                       erf GELU; Phi is evaluated to 7.5e-8 absolute
 *     Y[k][t,o] = bf16_rne( f32( sum_j h[t,j] * B[k][o,j] + b[k][o] ) )
 *   Products of bf16 values are exact in f32; the sums are accumulated in f32 on the matrix pipe (one
 *   v_mfma_f32_32x32x16_bf16 term per product) in an unspecified order. The result therefore differs from the layer-by-layer
 *   evaluation only where an f32 sum lands on a bf16 rounding tie. A NaN stays a NaN; a token's outputs depend on that
 *   token's row of X only. The hidden layer never reaches memory: X is read once, each Y[k] is written once.
 *   Limits: E a multiple of 8, 8 <= E <= 64; 1 <= h[k] <= 128; 1 <= O[k] <= 32; 1 <= K <= 32; T >= 1; X and every Y[k]
 *   16-byte aligned (PSF_E_ALIGN), weights and biases 2-byte aligned. Nothing outside Y[k][0 .. T*O[k]) is written, for odd
 *   O[k] and ragged T too. `workspace`: caller-owned, 16-byte-aligned device scratch of at least
 *   psf_mlp_fwd_bf16_workspace(E, K, h, O) bytes (6912 per 32 hidden rows of each MLP; -1: unsupported sizes). No allocation,
 *   no synchronisation; capturable in a HIP graph. Wider layers (E >= 128, O = 128: the LRA networks) are not covered; the
 *   backward is psf_mlp_bwd_bf16 (E <= 32).
 */
int64_t psf_mlp_fwd_bf16_workspace(int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int psf_mlp_fwd_bf16(const uint16_t* X, int64_t T, int32_t E, int32_t K, const uint16_t* const* A, const uint16_t* const* a,
                     const uint16_t* const* B, const uint16_t* const* b, const int32_t* h, const int32_t* O,
                     uint16_t* const* Y, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * The mixer with W produced INSIDE the chain step: V_M from `data` without any W_m in memory.
 * What PSFNet.forward does between the embedding and the head (SyntheticExperiments/psf.py:165-188, LRA/psf.py:214-240,
 * Genome_Clf/psf.py:204-230, attention_block.py:148-174; dropout2 between g and the loop must be inactive):
 *     V0 = g(X);   for m < M:  W_m = fs[m](X);  X_{m+1} = W_m (.) X_m [+ V0]            (X_0 = V0)
 * Each step is ONE kernel that computes its tile's rows of W_m on chip — `data` rows straight into matrix-core operand
 * order, the two layers of fs[m] on the bf16 matrix pipe at f32 accuracy (psf_mlp_fwd_f32's arithmetic), the W tile in LDS
 * — and then gathers and accumulates as psf_chord_spmm_fwd_f32 does (same order, uncontracted multiply and add). The
 * producer's W writes (4 M L bytes per token) and the chain's W reads never happen; a step reads the data row (4 E bytes)
 * instead of the W row (4 L bytes).
 *   X [B,N,E]; MLP 0 is g (E -> h[0] -> C), MLPs 1..M are fs[0..M) (E -> h[k] -> L): A, a, Bw, b, h are HOST tables of
 *   M + 1 entries laid out as for psf_mlp_fwd_f32 (nn.Linear layouts).
 *   V0 [B,N,C] receives g(X) (it is also the residual); out_steps as psf_chord_chain_fwd_f32 (may alternate two buffers);
 *   the result is out_steps[M-1]. Chord offsets only.
 *   Limits: E a multiple of 4, 4 <= E <= 32; 1 <= h[k] <= 128; C a multiple of 4, 4 <= C <= 32; 4 <= L <= 20; 1 <= M <= 31;
 *   N at least two tiles (tile = 256, 256, 128, 64 rows for C <= 4, 8, 16, 32); X, V0 and out_steps 16-byte aligned.
 *   Short sequences (N a multiple of 32, N * C / 4 <= 1024, C = 4 or 8 — BASELINE configs[0], Adding N = 128, among them) run
 *   as ONE launch in which V also stays on chip: a workgroup owns a sequence, keeps its data rows in registers and its V in
 *   LDS through all M steps (csrc/mixer_lds.h; knob "mixer_lds"); a step buffer that a later step overwrites is then not
 *   stored at all, as in psf_chord_chain_fwd_f32.
 *   psf_mixer_fwd_workspace returns the bytes of 16-byte-aligned device scratch needed (packed weight images), or -1 when
 *   the fused path does not cover the shape — the caller then uses psf_mlp_fwd_f32 + psf_chord_chain_fwd_f32.
 */
int64_t psf_mixer_fwd_workspace(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L);
/* Which form a call with this shape takes: 0 = none (outside the limits), 1 = M + 1 step launches, 2 = the single LDS-resident launch. */
int32_t psf_mixer_fwd_plan(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L);
int psf_mixer_fwd_f32(const float* X, int64_t B, int64_t N, int32_t E, int32_t M, const float* const* A,
                      const float* const* a, const float* const* Bw, const float* const* b, const int32_t* h, int64_t C,
                      int32_t L, int32_t use_residual, float* V0, float* const* out_steps, void* workspace,
                      int64_t workspace_bytes, void* stream);

/*
 * The mixer of a SHORT sequence for a bf16 model (raw bits), in one launch plus the packing of the weights
 * (csrc/mixer_lds_bf16.h): a workgroup owns a sequence, keeps its data rows in registers and its V in LDS as bf16 through
 * all M steps, computes V0 = g(X) and every W_m = fs[m](X) on chip, and rounds each W_m to bf16 before the step reads it.
 * THE RESULT IS THE BITS OF psf_mlp_fwd_bf16 FOLLOWED BY psf_chord_chain_fwd_bf16 on the same operands — V0 and every stored
 * step, NaN and Inf included: the two kernels' arithmetic (three roundings per MLP; f32 accumulator, links ascending with
 * the exact product fused, the residual added in f32, one rounding per step) is reused, not restated. What goes away is
 * the M + 1 producer outputs in memory (2 M L bytes per token written and read back) and two of the three launches.
 *   Tables as psf_mixer_fwd_f32: M + 1 entries, MLP 0 = g (E -> h[0] -> C), MLPs 1..M = fs[0..M) (E -> h[k] -> L); X [B,N,E].
 *   V0 [B,N,C] receives g(X) and may be NULL (nothing is written then); out_steps as psf_chord_chain_fwd_bf16: M pointers
 *   that may alternate two buffers, a buffer that a later step overwrites is not stored at all; the result is
 *   out_steps[M-1]. Chord offsets only. There is no recipe input and no per-step form for longer sequences.
 *   Limits: N a multiple of 32, 32 <= N <= 512; C = 8 or 16; E a multiple of 8, 8 <= E <= 64; 1 <= h[k] <= 128;
 *   4 <= L <= 20; 1 <= M <= 31; 0 <= B < 2^31; X, V0 and every out_steps[m] 16-byte aligned, weights and biases 2-byte aligned.
 *   psf_mixer_fwd_bf16_plan: 2 = the single launch runs, 0 = not covered (outside the limits, or knob "mixer_lds" = 0).
 *   psf_mixer_fwd_bf16_workspace: bytes of 16-byte-aligned device scratch (6912 per 32 hidden rows of each MLP), or -1
 *   outside the limits.
 *   Validation, before any HIP call and in this order: NULL tables (PSF_E_NULL); B (PSF_E_SHAPE); a shape that
 *   psf_mixer_fwd_bf16_plan answers 0 for, the knob included: PSF_E_UNSUPPORTED (not an error: the caller runs the two
 *   entries above); X, V0 alignment (PSF_E_ALIGN); workspace too small or misaligned (PSF_E_SHAPE); per MLP NULL / 2-byte
 *   alignment; per step NULL, 16-byte alignment, out == V0 or out == the step's input (PSF_E_ALIAS). B == 0 then returns 0.
 *   No allocation, no synchronisation; capturable in a HIP graph. Added without a version change (additive).
 */
int32_t psf_mixer_fwd_bf16_plan(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L);
int64_t psf_mixer_fwd_bf16_workspace(int64_t N, int32_t E, int32_t M, const int32_t* h, int64_t C, int32_t L);
int psf_mixer_fwd_bf16(const uint16_t* X, int64_t B, int64_t N, int32_t E, int32_t M, const uint16_t* const* A,
                       const uint16_t* const* a, const uint16_t* const* Bw, const uint16_t* const* b, const int32_t* h, int64_t C,
                       int32_t L, int32_t use_residual, uint16_t* V0, uint16_t* const* out_steps, void* workspace,
                       int64_t workspace_bytes, void* stream);

/*
 * The same with `data` itself never in memory: X is replaced by the recipe PSFNet.forward computes it by, and every kernel
 * of the mixer evaluates the rows it needs from that recipe (a step then reads 8 bytes per position instead of 4 E).
 *   PSF_MIXER_IN_DATA    src = float X [B,N,E]                                        (psf_mixer_fwd_f32)
 *   PSF_MIXER_IN_AFFINE  src = float in [B,N,K], K <= 3;  X = in * weight^T + bias  (+ pos[p])
 *                        weight [E,K], bias [E] or NULL — `init_linear` of the Adding network,
 *                        SyntheticExperiments/psf.py:136-141,153-154; the K products are summed first, then the bias
 *   PSF_MIXER_IN_TOKENS  src = int64 tokens [B,N] in [0, K);  X = weight[token] (+ pos[p])
 *                        weight = the embedding table [K,E], pos [N,E] or NULL — psf.py:151-152,157-162, LRA/psf.py:204-209,
 *                        attention_block.py:150-152; one rounded add, as psf_embed_tokens_f32. Tokens are device data and
 *                        cannot be range-checked by the host: an index outside [0, K) is CLAMPED into the table (row 0
 *                        or row K-1, as psf_embed_tokens_f32 does) — never a read outside it; nn.Embedding would raise.
 *   weight and pos 16-byte aligned, src aligned to its element type. Everything else as psf_mixer_fwd_f32.
 */
enum { PSF_MIXER_IN_DATA = 0, PSF_MIXER_IN_AFFINE = 1, PSF_MIXER_IN_TOKENS = 2 };
typedef struct psf_mixer_input {
  int32_t kind; /* PSF_MIXER_IN_* */
  int32_t K;    /* AFFINE: inputs per position (1..3); TOKENS: vocabulary size; DATA: ignored */
  const void* src;
  const float* weight;
  const float* bias;
  const float* pos;
} psf_mixer_input;
int psf_mixer_fwd_in_f32(const psf_mixer_input* in, int64_t B, int64_t N, int32_t E, int32_t M, const float* const* A,
                         const float* const* a, const float* const* Bw, const float* const* b, const int32_t* h, int64_t C,
                         int32_t L, int32_t use_residual, float* V0, float* const* out_steps, void* workspace,
                         int64_t workspace_bytes, void* stream);

/*
 * Producer side, backward (training) of the same K MLPs, fused in one pass over the tokens. What autograd does
 * for MLPBlock (SyntheticExperiments/psf.py:35-60) with 4K GEMMs, K GELU-backward kernels and K-1 accumulations
 * of the input gradient:
 *     Hpre  = X * A[k]^T + a[k]            (recomputed; nothing of size [T, h] is saved by the forward)
 *     dHpre = (dY[k] * B[k]) .* GELU'(Hpre)
 *     dA[k] = dHpre^T * X,  da[k] = sum_t dHpre,  dB[k] = dY[k]^T * GELU(Hpre),  db[k] = sum_t dY[k]
 *     dX    = sum_k dHpre_k * A[k]                                               (dX may be NULL: not computed)
 *   Layouts as psf_mlp_fwd_f32; dY[k] [T,O[k]]; dA/da/dB/db[k] have the nn.Linear parameter shapes and are fully
 *   overwritten. Limits: E a multiple of 4, 4 <= E <= 32; 1 <= h[k] <= 128; 1 <= O[k] <= 32; 1 <= K <= 32; X and
 *   dX 16-byte aligned. `workspace`: at least psf_mlp_bwd_workspace(T, E, K, h, O) bytes, 16-byte aligned (packed
 *   weights + per-wave partial sums; -1 for unsupported sizes).
 * Weight gradients are reduced in a fixed order (no float atomics): results are bit-reproducible run to run.
 */
int64_t psf_mlp_bwd_workspace(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int psf_mlp_bwd_f32(const float* X, int64_t T, int32_t E, int32_t K, const float* const* A, const float* const* a,
                    const float* const* B, const int32_t* h, const int32_t* O, const float* const* dY, float* dX,
                    float* const* dA, float* const* da, float* const* dB, float* const* db, void* workspace,
                    int64_t workspace_bytes, void* stream);

/*
 * The same backward for a bf16 model (raw bits), csrc/mlp_bwd_bf16.hip: table conventions, validation order and error codes as
 * psf_mlp_bwd_f32 and psf_mlp_fwd_bf16. Added without a version change (additive). The forward is psf_mlp_fwd_bf16, which
 * saves nothing: the hidden layer is recomputed here with the forward's bits.
 * Arithmetic — the sequence of roundings that PyTorch's bf16 autograd produces for nn.Linear -> nn.GELU() -> nn.Linear with
 * the first layers stacked: one rounding per tensor it materialises, f32 accumulation inside each GEMM and each sum. For
 * each MLP k, with z and hh exactly as in psf_mlp_fwd_bf16's contract (z = bf16_rne(f32(X A^T + a)), hh = bf16_rne(GELU_f32(z))):
 *     g[t,j]  = bf16_rne( f32( sum_o dY[t,o] * B[o,j] ) )
 *     d[t,j]  = bf16_rne( f32(g[t,j]) * GELU'_f32(z[t,j]) )      GELU' = Phi + z phi, Phi evaluated to 7.5e-8 absolute
 *     dA[j,e] = bf16_rne( f32( sum_t d[t,j] * X[t,e] ) )          da[j] = bf16_rne( f32( sum_t d[t,j] ) )
 *     dB[o,j] = bf16_rne( f32( sum_t dY[t,o] * hh[t,j] ) )        db[o] = bf16_rne( f32( sum_t dY[t,o] ) )
 *     dX[t,e] = bf16_rne( f32( sum_k sum_j d_k[t,j] * A_k[j,e] ) )       ONE rounding over all K MLPs
 *   Products of bf16 values are exact in f32; the sums are in f32, in an order that is unspecified but fixed: weight gradients
 *   are reduced in a fixed order without float atomics, so two calls on the same inputs give the same bits. A NaN stays a NaN.
 *   dX[t,:] depends on token t's rows of X and dY only. Every gradient tensor is fully overwritten; nothing outside the
 *   gradient tensors and the workspace is written; nothing at or beyond X + T*E or dY[k] + T*O[k] is read, for odd O[k] and
 *   ragged T too. dX may be NULL (not computed).
 *   Limits: E a multiple of 8, 8 <= E <= 32; 1 <= h[k] <= 128; 1 <= O[k] <= 32; 1 <= K <= 32; T >= 1; X, dX and every dY[k]
 *   16-byte aligned (PSF_E_ALIGN), weights, biases and their gradients 2-byte aligned. `workspace`: caller-owned,
 *   16-byte-aligned device scratch of at least psf_mlp_bwd_bf16_workspace(T, E, K, h, O) bytes (packed weight images, one f32
 *   partial-sum slot per workgroup, the reduction's stage; -1: unsupported sizes).
 *   Validation, before any HIP call and in this order: NULL tables (PSF_E_NULL); shape (PSF_E_SHAPE); X, dX, dY[k] alignment
 *   (PSF_E_ALIGN); workspace too small or misaligned (PSF_E_SHAPE); per MLP NULL / 2-byte alignment.
 *   No allocation, no synchronisation; capturable in a HIP graph.
 */
int64_t psf_mlp_bwd_bf16_workspace(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int psf_mlp_bwd_bf16(const uint16_t* X, int64_t T, int32_t E, int32_t K, const uint16_t* const* A, const uint16_t* const* a,
                     const uint16_t* const* B, const int32_t* h, const int32_t* O, const uint16_t* const* dY, uint16_t* dX,
                     uint16_t* const* dA, uint16_t* const* da, uint16_t* const* dB, uint16_t* const* db, void* workspace,
                     int64_t workspace_bytes, void* stream);

/*
 * Producer side at the WIDE (LRA) sizes — the same K MLPs for E up to 1024 and outputs up to 128: reference ListOps
 * E = 512, h = 128, outputs 12 (x 11 link MLPs) and 128 (LRA/psf_training_config.py:2-30; MLPBlock LRA/psf.py:35-60, call
 * sites LRA/psf.py:214,227). The K first layers run as ONE stacked GEMM on the bf16 matrix pipe at f32 accuracy (every
 * f32 operand split exactly into three bf16 terms, six product terms), forward, input gradient and weight gradient
 * alike; the second layers, GELU and its derivative are fused around them.
 *   psf_mlp_wide_fwd_f32  Y[k] as psf_mlp_fwd_f32. It also fills `saved` (caller-owned, 256-byte aligned, at least
 *                         psf_mlp_wide_saved_bytes bytes): X as bf16 term planes and the pre-activations of the hidden
 *                         layers — what the backward needs, so that nothing is recomputed (at these widths recomputing
 *                         is a fourth 100-GFLOP GEMM; keeping is 4 x sum(h) bytes per token). Inference passes saved =
 *                         NULL and a workspace of psf_mlp_wide_fwd_workspace + psf_mlp_wide_saved_bytes bytes.
 *   psf_mlp_wide_bwd_f32  the gradients of psf_mlp_bwd_f32 from `saved` and dY[k]; dX may be NULL (not computed).
 *   Layouts as psf_mlp_fwd_f32 / psf_mlp_bwd_f32. Limits: E a multiple of 16, 16 <= E <= 1024; 1 <= h[k] <= 128;
 *   1 <= O[k] <= 128; 1 <= K <= 24; T_pad * E and T_pad * (sum of h[k], each rounded up to 32) below 2^30, T_pad being T
 *   rounded up to 256; X and the forward's A[k] 16-byte aligned, every other array 4-byte aligned (any float pointer).
 *   Workspaces: caller-owned, 256-byte aligned, at least psf_mlp_wide_{fwd,bwd}_workspace bytes (-1: unsupported sizes).
 * Every reduction has a fixed order (no float atomics): results are bit-reproducible run to run.
 */
int64_t psf_mlp_wide_saved_bytes(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int64_t psf_mlp_wide_fwd_workspace(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int64_t psf_mlp_wide_bwd_workspace(int64_t T, int32_t E, int32_t K, const int32_t* h, const int32_t* O);
int psf_mlp_wide_fwd_f32(const float* X, int64_t T, int32_t E, int32_t K, const float* const* A, const float* const* a,
                         const float* const* B, const float* const* b, const int32_t* h, const int32_t* O,
                         float* const* Y, void* saved, int64_t saved_bytes, void* workspace, int64_t workspace_bytes,
                         void* stream);
int psf_mlp_wide_bwd_f32(const void* saved, int64_t saved_bytes, int64_t T, int32_t E, int32_t K,
                         const float* const* A, const float* const* B, const int32_t* h, const int32_t* O,
                         const float* const* dY, float* dX, float* const* dA, float* const* da, float* const* dB,
                         float* const* db, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * A plain streaming kernel with the forward step's byte mix, for measuring what the memory system of a box gives that
 * mix (bench.py's second denominator; no reference counterpart). Per 16-byte output vector i it reads w[2i], w[2i+1], v[i]
 * and r[i] and writes out[i]: W : V : residual : out = 2 : 1 : 1 : 1 (the step kernel at L = 15, C = 8 moves 15 : 8 : 8 : 8).
 *   w [2 n_vec4] float4, v / r / out [n_vec4] float4, all 16-byte aligned; bytes moved = 80 n_vec4.
 */
int psf_stream_mix_f32(const float* w, const float* v, const float* r, float* out, int64_t n_vec4, void* stream);
/*
 * The same for the BACKWARD step's byte mix: per index i it reads w[2i], w[2i+1], v[i], z[i] and writes dw[2i], dw[2i+1],
 * dv[i] — W : V : dZ read, dW : dV written = 2 : 1 : 1, 2 : 1 (the fused backward step at L = 15, C = 8 moves 15 : 8 : 8,
 * 15 : 8). Bytes moved = 112 n_vec4.
 */
int psf_stream_mix_bwd_f32(const float* w, const float* v, const float* z, float* dw, float* dv, int64_t n_vec4,
                           void* stream);

/*
 * Process-wide tuning knobs (benchmark / test use; the defaults are the shipped configuration). psf_chord_tuning.h, beside
 * this header, is the catalogue: every key with its range, its default and what it selects. psf_set_tuning returns PSF_OK, or
 * PSF_E_TUNING for a key that is not in the catalogue or a value outside the key's range; psf_get_tuning returns the value
 * (>= 0) or PSF_E_TUNING.
 * A knob picks the kernel or launch shape that computes a result; out, dV and the chain results are summed in the same
 * order on every route (f32: the CPU oracle's bits). What a caller can observe besides time:
 *   "fwd_variant", "dw_variant", "mlp_variant": a value that forces one kernel makes the call return PSF_E_TUNING where that
 *                      kernel does not apply. "mlp_variant" also moves psf_mlp_fwd_f32 between the f32-MFMA and the
 *                      split-bf16 arithmetic: equal to f32 accuracy, not bit for bit.
 *   "bwd_variant", "bwd_fused", "dw_variant", "dw_tgs": f32 dW is specified to 1e-5 relative, not to the bit (its sum over
 *                      a row's channels is a tree whose shape belongs to the kernel), so moving a backward step to another
 *                      dW kernel may change dW's last bits; bf16 dW is the same bits on the fused and the two-kernel route.
 *   "chain_fused"    : in the one launch a step buffer that a later step overwrites is not written at all
 *                      (psf_chord_chain_fwd_f32 above); 0 keeps the per-step launches, which write every step.
 *   "chain_bwd_fused": 0 makes psf_chord_chain_bwd_f32 / _bf16 return PSF_E_UNSUPPORTED and
 *                      psf_chord_chain_bwd_supported return 0: the caller runs the steps itself.
 *   "mixer_lds"      : 0 takes the single-launch mixer away: psf_mixer_fwd_bf16_plan answers 0 and psf_mixer_fwd_bf16 returns
 *                      PSF_E_UNSUPPORTED; psf_mixer_fwd_plan answers 1 (or 0) instead of 2, an input
 *                      recipe (psf_mixer_fwd_in_f32 with another kind than PSF_MIXER_IN_DATA) returns PSF_E_SHAPE, and a
 *                      shape that only the single launch covers returns PSF_E_TUNING.
 * Every other key ("wide_fuse" among them: same arithmetic in the same order) changes time only.
 * Change notes: the keys "mixer_ablate" and "bwd_ablate" (timing labs, ignored by every product build) are gone and answer
 * PSF_E_TUNING like any unknown key; the labs are kept as patches (profiles/bwd_fused_ablate_lab.patch,
 * profiles/mixer_ablate_lab.patch). No entry point changed: PSF_ABI_VERSION stays 2.
 */
int psf_set_tuning(const char* key, int32_t value);
int psf_get_tuning(const char* key);

/*
 * Name of the kernel variant the dispatcher would run for this forward shape (for profiles and bench
 * logs; e.g. "chord_fwd_win<f32,L=15,C=8>"). elem_bytes: 2 (bf16), 4 (f32) or 8 (f64). Writes a NUL-terminated string of at
 * most cap-1 chars.
 */
int psf_describe_fwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t elem_bytes,
                     char* buf, int32_t cap);
/* The same for a whole f32 forward chain of M steps: names the single-launch LDS-resident kernel when the chain takes it. */
int psf_describe_chain_fwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, char* buf, int32_t cap);
/* The same with the element size: 4 gives psf_describe_chain_fwd's string, 2 the bf16 chain's (chord_chain_lds_k<bf16,...> /
 * chord_chain_rows_k<bf16,...> when an inference chain of aligned operands takes the one launch, else what
 * psf_describe_fwd(..., 2, ...) says for its steps); any other size is PSF_E_SHAPE. Added without a version change. */
int psf_describe_chain_fwd_dtype(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, int32_t elem_bytes, char* buf,
                                 int32_t cap);
/* The backward twin of psf_describe_fwd: the kernel(s) a backward step that wants both dW and dV would run on 16-byte aligned
 * operands with a full-batch V and the chord offsets, under the current knobs — "chord_bwd_fused_k<bf16,L=15,TG=1,NT=256>
 * TR=256 near=10 far=5 fronts=2" for the fused step, "<dW kernel> + <dV kernel>" for the two-kernel routes (window, chunk or
 * generic kernels). elem_bytes: 2 (bf16), 4 (f32) or 8 (f64). Added without a version change. */
int psf_describe_bwd(int64_t B, int64_t N, int32_t L, int64_t C, int32_t elem_bytes, char* buf, int32_t cap);
/* What psf_chord_chain_last_f32 does with a chain of 16-byte aligned operands, a full-batch V0 and the chord offsets:
 * "chord_chain_regs_k<f32,L=15,T=512,J=32> one launch for all 14 steps, ..., automatic" (or "on request only": the entry runs
 * it, psf_chord_chain_last_supported answers 0), or "declined (PSF_E_UNSUPPORTED): ..." for a shape it does not cover. */
int psf_describe_chain_last(int64_t B, int64_t N, int32_t L, int64_t C, int32_t M, char* buf, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PSF_CHORD_H */
