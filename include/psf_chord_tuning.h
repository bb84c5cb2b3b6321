/*
 * psf_chord_tuning.h — the catalogue of libpsf_chord.so's tuning knobs: every key psf_set_tuning / psf_get_tuning
 * (psf_chord.h) know, with its legal range and its default.
 *
 *     PSF_TUNING_KNOBS(X)  expands to  X(key, lo, hi, default)  once per key (key is a bare token: stringify it)
 *
 * The library builds its own table from this list, so the list IS what the library accepts: a value outside [lo, hi] and a
 * key that is not here answer PSF_E_TUNING. The defaults are the shipped configuration. Knobs are for benchmarks, tests and
 * experiments: with the few exceptions that psf_chord.h names beside psf_set_tuning, a knob changes which kernel or launch
 * shape computes a result and how long that takes, never the result. "auto" is the rule the dispatcher
 * (csrc/psf_chord.hip) applies; the measurements behind each rule are written there, beside the rule.
 *
 * The list has two parts only because the library keeps the last two knobs elsewhere (the producer-MLP entry points read
 * them, not the chord dispatcher); a consumer expands PSF_TUNING_KNOBS.
 */
#ifndef PSF_CHORD_TUNING_H
#define PSF_CHORD_TUNING_H

#define PSF_TUNING_KNOBS_CHORD(X)                                                                                       \
  /* Forward step: 0 = auto (the LDS-window kernel where it applies, else the generic direct-gather kernel), 1 = generic  \
   * kernel, 2 = window kernel, or PSF_E_TUNING from the call where it does not apply. */                                \
  X(fwd_variant, 0, 2, 0)                                                                                               \
  /* Backward step: 0 = auto (the fused step or the LDS-window dV / dW kernels where they apply), 1 = generic kernels. */ \
  X(bwd_variant, 0, 1, 0)                                                                                               \
  /* Workgroup order of the tiled kernels: 1 = a batch element's tiles (a one-launch chain's workgroups of one sequence) \
   * stay on one XCD, 0 = linear. "chain_zigzag" reverses that walk and needs 1. */                                     \
  X(xcd_remap, 0, 1, 1)                                                                                                 \
  /* Window kernels (forward, dV, dW, the mixer's step kernel) on shapes with a ragged last tile per sequence: 1 = by    \
   * size: one launch of the predicated (edge) instance up to 300 MB of algorithmic bytes, as 2 above that; 2 = full     \
   * tiles on the predicate-free instance and the ragged tiles in a second launch; 0 = every tile on the edge instance,  \
   * ragged or not. */                                                                                                  \
  X(fwd_split, 0, 2, 1)                                                                                                 \
  /* f32 rows of >= 64 channels: 0 = auto: the forward step takes 32-channel chunks on 1024-thread workgroups (256-row   \
   * tiles) for rows of 64..256 channels and N <= 4096 when those tiles divide N or the whole-row tiles do not either,   \
   * and one workgroup per whole row otherwise; dV one workgroup per whole row; 1 = the 1024-thread chunks wherever they \
   * fit (forward and dV); 2 = 32-channel chunks on 256-thread workgroups (forward and dV); 3, 4 = one workgroup per     \
   * whole row always. */                                                                                               \
  X(fwd_wide, 0, 4, 0)                                                                                                  \
  /* f32 dW when the fused step does not run: 0 = auto (the chunk-looping kernel for rows of >= 32 channels whose        \
   * 4-channel groups are a multiple of 8, else the whole-row window kernel), 1 = whole-row window kernel, 2 =          \
   * chunk-looping kernel, or PSF_E_TUNING from the call where it does not apply. */                                     \
  X(dw_variant, 0, 2, 0)                                                                                                \
  /* f32 dV window kernel: 0 = auto (512 threads x 1 row for rows of <= 8 channels, else 256 threads x 2 rows), 1 = 256  \
   * threads x 2 rows always. */                                                                                        \
  X(dv_threads, 0, 1, 0)                                                                                                \
  /* A backward step that wants both dW and dV: 1 = ONE fused kernel where the measured gate takes it (f32: wherever it  \
   * applies — rows of 4, 8, 16, 32 or 64 channels, 128 up to N = 4096, at least two tiles: the aligned instance, or for \
   * any N, far offsets and W / dW alignment the general one; bf16: the aligned instance on the shapes measured faster); \
   * 2 = the aligned instance wherever it applies, else the two kernels; 0 = always the two kernels. */                  \
  X(bwd_fused, 0, 2, 1)                                                                                                 \
  /* Fused backward step (aligned instance), workgroups per CU: 0 = auto (f32 launches of >= 4096 tiles: three, four for \
   * rows of >= 64 channels; otherwise as many as fit), n = at most n (by requesting more LDS). */                       \
  X(bwd_fused_wg_limit, 0, 5, 0)                                                                                        \
  /* Chunk-looping dW, lanes per row chunk: 0 = auto (8; 16 when that spares the launch a ragged last tile), 5 = 16      \
   * where the row's groups allow, any other value = 8. */                                                              \
  X(dw_tgs, 0, 5, 0)                                                                                                    \
  /* LDS-window forward kernel, workgroups per CU: 0 = auto (three on 256-thread launches of >= 1536 tiles for rows of   \
   * <= 8 channels, >= 2048 tiles for 16 channels, >= 8192 tiles for 32; else as many as fit), 1 = as many as fit,       \
   * 2..4 = at most that many. */                                                                                       \
  X(fwd_wg_limit, 0, 4, 0)                                                                                              \
  /* Per-step launches of a forward chain and of the mixer: 1 = every XCD walks its tile range forwards on even steps    \
   * and backwards on odd ones, so a launch starts on the tiles whose inputs the previous launch wrote last; 0 = always  \
   * forwards. */                                                                                                       \
  X(chain_zigzag, 0, 1, 1)                                                                                              \
  /* psf_mixer_fwd_*'s step kernel, workgroups per CU: 0 = as many as fit (three), n = at most n. */                     \
  X(mixer_wg_limit, 0, 4, 0)                                                                                            \
  /* psf_mixer_fwd_*: 1 = short sequences take the single-launch LDS-resident mixer, 0 = per-step kernels only. */        \
  X(mixer_lds, 0, 1, 1)                                                                                                 \
  /* Fused backward step (aligned instance), interleaved fronts per batch element: 0 = auto (two from N = 8192 on: every \
   * XCD walks a batch element's tiles as two fronts half a sequence apart), 1 = one; 2, 4, 8 = that many (other values  \
   * round down to a power of two; one front where the count does not divide the tiles). */                              \
  X(bwd_fronts, 0, 8, 0)                                                                                                \
  /* f32 LDS-window forward kernel, rows per thread: 0 = auto (four for rows of 16..64 channels from N = 4096 on where   \
   * the four-row tile divides N, else two), 2 = two, 4 = four wherever that instance is compiled and N holds two of its \
   * tiles; 1 and 3 act as 0. */                                                                                        \
  X(fwd_rows, 0, 4, 0)                                                                                                  \
  /* psf_chord_chain_fwd_f32 / _bf16, 2 <= M <= 64, L <= 20: 1 = short sequences (N <= 2112; to 4160 with the large      \
   * instances of "chain_cc") run as ONE launch with the sequence resident in LDS where the measured gate takes it —     \
   * f32: whenever at most two step results are kept (inference on alternating buffers), and with every step kept up to  \
   * 65536 elements per sequence (131072 for N <= 1024, 524288 on the two-group large instance); bf16: up to 1048576     \
   * elements, never the long-row instance; 2 = the one launch wherever it fits; 0 = always M per-step launches. */       \
  X(chain_fused, 0, 2, 1)                                                                                               \
  /* One-launch chain, channel groups (16 bytes of a row) per workgroup: 0 = auto: two where the rows allow (N <= 1056;  \
   * up to N = 2048 on the one-workgroup-per-CU instance when the launch keeps >= 256 workgroups; that instance with one \
   * group runs 2113 <= N <= 4160 under the same condition), 1 = one, and no instance beyond N = 2112, 2 = the           \
   * one-workgroup-per-CU instances wherever they fit. */                                                               \
  X(chain_cc, 0, 2, 0)                                                                                                  \
  /* psf_chord_chain_bwd_f32 / _bf16: 1 = the library runs the backward chain (f32: one launch where it fits), 0 = it    \
   * answers PSF_E_UNSUPPORTED and psf_chord_chain_bwd_supported answers 0: the caller runs the steps. */                 \
  X(chain_bwd_fused, 0, 1, 1)

#define PSF_TUNING_KNOBS_PRODUCER(X)                                                                                    \
  /* psf_mlp_fwd_f32: 0 = auto (the split-bf16 kernel where it applies, E <= 32; else the f32-MFMA kernel, its weights   \
   * LDS-resident on long inputs when they fit), 1 = f32 MFMA with streamed weights, 2 = f32 MFMA with LDS-resident      \
   * weights, 3 = split-bf16 (each f32 operand as three exact bf16 terms, six product terms: f32 accuracy); 2 and 3      \
   * answer PSF_E_TUNING from the call where they do not apply (weights beyond LDS; E > 32). */                           \
  X(mlp_variant, 0, 3, 0)                                                                                               \
  /* psf_mlp_wide_fwd_f32: 1 = the second layers of the MLPs with <= 32 outputs run inside the first layers' GEMM        \
   * epilogue when every MLP has 97..128 hidden rows (same arithmetic, same order, same bits), 0 = always the separate   \
   * kernel. */                                                                                                         \
  X(wide_fuse, 0, 1, 1)

#define PSF_TUNING_KNOBS(X) PSF_TUNING_KNOBS_CHORD(X) PSF_TUNING_KNOBS_PRODUCER(X)

#endif /* PSF_CHORD_TUNING_H */
