/*
 * posetraj_batch.h - clip-batch extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is frozen at PT_ABI_VERSION 10.  Its pt_add_rowvec_f16 / pt_colsum_f16 pair adds one row vector to a
 * CONTIGUOUS run of rows and sums the gradient back: what the training tape needs for the time-embedding rows and the spatial
 * blocks' collapsed cross-attention at any batch size.  The TEMPORAL blocks' collapsed cross-attention of a batch of B clips is not
 * of that shape: the reference builds the context [H W, B]-major against [B, H W]-major tokens, so token row
 *     r = (b F + f) S + s        (clip b, frame f, position s; S = H W)
 * receives the context row of clip
 *     j(r) = (b S + s) mod B,
 * the index the inference path applies in the igemm tail (pt_igemm_params.vec_mode = 2).  The pair below is that add and its
 * backward for ControlNetTrainer at per_gpu_batch_size > 1 (csrc/batch.hip).
 *
 * Same library, prefix `ptb_`, a version of its own.  Conventions (device pointers, `stream`, status, pt_last_error()) are those of
 * posetraj_hip.h; the workspace of the deterministic form follows posetraj_det.h.  All tensors are dense: x, y, dy [B F S, C] fp16,
 * vec [B, C] fp16, C a multiple of 8 (as pt_add_rowvec_f16), B F S C / 8 < 2^31.
 */
#ifndef POSETRAJ_BATCH_H
#define POSETRAJ_BATCH_H

#include <stdint.h>

#include "posetraj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_BATCH_ABI_VERSION 1

int ptb_abi_version(void);

/* y[r, :] = x[r, :] + vec[j(r), :] (x is read once; y must not overlap x) */
int ptb_add_rowvec_interleaved_f16(const void* x, const void* vec, int32_t B, int32_t F, int32_t S, int32_t C, void* y, void* stream);

/* out[j, c] += sum over {r : j(r) = j} of dy[r, c] (fp32 `out` [B, C], fp32 sums, one pass over dy; every class j has exactly
 * F S rows).  Workgroups meet in `out` through fp32 atomics. */
int ptb_colsum_interleaved_f16(const void* dy, int32_t B, int32_t F, int32_t S, int32_t C, float* out, void* stream);

/* the same without atomics, in two launches: one partial per workgroup into ws [slabs][B][C], then an ascending fold that adds to
 * `out`.  ws_floats = slabs * B * C.  A NULL or too small workspace is refused on the host (status 1), nothing is launched. */
int64_t ptb_colsum_interleaved_ws_floats(int32_t B, int32_t F, int32_t S, int32_t C);
int ptb_colsum_interleaved_det_f16(const void* dy, int32_t B, int32_t F, int32_t S, int32_t C, float* out, float* ws, int64_t ws_floats,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_BATCH_H */
