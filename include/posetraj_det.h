/*
 * posetraj_det.h - deterministic-reduction extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is frozen at PT_ABI_VERSION 10.  Its reverse-pass reductions accumulate with fp32 (sumsq: fp64) atomics,
 * so their results depend on the order in which workgroups retire.  ControlNetTrainer(deterministic=True) calls the entry points
 * below instead: the same kernels with the atomics taken out - every workgroup STORES its partial result to a slot of a caller-
 * provided workspace addressed by its block coordinates - followed by one small launch that adds the partials of each output in
 * a fixed ascending order and stores the sum, or `+=`s it where the destination accumulates (parameter gradients do).  No atomics
 * of any kind, no waiting between workgroups: always two launches, ordered by the stream.  The result is a pure function of the
 * inputs for a fixed build of the library.
 *
 * Same library, prefix `ptd_`, a version of its own.  Conventions (device pointers, `stream`, status, pt_last_error()) are those of
 * posetraj_hip.h, and so are the arguments each entry point shares with its `pt_` namesake.  New everywhere:
 *   ws, ws_floats   the workspace (device memory, 4-byte aligned; ptd_sumsq_f32: 8) and its size in floats.  It is written and read
 *                   by this call alone: calls that may run concurrently (other streams) need workspaces of their own.  A NULL or
 *                   too small workspace is refused on the host (status 1, pt_last_error() names the entry point), nothing is launched.
 *   *_ws_floats()   the size a call with these arguments needs: (partials per output) x (outputs), as spelled out per entry point.
 */
#ifndef POSETRAJ_DET_H
#define POSETRAJ_DET_H

#include <stdint.h>

#include "posetraj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_DET_ABI_VERSION 1

int ptd_abi_version(void);

/* pt_groupnorm_bwd.  Partials: one per (slab, strip) for the four statistics of a (sample, group), one per (sample, slab) for
 * dgamma / dbeta.  ws_floats = slabs * (strips * n_samples * groups * 2 + (with_params ? n_samples * 2 * channels : 0)), strips =
 * ceil(channels / 256), channels = C0 + C1.  `stat` is stored, dgamma / dbeta are added to. */
int64_t ptd_groupnorm_bwd_ws_floats(int32_t channels, int32_t groups, int64_t rows_per_sample, int32_t n_samples, int32_t with_params);
int ptd_groupnorm_bwd(const void* x0, const void* x1, int32_t C0, int32_t C1, int32_t groups, int64_t rows_per_sample, int32_t n_samples,
                      float eps, const void* gamma, const void* beta, int32_t silu, const void* dy, void* dx0, void* dx1, float* dgamma,
                      float* dbeta, float* stat, float* ws, int64_t ws_floats, void* stream);

/* pt_layernorm_bwd.  dx never crossed workgroups; with dgamma / dbeta: ws_floats = partials * 2 * C (one partial per slab of rows
 * for C <= 768, per block of rows above; inside a block the four waves meet in LDS slots of their own, added in wave order).
 * Without parameter gradients the workspace is not used and may be NULL. */
int64_t ptd_layernorm_bwd_ws_floats(int64_t M, int32_t C);
int ptd_layernorm_bwd(const void* x, int64_t M, int32_t C, const void* gamma, float eps, const void* dy, void* dx, float* dgamma,
                      float* dbeta, float* rowstat, float* ws, int64_t ws_floats, void* stream);

/* pt_colsum_f16: out[seg, c] += the column sums.  ws_floats = slabs * nseg * C. */
int64_t ptd_colsum_ws_floats(int64_t rows_per_seg, int32_t nseg, int32_t C);
int ptd_colsum_f16(const void* dy, int64_t rows_per_seg, int32_t nseg, int32_t C, int32_t ld, float* out, float* ws, int64_t ws_floats,
                   void* stream);

/* pt_dot_diff / pt_dot_diff_dev: out[0] += scale * sum dy (a - b).  ws_floats = workgroups (one term each). */
int64_t ptd_dot_diff_ws_floats(int64_t n);
int ptd_dot_diff(const void* dy, const void* a, const void* b, int64_t n, float scale, float* out, float* ws, int64_t ws_floats, void* stream);
int ptd_dot_diff_dev(const void* dy, const void* a, const void* b, int64_t n, const float* alpha_dev, float* out, float* ws, int64_t ws_floats,
                     void* stream);

/* pt_sumsq_f32: out[0] += sum g^2 in fp64.  The workspace holds one DOUBLE per workgroup: ws_floats = 2 * workgroups. */
int64_t ptd_sumsq_ws_floats(int64_t n);
int ptd_sumsq_f32(const float* g, int64_t n, double* out, float* ws, int64_t ws_floats, void* stream);

/* pt_gemm_f16 as the weight gradients use it: C += alpha op(A) op(B) in fp32, p->out_mode 2 or 3 (either means "accumulate" here),
 * p->splits as there.  With more than one split C must cover ONE dense block of memory (the store's [T][Co][Ci] gradient does):
 * split s stores its alpha * acc tiles to slice s of ws [splits][that block], the slices are added into C in ascending s.
 * ws_floats = splits * (block elements), 0 for a single split (C += by its only writer; ws may be NULL). */
int64_t ptd_gemm_ws_floats(const pt_gemm_params* p);
int ptd_gemm_f16(const pt_gemm_params* p, float* ws, int64_t ws_floats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_DET_H */
