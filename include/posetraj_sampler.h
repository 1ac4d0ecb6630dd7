/*
 * posetraj_sampler.h - sampler extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is frozen at PT_ABI_VERSION 10.  Its pt_cfg_euler_step / pt_euler_step take (sigma, sigma_next) and are the
 * first-order Euler update.  A linear multistep solver (posetraj_amd.DPMPP2MDiscreteScheduler: DPM-Solver++(2M)) updates the sample
 * from the current AND the previous denoised estimate:  x' = a x + b D + c D_prev.  The two passes below (csrc/sampler.hip) are that
 * update with the step's five scalars computed by the host in fp64 and passed as `float`; they keep the previous estimate in a buffer
 * the caller owns.
 *
 * Same library, prefix `pts_`, a version of its own.  Conventions (device pointers, `stream`, status, pt_last_error()) are those
 * of posetraj_hip.h.
 *
 * Arithmetic of both entry points, per element, every operation ONE fp32 rounding, no fused multiply-add, in this order:
 *     D  = mo * c_out + x * c_skip                      (the denoised estimate: two products, one sum)
 *     x' = a * x + b * D                 when c == 0    (denoised_prev is NOT read: on a run's first step it is uninitialised)
 *     x' = (a * x + b * D) + c * Dp      otherwise      (Dp: the value denoised_prev holds)
 *     denoised_prev <- D,  latents / prev_sample <- x'
 * so the result equals plain fp32 tensor arithmetic on the same scalars bit for bit (tests/test_sampler_gpu.py).  All five scalars
 * must be finite.
 */
#ifndef POSETRAJ_SAMPLER_H
#define POSETRAJ_SAMPLER_H

#include <stdint.h>

#include "posetraj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_SAMPLER_ABI_VERSION 1

int pts_abi_version(void);

/* Classifier-free guidance + one multistep update, the counterpart of pt_cfg_euler_step (same layouts):
 * pred [2 Bc, F, h, w, ldn] channels-last, fp32 (pred_is_f32) or fp16, uncond halves first, ldn >= 4, channels >= 4 not read;
 * guidance fp32 [Bc, F]; latents fp32 [Bc, F, 4, h, w], updated in place; denoised_prev fp32, the shape of latents, updated in place.
 * mo = pu + g * (pc - pu)  (difference, product, sum: three roundings); an fp16 pred rounds mo to fp16, as pt_cfg_euler_step does. */
int pts_cfg_multistep_step(const void* pred, int32_t pred_is_f32, int32_t ldn, const float* guidance, float c_skip, float c_out,
                           float a, float b, float c, int32_t Bc, int32_t F, int32_t h, int32_t w, float* latents,
                           float* denoised_prev, void* stream);

/* The same update on flat tensors of n elements without guidance, the counterpart of pt_euler_step: model_output fp32
 * (mo_is_f32) or fp16, sample / denoised_prev / prev_sample fp32.  prev_sample may alias sample. */
int pts_multistep_step(const void* model_output, int32_t mo_is_f32, const float* sample, float c_skip, float c_out, float a, float b,
                       float c, float* denoised_prev, float* prev_sample, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_SAMPLER_H */
