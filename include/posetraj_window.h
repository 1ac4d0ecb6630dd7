/*
 * posetraj_window.h - C ABI of libposetraj_window.so, the add-on library of the windowed denoise loop (gfx950 / MI355X only).
 *
 * A long latent video of Ft frames is denoised as K overlapping windows of Fw frames (posetraj_amd/windows.py: window_plan); each
 * window is one ordinary clip evaluation.  The two passes below (csrc/window.hip) are the loop's prologue and epilogue: the first
 * cuts the windows out of the long latent into the networks' input, the second guides the K predictions and blends them back into
 * one long prediction.  Both are HBM-bound.
 *
 * A library of its own: it links against nothing of libposetraj_hip.so and that library's headers do not list this one.  Prefix
 * `ptw_`, a version of its own.  Conventions: every pointer is a device pointer unless called HOST; `stream` is a hipStream_t; an
 * `int` entry point returns a status, 0 = ok, non-zero = refused or failed with the reason in ptw_last_error() (thread-local, names
 * the entry point); a refused call launches nothing.
 *
 * `starts`: a HOST pointer to K int32 values, 1 <= K <= 64, read before the call returns and passed to the kernel by value.  Both
 * entry points check the rules of the plan: 1 <= Fw <= Ft, starts[0] == 0, starts ascending by 1 .. Fw (no gap, no duplicate),
 * starts[K - 1] == Ft - Fw (the last window ends on the last frame).
 */
#ifndef POSETRAJ_WINDOW_H
#define POSETRAJ_WINDOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_WINDOW_ABI_VERSION 1

int ptw_abi_version(void);

const char* ptw_last_error(void);

/* The networks' input of K windows, the windowed counterpart of pt_scale_concat_input (posetraj_hip.h):
 * latents fp32 [Ft, 4, h, w]; image_latents fp16 [2, 4, h, w] (uncond half first); out fp16 [2 K, Fw, h, w, 8], halves-major
 * (row half * K + k):
 *     out[half K + k, j, y, x, 0:4] = fp16(latents[starts[k] + j, :, y, x] * inv)       inv = 1.0f / sqrtf(sigma * sigma + 1.0f)
 *     out[half K + k, j, y, x, 4:8] = image_latents[half, :, y, x]
 * inv is computed as pt_scale_concat_input's launcher computes it: the rows of window k are that entry point's output for the
 * frames of window k, bit for bit. */
int ptw_scale_concat_windows(const float* latents, const void* image_latents, float sigma, const int32_t* starts, int32_t K,
                             int32_t Fw, int32_t Ft, int32_t h, int32_t w, void* out, void* stream);

/* Classifier-free guidance per window + the blend of the windows that cover a frame:
 * pred [2 K, Fw, h, w, ldn] channels-last, fp32 (pred_is_f32) or fp16, halves-major, ldn >= 4, channels >= 4 not read;
 * guidance fp32 [Fw], the window-local ramp (every window is guided as a clip of its own); weights fp32 [K, Fw];
 * out fp32 [Ft, 4, h, w].  Per element, every operation ONE fp32 rounding, no fused multiply-add, in this order:
 *     for k ascending over the windows with starts[k] <= f < starts[k] + Fw,  j = f - starts[k]:
 *         d    = pc - pu
 *         gd   = guidance[j] * d
 *         mo   = pu + gd                     (an fp16 pred rounds mo to fp16 and back, as pts_cfg_multistep_step does)
 *         term = weights[k, j] * mo
 *         acc  = term  for the first covering window,  acc + term  after it
 *     out = acc
 * so the result equals plain fp32 tensor arithmetic bit for bit (tests/test_windows_gpu.py). */
int ptw_cfg_window_merge(const void* pred, int32_t pred_is_f32, int32_t ldn, const float* guidance, const float* weights,
                         const int32_t* starts, int32_t K, int32_t Fw, int32_t Ft, int32_t h, int32_t w, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_WINDOW_H */
