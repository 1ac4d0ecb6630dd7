/*
 * posetraj_control.h - control-weight extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is frozen at PT_ABI_VERSION 10.  Its pt_igemm_f16 accumulates a ControlNet zero-conv straight into a
 * U-Net skip with ONE scalar (out_scale, res_post): skip += scale * zero_conv(tap).  A spatial control weight
 * (StableVideoDiffusionPipelineControlNet.denoise(control_weight=...)) and a per-step scale need one factor PER ROW (frame and
 * pixel) that a captured graph can read from device memory.  The zero-conv then writes its fp32 result to a scratch buffer and the
 * pass below accumulates it (csrc/control.hip); the igemm tail is not touched.
 *
 * Same library, prefix `ptc_`, a version of its own.  Conventions (device pointers, `stream`, status, pt_last_error()) are those
 * of posetraj_hip.h.
 */
#ifndef POSETRAJ_CONTROL_H
#define POSETRAJ_CONTROL_H

#include <stdint.h>

#include "posetraj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_CONTROL_ABI_VERSION 1

int ptc_abi_version(void);

/* y[r, c] = fp16( (scale * w[r]) * t[r, c] + ((float)y[r, c] + (y_lo ? (float)y_lo[r, c] : 0)) ),  r < rows, c < C.
 * t: fp32, pitch ldt (floats); w: fp32 [rows]; y: fp16, updated in place, pitch ldy; y_lo: optional fp16 low half of a
 * wide-stream tensor, pitch ldy, read only (the result is plain fp16; the caller drops the pair).  C % 8 == 0, pitches % 8 == 0,
 * t / y / y_lo 16-byte aligned.  Elements with c >= C inside a pitch and rows >= rows are not touched.
 * Operation order (each step one fp32 rounding, no fused multiply-add): k = scale * w[r]; x = t * k; rs = y + y_lo; x += rs;
 * one rounding to fp16 - with w = 1 the operations of pt_igemm_f16's res_post tail. */
int ptc_weighted_residual_add_f16(const float* t, int64_t ldt, const float* w, float scale, void* y, const void* y_lo,
                                  int64_t ldy, int64_t rows, int32_t C, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_CONTROL_H */
