/*
 * posetraj_temporal.h - long-clip extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is frozen at PT_ABI_VERSION 10.  Its temporal attention forward, pt_attn_temporal_f16, takes clips of
 * 1 .. 128 frames through the entry point it always had; its backward, pt_attn_temporal_bwd_f16, keeps the range 1 .. 32 (one wave
 * holds the whole F x F problem in registers).  The backward of clips of 33 .. 128 frames is the entry point below: one launch,
 * one wave per (clip, position, head), two sweeps over operands staged in the wave's LDS slab (csrc/attn_bwd.hip).
 *
 * Same library, prefix `ptt_`, a version of its own.  Conventions (device pointers, `stream`, status, pt_last_error()) are those of
 * posetraj_hip.h.
 */
#ifndef POSETRAJ_TEMPORAL_H
#define POSETRAJ_TEMPORAL_H

#include <stdint.h>

#include "posetraj_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PT_TEMPORAL_ABI_VERSION 1

int ptt_abi_version(void);

/* backward of pt_attn_temporal_f16 for 33 <= F <= 128 frames, head_dim 64 or 128; arguments and addressing of
 * pt_attn_temporal_bwd_f16: token f of (clip b, position s) is row (b F + f) S + s of the fused projection qkv (pitch ld, K at
 * column k_off, V at v_off) and of dout (pitch ldo); dqkv gets dQ | dK | dV at the offsets 0 / k_off / v_off of its rows (pitch
 * ldd).  P and dS are rounded to fp16 once, sums are fp32, every gradient element is stored once: no atomics, the result is a
 * pure function of the inputs.  Any other frame count or head size is refused on the host (status 1), nothing is launched. */
int ptt_attn_temporal_bwd_long_f16(const void* qkv, int32_t ld, int32_t k_off, int32_t v_off, const void* dout, int32_t ldo, void* dqkv,
                                   int32_t ldd, int32_t B, int32_t F, int32_t S, int32_t heads, int32_t head_dim, float scale, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_TEMPORAL_H */
