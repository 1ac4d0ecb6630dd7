/*
 * posetraj_optim.h - optimizer extension of libposetraj_hip.so's C ABI (gfx950 / MI355X only).
 *
 * include/posetraj_hip.h is the drop-in boundary of the denoising path and of the training step as the reference's launch scripts
 * run it; its version and its list of entry points are frozen at PT_ABI_VERSION 10.  The optional optimizer stage of the training
 * script that needs entry points of its own (--use_8bit_adam, scripts/train_svd_traj_VIPSeg_14.py:1041-1049) lives here, in the same
 * library, under the prefix `pto_` and a version of its own.  Conventions (device pointers, `stream`, status and pt_last_error())
 * are those of posetraj_hip.h.
 */
#ifndef POSETRAJ_OPTIM_H
#define POSETRAJ_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OPTIM_ABI_VERSION 1

int pto_abi_version(void);

/* --use_8bit_adam (round 8): AdamW with block-quantised moments (the published blockwise 8-bit Adam the reference gets from
 * bitsandbytes' AdamW8bit, restated).  A parameter of at least 4096 elements keeps, per element, one uint8 code into
 * qmap1 (exp_avg; signed book) and one into qmap2 (exp_avg_sq; unsigned book) and, per block of 256 consecutive stored elements,
 * one fp32 absmax each: the stored moment is qmap[code] * absmax.  Blocks start at the parameter's offset and never cross into the
 * next one (the last may be short); block b's codes lie at state[256 b ..], so the code buffers hold 256 n_blocks bytes.  Smaller
 * parameters keep fp32 moments in two compact buffers of n_f32 floats.  One table entry per parameter, in the order of the store
 * (`work` ascending), in DEVICE memory: */
typedef struct pt_adam8_segment {
    int64_t start;      /* first element in p / g / half_mirror / ema_shadow; a multiple of 4 */
    int64_t count;      /* elements; the buffers are readable and writable up to the next multiple of 4 */
    int64_t state;      /* kind 1: its first block in absmax1 / absmax2; kind 0: its offset in exp_avg_f32 / exp_avg_sq_f32, a multiple of 4 */
    int32_t kind;       /* 1: 8-bit moments, 0: fp32 moments */
    int32_t work;       /* units of 256 elements in front of it: the sum of ceil(count / 256) over the earlier entries */
} pt_adam8_segment;
/* One launch over the whole store: the statements of pt_adamw_fused_f32 (weight decay first, torch's order) with the moments
 * dequantised on the way in; p moves by the FRESH fp32 m and v; per block absmax' = max |m| resp. max v and the new codes are the
 * book entries nearest to m / absmax1' and v / absmax2' (a block whose absmax' is 0 stores the code of 0.0).  kind 0 entries run
 * pt_adamw_fused_f32's statements on their fp32 moments.  half_mirror / zero_grad as there; ema_shadow (may be NULL) and
 * one_minus_decay as in pt_adamw_ema_f32.  Elements between two parameters are left as they are in p.  n: floats in p and g;
 * n_work: the table's total of units.  A unit that would leave p, the block range or the fp32 moments is skipped, not run.
 * 16-byte aligned: p, g, ema_shadow, exp_avg_f32, exp_avg_sq_f32; 8: half_mirror, segments; 4: state1, state2, absmax, qmaps. */
int pto_adamw8_f32(float* p, float* g, void* state1, void* state2, float* absmax1, float* absmax2, const float* qmap1, const float* qmap2,
                   float* exp_avg_f32, float* exp_avg_sq_f32, const pt_adam8_segment* segments, int32_t n_segments, int64_t n_work, int64_t n,
                   int64_t n_blocks, int64_t n_f32, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                   float inv_scale, void* half_mirror, int32_t zero_grad, float* ema_shadow, float one_minus_decay, void* stream);
/* the state of pto_adamw8_f32 as two fp32 moment buffers in the layout of p (n floats each): qmap[code] * absmax, one rounded fp32
 * product, for kind 1 entries, a copy of the fp32 moments for kind 0; elements between two parameters are not written. */
int pto_adam8_dequant_f32(const void* state1, const void* state2, const float* absmax1, const float* absmax2, const float* qmap1,
                          const float* qmap2, const float* exp_avg_f32, const float* exp_avg_sq_f32, const pt_adam8_segment* segments,
                          int32_t n_segments, int64_t n_work, int64_t n, int64_t n_blocks, int64_t n_f32, float* exp_avg, float* exp_avg_sq,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSETRAJ_OPTIM_H */
