// The optimizer step of the ControlNet training (scripts/train_svd_traj_VIPSeg_14.py:1414-1430: `optimizer.step()`, `ema.step()`):
// AdamW in fp32 - plain, fused with the fp16 mirror / gradient zeroing / EMA, and over block-quantised 8-bit moments
// (include/posetraj_optim.h) - the EMA update alone, and the fp16 weight packs that are refreshed from the fp32 master after every step.
#include "pt_common.h"
#include "../../include/posetraj_optim.h"
#include "pt_launch.h"

namespace {

// AdamW (torch.optim.AdamW, the optimizer of scripts/train_svd_traj_VIPSeg_14.py:1051,1070-1076), fp32, in place:
//   g' = g * inv_scale ; p *= 1 - lr wd ; m = b1 m + (1 - b1) g' ; v = b2 v + (1 - b2) g'^2 ;
//   p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                                                    float bc1, float bc2_sqrt, float inv_scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * inv_scale;
        float pi = p[i] * (1.0f - lr * wd);
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        p[i] = pi;
    }
}

// The same update, four values per thread, and the two passes that follow an optimizer step in the trainer folded in (round 6): the fp16
// mirror of the parameters (ParamStore.flat16: norm weights / biases are read from it) is written here instead of by a cast over the
// whole buffer, and the gradient is zeroed here instead of by a fill - 5.4 GB of the step's 28 GB of optimizer traffic.
//
// EMA (round 7): diffusers' EMAModel.step over the same parameters (--use_ema; scripts/train_svd_traj_VIPSeg_14.py:1428-1430),
//   shadow.sub_((1 - decay) * (shadow - param))   =   d = s - p ; t = omd d ; s = s - t      three separately rounded fp32 operations.
// Left to itself the compiler contracts t and the last subtraction into one v_fma (the rounding intrinsics do not stop it), so the
// statements sit under `fp contract(off)` - and only they: AdamW's own expressions keep the contraction they always had.
__device__ __forceinline__ float ema_update(float s, float p, float omd) {
#pragma clang fp contract(off)
    const float d = s - p;
    const float t = omd * d;
    return s - t;
}

// AdamW's statements for one element (those of adamw_kernel): p, m, v in and out, g un-scaled on the way in.  One copy for the fused
// kernel and the 8-bit one, and every multiply-add spelled out under `fp contract(off)`: left to the compiler, WHICH product of
// `c p - k q` or `b1 m + (1 - b1) g` joins the addition in a v_fma depends on the code around the statement, and the two kernels
// then differ in the last bit.  The roundings below are the ones the fused kernel has always had.
struct AdamwScalars { float lr, b1, b2, eps, wd, bc1, bc2_sqrt, inv_scale; };
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamwScalars& a) {
#pragma clang fp contract(off)
    const float gi = g * a.inv_scale;
    const float mi = __builtin_fmaf(a.b1, m, (1.0f - a.b1) * gi);
    const float vi = __builtin_fmaf(a.b2, v, (1.0f - a.b2) * gi * gi);
    m = mi; v = vi;
    const float denom = sqrtf(vi) / a.bc2_sqrt + a.eps;
    const float step = -(a.lr / a.bc1) * (mi / denom);           // (the sign rides on the uniform factor: no negation per element)
    p = __builtin_fmaf(__builtin_fmaf(-a.lr, a.wd, 1.0f), p, step);
}

// EMA = true: the shadow follows the NEW parameter while it is still in a register (one more read and one more write of a buffer whose
// neighbours are already here: 8 bytes per parameter on top of 34, against 12 for a launch of its own).
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_fused_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          int64_t n4, float lr, float b1, float b2, float eps, float wd, float bc1,
                                                          float bc2_sqrt, float inv_scale, f16* __restrict__ mirror, int zero_g,
                                                          float* __restrict__ shadow, float omd) {
    const AdamwScalars a = {lr, b1, b2, eps, wd, bc1, bc2_sqrt, inv_scale};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 g4 = *(const f32x4*)(g + 4 * i), m4 = *(const f32x4*)(m + 4 * i), v4 = *(const f32x4*)(v + 4 * i);
        f32x4 p4 = *(const f32x4*)(p + 4 * i), mo, vo, s4;
        f16x4 h4;
        if constexpr (EMA) s4 = *(const f32x4*)(shadow + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pi = p4[j], mi = m4[j], vi = v4[j];
            adamw_one(pi, g4[j], mi, vi, a);
            mo[j] = mi; vo[j] = vi;
            p4[j] = pi;
            h4[j] = (f16)pi;
            if constexpr (EMA) s4[j] = ema_update(s4[j], pi, omd);
        }
        *(f32x4*)(p + 4 * i) = p4; *(f32x4*)(m + 4 * i) = mo; *(f32x4*)(v + 4 * i) = vo;
        if (mirror) *(f16x4*)(mirror + 4 * i) = h4;
        if (zero_g) *(f32x4*)(g + 4 * i) = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) *(f32x4*)(shadow + 4 * i) = s4;
    }
}

// The EMA update alone: the step the GradScaler skipped (the shadow moves toward the unchanged parameters), and the stand-alone EMAModel.step()
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ shadow, const float* __restrict__ p, int64_t n4, float omd) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 p4 = *(const f32x4*)(p + 4 * i);
        f32x4 s4 = *(const f32x4*)(shadow + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) s4[j] = ema_update(s4[j], p4[j], omd);
        *(f32x4*)(shadow + 4 * i) = s4;
    }
}

// ---- --use_8bit_adam (round 8): AdamW over block-quantised moments (include/posetraj_optim.h: pto_adamw8_f32) -------------
// The store is cut into UNITS of 256 elements that never cross a parameter (pt_adam8_segment.work counts them); one wave takes one
// unit at a time, 4 elements per lane (16-byte loads of p and g, 4 bytes of codes), and every wave owns a contiguous run of units:
// it looks its first unit's parameter up once (binary search over the table's `work` column) and then walks the table forward.
// Everything that places a unit is wave-uniform.  A unit is checked against the buffers' extents before anything is touched.
constexpr int ADAM8_BLOCK = 256;

struct Adam8Unit {
    int64_t e0;          // first element of the unit in p
    int64_t st;          // kind 1: its block; kind 0: offset of its first fp32 moment
    int len, kind;       // elements (1 .. 256)
};

struct Adam8Walk {
    const pt_adam8_segment* seg;
    int nseg, s;
    int64_t n, n_blocks, n_f32;
    __device__ __forceinline__ void seek(int64_t w) {           // the last entry whose `work` is <= w
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int64_t)seg[mid].work <= w) lo = mid; else hi = mid - 1;
        }
        s = lo;
    }
    // unit w (not below the last one asked for); false: the table is inconsistent with the buffers there, nothing may be touched
    __device__ __forceinline__ bool unit(int64_t w, Adam8Unit& u) {
        while (s + 1 < nseg && (int64_t)seg[s + 1].work <= w) ++s;
        const pt_adam8_segment e = seg[s];
        const int64_t local = w - e.work, first = local * ADAM8_BLOCK, left = e.count - first;
        u.e0 = e.start + first;
        u.len = (int)(left < ADAM8_BLOCK ? left : ADAM8_BLOCK);
        u.kind = e.kind;
        u.st = e.kind ? e.state + local : e.state + first;
        const int64_t len4 = (u.len + 3) & ~3;
        bool ok = local >= 0 && left > 0 && e.start >= 0 && (e.start & 3) == 0 && u.e0 + len4 <= n && e.state >= 0;
        ok = ok && (e.kind ? u.st < n_blocks : ((e.state & 3) == 0 && u.st + len4 <= n_f32));
        return ok;
    }
};

// largest i with book[i] <= x (0 if there is none), then the nearer of book[i] and book[i + 1]; a tie keeps the lower.  book: 256
// ascending floats in LDS - 9 dependent ds_read_b32 per value
__device__ __forceinline__ int adam8_nearest(const float* book, float x) {
    int lo = 0;
    float below = book[0];
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        const float t = book[lo + s];
        if (t <= x) { lo += s; below = t; }
    }
    const int up = lo < 255 ? lo + 1 : 255;
    return (x - below > book[up] - x) ? up : lo;
}

__device__ __forceinline__ float adam8_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw8_kernel(float* __restrict__ p, float* __restrict__ g, uint8_t* __restrict__ c1, uint8_t* __restrict__ c2,
                                                     float* __restrict__ am1, float* __restrict__ am2, const float* __restrict__ q1,
                                                     const float* __restrict__ q2, float* __restrict__ m32, float* __restrict__ v32,
                                                     Adam8Walk walk, int64_t n_work, int64_t per_wave, AdamwScalars a, f16* __restrict__ mirror,
                                                     int zero_g, float* __restrict__ shadow, float omd) {
    __shared__ float book1[256], book2[256];
    book1[threadIdx.x] = q1[threadIdx.x];
    book2[threadIdx.x] = q2[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t w0 = wave * per_wave, w1 = w0 + per_wave < n_work ? w0 + per_wave : n_work;
    if (w0 >= w1) return;
    walk.seek(w0);
    for (int64_t w = w0; w < w1; ++w) {
        Adam8Unit u;
        if (!walk.unit(w, u)) continue;
        const bool on = 4 * lane < u.len;                       // this lane's four elements hold at least one of the unit's
        const int64_t e = u.e0 + 4 * lane;
        f32x4 p4 = {0.f, 0.f, 0.f, 0.f}, g4 = p4, m4 = p4, v4 = p4, s4 = p4;
        uint32_t k1 = 0, k2 = 0;
        if (on) {
            p4 = *(const f32x4*)(p + e); g4 = *(const f32x4*)(g + e);
            if constexpr (EMA) s4 = *(const f32x4*)(shadow + e);
        }
        if (u.kind) {
            const float a1 = am1[u.st], a2 = am2[u.st];
            if (on) {
                k1 = *(const uint32_t*)(c1 + u.st * ADAM8_BLOCK + 4 * lane); k2 = *(const uint32_t*)(c2 + u.st * ADAM8_BLOCK + 4 * lane);
#pragma unroll
                for (int j = 0; j < 4; ++j) { m4[j] = book1[(k1 >> (8 * j)) & 255] * a1; v4[j] = book2[(k2 >> (8 * j)) & 255] * a2; }
            }
        } else if (on) {
            m4 = *(const f32x4*)(m32 + u.st + 4 * lane); v4 = *(const f32x4*)(v32 + u.st + 4 * lane);
        }
        f32x4 po = p4, so = s4;
        f16x4 h4;
        float mx1 = 0.f, mx2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pi = p4[j], mi = m4[j], vi = v4[j];
            adamw_one(pi, g4[j], mi, vi, a);
            const bool live = 4 * lane + j < u.len;             // an element past the parameter's end keeps its value everywhere
            if (live) { po[j] = pi; if constexpr (EMA) so[j] = ema_update(s4[j], pi, omd); }
            m4[j] = live ? mi : 0.f; v4[j] = live ? vi : 0.f;
            h4[j] = (f16)po[j];
            mx1 = fmaxf(mx1, fabsf(m4[j])); mx2 = fmaxf(mx2, v4[j]);
        }
        if (u.kind) {
            mx1 = adam8_wave_max(mx1); mx2 = adam8_wave_max(mx2);
            if (on) {
                k1 = k2 = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {                   // absmax' == 0: every m (v) of the block is 0 - no division, the code of 0.0
                    k1 |= (uint32_t)adam8_nearest(book1, mx1 > 0.f ? m4[j] / mx1 : 0.f) << (8 * j);
                    k2 |= (uint32_t)adam8_nearest(book2, mx2 > 0.f ? v4[j] / mx2 : 0.f) << (8 * j);
                }
                *(uint32_t*)(c1 + u.st * ADAM8_BLOCK + 4 * lane) = k1; *(uint32_t*)(c2 + u.st * ADAM8_BLOCK + 4 * lane) = k2;
            }
            if (lane == 0) { am1[u.st] = mx1; am2[u.st] = mx2; }
        } else if (on) {
            *(f32x4*)(m32 + u.st + 4 * lane) = m4; *(f32x4*)(v32 + u.st + 4 * lane) = v4;
        }
        if (on) {
            *(f32x4*)(p + e) = po;
            if (mirror) *(f16x4*)(mirror + e) = h4;
            if (zero_g) *(f32x4*)(g + e) = (f32x4){0.f, 0.f, 0.f, 0.f};
            if constexpr (EMA) *(f32x4*)(shadow + e) = so;
        }
    }
}

// the 8-bit state as fp32 moments in the layout of p: book[code] * absmax (kind 1), a copy (kind 0)
__global__ __launch_bounds__(256) void adam8_dequant_kernel(const uint8_t* __restrict__ c1, const uint8_t* __restrict__ c2, const float* __restrict__ am1,
                                                            const float* __restrict__ am2, const float* __restrict__ q1, const float* __restrict__ q2,
                                                            const float* __restrict__ m32, const float* __restrict__ v32, Adam8Walk walk,
                                                            int64_t n_work, int64_t per_wave, float* __restrict__ m, float* __restrict__ v) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int64_t w0 = wave * per_wave, w1 = w0 + per_wave < n_work ? w0 + per_wave : n_work;
    if (w0 >= w1) return;
    walk.seek(w0);
    for (int64_t w = w0; w < w1; ++w) {
        Adam8Unit u;
        if (!walk.unit(w, u)) continue;
        for (int i = lane; i < u.len; i += 64) {
            if (u.kind) {
                m[u.e0 + i] = q1[c1[u.st * ADAM8_BLOCK + i]] * am1[u.st];
                v[u.e0 + i] = q2[c2[u.st * ADAM8_BLOCK + i]] * am2[u.st];
            } else {
                m[u.e0 + i] = m32[u.st + i];
                v[u.e0 + i] = v32[u.st + i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ weight packs from the fp32 master
// w fp32 [T][Co][Ci] (the ParamStore's tap-major layout; T = kh kw taps, 1 for a linear layer) -> the fp16 image
// pt_igemm_f16 streams:
//   forward pack   dst[co][t Cpad + ci]
//   transposed     dst[ci][(T - 1 - t) Cpad + co]      (the data gradient's weight: channels swapped, taps flipped)
// A block moves a 32 (co) x 32 (ci) tile of every tap: 128-byte runs in, 64-byte runs out (through LDS when transposing).
// Padding of dst is never written (the buffers are zero-filled once).
__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, int Co, int Ci, int T, int transposed,
                                                          f16* __restrict__ dst, int Kpad, int Cpad, const float* __restrict__ bias,
                                                          f16* __restrict__ dst_bias) {
    __shared__ f16 tile[32][33];
    const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int t = 0; t < T; ++t) {
        const float* src = w + (int64_t)t * Co * Ci;
        if (!transposed) {
            for (int r = r0; r < 32; r += 8)
                if (co0 + r < Co && ci0 + c < Ci) dst[(int64_t)(co0 + r) * Kpad + t * Cpad + ci0 + c] = (f16)src[(int64_t)(co0 + r) * Ci + ci0 + c];
        } else {
            __syncthreads();
            for (int r = r0; r < 32; r += 8) tile[r][c] = (co0 + r < Co && ci0 + c < Ci) ? (f16)src[(int64_t)(co0 + r) * Ci + ci0 + c] : (f16)0.f;
            __syncthreads();
            for (int q = r0; q < 32; q += 8)          // q: ci within the tile, c: co within the tile
                if (ci0 + q < Ci && co0 + c < Co) dst[(int64_t)(ci0 + q) * Kpad + (T - 1 - t) * Cpad + co0 + c] = tile[c][q];
        }
    }
    if (!transposed && blockIdx.x == 0 && bias && dst_bias && threadIdx.x < 32 && co0 + (int)threadIdx.x < Co)
        dst_bias[co0 + threadIdx.x] = (f16)bias[co0 + threadIdx.x];
}

}  // namespace

extern "C" int pt_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int32_t step, float inv_scale, void* stream) {
    PT_CHECK(p && g && m && v && n > 0 && step >= 1, "pt_adamw_f32: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    return launch_ew("pt_adamw_f32", adamw_kernel, n, stream, p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), inv_scale);
}

// one launcher for pt_adamw_fused_f32 (shadow == nullptr) and pt_adamw_ema_f32
static int adamw_fused_launch(const char* who, float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int32_t step, float inv_scale, void* half_mirror, int32_t zero_grad, float* shadow,
                              float one_minus_decay, void* stream) {
    PT_CHECK(p && g && m && v && n > 0 && n % 4 == 0 && step >= 1, "%s: bad arguments (n must be a multiple of 4)", who);
    auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
    PT_CHECK(al16(p) && al16(g) && al16(m) && al16(v) && al16(shadow) && (!half_mirror || ((uintptr_t)half_mirror & 7) == 0),
             "%s: buffers must be 16-byte aligned", who);
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    if (shadow)
        return launch_ew(who, adamw_fused_kernel<true>, n / 4, stream, p, g, m, v, n / 4, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2),
                         inv_scale, (f16*)half_mirror, zero_grad, shadow, one_minus_decay);
    return launch_ew(who, adamw_fused_kernel<false>, n / 4, stream, p, g, m, v, n / 4, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2),
                     inv_scale, (f16*)half_mirror, zero_grad, (float*)nullptr, 0.0f);
}

extern "C" int pt_adamw_fused_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  int32_t step, float inv_scale, void* half_mirror, int32_t zero_grad, void* stream) {
    return adamw_fused_launch("pt_adamw_fused_f32", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, inv_scale, half_mirror, zero_grad, nullptr,
                              0.0f, stream);
}

extern "C" int pt_adamw_ema_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                int32_t step, float inv_scale, void* half_mirror, int32_t zero_grad, float* ema_shadow, float one_minus_decay,
                                void* stream) {
    PT_CHECK(ema_shadow && ema_shadow != p, "pt_adamw_ema_f32: ema_shadow must be a buffer of its own");
    return adamw_fused_launch("pt_adamw_ema_f32", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, inv_scale, half_mirror, zero_grad, ema_shadow,
                              one_minus_decay, stream);
}

extern "C" int pt_ema_update_f32(float* shadow, const float* p, int64_t n, float one_minus_decay, void* stream) {
    PT_CHECK(shadow && p && shadow != p && n > 0 && n % 4 == 0, "pt_ema_update_f32: bad arguments (n must be a multiple of 4)");
    PT_CHECK(((uintptr_t)shadow & 15) == 0 && ((uintptr_t)p & 15) == 0, "pt_ema_update_f32: buffers must be 16-byte aligned");
    return launch_ew("pt_ema_update_f32", ema_update_kernel, n / 4, stream, shadow, p, n / 4, one_minus_decay);
}

// the grid of the two 8-bit kernels: waves that each own `per_wave` consecutive units - at most 8 workgroups of 4 waves per CU
static unsigned adam8_grid(int64_t n_work, int64_t* per_wave) {
    const int64_t max_waves = 256 * 8 * 4;
    *per_wave = (n_work + max_waves - 1) / max_waves;
    const int64_t waves = (n_work + *per_wave - 1) / *per_wave;
    return (unsigned)((waves + 3) / 4);
}

extern "C" int pto_abi_version(void) { return PT_OPTIM_ABI_VERSION; }

extern "C" int pto_adamw8_f32(float* p, float* g, void* state1, void* state2, float* absmax1, float* absmax2, const float* qmap1, const float* qmap2,
                             float* exp_avg_f32, float* exp_avg_sq_f32, const pt_adam8_segment* segments, int32_t n_segments, int64_t n_work,
                             int64_t n, int64_t n_blocks, int64_t n_f32, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int32_t step, float inv_scale, void* half_mirror, int32_t zero_grad, float* ema_shadow, float one_minus_decay,
                             void* stream) {
    PT_CHECK(p && g && segments && n_segments > 0 && n_work > 0 && n > 0 && n % 4 == 0 && step >= 1, "pto_adamw8_f32: bad arguments (n must be a multiple of 4)");
    PT_CHECK(qmap1 && qmap2, "pto_adamw8_f32: qmap1 / qmap2 (the two code books of 256 floats) must not be null");
    PT_CHECK(n_blocks >= 0 && n_f32 >= 0 && n_f32 % 4 == 0 && n_work < ((int64_t)1 << 31), "pto_adamw8_f32: bad state extents (n_f32 must be a multiple of 4)");
    PT_CHECK(n_blocks == 0 || (state1 && state2 && absmax1 && absmax2), "pto_adamw8_f32: n_blocks > 0 needs state1, state2, absmax1, absmax2");
    PT_CHECK(n_f32 == 0 || (exp_avg_f32 && exp_avg_sq_f32), "pto_adamw8_f32: n_f32 > 0 needs exp_avg_f32, exp_avg_sq_f32");
    PT_CHECK(ema_shadow != p, "pto_adamw8_f32: ema_shadow must be a buffer of its own");
    auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
    PT_CHECK(al(p, 16) && al(g, 16) && al(ema_shadow, 16) && al(exp_avg_f32, 16) && al(exp_avg_sq_f32, 16) && al(half_mirror, 8) && al(segments, 8) &&
                 al(state1, 4) && al(state2, 4) && al(absmax1, 4) && al(absmax2, 4) && al(qmap1, 4) && al(qmap2, 4),
             "pto_adamw8_f32: buffers must be aligned (p, g, ema_shadow, fp32 moments: 16 bytes; half_mirror, segments: 8; the rest: 4)");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const AdamwScalars a = {lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), inv_scale};
    const Adam8Walk walk = {segments, n_segments, 0, n, n_blocks, n_f32};
    int64_t per_wave;
    const unsigned blocks = adam8_grid(n_work, &per_wave);
    if (ema_shadow)
        hipLaunchKernelGGL(adamw8_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1, (uint8_t*)state2, absmax1, absmax2,
                           qmap1, qmap2, exp_avg_f32, exp_avg_sq_f32, walk, n_work, per_wave, a, (f16*)half_mirror, zero_grad, ema_shadow, one_minus_decay);
    else
        hipLaunchKernelGGL(adamw8_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, (uint8_t*)state1, (uint8_t*)state2, absmax1, absmax2,
                           qmap1, qmap2, exp_avg_f32, exp_avg_sq_f32, walk, n_work, per_wave, a, (f16*)half_mirror, zero_grad, (float*)nullptr, 0.0f);
    PT_LAUNCH_CHECK("pto_adamw8_f32");
    return 0;
}

extern "C" int pto_adam8_dequant_f32(const void* state1, const void* state2, const float* absmax1, const float* absmax2, const float* qmap1,
                                    const float* qmap2, const float* exp_avg_f32, const float* exp_avg_sq_f32, const pt_adam8_segment* segments,
                                    int32_t n_segments, int64_t n_work, int64_t n, int64_t n_blocks, int64_t n_f32, float* exp_avg, float* exp_avg_sq,
                                    void* stream) {
    PT_CHECK(exp_avg && exp_avg_sq && segments && n_segments > 0 && n_work > 0 && n > 0, "pto_adam8_dequant_f32: bad arguments");
    PT_CHECK(qmap1 && qmap2, "pto_adam8_dequant_f32: qmap1 / qmap2 (the two code books of 256 floats) must not be null");
    PT_CHECK(n_blocks >= 0 && n_f32 >= 0 && n_work < ((int64_t)1 << 31), "pto_adam8_dequant_f32: bad state extents");
    PT_CHECK(n_blocks == 0 || (state1 && state2 && absmax1 && absmax2), "pto_adam8_dequant_f32: n_blocks > 0 needs state1, state2, absmax1, absmax2");
    PT_CHECK(n_f32 == 0 || (exp_avg_f32 && exp_avg_sq_f32), "pto_adam8_dequant_f32: n_f32 > 0 needs exp_avg_f32, exp_avg_sq_f32");
    PT_CHECK(((uintptr_t)segments & 7) == 0 && (((uintptr_t)absmax1 | (uintptr_t)absmax2 | (uintptr_t)qmap1 | (uintptr_t)qmap2 | (uintptr_t)exp_avg_f32 |
                                                 (uintptr_t)exp_avg_sq_f32 | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3) == 0,
             "pto_adam8_dequant_f32: buffers must be aligned (segments: 8 bytes; floats: 4)");
    const Adam8Walk walk = {segments, n_segments, 0, n, n_blocks, n_f32};
    int64_t per_wave;
    const unsigned blocks = adam8_grid(n_work, &per_wave);
    hipLaunchKernelGGL(adam8_dequant_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)state1, (const uint8_t*)state2, absmax1,
                       absmax2, qmap1, qmap2, exp_avg_f32, exp_avg_sq_f32, walk, n_work, per_wave, exp_avg, exp_avg_sq);
    PT_LAUNCH_CHECK("pto_adam8_dequant_f32");
    return 0;
}

extern "C" int pt_pack_weight_f32(const float* w, int32_t Co, int32_t Ci, int32_t T, int32_t transposed, const float* bias, void* dst,
                                  int32_t Kpad, int32_t Cpad, void* dst_bias, void* stream) {
    PT_CHECK(w && dst, "pt_pack_weight_f32: null pointer");
    PT_CHECK(Co > 0 && Ci > 0 && T > 0 && T <= 9 && Kpad > 0 && Cpad > 0, "pt_pack_weight_f32: bad sizes (Co %d Ci %d T %d)", Co, Ci, T);
    PT_CHECK((transposed ? Co : Ci) <= Cpad && (T - 1) * Cpad + (transposed ? Co : Ci) <= Kpad, "pt_pack_weight_f32: the taps do not fit the row (Cpad %d, Kpad %d)", Cpad, Kpad);
    const dim3 grid((Ci + 31) / 32, (Co + 31) / 32);
    PT_CHECK(grid.y < 65536, "pt_pack_weight_f32: too many output channels");
    hipLaunchKernelGGL(pack_weight_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, Co, Ci, T, transposed, (f16*)dst,
                       Kpad, Cpad, bias, (f16*)dst_bias);
    PT_LAUNCH_CHECK("pt_pack_weight_f32");
    return 0;
}
