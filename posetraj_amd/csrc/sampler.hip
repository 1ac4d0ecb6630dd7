// Linear multistep sampler step (include/posetraj_sampler.h): x' = a x + b D + c D_prev with D = mo c_out + x c_skip, the update of
// DPM-Solver++(2M) (posetraj_amd/scheduling_dpmpp_2m.py).  The host computes the five scalars of a step in fp64; the kernels only
// multiply and add.  HBM-bound: per latent pixel the guided pass reads two predictions (16 bytes each in fp32), reads and writes 4
// latent channels and writes - from the second step on also reads - 4 channels of the previous estimate.  One thread per pixel like
// cfg_euler_kernel (elementwise.hip): the prediction's 4 channels are one 16-byte (fp32) / 8-byte (fp16) access, the planar fp32
// tensors are coalesced across the pixels of a wave.
#include "pt_common.h"
#include "../../include/posetraj_sampler.h"

#include <cmath>

namespace {

// One element.  Every operation is rounded to fp32 on its own, in the header's order: equal to plain fp32 tensor arithmetic bit for
// bit.  Plain operators under `fp contract(off)` (control.hip: the rounding intrinsics are inlined with their header's contraction).
// PREV = false is the c == 0 step: Dp is never loaded by the callers.
template <bool PREV>
__device__ __forceinline__ float multistep_update(float mo, float x, float Dp, float c_skip, float c_out, float a, float b, float c, float& D) {
#pragma clang fp contract(off)
    const float t0 = mo * c_out;
    const float t1 = x * c_skip;
    D = t0 + t1;
    const float u0 = a * x;
    const float u1 = b * D;
    float s = u0 + u1;
    if (PREV) {
        const float u2 = c * Dp;
        s = s + u2;
    }
    return s;
}

// guided prediction of one channel: difference, product, sum - three roundings; fp16 predictions round the result to fp16
template <typename T>
__device__ __forceinline__ float guided(float pu, float pc, float g) {
#pragma clang fp contract(off)
    const float d = pc - pu;
    const float gd = g * d;
    const float mo = pu + gd;
    return sizeof(T) == 2 ? (float)(f16)mo : mo;
}

template <typename T> struct vec4;
template <> struct vec4<float> { typedef f32x4 type; };
template <> struct vec4<f16> { typedef f16x4 type; };

// VEC: the 4 channels of a pixel are one aligned vector (ldn % 4 == 0 and an aligned base; the host decides)
template <typename T, bool PREV, bool VEC>
__global__ __launch_bounds__(256) void cfg_multistep_kernel(const T* __restrict__ pred, int ldn, const float* __restrict__ guidance, float c_skip,
                                                            float c_out, float a, float b, float c, int Bc, int F, int HW, float* __restrict__ lat,
                                                            float* __restrict__ dprev, int64_t total_pix) {
    typedef typename vec4<T>::type V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_pix; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const int64_t nf = i / HW;                                                      // clip * F + f
        const T* u = pred + (nf * HW + p) * ldn;                                        // uncond half
        const T* cd = pred + (((int64_t)Bc * F + nf) * HW + p) * ldn;                   // cond half
        const float g = guidance[nf];
        float pu[4], pc[4];
        if (VEC) {
            const V vu = *(const V*)u, vc = *(const V*)cd;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) { pu[ch] = (float)vu[ch]; pc[ch] = (float)vc[ch]; }
        } else {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) { pu[ch] = (float)u[ch]; pc[ch] = (float)cd[ch]; }
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int64_t o = (nf * 4 + ch) * HW + p;
            const float x = lat[o];
            const float Dp = PREV ? dprev[o] : 0.f;
            float D;
            lat[o] = multistep_update<PREV>(guided<T>(pu[ch], pc[ch], g), x, Dp, c_skip, c_out, a, b, c, D);
            dprev[o] = D;
        }
    }
}

// flat: n4 groups of 4 elements as 16-byte (fp32) / 8-byte (fp16 model output) accesses, the n - 4 n4 others one by one (n4 = 0 when
// a pointer is not aligned).  out may alias x: a thread reads its own elements before it writes them.
template <typename T, bool PREV>
__global__ __launch_bounds__(256) void multistep_flat_kernel(const T* __restrict__ mo, const float* x, float c_skip, float c_out, float a, float b,
                                                             float c, float* __restrict__ dprev, float* out, int64_t n4, int64_t n) {
    typedef typename vec4<T>::type V;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < n4; i += stride) {
        const V m = *(const V*)(mo + i * 4);
        const f32x4 xv = *(const f32x4*)(x + i * 4);
        f32x4 dp = {};
        if (PREV) dp = *(const f32x4*)(dprev + i * 4);
        f32x4 o, d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float D;
            o[j] = multistep_update<PREV>((float)m[j], xv[j], dp[j], c_skip, c_out, a, b, c, D);
            d[j] = D;
        }
        *(f32x4*)(dprev + i * 4) = d;
        *(f32x4*)(out + i * 4) = o;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) {
        const float xv = x[i];
        const float dp = PREV ? dprev[i] : 0.f;
        float D;
        out[i] = multistep_update<PREV>((float)mo[i], xv, dp, c_skip, c_out, a, b, c, D);
        dprev[i] = D;
    }
}

unsigned grid_for(int64_t n) {                               // 256 CUs x 16 workgroups; the elements beyond are grid-strided
    int64_t b = (n + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

inline bool finite5(float c_skip, float c_out, float a, float b, float c) {
    return std::isfinite(c_skip) && std::isfinite(c_out) && std::isfinite(a) && std::isfinite(b) && std::isfinite(c);
}

template <typename T>
void launch_cfg(const void* pred, int ldn, const float* guidance, float c_skip, float c_out, float a, float b, float c, int Bc, int F, int HW,
                float* lat, float* dprev, int64_t total, hipStream_t stream) {
    const bool vec = ldn % 4 == 0 && ((uintptr_t)pred & (4 * sizeof(T) - 1)) == 0;
    const dim3 grid(grid_for(total)), block(256);
#define PTS_LAUNCH(PREV, VEC)                                                                                                               \
    hipLaunchKernelGGL((cfg_multistep_kernel<T, PREV, VEC>), grid, block, 0, stream, (const T*)pred, ldn, guidance, c_skip, c_out, a, b, c, \
                       Bc, F, HW, lat, dprev, total)
    if (c != 0.0f) { if (vec) PTS_LAUNCH(true, true); else PTS_LAUNCH(true, false); }
    else           { if (vec) PTS_LAUNCH(false, true); else PTS_LAUNCH(false, false); }
#undef PTS_LAUNCH
}

template <typename T>
void launch_flat(const void* mo, const float* x, float c_skip, float c_out, float a, float b, float c, float* dprev, float* out, int64_t n,
                 hipStream_t stream) {
    const bool vec = (((uintptr_t)x | (uintptr_t)dprev | (uintptr_t)out) & 15) == 0 && ((uintptr_t)mo & (4 * sizeof(T) - 1)) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t threads = n4 > n - 4 * n4 ? n4 : n - 4 * n4;
    const dim3 grid(grid_for(threads)), block(256);
    if (c != 0.0f)
        hipLaunchKernelGGL((multistep_flat_kernel<T, true>), grid, block, 0, stream, (const T*)mo, x, c_skip, c_out, a, b, c, dprev, out, n4, n);
    else
        hipLaunchKernelGGL((multistep_flat_kernel<T, false>), grid, block, 0, stream, (const T*)mo, x, c_skip, c_out, a, b, c, dprev, out, n4, n);
}

}  // namespace

extern "C" int pts_abi_version(void) { return PT_SAMPLER_ABI_VERSION; }

extern "C" int pts_cfg_multistep_step(const void* pred, int32_t pred_is_f32, int32_t ldn, const float* guidance, float c_skip, float c_out,
                                      float a, float b, float c, int32_t Bc, int32_t F, int32_t h, int32_t w, float* latents,
                                      float* denoised_prev, void* stream) {
    PT_CHECK(pred && guidance && latents && denoised_prev, "pts_cfg_multistep_step: null pointer");
    PT_CHECK(ldn >= 4, "pts_cfg_multistep_step: ldn %d < 4 (the prediction's 4 latent channels)", ldn);
    PT_CHECK(Bc > 0 && F > 0 && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31) && (int64_t)Bc * F * h * w < ((int64_t)1 << 40),
             "pts_cfg_multistep_step: bad sizes (Bc=%d F=%d h=%d w=%d)", Bc, F, h, w);
    PT_CHECK(finite5(c_skip, c_out, a, b, c), "pts_cfg_multistep_step: non-finite scalar (c_skip=%g c_out=%g a=%g b=%g c=%g)", c_skip, c_out, a, b, c);
    PT_CHECK(((uintptr_t)guidance & 3) == 0 && ((uintptr_t)latents & 3) == 0 && ((uintptr_t)denoised_prev & 3) == 0 &&
             ((uintptr_t)pred & (pred_is_f32 ? 3 : 1)) == 0, "pts_cfg_multistep_step: misaligned pointer");
    const int64_t total = (int64_t)Bc * F * h * w;
    if (pred_is_f32) launch_cfg<float>(pred, ldn, guidance, c_skip, c_out, a, b, c, Bc, F, h * w, latents, denoised_prev, total, (hipStream_t)stream);
    else             launch_cfg<f16>(pred, ldn, guidance, c_skip, c_out, a, b, c, Bc, F, h * w, latents, denoised_prev, total, (hipStream_t)stream);
    PT_LAUNCH_CHECK("pts_cfg_multistep_step");
    return 0;
}

extern "C" int pts_multistep_step(const void* model_output, int32_t mo_is_f32, const float* sample, float c_skip, float c_out, float a, float b,
                                  float c, float* denoised_prev, float* prev_sample, int64_t n, void* stream) {
    PT_CHECK(model_output && sample && denoised_prev && prev_sample, "pts_multistep_step: null pointer");
    PT_CHECK(n > 0 && n < ((int64_t)1 << 40), "pts_multistep_step: bad size (n=%lld)", (long long)n);
    PT_CHECK(finite5(c_skip, c_out, a, b, c), "pts_multistep_step: non-finite scalar (c_skip=%g c_out=%g a=%g b=%g c=%g)", c_skip, c_out, a, b, c);
    PT_CHECK(((uintptr_t)sample & 3) == 0 && ((uintptr_t)denoised_prev & 3) == 0 && ((uintptr_t)prev_sample & 3) == 0 &&
             ((uintptr_t)model_output & (mo_is_f32 ? 3 : 1)) == 0, "pts_multistep_step: misaligned pointer");
    if (mo_is_f32) launch_flat<float>(model_output, sample, c_skip, c_out, a, b, c, denoised_prev, prev_sample, n, (hipStream_t)stream);
    else           launch_flat<f16>(model_output, sample, c_skip, c_out, a, b, c, denoised_prev, prev_sample, n, (hipStream_t)stream);
    PT_LAUNCH_CHECK("pts_multistep_step");
    return 0;
}
