// The windowed denoise loop's prologue and epilogue (include/posetraj_window.h) - libposetraj_window.so, a library of its own: no
// symbol of libposetraj_hip.so is used (pt_common.h for the vector types only).  Both passes are HBM-bound and follow
// scale_concat_kernel (elementwise.hip) / cfg_multistep_kernel (sampler.hip): one thread per latent pixel, the 8 (4) channels of a
// pixel as one 16-byte access, the planar fp32 tensors coalesced across the pixels of a wave, grid-strided, 64-bit indices.  The
// window starts are a kernel argument (K <= 64 values by value): indexed by a wave-uniform k they are scalar loads from the kernel's
// argument segment, no table in device memory and nothing to upload per call.
#include "pt_common.h"
#include "../../include/posetraj_window.h"

#include <stdarg.h>

#include <cmath>

namespace {

constexpr int MAX_WINDOWS = 64;
struct Starts { int32_t v[MAX_WINDOWS]; };

thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define PTW_CHECK(cond, ...)          \
    do {                              \
        if (!(cond)) {                \
            set_error(__VA_ARGS__);   \
            return 1;                 \
        }                             \
    } while (0)

// blockIdx.y = window k (uniform: its start is one scalar load); a thread reads the 4 latent channels of pixel (j, p) once and writes
// the pixel of both halves, 16 bytes each.
__global__ __launch_bounds__(256) void scale_concat_windows_kernel(const float* __restrict__ lat, const f16* __restrict__ img, float inv,
                                                                   Starts starts, int K, int Fw, int HW, f16* __restrict__ out,
                                                                   int64_t pix_per_window) {
    const int k = blockIdx.y;
    const int64_t f0 = starts.v[k];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pix_per_window; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const int64_t j = i / HW;
        // The pixel of the uncond half is built by scale_concat_kernel's own statements (elementwise.hip): the product's rounding to
        // fp16 is then the compiler's choice there too (it fuses the product and the conversion of some channels into one rounding,
        // v_fma_mix, and keeps two roundings for the others), and the rows agree with that kernel's bit for bit.
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[c] = (f16)(lat[((f0 + j) * 4 + c) * HW + p] * inv);
            o[4 + c] = img[(int64_t)c * HW + p];
        }
        *(f16x8*)(out + ((int64_t)k * pix_per_window + i) * 8) = o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[4 + c] = img[(int64_t)(4 + c) * HW + p];
        *(f16x8*)(out + ((int64_t)(K + k) * pix_per_window + i) * 8) = o;
    }
}

// guided prediction of one channel, the arithmetic of guided<T> in sampler.hip: difference, product, sum - three roundings; fp16
// predictions round the result to fp16
template <typename T>
__device__ __forceinline__ float guided(float pu, float pc, float g) {
#pragma clang fp contract(off)
    const float d = pc - pu;
    const float gd = g * d;
    const float mo = pu + gd;
    return sizeof(T) == 2 ? (float)(f16)mo : mo;
}

__device__ __forceinline__ float blend(float acc, float wt, float mo, bool first) {
#pragma clang fp contract(off)
    const float term = wt * mo;
    return first ? term : acc + term;
}

template <typename T> struct vec4;
template <> struct vec4<float> { typedef f32x4 type; };
template <> struct vec4<f16> { typedef f16x4 type; };

// One thread per pixel (f, p) of the LONG video; the covering windows in ascending k (the starts ascend: the loop ends at the first
// window that begins beyond f).  VEC: the 4 channels of a prediction pixel are one aligned vector (the host decides).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cfg_window_merge_kernel(const T* __restrict__ pred, int ldn, const float* __restrict__ guidance,
                                                               const float* __restrict__ weights, Starts starts, int K, int Fw, int HW,
                                                               float* __restrict__ out, int64_t total_pix) {
    typedef typename vec4<T>::type V;
    const int64_t half = (int64_t)K * Fw * HW;                                          // pixels of one CFG half
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_pix; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const int f = (int)(i / HW);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        bool first = true;
        for (int k = 0; k < K; ++k) {
            const int s = starts.v[k];
            if (s > f) break;
            const int j = f - s;
            if (j >= Fw) continue;
            const int64_t pix = ((int64_t)k * Fw + j) * HW + p;
            const T* u = pred + pix * ldn;                                              // uncond half
            const T* cd = pred + (half + pix) * ldn;                                    // cond half
            const float g = guidance[j], wt = weights[k * Fw + j];
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
            for (int ch = 0; ch < 4; ++ch) acc[ch] = blend(acc[ch], wt, guided<T>(pu[ch], pc[ch], g), first);
            first = false;
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) out[((int64_t)f * 4 + ch) * HW + p] = acc[ch];
    }
}

unsigned grid_for(int64_t n) {                               // 256 CUs x 16 workgroups; the elements beyond are grid-strided
    int64_t b = (n + 255) / 256;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// The plan's rules (posetraj_amd/windows.py: window_plan) on the HOST table; every frame of 0 .. Ft - 1 is covered when they hold.
int check_plan(const char* who, const int32_t* starts, int K, int Fw, int Ft, int h, int w, Starts& by_value) {
    PTW_CHECK(starts, "%s: null pointer (starts)", who);
    PTW_CHECK(K >= 1 && K <= MAX_WINDOWS, "%s: K = %d windows, need 1 .. %d", who, K, MAX_WINDOWS);
    PTW_CHECK(Fw >= 1 && Ft >= Fw, "%s: bad frame counts (Fw=%d Ft=%d), need 1 <= Fw <= Ft", who, Fw, Ft);
    PTW_CHECK(h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31) && (int64_t)Ft * h * w < ((int64_t)1 << 40) &&
              (int64_t)K * Fw * h * w < ((int64_t)1 << 40), "%s: bad sizes (K=%d Fw=%d Ft=%d h=%d w=%d)", who, K, Fw, Ft, h, w);
    PTW_CHECK(starts[0] == 0, "%s: starts[0] = %d, the first window begins at frame 0", who, starts[0]);
    for (int k = 1; k < K; ++k)
        PTW_CHECK(starts[k] > starts[k - 1] && starts[k] - starts[k - 1] <= Fw,
                  "%s: starts[%d] = %d after %d: windows ascend by 1 .. Fw = %d frames (no gap)", who, k, starts[k], starts[k - 1], Fw);
    PTW_CHECK(starts[K - 1] == Ft - Fw, "%s: starts[%d] = %d, the last window ends on the last frame (Ft - Fw = %d)", who, K - 1,
              starts[K - 1], Ft - Fw);
    for (int k = 0; k < MAX_WINDOWS; ++k) by_value.v[k] = k < K ? starts[k] : 0;
    return 0;
}

int launch_failed(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    set_error("%s: launch failed: %s", who, hipGetErrorString(e));
    return 2;
}

}  // namespace

extern "C" int ptw_abi_version(void) { return PT_WINDOW_ABI_VERSION; }

extern "C" const char* ptw_last_error(void) { return g_err; }

extern "C" int ptw_scale_concat_windows(const float* latents, const void* image_latents, float sigma, const int32_t* starts, int32_t K,
                                        int32_t Fw, int32_t Ft, int32_t h, int32_t w, void* out, void* stream) {
    const char* who = "ptw_scale_concat_windows";
    PTW_CHECK(latents && image_latents && out, "%s: null pointer", who);
    Starts sv;
    if (check_plan(who, starts, K, Fw, Ft, h, w, sv)) return 1;
    PTW_CHECK(std::isfinite(sigma), "%s: non-finite sigma", who);
    PTW_CHECK(((uintptr_t)latents & 3) == 0 && ((uintptr_t)image_latents & 1) == 0 && ((uintptr_t)out & 15) == 0, "%s: misaligned pointer", who);
    const int64_t per_window = (int64_t)Fw * h * w;
    const float inv = 1.0f / sqrtf(sigma * sigma + 1.0f);
    unsigned gx = grid_for(per_window);
    if (gx > 256u * 16u / (unsigned)K) gx = 256u * 16u / (unsigned)K;                   // K rows of blocks: the same total as a flat grid
    hipLaunchKernelGGL(scale_concat_windows_kernel, dim3(gx, (unsigned)K), dim3(256), 0, (hipStream_t)stream, latents,
                       (const f16*)image_latents, inv, sv, K, Fw, h * w, (f16*)out, per_window);
    return launch_failed(who);
}

extern "C" int ptw_cfg_window_merge(const void* pred, int32_t pred_is_f32, int32_t ldn, const float* guidance, const float* weights,
                                    const int32_t* starts, int32_t K, int32_t Fw, int32_t Ft, int32_t h, int32_t w, float* out,
                                    void* stream) {
    const char* who = "ptw_cfg_window_merge";
    PTW_CHECK(pred && guidance && weights && out, "%s: null pointer", who);
    PTW_CHECK(ldn >= 4, "%s: ldn %d < 4 (the prediction's 4 latent channels)", who, ldn);
    Starts sv;
    if (check_plan(who, starts, K, Fw, Ft, h, w, sv)) return 1;
    PTW_CHECK(((uintptr_t)guidance & 3) == 0 && ((uintptr_t)weights & 3) == 0 && ((uintptr_t)out & 3) == 0 &&
              ((uintptr_t)pred & (pred_is_f32 ? 3 : 1)) == 0, "%s: misaligned pointer", who);
    const int64_t total = (int64_t)Ft * h * w;
    const size_t esz = pred_is_f32 ? 4 : 2;
    const bool vec = ldn % 4 == 0 && ((uintptr_t)pred & (4 * esz - 1)) == 0;
    const dim3 grid(grid_for(total)), block(256);
#define PTW_LAUNCH(T, VEC)                                                                                                            \
    hipLaunchKernelGGL((cfg_window_merge_kernel<T, VEC>), grid, block, 0, (hipStream_t)stream, (const T*)pred, ldn, guidance, weights, \
                       sv, K, Fw, h * w, out, total)
    if (pred_is_f32) { if (vec) PTW_LAUNCH(float, true); else PTW_LAUNCH(float, false); }
    else             { if (vec) PTW_LAUNCH(f16, true); else PTW_LAUNCH(f16, false); }
#undef PTW_LAUNCH
    return launch_failed(who);
}
