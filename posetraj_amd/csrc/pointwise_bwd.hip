// Pointwise passes of the ControlNet training step's tape: what the reverse pass - and the forward pass it replays -
// needs that is neither a matrix product nor a reduction across workgroups (those are norm_bwd.hip): softmax rows of the attention
// backward, GEGLU, SiLU, the AlphaBlender's blend, the resampling gradients, the EDM loss gradient.  HBM-bound, 16-byte lanes.
#include "pt_common.h"
#include "pt_launch.h"

namespace {

// ------------------------------------------------------------------------------------------ softmax rows (attention backward)
// one wave per row of n fp32 scores (already scaled): P = softmax(S) as fp16;  dS = P (dP - sum_j P_j dP_j) as fp16.
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, int64_t rows, int n, int64_t ld, f16* __restrict__ P,
                                                           int64_t ldp) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* s = S + r * ld;
    float m = -3.0e38f;
    for (int j = lane; j < n; j += 64) m = fmaxf(m, s[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float z = 0.f;
    for (int j = lane; j < n; j += 64) z += __expf(s[j] - m);
    z = pt_wave_sum(z);
    const float inv = 1.0f / z;
    for (int j = lane; j < n; j += 64) P[r * ldp + j] = (f16)(__expf(s[j] - m) * inv);
}

__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const f16* __restrict__ P, int64_t ldp, const float* __restrict__ dP, int64_t ld,
                                                               int64_t rows, int n, f16* __restrict__ dS, int64_t lds_) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float dot = 0.f;
    for (int j = lane; j < n; j += 64) dot += (float)P[r * ldp + j] * dP[r * ld + j];
    dot = pt_wave_sum(dot);
    for (int j = lane; j < n; j += 64) dS[r * lds_ + j] = (f16)((float)P[r * ldp + j] * (dP[r * ld + j] - dot));
}

// ------------------------------------------------------------------------------------------ element-wise
__device__ __forceinline__ float gelu_erf_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_erf(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) + x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// GEGLU (diffusers GEGLU.forward: hidden, gate = proj.chunk(2, -1); hidden * gelu(gate)): h [M, 2 I] -> y [M, I]
__global__ __launch_bounds__(256) void geglu_kernel(const f16* __restrict__ h, int64_t M, int I, f16* __restrict__ y) {
    const int64_t n8 = M * (I >> 3);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / (I >> 3);
        const int c = (int)(i % (I >> 3)) * 8;
        const f16x8 v = *(const f16x8*)(h + r * 2 * I + c), g = *(const f16x8*)(h + r * 2 * I + I + c);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)v[j] * pt_gelu_erf((float)g[j]));
        *(f16x8*)(y + r * I + c) = o;
    }
}

__global__ __launch_bounds__(256) void geglu_bwd_kernel(const f16* __restrict__ h, const f16* __restrict__ dy, int64_t M, int I,
                                                        f16* __restrict__ dh) {
    const int64_t n8 = M * (I >> 3);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / (I >> 3);
        const int c = (int)(i % (I >> 3)) * 8;
        const f16x8 v = *(const f16x8*)(h + r * 2 * I + c), g = *(const f16x8*)(h + r * 2 * I + I + c), d = *(const f16x8*)(dy + r * I + c);
        f16x8 dv, dg;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float gj = (float)g[j], dj = (float)d[j];
            dv[j] = (f16)(dj * gelu_erf_exact(gj));
            dg[j] = (f16)(dj * (float)v[j] * dgelu_erf(gj));
        }
        *(f16x8*)(dh + r * 2 * I + c) = dv;
        *(f16x8*)(dh + r * 2 * I + I + c) = dg;
    }
}

__global__ __launch_bounds__(256) void silu_bwd_kernel(const f16* __restrict__ x, const f16* __restrict__ dy, int64_t n, f16* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dx[i] = (f16)((float)dy[i] * pt_dsilu((float)x[i]));
}

// out = alpha a + (1 - alpha) b      (AlphaBlender with the clip-wide scalar alpha = sigmoid(mix_factor), which
// sigmoid_gather_kernel leaves in device memory: DEV)
template <bool DEV>
__global__ __launch_bounds__(256) void lerp_kernel(const f16* __restrict__ a, const f16* __restrict__ b, pt_scalar_arg<DEV> alpha_arg, int64_t n8,
                                                   f16* __restrict__ out) {
    const float alpha = pt_scalar(alpha_arg);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const f16x8 x = *(const f16x8*)(a + i * 8), y = *(const f16x8*)(b + i * 8);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)(alpha * (float)x[j] + (1.0f - alpha) * (float)y[j]);
        *(f16x8*)(out + i * 8) = o;
    }
}

// y = k x (one_minus = 0) or (1 - k) x (one_minus = 1), k from device memory
__global__ __launch_bounds__(256) void scale_dev_kernel(const f16* __restrict__ x, const float* __restrict__ k_p, int one_minus, int64_t n8,
                                                        f16* __restrict__ y) {
    const float k = one_minus ? 1.0f - *k_p : *k_p;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const f16x8 v = *(const f16x8*)(x + i * 8);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)v[j] * k);
        *(f16x8*)(y + i * 8) = o;
    }
}

// out[i] = sigmoid(flat[idx[i]]): every AlphaBlender weight of the trainable network in one launch
__global__ __launch_bounds__(256) void sigmoid_gather_kernel(const float* __restrict__ flat, const int64_t* __restrict__ idx, int n,
                                                             float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 1.0f / (1.0f + expf(-flat[idx[i]]));
}

// y[r, :] = x[r, :] + vec[r / rows_per_vec, :]
__global__ __launch_bounds__(256) void add_rowvec_kernel(const f16* __restrict__ x, const f16* __restrict__ vec, int64_t rows, int C,
                                                         int64_t rows_per_vec, f16* __restrict__ y) {
    const int CH = C >> 3;
    const int64_t n8 = rows * CH;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / CH;
        const int c = (int)(i % CH) * 8;
        const f16x8 a = *(const f16x8*)(x + r * C + c), v = *(const f16x8*)(vec + (r / rows_per_vec) * C + c);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)((float)a[j] + (float)v[j]);
        *(f16x8*)(y + r * C + c) = o;
    }
}

// backward of nearest 2x upsampling: dx[n, y, x, :] = sum of the 2 x 2 block of du [n, 2H, 2W, C]
__global__ __launch_bounds__(256) void sumpool2x_kernel(const f16* __restrict__ du, int N, int H, int W, int C, f16* __restrict__ dx) {
    const int CH = C >> 3;
    const int64_t n8 = (int64_t)N * H * W * CH;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % CH) * 8;
        int64_t p = i / CH;
        const int xx = (int)(p % W); p /= W;
        const int yy = (int)(p % H);
        const int64_t n = p / H;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int dy_ = 0; dy_ < 2; ++dy_)
#pragma unroll
            for (int dx_ = 0; dx_ < 2; ++dx_) {
                const f16x8 v = *(const f16x8*)(du + (((n * 2 * H + 2 * yy + dy_) * 2 * W) + 2 * xx + dx_) * C + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
            }
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)acc[j];
        *(f16x8*)(dx + i * 8) = o;
    }
}

// data gradient of a stride-2 convolution = stride-1 convolution (flipped taps) over the zero-interleaved output gradient:
// z[n, 2 y, 2 x, :] = dy[n, y, x, :], zero elsewhere; z is [N, H, W, C]
__global__ __launch_bounds__(256) void zero_insert2x_kernel(const f16* __restrict__ dy, int N, int OH, int OW, int H, int W, int C,
                                                            f16* __restrict__ z) {
    const int CH = C >> 3;
    const int64_t n8 = (int64_t)N * H * W * CH;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % CH) * 8;
        int64_t p = i / CH;
        const int xx = (int)(p % W); p /= W;
        const int yy = (int)(p % H);
        const int64_t n = p / H;
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)0.f;
        if (!(yy & 1) && !(xx & 1) && (yy >> 1) < OH && (xx >> 1) < OW) o = *(const f16x8*)(dy + ((n * OH + (yy >> 1)) * OW + (xx >> 1)) * C + c);
        *(f16x8*)(z + i * 8) = o;
    }
}

// d loss / d pred of the EDM objective (pt_edm_loss) times `scale` (loss scale x the term's weight):
//   2 w c_out (pred c_out + c_skip noisy - target) / (F 4 HW) / B  -> fp16 channels-last [B, F, HW, 8] (channels 4..7 zero)
template <typename T>
__global__ __launch_bounds__(256) void edm_loss_bwd_kernel(const T* __restrict__ pred, int ldp, const float* __restrict__ noisy,
                                                           const float* __restrict__ target, const float* __restrict__ sigma, int B, int F,
                                                           int64_t HW, float scale, f16* __restrict__ dpred) {
    const int64_t total = (int64_t)B * F * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i % HW, bf = i / HW, b = bf / F;
        const float s = sigma[b], c_out = -s / sqrtf(s * s + 1.0f), c_skip = 1.0f / (s * s + 1.0f), w = (1.0f + s * s) / (s * s);
        const float k = 2.0f * w * c_out * scale / ((float)F * 4.0f * (float)HW * (float)B);
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t e = (bf * 4 + c) * HW + p;
            const float d = (float)pred[i * ldp + c] * c_out + c_skip * noisy[e] - target[e];
            o[c] = (f16)(k * d);
            o[4 + c] = (f16)0.f;
        }
        *(f16x8*)(dpred + i * 8) = o;
    }
}

}  // namespace

extern "C" int pt_softmax_rows(const float* S, int64_t rows, int32_t n, int64_t ld, void* P, int64_t ldp, void* stream) {
    PT_CHECK(S && P && rows > 0 && n > 0 && ld >= n && ldp >= n, "pt_softmax_rows: bad arguments");
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S, rows, n, ld, (f16*)P, ldp);
    PT_LAUNCH_CHECK("pt_softmax_rows");
    return 0;
}

extern "C" int pt_softmax_bwd_rows(const void* P, int64_t ldp, const float* dP, int64_t ld, int64_t rows, int32_t n, void* dS, int64_t lds,
                                   void* stream) {
    PT_CHECK(P && dP && dS && rows > 0 && n > 0 && ld >= n && ldp >= n && lds >= n, "pt_softmax_bwd_rows: bad arguments");
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f16*)P, ldp, dP, ld, rows,
                       n, (f16*)dS, lds);
    PT_LAUNCH_CHECK("pt_softmax_bwd_rows");
    return 0;
}

extern "C" int pt_geglu_f16(const void* h, int64_t M, int32_t I, void* y, void* stream) {
    PT_CHECK(h && y && M > 0 && I > 0 && I % 8 == 0, "pt_geglu_f16: bad arguments");
    return launch_ew("pt_geglu_f16", geglu_kernel, M * (I / 8), stream, (const f16*)h, M, I, (f16*)y);
}

extern "C" int pt_geglu_bwd(const void* h, const void* dy, int64_t M, int32_t I, void* dh, void* stream) {
    PT_CHECK(h && dy && dh && M > 0 && I > 0 && I % 8 == 0, "pt_geglu_bwd: bad arguments");
    return launch_ew("pt_geglu_bwd", geglu_bwd_kernel, M * (I / 8), stream, (const f16*)h, (const f16*)dy, M, I, (f16*)dh);
}

extern "C" int pt_silu_bwd(const void* x, const void* dy, int64_t n, void* dx, void* stream) {
    PT_CHECK(x && dy && dx && n > 0, "pt_silu_bwd: bad arguments");
    return launch_ew("pt_silu_bwd", silu_bwd_kernel, n, stream, (const f16*)x, (const f16*)dy, n, (f16*)dx);
}

extern "C" int pt_lerp_f16(const void* a, const void* b, float alpha, int64_t n, void* out, void* stream) {
    PT_CHECK(a && b && out && n > 0 && n % 8 == 0, "pt_lerp_f16: bad arguments");
    return launch_ew("pt_lerp_f16", lerp_kernel<false>, n / 8, stream, (const f16*)a, (const f16*)b, alpha, n / 8, (f16*)out);
}

extern "C" int pt_lerp_f16_dev(const void* a, const void* b, const float* alpha_dev, int64_t n, void* out, void* stream) {
    PT_CHECK(a && b && out && alpha_dev && n > 0 && n % 8 == 0, "pt_lerp_f16_dev: bad arguments");
    return launch_ew("pt_lerp_f16_dev", lerp_kernel<true>, n / 8, stream, (const f16*)a, (const f16*)b, alpha_dev, n / 8, (f16*)out);
}

extern "C" int pt_scale_f16_dev(const void* x, const float* k_dev, int32_t one_minus, int64_t n, void* y, void* stream) {
    PT_CHECK(x && y && k_dev && n > 0 && n % 8 == 0, "pt_scale_f16_dev: bad arguments");
    return launch_ew("pt_scale_f16_dev", scale_dev_kernel, n / 8, stream, (const f16*)x, k_dev, one_minus, n / 8, (f16*)y);
}

extern "C" int pt_sigmoid_gather_f32(const float* flat, const int64_t* idx, int32_t n, float* out, void* stream) {
    PT_CHECK(flat && idx && out && n > 0, "pt_sigmoid_gather_f32: bad arguments");
    hipLaunchKernelGGL(sigmoid_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, flat, idx, n, out);
    PT_LAUNCH_CHECK("pt_sigmoid_gather_f32");
    return 0;
}

extern "C" int pt_add_rowvec_f16(const void* x, const void* vec, int64_t rows, int32_t Cc, int64_t rows_per_vec, void* y, void* stream) {
    PT_CHECK(x && vec && y && rows > 0 && Cc > 0 && Cc % 8 == 0 && rows_per_vec > 0, "pt_add_rowvec_f16: bad arguments");
    return launch_ew("pt_add_rowvec_f16", add_rowvec_kernel, rows * (Cc / 8), stream, (const f16*)x, (const f16*)vec, rows, Cc, rows_per_vec, (f16*)y);
}

extern "C" int pt_sumpool2x_f16(const void* du, int32_t N, int32_t H, int32_t W, int32_t Cc, void* dx, void* stream) {
    PT_CHECK(du && dx && N > 0 && H > 0 && W > 0 && Cc > 0 && Cc % 8 == 0, "pt_sumpool2x_f16: bad arguments");
    return launch_ew("pt_sumpool2x_f16", sumpool2x_kernel, (int64_t)N * H * W * (Cc / 8), stream, (const f16*)du, N, H, W, Cc, (f16*)dx);
}

extern "C" int pt_zero_insert2x_f16(const void* dy, int32_t N, int32_t OH, int32_t OW, int32_t H, int32_t W, int32_t Cc, void* z, void* stream) {
    PT_CHECK(dy && z && N > 0 && OH > 0 && OW > 0 && H > 0 && W > 0 && Cc > 0 && Cc % 8 == 0, "pt_zero_insert2x_f16: bad arguments");
    return launch_ew("pt_zero_insert2x_f16", zero_insert2x_kernel, (int64_t)N * H * W * (Cc / 8), stream, (const f16*)dy, N, OH, OW, H, W, Cc, (f16*)z);
}

extern "C" int pt_edm_loss_bwd(const void* pred, int32_t pred_is_f32, int32_t ldp, const float* noisy, const float* target, const float* sigma,
                               int32_t B, int32_t F, int64_t HW, float scale, void* dpred, void* stream) {
    PT_CHECK(pred && noisy && target && sigma && dpred, "pt_edm_loss_bwd: null pointer");
    PT_CHECK(B > 0 && F > 0 && HW > 0 && ldp >= 4, "pt_edm_loss_bwd: bad sizes");
    const int64_t n = (int64_t)B * F * HW;
    if (pred_is_f32) return launch_ew("pt_edm_loss_bwd", edm_loss_bwd_kernel<float>, n, stream, (const float*)pred, ldp, noisy, target, sigma, B, F, HW, scale, (f16*)dpred);
    return launch_ew("pt_edm_loss_bwd", edm_loss_bwd_kernel<f16>, n, stream, (const f16*)pred, ldp, noisy, target, sigma, B, F, HW, scale, (f16*)dpred);
}
