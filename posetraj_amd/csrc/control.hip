// Spatial control weights (include/posetraj_control.h): a ControlNet zero-conv's fp32 output t [rows, C] is accumulated into the
// U-Net's fp16 skip y with one factor per row - (frame, pixel) - read from device memory:  y = fp16((scale w[r]) t + (y + y_lo)).
// The pipeline's plain steps keep this add in the igemm tail (one scalar); this pass serves denoise(control_weight=...) and per-step
// scales, where a captured graph must find the factors in a buffer.  HBM-bound: 48 + 16 (+ 16) bytes per 8 channels, 16-byte lanes,
// a group of lanes per row segment, w[r] read once per row and lane, rows grid-strided.
#include "pt_common.h"
#include "../../include/posetraj_control.h"

namespace {

// The operation order of igemm_tail.h's res_post tail (x = acc; x *= out_scale; rs = res + res_lo; x += rs; one rounding), every
// step rounded to fp32 on its own: equal to plain fp32 tensor arithmetic bit for bit (tests/test_control_schedule_gpu.py).  Plain
// operators under `fp contract(off)`: the rounding intrinsics (__fmul_rn, ...) are inlined WITH their header's contraction and end
// up in a v_fma all the same.
__device__ __forceinline__ f16x8 accumulate8(const f32x4& t0, const f32x4& t1, float k, const f16x8& y, const f16x8& lo, bool has_lo) {
#pragma clang fp contract(off)
    const float t[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x = t[j] * k;
        float rs = (float)y[j];
        if (has_lo) rs = rs + (float)lo[j];
        const float s = x + rs;
        o[j] = (f16)s;
    }
    return o;
}

// thread = (row slot tid / L, lane tid % L of the row's group); L a power of two <= 64, CH = C / 8 chunks of 8 channels per row
__global__ __launch_bounds__(256) void weighted_residual_add_kernel(const float* __restrict__ t, int64_t ldt, const float* __restrict__ w, float scale,
                                                                    f16* y, const f16* __restrict__ y_lo, int64_t ldy, int64_t rows, int CH, int L) {
#pragma clang fp contract(off)
    const int rpb = 256 / L, lane = threadIdx.x & (L - 1);
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + threadIdx.x / L; r < rows; r += stride) {
        const float k = scale * w[r];
        const float* tr = t + (size_t)r * ldt;
        f16* yr = y + (size_t)r * ldy;
        const f16* lr = y_lo ? y_lo + (size_t)r * ldy : nullptr;
        for (int c = lane; c < CH; c += L) {
            const f32x4 t0 = *(const f32x4*)(tr + c * 8), t1 = *(const f32x4*)(tr + c * 8 + 4);
            const f16x8 yv = *(const f16x8*)(yr + c * 8);
            f16x8 lv = {};
            if (lr) lv = *(const f16x8*)(lr + c * 8);
            *(f16x8*)(yr + c * 8) = accumulate8(t0, t1, k, yv, lv, lr != nullptr);
        }
    }
}

// lanes per row: the largest power of two that divides CH (no idle lane in any pass), 64 at most; rows of an odd chunk count still
// get up to 8 lanes (the last pass of a row then idles some)
inline int lanes_per_row(int CH) {
    int L = 1;
    while (L < 64 && CH % (2 * L) == 0) L *= 2;
    while (L < 8 && L < CH) L *= 2;
    return L;
}

}  // namespace

extern "C" int ptc_abi_version(void) { return PT_CONTROL_ABI_VERSION; }

extern "C" int ptc_weighted_residual_add_f16(const float* t, int64_t ldt, const float* w, float scale, void* y, const void* y_lo, int64_t ldy,
                                             int64_t rows, int32_t Cc, void* stream) {
    PT_CHECK(t && w && y, "ptc_weighted_residual_add_f16: null pointer");
    PT_CHECK(rows > 0 && rows < ((int64_t)1 << 40) && Cc > 0 && Cc % 8 == 0, "ptc_weighted_residual_add_f16: bad sizes (rows=%lld C=%d: C %% 8 == 0)",
             (long long)rows, Cc);
    PT_CHECK(ldt >= Cc && ldy >= Cc && ldt % 8 == 0 && ldy % 8 == 0 && ldt < ((int64_t)1 << 31) && ldy < ((int64_t)1 << 31),
             "ptc_weighted_residual_add_f16: bad pitches (ldt=%lld ldy=%lld C=%d: >= C, multiples of 8)", (long long)ldt, (long long)ldy, Cc);
    PT_CHECK(((uintptr_t)t & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)y_lo & 15) == 0 && ((uintptr_t)w & 3) == 0,
             "ptc_weighted_residual_add_f16: t / y / y_lo must be 16-byte aligned (w 4-byte)");
    const int CH = Cc / 8, L = lanes_per_row(CH), rpb = 256 / L;
    int64_t blocks = (rows + rpb - 1) / rpb;
    if (blocks > 2048) blocks = 2048;                        // 256 CUs x 8 workgroups; the rows beyond are grid-strided
    hipLaunchKernelGGL(weighted_residual_add_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t, ldt, w, scale, (f16*)y,
                       (const f16*)y_lo, ldy, rows, CH, L);
    PT_LAUNCH_CHECK("ptc_weighted_residual_add_f16");
    return 0;
}
