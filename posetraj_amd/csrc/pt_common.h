// Shared helpers for the gfx950 kernels of libposetraj_hip.so.  CDNA4 only: wave64, MFMA, LDS-DMA.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "../../include/posetraj_hip.h"

typedef _Float16 f16;
typedef f16   f16x2 __attribute__((ext_vector_type(2)));
typedef f16   f16x4 __attribute__((ext_vector_type(4)));
typedef f16   f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define PT_WAVE 64

void pt_set_error(const char* fmt, ...);
const void* pt_zero_page();      // the current device's zero page (nullptr until pt_set_zero_page ran on it)
int pt_device();                 // current HIP device, clamped to the per-device tables' range

#define PT_CHECK(cond, ...)                 \
    do {                                    \
        if (!(cond)) {                      \
            pt_set_error(__VA_ARGS__);      \
            return 1;                       \
        }                                   \
    } while (0)

#define PT_LAUNCH_CHECK(name)                                                       \
    do {                                                                            \
        hipError_t e__ = hipGetLastError();                                         \
        if (e__ != hipSuccess) {                                                    \
            pt_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));    \
            return 2;                                                               \
        }                                                                           \
    } while (0)

// ---- profiling hooks (api.hip); families: 0 igemm, 1 spatial attention, 2 pt_gemm_f16 (training)
constexpr int PT_PROF_IGEMM = 0, PT_PROF_ATTN = 1, PT_PROF_GEMM = 2, PT_PROF_FAMILIES = 3;
void pt_prof_begin(int family, hipStream_t s, double flops);
void pt_prof_end(int family, hipStream_t s);

// ---- device helpers
// x * sigmoid(x) with v_exp_f32 + v_rcp_f32 (1 ulp each): an IEEE fp32 division would cost ~10 more instructions per value,
// which made the GroupNorm apply pass VALU-bound; outputs are rounded to fp16 (11 bits) anyway
__device__ __forceinline__ float pt_silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f));
}

// d silu(z) / dz of the training step's reverse pass (GroupNorm + SiLU backward, pt_silu_bwd), IEEE division
__device__ __forceinline__ float pt_sigmoid(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float pt_dsilu(float z) { const float s = pt_sigmoid(z); return s * (1.0f + z * (1.0f - s)); }

// A scalar that a kernel takes as a launch argument or (DEV) from device memory, read once before its loop: a captured launch
// (the training step as a hipGraph) cannot take a host float that changes every step.  pt_scalar_arg<DEV> is the parameter's type
// (`__restrict__` like the kernel's other pointers: without it lerp_kernel<true> compiles to a different instruction stream).
template <bool DEV> using pt_scalar_arg = std::conditional_t<DEV, const float* __restrict__, float>;
__device__ __forceinline__ float pt_scalar(float v) { return v; }
__device__ __forceinline__ float pt_scalar(const float* p) { return *p; }

// erf-GELU.  With z = |x| / sqrt(2):  gelu(x) = x * Phi(x) = relu(x) - (|x| / 2) * erfc(z), and
//   erfc(z) ~= 2^(-z (c1 + c2 z + c3 z^2 + c4 z^3 + c5 z^4))
// (weighted minimax fit on [0, 4.2], tools/fit_gelu.py; the exponent keeps growing beyond, so erfc -> 0 without a
// clamp): |erf error| <= 6.3e-7, |gelu error| <= 1.1e-6 evaluated in fp32 - far below the fp16 output's 5e-4.
// 9 plain VALU + 1 transcendental, no reciprocal and no sign fix-up (Abramowitz-Stegun 7.1.26 needed 13 + 2, libm
// erff ~40 with a branch): the GEGLU epilogue of the K = 320 feed-forward GEMMs costs as much as their main loop.
// pt_gelu_erf2 does two values with the polynomial in packed fp32 (v_pk_fma_f32 / v_pk_mul_f32).
// relu(x) is written (x + |x|) / 2 - exact in fp32, so the same value as fmaxf(x, 0) - because fmaxf() on a value that comes out of
// an MFMA costs TWO instructions (hipcc first quiets a possible signalling NaN: `v_max_f32 x, x, x`; an fmed3 builtin is folded
// back to the same pair) and the kernels that run this are bound by instruction count (energy): 4 -> 2 instructions per
// pair of values in the packed form.
__device__ __forceinline__ float pt_gelu_erf(float x) {
    const float ax = fabsf(x);
    const float z = ax * 0.70710678118654752f;
    float q = 0.00294415708f;
    q = q * z - 0.0295900398f;
    q = q * z + 0.148665627f;
    q = q * z + 0.918509366f;
    q = q * z + 1.62788901f;
    const float e = __builtin_amdgcn_exp2f(-(q * z));
    return (x + ax) * 0.5f - 0.5f * ax * e;
}
__device__ __forceinline__ f32x2 pt_gelu_erf2(f32x2 x) {
    f32x2 ax; ax[0] = fabsf(x[0]); ax[1] = fabsf(x[1]);
    const f32x2 z = ax * 0.70710678118654752f;
    f32x2 q = z * 0.00294415708f - 0.0295900398f;
    q = q * z + 0.148665627f;
    q = q * z + 0.918509366f;
    q = q * z + 1.62788901f;
    const f32x2 pz = q * z;
    f32x2 e; e[0] = __builtin_amdgcn_exp2f(-pz[0]); e[1] = __builtin_amdgcn_exp2f(-pz[1]);
    const f32x2 r = (x + ax) * 0.5f;
    return r - (ax * 0.5f) * e;
}

// async 16-byte global -> LDS copy (LDS-DMA).  `lds_wave_base` must be wave-uniform; lane i lands at base + 16*i.
__device__ __forceinline__ void pt_glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// 4-byte variant: lane i lands at base + 4*i.  Used as a cache-line touch (L2 prefetch with no register destination).
__device__ __forceinline__ void pt_glds4(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

// s_waitcnt immediates.  gfx9 layout: vmcnt in bits 3:0 and 15:14 (0 .. 63), expcnt in 6:4, lgkmcnt in 11:8 (0 .. 15); a counter
// left at its maximum is not waited for.  pt_vmcnt(n) / pt_lgkmcnt(n) wait for one counter and leave the others untouched.
constexpr int pt_waitcnt(int vm, int lgkm) { return (vm & 15) | ((vm >> 4) << 14) | 0x0070 | (lgkm << 8); }
constexpr int pt_vmcnt(int n) { return pt_waitcnt(n, 15); }
constexpr int pt_lgkmcnt(int n) { return pt_waitcnt(63, n); }
static_assert(pt_vmcnt(0) == 0x0F70 && pt_vmcnt(6) == 0x0F76 && pt_vmcnt(15) == 0x0F7F && pt_vmcnt(17) == 0x4F71, "vmcnt encoding");
static_assert(pt_lgkmcnt(0) == 0xC07F && pt_lgkmcnt(8) == 0xC87F && pt_waitcnt(9, 0) == 0x0079, "lgkmcnt encoding");

// ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block of halfs, delivered column-major
__device__ __forceinline__ f16x4 pt_lds_tr16(const void* p) {
    typedef __fp16 hw_f16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    const hw_f16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) hw_f16x4*)p);
    return __builtin_bit_cast(f16x4, v);
}

// Cross-lane exchanges without LDS: v_permlane32_swap exchanges the upper half of its first operand with the lower half of its
// second (v_permlane16_swap: odd rows of 16 lanes with even rows), so with both operands holding v the two registers hold
// {own, partner's} in every lane.  Written as inline asm: through __builtin_amdgcn_permlane32_swap hipcc (ROCm 7.2) used result 0
// for both elements of the returned pair (max(r0, r1) compiled to r0 - every lane silently kept only the LOWER lane's value).
// The s_nop covers the VALU-write -> permlane-read hazard (2 wait states) inside the statement.  T: any 32-bit register type.
template <class T>
__device__ __forceinline__ void pt_swap32(T& a, T& b) {                // a's upper 32 lanes <-> b's lower 32 lanes
    static_assert(sizeof(T) == 4, "one VGPR");
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
template <class T>
__device__ __forceinline__ void pt_swap16(T& a, T& b) {                // rows of 16 lanes: a's odd rows <-> b's even rows
    static_assert(sizeof(T) == 4, "one VGPR");
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

__device__ __forceinline__ float pt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// GroupNorm statistics are sums of x - P_g, not of x: E[x^2] - mean^2 from fp32 sums cancels to nothing once |mean| / sigma
// reaches ~100 (an fp16 activation at 300 sigma carries no variance in fp32 sums of its squares).  The pivot P_g of a group is
// its first element, x[sample, row 0, first channel of the group] - one fp16 value that every block of every pass reads alike;
// then mean = P_g + S / n and var = Q / n - (S / n)^2 with S, Q of the order of sigma (tests/test_norm_numerics_gpu.py).
// x0 [.., C0] and x1 [.., C1] are the two sources of a concatenation (channel ch of the group may lie in either).
__device__ __forceinline__ float pt_gn_pivot(const f16* x0, const f16* x1, int C0, int C1, int64_t rows_per_sample, int sample, int ch) {
    const int64_t r = (int64_t)sample * rows_per_sample;
    return ch < C0 ? (float)x0[r * C0 + ch] : (float)x1[r * C1 + (ch - C0)];
}

// XCD-aware bijective remap of a linear workgroup id: workgroups that share an XCD (id % 8 equal under the
// round-robin dispatch) get a contiguous chunk of the tile space, so neighbouring tiles hit the same L2.
__device__ __forceinline__ int pt_xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}
