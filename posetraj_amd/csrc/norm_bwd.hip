// Backward kernels of the ControlNet training step (scripts/train_svd_traj_VIPSeg_14.py:1414-1425:
// `accelerator.backward(loss)`, `optimizer.step()`) that REDUCE ACROSS WORKGROUPS, each with its deterministic twin
// (include/posetraj_det.h): GroupNorm and LayerNorm backward, segmented column sums, the blend weight's gradient, the gradient norm.
// (The matrix products of the reverse pass are pt_igemm_f16 with a transposed pack - data gradients - and pt_gemm_f16 - weight
// gradients and attention; the passes that reduce nothing are pointwise_bwd.hip, the optimizer is optim.hip.)
// HBM-bound passes over channels-last fp16 activations with fp32 statistics; parameter gradients are ACCUMULATED into fp32
// buffers with atomics (the caller zeroes them once per optimizer step, so gradient accumulation over micro-batches is free).
#include "pt_common.h"
#include "../../include/posetraj_det.h"
#include "pt_fold.h"
#include "pt_launch.h"

namespace {

constexpr int TX = 32, TY = 8;           // thread (ty, tx): chunk column tx (8 channels) of a 256-channel strip, rows ty, ty + 8, ...

// fold the (ty) partials of a strip's 256 channels: red[ty][ch][2] -> out through f(channel_in_strip, a, b)
template <typename F>
__device__ __forceinline__ void fold_strip(float (*red)[256 * 2], const float* s, const float* q, F f) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[ty][(tx * 8 + j) * 2] = s[j]; red[ty][(tx * 8 + j) * 2 + 1] = q[j]; }
    __syncthreads();
    const int ch = threadIdx.x;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int y = 0; y < TY; ++y) { a += red[y][ch * 2]; b += red[y][ch * 2 + 1]; }
    f(ch, a, b);
}

// ------------------------------------------------------------------------------------------ GroupNorm backward
// y = silu?(xh * gamma + beta), xh = (x - mean_g) * rstd_g over the (rows_per_sample x C/groups) elements of a group.
//   g  = dy * silu'(z)                                   dgamma[c] += sum g xh      dbeta[c] += sum g
//   dx = rstd (g gamma - (s1 + xh s2) / n),  s1 = sum_group g gamma,  s2 = sum_group g gamma xh
// stat[sample][group][4] = (sum x - P_g, sum (x - P_g)^2, s1, s2) in fp32, P_g the group's pivot (pt_gn_pivot: mean = P_g + S / n).
// Three passes: MODE 0 (x statistics), MODE 1 (s1, s2 and the parameter gradients), apply.  grid (slabs, strips, samples).
// DET (ptd_groupnorm_bwd): no atomics - a block's group sums go to part_stat[slab * strips + strip][sample][group][2] (zero for the
// groups its strip does not touch), its channel sums to part_par[sample * slabs + slab][dgamma | dbeta][Ct]; pt_fold.h adds them up.
template <int MODE, bool DET>
__global__ __launch_bounds__(256) void gnb_reduce_kernel(const f16* __restrict__ x0, const f16* __restrict__ x1, int C0, int C1, int groups,
                                                         int64_t rows_per_sample, int rows_per_slab, float eps,
                                                         const f16* __restrict__ gamma, const f16* __restrict__ beta, int silu,
                                                         const f16* __restrict__ dy, float* __restrict__ stat,
                                                         float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                         float* __restrict__ part_stat, float* __restrict__ part_par) {
    __shared__ float red[TY][256 * 2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int slab = blockIdx.x, strip = blockIdx.y, sample = blockIdx.z;
    const int Ct = C0 + C1, cg = Ct / groups;
    const int c = strip * 256 + tx * 8;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (c < Ct) {
        const f16* src; int ld, co;
        if (c < C0) { src = x0; ld = C0; co = c; } else { src = x1; ld = C1; co = c - C0; }
        const int64_t r0 = (int64_t)slab * rows_per_slab;
        int64_t r1 = r0 + rows_per_slab; if (r1 > rows_per_sample) r1 = rows_per_sample;
        const int64_t row_base = (int64_t)sample * rows_per_sample;
        float mean[8], rstd[8], ga[8], be[8], pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pv[j] = pt_gn_pivot(x0, x1, C0, C1, rows_per_sample, sample, (c + j) / cg * cg);
        if (MODE == 1) {
            const double cnt = (double)rows_per_sample * cg;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int g = (c + j) / cg;
                const float* st = stat + ((int64_t)sample * groups + g) * 4;
                const double d = (double)st[0] / cnt;
                double var = (double)st[1] / cnt - d * d;
                if (var < 0.0) var = 0.0;
                mean[j] = (float)((double)pv[j] + d); rstd[j] = (float)(1.0 / sqrt(var + (double)eps));
                ga[j] = (float)gamma[c + j]; be[j] = (float)beta[c + j];
            }
        }
        for (int64_t r = r0 + ty; r < r1; r += TY) {
            const f16x8 v = *(const f16x8*)(src + (row_base + r) * ld + co);
            if (MODE == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float f = (float)v[j] - pv[j]; s[j] += f; q[j] += f * f; }
            } else {
                const f16x8 d = *(const f16x8*)(dy + (row_base + r) * Ct + c);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)v[j] - mean[j]) * rstd[j];
                    float g = (float)d[j];
                    if (silu) g *= pt_dsilu(xh * ga[j] + be[j]);
                    s[j] += g; q[j] += g * xh;
                }
            }
        }
    }
    // per-channel totals of the strip -> LDS; then one thread per (group touched by the strip, statistic) folds its channels:
    // two atomics per group and block instead of two per channel (the group sums were 10 x more contended than the rest)
    __shared__ float chan[256 * 2];
    fold_strip(red, s, q, [&](int ch, float a, float b) {
        const int cc = strip * 256 + ch;
        float wa = a, wb = b;
        if (MODE == 1 && cc < Ct) {
            const float gm = (float)gamma[cc];
            wa = gm * a; wb = gm * b;
            if (dgamma) {
                if constexpr (DET) {
                    float* pp = part_par + ((int64_t)sample * gridDim.x + slab) * 2 * Ct;
                    pp[cc] = b; pp[Ct + cc] = a;
                } else {
                    atomicAdd(dgamma + cc, b); atomicAdd(dbeta + cc, a);
                }
            }
        }
        chan[ch * 2] = cc < Ct ? wa : 0.f;
        chan[ch * 2 + 1] = cc < Ct ? wb : 0.f;
    });
    __syncthreads();
    const int c_lo = strip * 256, c_hi = (c_lo + 256 < Ct) ? c_lo + 256 : Ct;
    const int g_lo = c_lo / cg, g_hi = (c_hi - 1) / cg;
    const int ng = g_hi - g_lo + 1;
    if constexpr (DET) {
        float* ps = part_stat + (((int64_t)slab * gridDim.y + strip) * gridDim.z + sample) * 2 * groups;
        for (int i = threadIdx.x; i < 2 * groups; i += 256) {
            const int g = i >> 1, which = i & 1;
            float acc = 0.f;
            if (g >= g_lo && g <= g_hi) {
                int a0 = g * cg, a1 = a0 + cg;
                if (a0 < c_lo) a0 = c_lo;
                if (a1 > c_hi) a1 = c_hi;
                for (int ch = a0; ch < a1; ++ch) acc += chan[(ch - c_lo) * 2 + which];
            }
            ps[i] = acc;
        }
        return;
    }
    for (int i = threadIdx.x; i < 2 * ng; i += 256) {
        const int g = g_lo + (i >> 1), which = i & 1;
        int a0 = g * cg, a1 = a0 + cg;
        if (a0 < c_lo) a0 = c_lo;
        if (a1 > c_hi) a1 = c_hi;
        float acc = 0.f;
        for (int ch = a0; ch < a1; ++ch) acc += chan[(ch - c_lo) * 2 + which];
        atomicAdd(stat + ((int64_t)sample * groups + g) * 4 + (MODE == 0 ? 0 : 2) + which, acc);
    }
}

__global__ __launch_bounds__(256) void gnb_apply_kernel(const f16* __restrict__ x0, const f16* __restrict__ x1, int C0, int C1, int groups,
                                                        int64_t rows_per_sample, int rows_per_slab, float eps,
                                                        const f16* __restrict__ gamma, const f16* __restrict__ beta, int silu,
                                                        const f16* __restrict__ dy, const float* __restrict__ stat,
                                                        f16* __restrict__ dx0, f16* __restrict__ dx1) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int slab = blockIdx.x, strip = blockIdx.y, sample = blockIdx.z;
    const int Ct = C0 + C1, cg = Ct / groups;
    const int c = strip * 256 + tx * 8;
    if (c >= Ct) return;
    const f16* src; f16* dst; int ld, co;
    if (c < C0) { src = x0; dst = dx0; ld = C0; co = c; } else { src = x1; dst = dx1; ld = C1; co = c - C0; }
    float mean[8], rstd[8], ga[8], be[8], k1[8], k2[8];
    const double cnt = (double)rows_per_sample * cg;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* st = stat + ((int64_t)sample * groups + (c + j) / cg) * 4;
        const double d = (double)st[0] / cnt;
        double var = (double)st[1] / cnt - d * d;
        if (var < 0.0) var = 0.0;
        mean[j] = (float)((double)pt_gn_pivot(x0, x1, C0, C1, rows_per_sample, sample, (c + j) / cg * cg) + d);
        rstd[j] = (float)(1.0 / sqrt(var + (double)eps));
        ga[j] = (float)gamma[c + j]; be[j] = (float)beta[c + j];
        k1[j] = (float)((double)st[2] / cnt); k2[j] = (float)((double)st[3] / cnt);
    }
    const int64_t r0 = (int64_t)slab * rows_per_slab;
    int64_t r1 = r0 + rows_per_slab; if (r1 > rows_per_sample) r1 = rows_per_sample;
    const int64_t row_base = (int64_t)sample * rows_per_sample;
    for (int64_t r = r0 + ty; r < r1; r += TY) {
        const f16x8 v = *(const f16x8*)(src + (row_base + r) * ld + co);
        const f16x8 d = *(const f16x8*)(dy + (row_base + r) * Ct + c);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float xh = ((float)v[j] - mean[j]) * rstd[j];
            float g = (float)d[j];
            if (silu) g *= pt_dsilu(xh * ga[j] + be[j]);
            o[j] = (f16)(rstd[j] * (g * ga[j] - k1[j] - xh * k2[j]));
        }
        *(f16x8*)(dst + (row_base + r) * ld + co) = o;
    }
}

// ------------------------------------------------------------------------------------------ LayerNorm backward
// one wave per row; a block of 4 waves owns 64 rows.  A lane keeps the dgamma / dbeta contributions of ITS channels (chunk
// lane, lane + 64, ...: C <= 1536) in registers over the wave's 16 rows, the four waves meet in LDS, one global atomic per
// channel and block.
// DET (ptd_layernorm_bwd): the four waves leave their sums in LDS slots of their own, [wave][2][C], added in wave order into
// part[block][dgamma | dbeta][C] - no LDS atomics, no global ones.
constexpr int LN_MAXCH = 3;                          // chunks of 8 channels per lane (C <= 1536)
template <bool DET>
__global__ __launch_bounds__(256) void lnb_kernel(const f16* __restrict__ x, int64_t M, int C, const f16* __restrict__ gamma, float eps,
                                                  const f16* __restrict__ dy, f16* __restrict__ dx, float* __restrict__ dgamma,
                                                  float* __restrict__ dbeta, int rows_per_block, float* __restrict__ part) {
    extern __shared__ float lds[];                 // [2][C] when dgamma (DET: [4][2][C])
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int CH = C >> 3;
    float pg[LN_MAXCH][8], pb[LN_MAXCH][8];
#pragma unroll
    for (int u = 0; u < LN_MAXCH; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) { pg[u][j] = 0.f; pb[u][j] = 0.f; }
    if (!DET && dgamma) {
        for (int i = threadIdx.x; i < 2 * C; i += 256) lds[i] = 0.f;
        __syncthreads();
    }
    const int64_t rb = (int64_t)blockIdx.x * rows_per_block;
    for (int rr = wave; rr < rows_per_block; rr += 4) {
        const int64_t r = rb + rr;
        if (r >= M) break;
        const f16* xr = x + r * C;
        const f16* dr = dy + r * C;
        f16x8 xv[LN_MAXCH], dv[LN_MAXCH];
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u) {
            const int ch = lane + 64 * u;
            if (ch < CH) {
                xv[u] = *(const f16x8*)(xr + ch * 8);
                dv[u] = *(const f16x8*)(dr + ch * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += (float)xv[u][j];
            }
        }
        const float mean = pt_wave_sum(s) / C;
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u)                  // two passes over the registers: the centred variance (q / C - mean^2
            if (lane + 64 * u < CH)                          // from fp32 sums lost it at ~100 sigma, tests/test_norm_numerics_gpu.py)
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = (float)xv[u][j] - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(pt_wave_sum(q) / C + eps);
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u) {
            const int ch = lane + 64 * u;
            if (ch < CH) {
                const f16x8 gm = *(const f16x8*)(gamma + ch * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[u][j] - mean) * rstd, g = (float)dv[u][j] * (float)gm[j];
                    a += g; b += g * xh;
                }
            }
        }
        a = pt_wave_sum(a) / C; b = pt_wave_sum(b) / C;
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u) {
            const int ch = lane + 64 * u;
            if (ch < CH) {
                const f16x8 gm = *(const f16x8*)(gamma + ch * 8);
                f16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[u][j] - mean) * rstd, dyj = (float)dv[u][j];
                    o[j] = (f16)(rstd * (dyj * (float)gm[j] - a - xh * b));
                    pg[u][j] += dyj * xh; pb[u][j] += dyj;
                }
                *(f16x8*)(dx + r * C + ch * 8) = o;
            }
        }
    }
    if (DET && dgamma) {
        float* mine = lds + wave * 2 * C;
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u) {
            const int ch = lane + 64 * u;
            if (ch < CH)
#pragma unroll
                for (int j = 0; j < 8; ++j) { mine[ch * 8 + j] = pg[u][j]; mine[C + ch * 8 + j] = pb[u][j]; }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * C; i += 256)
            part[(int64_t)blockIdx.x * 2 * C + i] = ((lds[i] + lds[2 * C + i]) + lds[4 * C + i]) + lds[6 * C + i];
        return;
    }
    if (dgamma) {
#pragma unroll
        for (int u = 0; u < LN_MAXCH; ++u) {
            const int ch = lane + 64 * u;
            if (ch < CH)
#pragma unroll
                for (int j = 0; j < 8; ++j) { atomicAdd(&lds[ch * 8 + j], pg[u][j]); atomicAdd(&lds[C + ch * 8 + j], pb[u][j]); }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < C; i += 256) { atomicAdd(dgamma + i, lds[i]); atomicAdd(dbeta + i, lds[C + i]); }
    }
}

// Narrow rows: LPR lanes per row (3 chunks of 8 channels each), 64 / LPR rows of a wave in flight together - the one-wave-per-row
// kernel above is latency-bound there (two dependent wave reductions per 640-byte row: 61 us for [40320, 320] against 8 us for
// the forward).  With parameter gradients it also writes (mean, rstd) per row for lnb_param_kernel below - LDS atomics from the
// 4-8 rows a wave has in flight serialise (166 us), register partials push the kernel to 2 waves per SIMD (61 us); two lean
// passes take 21 + 20.
template <int LPR, bool PARAMS>
__global__ __launch_bounds__(256) void lnb_narrow_kernel(const f16* __restrict__ x, int64_t M, int C, const f16* __restrict__ gamma, float eps,
                                                         const f16* __restrict__ dy, f16* __restrict__ dx, float* __restrict__ rowstat,
                                                         int rows_per_block) {
    constexpr int NCH = 3, RPW = 64 / LPR;               // chunks of 8 channels per lane; rows per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane % LPR, grp = lane / LPR;
    const int CH = C >> 3;
    const int64_t rb = (int64_t)blockIdx.x * rows_per_block;
    const float invC = 1.0f / C;
    for (int rr = wave * RPW + grp; rr < rows_per_block; rr += 4 * RPW) {
        const int64_t r = rb + rr;
        const bool ok = r < M;                            // lanes of a missing row still take part in the shuffles
        f16x8 xv[NCH], dv[NCH];
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            const int ch = li + LPR * u;
            if (ok && ch < CH) {
                xv[u] = *(const f16x8*)(x + r * C + ch * 8);
                dv[u] = *(const f16x8*)(dy + r * C + ch * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) s += (float)xv[u][j];
            }
        }
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
        const float mean = s * invC;
#pragma unroll
        for (int u = 0; u < NCH; ++u)                       // the centred variance, second pass over the registers (as lnb_kernel)
            if (ok && li + LPR * u < CH)
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = (float)xv[u][j] - mean; q += d * d; }
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q * invC + eps);
        if (PARAMS && ok && li == 0) *(f32x2*)(rowstat + 2 * r) = f32x2{mean, rstd};
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            const int ch = li + LPR * u;
            if (ok && ch < CH) {
                const f16x8 gm = *(const f16x8*)(gamma + ch * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[u][j] - mean) * rstd, g = (float)dv[u][j] * (float)gm[j];
                    a += g; b += g * xh;
                }
            }
        }
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
        a *= invC; b *= invC;
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            const int ch = li + LPR * u;
            if (ok && ch < CH) {
                const f16x8 gm = *(const f16x8*)(gamma + ch * 8);
                f16x8 o8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xh = ((float)xv[u][j] - mean) * rstd, dyj = (float)dv[u][j];
                    o8[j] = (f16)(rstd * (dyj * (float)gm[j] - a - xh * b));
                }
                *(f16x8*)(dx + r * C + ch * 8) = o8;
            }
        }
    }
}

// dgamma[c] += sum_rows dy xh, dbeta[c] += sum_rows dy with (mean, rstd) per row from the pass above; grid (slabs, strips)
// DET: dgamma is the workspace, part[slab][dgamma | dbeta][C]
template <bool DET>
__global__ __launch_bounds__(256) void lnb_param_kernel(const f16* __restrict__ x, const f16* __restrict__ dy, const float* __restrict__ rowstat,
                                                        int64_t M, int rows_per_slab, int C, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float red[TY][256 * 2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int slab = blockIdx.x, strip = blockIdx.y;
    const int c = strip * 256 + tx * 8;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (c < C) {
        const int64_t r0 = (int64_t)slab * rows_per_slab;
        int64_t r1 = r0 + rows_per_slab; if (r1 > M) r1 = M;
        for (int64_t r = r0 + ty; r < r1; r += TY) {
            const f16x8 v = *(const f16x8*)(x + r * C + c), d = *(const f16x8*)(dy + r * C + c);
            const f32x2 st = *(const f32x2*)(rowstat + 2 * r);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float dj = (float)d[j]; s[j] += dj; q[j] += dj * ((float)v[j] - st[0]) * st[1]; }
        }
    }
    fold_strip(red, s, q, [&](int ch, float a, float b) {
        const int cc = strip * 256 + ch;
        if (cc < C) {
            if constexpr (DET) {
                float* pp = dgamma + (int64_t)slab * 2 * C;
                pp[cc] = b; pp[C + cc] = a;
            } else {
                atomicAdd(dbeta + cc, a); atomicAdd(dgamma + cc, b);
            }
        }
    });
}

template <int LPR>
void launch_lnb_narrow(const f16* x, int64_t M, int C, const f16* gamma, float eps, const f16* dy, f16* dx, float* dgamma, float* dbeta,
                       float* rowstat, hipStream_t s, float* ws = nullptr) {
    const int rpb = 64;
    const unsigned blocks = (unsigned)((M + rpb - 1) / rpb);
    if (dgamma) {
        hipLaunchKernelGGL((lnb_narrow_kernel<LPR, true>), dim3(blocks), dim3(256), 0, s, x, M, C, gamma, eps, dy, dx, rowstat, rpb);
        const int strips = (C + 255) / 256;
        const int rps = slab_rows(M, strips, TY);
        const int slabs = (int)((M + rps - 1) / rps);
        if (ws) {
            hipLaunchKernelGGL(lnb_param_kernel<true>, dim3(slabs, strips), dim3(256), 0, s, x, dy, (const float*)rowstat, M, rps, C, ws, (float*)nullptr);
            FoldJob j = fold_job(ws, 2 * (int64_t)C, slabs, dgamma, 1);
            j.n0 = C; j.grp = C; j.out1 = dbeta;
            launch_fold<float>(s, j);
        } else
            hipLaunchKernelGGL(lnb_param_kernel<false>, dim3(slabs, strips), dim3(256), 0, s, x, dy, (const float*)rowstat, M, rps, C, dgamma, dbeta);
    } else {
        hipLaunchKernelGGL((lnb_narrow_kernel<LPR, false>), dim3(blocks), dim3(256), 0, s, x, M, C, gamma, eps, dy, dx, rowstat, rpb);
    }
}

// ------------------------------------------------------------------------------------------ segmented column sums
// out[seg, c] += sum over the rows of segment seg of dy[row, c]: bias gradients (one segment), the gradient of a per-frame /
// per-clip row vector broadcast over its rows (time-embedding rows, collapsed cross-attention, frame position embedding).
// DET: out is the workspace, part[slab][seg][C]
template <bool DET>
__global__ __launch_bounds__(256) void colsum_kernel(const f16* __restrict__ dy, int64_t rows_per_seg, int rows_per_slab, int C, int ld,
                                                     float* __restrict__ out) {
    __shared__ float red[TY][256 * 2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int slab = blockIdx.x, strip = blockIdx.y, seg = blockIdx.z;
    const int c = strip * 256 + tx * 8;
    float s[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[j] = 0.f; q[j] = 0.f; }
    if (c < C) {
        const int64_t r0 = (int64_t)slab * rows_per_slab;
        int64_t r1 = r0 + rows_per_slab; if (r1 > rows_per_seg) r1 = rows_per_seg;
        const f16* base = dy + (int64_t)seg * rows_per_seg * ld + c;
        int64_t r = r0 + ty;
        if (c + 8 <= C) {
            for (; r + 3 * TY < r1; r += 4 * TY) {           // four rows' loads in flight: one per iteration is a latency chain
                f16x8 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *(const f16x8*)(base + (r + u * TY) * ld);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 8; ++j) s[j] += (float)v[u][j];
            }
            for (; r < r1; r += TY) {
                const f16x8 v = *(const f16x8*)(base + r * ld);
#pragma unroll
                for (int j = 0; j < 8; ++j) s[j] += (float)v[j];
            }
        } else {
            for (; r < r1; r += TY) {
                const f16* src = base + r * ld;
                for (int j = 0; j < 8; ++j) if (c + j < C) s[j] += (float)src[j];
            }
        }
    }
    fold_strip(red, s, q, [&](int ch, float a, float) {
        const int cc = strip * 256 + ch;
        if (cc < C) {
            if constexpr (DET) out[((int64_t)slab * gridDim.z + seg) * C + cc] = a;
            else atomicAdd(out + (int64_t)seg * C + cc, a);
        }
    });
}

// out += scale * sum_i dy_i (a_i - b_i)     (gradient of the blend weight; fp32, one atomic per block; DET: out[block] = its term)
// DEV: the argument points at the blend weight alpha in device memory, and scale = alpha (1 - alpha) = d alpha / d mix_factor
template <bool DET, bool DEV>
__global__ __launch_bounds__(256) void dot_diff_kernel(const f16* __restrict__ dy, const f16* __restrict__ a, const f16* __restrict__ b,
                                                       int64_t n, pt_scalar_arg<DEV> scale_arg, float* __restrict__ out) {
    __shared__ float red[4];
    float scale = pt_scalar(scale_arg);
    if constexpr (DEV) scale = scale * (1.0f - scale);
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        acc += (float)dy[i] * ((float)a[i] - (b ? (float)b[i] : 0.f));
    acc = pt_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = scale * (red[0] + red[1] + red[2] + red[3]);
        if constexpr (DET) out[blockIdx.x] = v;
        else atomicAdd(out, v);
    }
}

// out[0] += sum g^2 (fp32 in, fp64 block sums); a non-finite gradient anywhere makes the result non-finite (the GradScaler check)
// DET: out[block] = the block's sum
template <bool DET>
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) acc += (double)g[i] * (double)g[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if constexpr (DET) out[blockIdx.x] = red[0];
        else atomicAdd(out, red[0]);
    }
}

}  // namespace

// The host side of a reduction and of its deterministic twin (include/posetraj_det.h) is ONE function: `det` only chooses the
// kernels' DET instance, checks the workspace and adds the fold launch.  With det == false nothing differs from what it was.
struct GnGeom { int strips, rps, slabs; int64_t stat_floats, par_floats; };
static GnGeom gn_geom(int Ct, int groups, int64_t rows_per_sample, int n_samples, bool with_params) {
    GnGeom g;
    g.strips = (Ct + 255) / 256;
    g.rps = slab_rows(rows_per_sample, (int64_t)g.strips * n_samples, TY);
    g.slabs = (int)((rows_per_sample + g.rps - 1) / g.rps);
    g.stat_floats = (int64_t)g.slabs * g.strips * n_samples * groups * 2;
    g.par_floats = with_params ? (int64_t)n_samples * g.slabs * 2 * Ct : 0;
    return g;
}

static int groupnorm_bwd_launch(const char* who, bool det, const void* x0, const void* x1, int32_t C0, int32_t C1, int32_t groups,
                                int64_t rows_per_sample, int32_t n_samples, float eps, const void* gamma, const void* beta, int32_t silu,
                                const void* dy, void* dx0, void* dx1, float* dgamma, float* dbeta, float* stat, float* ws, int64_t ws_floats,
                                void* stream) {
    const int Ct = C0 + C1;
    PT_CHECK(x0 && gamma && beta && dy && dx0 && stat, "%s: null pointer", who);
    PT_CHECK((((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)dy | (uintptr_t)dx0 | (uintptr_t)dx1) & 15) == 0, "%s: 16-byte aligned rows required", who);
    PT_CHECK(C0 > 0 && C0 % 8 == 0 && C1 >= 0 && C1 % 8 == 0 && (C1 == 0 || (x1 && dx1)), "%s: channel counts %d + %d", who, C0, C1);
    PT_CHECK(groups > 0 && Ct % groups == 0, "%s: %d channels / %d groups", who, Ct, groups);
    PT_CHECK(rows_per_sample > 0 && n_samples > 0 && n_samples < 65536, "%s: bad sizes", who);
    PT_CHECK((dgamma == nullptr) == (dbeta == nullptr), "%s: dgamma and dbeta come together", who);
    hipStream_t s = (hipStream_t)stream;
    const GnGeom g = gn_geom(Ct, groups, rows_per_sample, n_samples, dgamma != nullptr);
    const dim3 grid(g.slabs, g.strips, n_samples);
#define PT_GNB_ARGS (const f16*)x0, (const f16*)x1, C0, C1, groups, rows_per_sample, g.rps, eps, (const f16*)gamma, (const f16*)beta, silu, (const f16*)dy
    if (det) {
        PT_CHECK_WS(who, ws, ws_floats, g.stat_floats + g.par_floats);
        float* ps = ws;
        float* pp = ws + g.stat_floats;
        const int64_t ns = (int64_t)n_samples * groups * 2;
        FoldJob js = fold_job(ps, ns, g.slabs * g.strips, stat, 0);
        js.grp = 2; js.stride = 4;
        hipLaunchKernelGGL((gnb_reduce_kernel<0, true>), grid, dim3(256), 0, s, PT_GNB_ARGS, stat, dgamma, dbeta, ps, pp);
        launch_fold<float>(s, js);
        hipLaunchKernelGGL((gnb_reduce_kernel<1, true>), grid, dim3(256), 0, s, PT_GNB_ARGS, stat, dgamma, dbeta, ps, pp);
        js.off = 2;
        if (dgamma) {
            FoldJob jp = fold_job(pp, 2 * (int64_t)Ct, n_samples * g.slabs, dgamma, 1);
            jp.n0 = Ct; jp.grp = Ct; jp.out1 = dbeta;
            launch_fold<float>(s, js, &jp);
        } else {
            launch_fold<float>(s, js);
        }
    } else {
        if (hipMemsetAsync(stat, 0, sizeof(float) * 4 * (size_t)n_samples * groups, s) != hipSuccess) { pt_set_error("%s: memset failed", who); return 2; }
        hipLaunchKernelGGL((gnb_reduce_kernel<0, false>), grid, dim3(256), 0, s, PT_GNB_ARGS, stat, dgamma, dbeta, (float*)nullptr, (float*)nullptr);
        hipLaunchKernelGGL((gnb_reduce_kernel<1, false>), grid, dim3(256), 0, s, PT_GNB_ARGS, stat, dgamma, dbeta, (float*)nullptr, (float*)nullptr);
    }
    hipLaunchKernelGGL(gnb_apply_kernel, grid, dim3(256), 0, s, PT_GNB_ARGS, (const float*)stat, (f16*)dx0, (f16*)dx1);
#undef PT_GNB_ARGS
    PT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int pt_groupnorm_bwd(const void* x0, const void* x1, int32_t C0, int32_t C1, int32_t groups, int64_t rows_per_sample,
                                int32_t n_samples, float eps, const void* gamma, const void* beta, int32_t silu, const void* dy,
                                void* dx0, void* dx1, float* dgamma, float* dbeta, float* stat, void* stream) {
    return groupnorm_bwd_launch("pt_groupnorm_bwd", false, x0, x1, C0, C1, groups, rows_per_sample, n_samples, eps, gamma, beta, silu, dy, dx0, dx1,
                                dgamma, dbeta, stat, nullptr, 0, stream);
}

extern "C" int64_t ptd_groupnorm_bwd_ws_floats(int32_t channels, int32_t groups, int64_t rows_per_sample, int32_t n_samples, int32_t with_params) {
    if (channels <= 0 || groups <= 0 || rows_per_sample <= 0 || n_samples <= 0) return 0;
    const GnGeom g = gn_geom(channels, groups, rows_per_sample, n_samples, with_params != 0);
    return g.stat_floats + g.par_floats;
}

extern "C" int ptd_groupnorm_bwd(const void* x0, const void* x1, int32_t C0, int32_t C1, int32_t groups, int64_t rows_per_sample,
                                 int32_t n_samples, float eps, const void* gamma, const void* beta, int32_t silu, const void* dy,
                                 void* dx0, void* dx1, float* dgamma, float* dbeta, float* stat, float* ws, int64_t ws_floats, void* stream) {
    return groupnorm_bwd_launch("ptd_groupnorm_bwd", true, x0, x1, C0, C1, groups, rows_per_sample, n_samples, eps, gamma, beta, silu, dy, dx0, dx1,
                                dgamma, dbeta, stat, ws, ws_floats, stream);
}

// blocks of the wide LayerNorm backward (one wave per row) and rows per block
static int64_t lnb_wide_blocks(int64_t M, int* rows_per_block) {
    // the wide rows of this network are its low-resolution levels (630 / 2 520 rows of 1 280 channels): 64 rows per
    // block left 10 - 40 blocks for 256 CUs (83 us per launch); 8 ... 64 rows per block, aiming at ~512 blocks
    int rpb = (int)((M + 511) / 512);
    rpb = rpb < 8 ? 8 : (rpb > 64 ? 64 : (rpb + 3) / 4 * 4);
    *rows_per_block = rpb;
    return (M + rpb - 1) / rpb;
}

// partials of the parameter gradients: slabs of lnb_param_kernel (narrow rows) or blocks of lnb_kernel
static int64_t lnb_partials(int64_t M, int Cc) {
    if (Cc / 8 <= 96) {
        const int rps = slab_rows(M, (Cc + 255) / 256, TY);
        return (M + rps - 1) / rps;
    }
    int rpb;
    return lnb_wide_blocks(M, &rpb);
}

static int layernorm_bwd_launch(const char* who, bool det, const void* x, int64_t M, int32_t Cc, const void* gamma, float eps, const void* dy,
                                void* dx, float* dgamma, float* dbeta, float* rowstat, float* ws, int64_t ws_floats, void* stream) {
    PT_CHECK(x && gamma && dy && dx, "%s: null pointer", who);
    PT_CHECK((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)gamma) & 15) == 0, "%s: 16-byte aligned rows required", who);
    PT_CHECK(M > 0 && Cc > 0 && Cc % 8 == 0 && Cc <= 512 * LN_MAXCH, "%s: bad sizes (M %lld, C %d)", who, (long long)M, Cc);
    PT_CHECK((dgamma == nullptr) == (dbeta == nullptr), "%s: dgamma and dbeta come together", who);
    PT_CHECK(!dgamma || rowstat, "%s: parameter gradients need the 2 M floats of rowstat scratch", who);
    det = det && dgamma;                                           // without parameter gradients nothing is reduced across blocks
    if (det) {
        const int64_t need = lnb_partials(M, Cc) * 2 * Cc;
        PT_CHECK_WS(who, ws, ws_floats, need);
    }
    float* w = det ? ws : nullptr;
    const int CH = Cc / 8;
    hipStream_t s = (hipStream_t)stream;
    if (CH <= 24) launch_lnb_narrow<8>((const f16*)x, M, Cc, (const f16*)gamma, eps, (const f16*)dy, (f16*)dx, dgamma, dbeta, rowstat, s, w);
    else if (CH <= 48) launch_lnb_narrow<16>((const f16*)x, M, Cc, (const f16*)gamma, eps, (const f16*)dy, (f16*)dx, dgamma, dbeta, rowstat, s, w);
    else if (CH <= 96) launch_lnb_narrow<32>((const f16*)x, M, Cc, (const f16*)gamma, eps, (const f16*)dy, (f16*)dx, dgamma, dbeta, rowstat, s, w);
    else {
        int rpb;
        const int64_t blocks = lnb_wide_blocks(M, &rpb);
        if (det) {
            hipLaunchKernelGGL(lnb_kernel<true>, dim3((unsigned)blocks), dim3(256), sizeof(float) * 8 * Cc, s, (const f16*)x, M, Cc, (const f16*)gamma, eps,
                               (const f16*)dy, (f16*)dx, dgamma, dbeta, rpb, w);
            FoldJob j = fold_job(w, 2 * (int64_t)Cc, (int)blocks, dgamma, 1);
            j.n0 = Cc; j.grp = Cc; j.out1 = dbeta;
            launch_fold<float>(s, j);
        } else {
            hipLaunchKernelGGL(lnb_kernel<false>, dim3((unsigned)blocks), dim3(256), dgamma ? sizeof(float) * 2 * Cc : 0, s, (const f16*)x, M, Cc,
                               (const f16*)gamma, eps, (const f16*)dy, (f16*)dx, dgamma, dbeta, rpb, (float*)nullptr);
        }
    }
    PT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int pt_layernorm_bwd(const void* x, int64_t M, int32_t Cc, const void* gamma, float eps, const void* dy, void* dx,
                                float* dgamma, float* dbeta, float* rowstat, void* stream) {
    return layernorm_bwd_launch("pt_layernorm_bwd", false, x, M, Cc, gamma, eps, dy, dx, dgamma, dbeta, rowstat, nullptr, 0, stream);
}

extern "C" int64_t ptd_layernorm_bwd_ws_floats(int64_t M, int32_t Cc) {
    return (M > 0 && Cc > 0) ? lnb_partials(M, Cc) * 2 * Cc : 0;
}

extern "C" int ptd_layernorm_bwd(const void* x, int64_t M, int32_t Cc, const void* gamma, float eps, const void* dy, void* dx,
                                 float* dgamma, float* dbeta, float* rowstat, float* ws, int64_t ws_floats, void* stream) {
    return layernorm_bwd_launch("ptd_layernorm_bwd", true, x, M, Cc, gamma, eps, dy, dx, dgamma, dbeta, rowstat, ws, ws_floats, stream);
}

static int colsum_launch(const char* who, bool det, const void* dy, int64_t rows_per_seg, int32_t nseg, int32_t Cc, int32_t ld, float* out,
                         float* ws, int64_t ws_floats, void* stream) {
    PT_CHECK(dy && out, "%s: null pointer", who);
    PT_CHECK(rows_per_seg > 0 && nseg > 0 && nseg < 65536 && Cc > 0 && ld >= Cc && ld % 8 == 0, "%s: bad sizes", who);
    const int strips = (Cc + 255) / 256;
    const int rps = slab_rows(rows_per_seg, (int64_t)strips * nseg, TY);
    const int slabs = (int)((rows_per_seg + rps - 1) / rps);
    const dim3 grid(slabs, strips, nseg);
    hipStream_t s = (hipStream_t)stream;
    if (det) {
        const int64_t n = (int64_t)nseg * Cc;
        PT_CHECK_WS(who, ws, ws_floats, slabs * n);
        hipLaunchKernelGGL(colsum_kernel<true>, grid, dim3(256), 0, s, (const f16*)dy, rows_per_seg, rps, Cc, ld, ws);
        launch_fold<float>(s, fold_job(ws, n, slabs, out, 1));
    } else {
        hipLaunchKernelGGL(colsum_kernel<false>, grid, dim3(256), 0, s, (const f16*)dy, rows_per_seg, rps, Cc, ld, out);
    }
    PT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int pt_colsum_f16(const void* dy, int64_t rows_per_seg, int32_t nseg, int32_t Cc, int32_t ld, float* out, void* stream) {
    return colsum_launch("pt_colsum_f16", false, dy, rows_per_seg, nseg, Cc, ld, out, nullptr, 0, stream);
}

extern "C" int64_t ptd_colsum_ws_floats(int64_t rows_per_seg, int32_t nseg, int32_t Cc) {
    if (rows_per_seg <= 0 || nseg <= 0 || Cc <= 0) return 0;
    const int rps = slab_rows(rows_per_seg, (int64_t)((Cc + 255) / 256) * nseg, TY);
    return (rows_per_seg + rps - 1) / rps * nseg * Cc;
}

extern "C" int ptd_colsum_f16(const void* dy, int64_t rows_per_seg, int32_t nseg, int32_t Cc, int32_t ld, float* out, float* ws,
                              int64_t ws_floats, void* stream) {
    return colsum_launch("ptd_colsum_f16", true, dy, rows_per_seg, nseg, Cc, ld, out, ws, ws_floats, stream);
}

static unsigned dot_diff_blocks(int64_t n) {
    const unsigned blocks = ew_blocks(n);
    return blocks > 1024 ? 1024 : blocks;
}

// DEV = false: `scale` is the host's float; true: a pointer to alpha in device memory, scale = alpha (1 - alpha)
template <bool DEV>
static int dot_diff_launch(const char* who, bool det, const void* dy, const void* a, const void* b, int64_t n, pt_scalar_arg<DEV> scale, float* out,
                           float* ws, int64_t ws_floats, void* stream) {
    const unsigned blocks = dot_diff_blocks(n > 0 ? n : 1);
    hipStream_t s = (hipStream_t)stream;
    if (det) {
        PT_CHECK_WS(who, ws, ws_floats, (int64_t)blocks);
        hipLaunchKernelGGL((dot_diff_kernel<true, DEV>), dim3(blocks), dim3(256), 0, s, (const f16*)dy, (const f16*)a, (const f16*)b, n, scale, ws);
        launch_fold<float>(s, fold_job(ws, 1, (int)blocks, out, 1));
    } else {
        hipLaunchKernelGGL((dot_diff_kernel<false, DEV>), dim3(blocks), dim3(256), 0, s, (const f16*)dy, (const f16*)a, (const f16*)b, n, scale, out);
    }
    PT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int pt_dot_diff(const void* dy, const void* a, const void* b, int64_t n, float scale, float* out, void* stream) {
    PT_CHECK(dy && a && out && n > 0, "pt_dot_diff: bad arguments");
    return dot_diff_launch<false>("pt_dot_diff", false, dy, a, b, n, scale, out, nullptr, 0, stream);
}

extern "C" int64_t ptd_dot_diff_ws_floats(int64_t n) { return n > 0 ? (int64_t)dot_diff_blocks(n) : 0; }

extern "C" int ptd_dot_diff(const void* dy, const void* a, const void* b, int64_t n, float scale, float* out, float* ws, int64_t ws_floats,
                            void* stream) {
    PT_CHECK(dy && a && out && n > 0, "ptd_dot_diff: bad arguments");
    return dot_diff_launch<false>("ptd_dot_diff", true, dy, a, b, n, scale, out, ws, ws_floats, stream);
}

extern "C" int ptd_dot_diff_dev(const void* dy, const void* a, const void* b, int64_t n, const float* alpha_dev, float* out, float* ws,
                                int64_t ws_floats, void* stream) {
    PT_CHECK(dy && a && out && alpha_dev && n > 0, "ptd_dot_diff_dev: bad arguments");
    return dot_diff_launch<true>("ptd_dot_diff_dev", true, dy, a, b, n, alpha_dev, out, ws, ws_floats, stream);
}

extern "C" int pt_dot_diff_dev(const void* dy, const void* a, const void* b, int64_t n, const float* alpha_dev, float* out, void* stream) {
    PT_CHECK(dy && a && out && alpha_dev && n > 0, "pt_dot_diff_dev: bad arguments");
    return dot_diff_launch<true>("pt_dot_diff_dev", false, dy, a, b, n, alpha_dev, out, nullptr, 0, stream);
}

static unsigned sumsq_blocks(int64_t n) {
    const unsigned blocks = ew_blocks(n);
    return blocks > 2048 ? 2048 : blocks;
}

extern "C" int pt_sumsq_f32(const float* g, int64_t n, double* out, void* stream) {
    PT_CHECK(g && out && n > 0, "pt_sumsq_f32: bad arguments");
    hipLaunchKernelGGL(sumsq_kernel<false>, dim3(sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, n, out);
    PT_LAUNCH_CHECK("pt_sumsq_f32");
    return 0;
}

extern "C" int ptd_abi_version(void) { return PT_DET_ABI_VERSION; }

extern "C" int64_t ptd_sumsq_ws_floats(int64_t n) { return n > 0 ? 2 * (int64_t)sumsq_blocks(n) : 0; }

extern "C" int ptd_sumsq_f32(const float* g, int64_t n, double* out, float* ws, int64_t ws_floats, void* stream) {
    PT_CHECK(g && out && n > 0, "ptd_sumsq_f32: bad arguments");
    const unsigned blocks = sumsq_blocks(n);
    PT_CHECK(ws && ((uintptr_t)ws & 7) == 0 && ws_floats >= 2 * (int64_t)blocks, "ptd_sumsq_f32: the workspace (8-byte aligned) holds %lld floats, %lld needed",
             (long long)(ws ? ws_floats : 0), (long long)(2 * (int64_t)blocks));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sumsq_kernel<true>, dim3(blocks), dim3(256), 0, s, g, n, (double*)ws);
    launch_fold<double>(s, fold_job(ws, 1, (int)blocks, out, 1));
    PT_LAUNCH_CHECK("ptd_sumsq_f32");
    return 0;
}
