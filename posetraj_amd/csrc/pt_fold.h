// Second stage of the deterministic reductions (include/posetraj_det.h): the first stage - the atomic kernel minus its
// atomics - leaves one partial per workgroup in a workspace slot addressed by its block coordinates, part[p][i]; this kernel adds
// them in a fixed order and stores, or `+=`s where the destination accumulates.  No atomics, no waiting between workgroups: the
// stream orders the two launches.
//
// Order: the partials of an output are cut into CHAINS contiguous runs of ceil(parts / CHAINS); a thread adds one run in ascending
// p, the runs meet in LDS and thread 0 of the output adds the run totals in ascending order.  A function of (parts, CHAINS) alone,
// and CHAINS is chosen from the shape, never from the machine's state.  The folds are latency: a handful of outputs over hundreds
// of partials, so the runs give independent load chains (64 when there are at most four outputs, 8 otherwise; 1 - a plain
// ascending sum, 256 outputs per block - when there are at most 16 partials, the weight-gradient GEMM's case).
#pragma once
#include "pt_common.h"

namespace {

struct FoldJob {
    const void* part;        // [parts][n]
    void* out0;              // output i < n0 -> out0[(i / grp) * stride + off + i % grp]
    void* out1;              // output i >= n0 -> out1[i - n0]
    int64_t n, n0, grp, stride, off;
    int parts, accumulate;
};

inline FoldJob fold_job(const void* part, int64_t n, int parts, void* out, int accumulate) {
    return FoldJob{part, out, nullptr, n, n, n > 0 ? n : 1, 0, 0, parts, accumulate};
}

// grid (blocks, jobs): blockIdx.y picks the job (two reductions of one pass fold in one launch)
template <typename T, int CHAINS>
__global__ __launch_bounds__(256) void fold_kernel(FoldJob j0, FoldJob j1) {
    constexpr int OPB = 256 / CHAINS;                   // outputs per block
    __shared__ T red[CHAINS > 1 ? 256 : 1];
    const FoldJob j = blockIdx.y ? j1 : j0;
    const int tx = threadIdx.x % OPB, chain = threadIdx.x / OPB;
    const int64_t i = (int64_t)blockIdx.x * OPB + tx;
    const int per = (j.parts + CHAINS - 1) / CHAINS;
    const int p0 = chain * per, p1 = p0 + per < j.parts ? p0 + per : j.parts;
    T acc = (T)0;
    if (i < j.n) {
        const T* src = (const T*)j.part + i;
#pragma unroll 4
        for (int p = p0; p < p1; ++p) acc += src[(int64_t)p * j.n];
    }
    if (CHAINS > 1) {
        red[chain * OPB + tx] = acc;
        __syncthreads();
        if (chain != 0) return;
        acc = red[tx];
#pragma unroll
        for (int c = 1; c < CHAINS; ++c) acc += red[c * OPB + tx];
    }
    if (i >= j.n) return;
    T* dst = i < j.n0 ? (T*)j.out0 + (i / j.grp) * j.stride + j.off + i % j.grp : (T*)j.out1 + (i - j.n0);
    *dst = j.accumulate ? *dst + acc : acc;
}

template <typename T>
inline void launch_fold(hipStream_t s, const FoldJob& a, const FoldJob* b = nullptr) {
    const FoldJob& bb = b ? *b : a;
    const int64_t n = a.n > bb.n ? a.n : bb.n;
    const int parts = a.parts > bb.parts ? a.parts : bb.parts;
    const int chains = n <= 4 ? 64 : (parts <= 16 ? 1 : 8);
    const int opb = 256 / chains;
    const dim3 grid((unsigned)((n + opb - 1) / opb), b ? 2 : 1);
    if (chains == 64) hipLaunchKernelGGL((fold_kernel<T, 64>), grid, dim3(256), 0, s, a, bb);
    else if (chains == 8) hipLaunchKernelGGL((fold_kernel<T, 8>), grid, dim3(256), 0, s, a, bb);
    else hipLaunchKernelGGL((fold_kernel<T, 1>), grid, dim3(256), 0, s, a, bb);
}

}  // namespace
