// Clip batches on the training tape (include/posetraj_batch.h): the temporal blocks' collapsed cross-attention of B clips.  Token row
// r = (b F + f) S + s receives the context row j(r) = (b S + s) mod B (igemm_tail.h: vec_index, vec_mode 2) - the add and
// the gradient of the B context rows.  Both are HBM-bound passes over a [B F S, C] fp16 activation: 16-byte lanes, four loads in
// flight per thread, index arithmetic in 32 bits (the host refuses B F S C / 8 >= 2^31).
#include "pt_common.h"
#include "../../include/posetraj_batch.h"
#include "pt_fold.h"
#include "pt_launch.h"

namespace {

constexpr int TY = 8;                    // thread (ty, tx): chunk column tx (8 channels) of a 256-channel strip, rows ty, ty + 8, ...

__device__ __forceinline__ uint32_t ctx_index(uint32_t r, uint32_t FS, uint32_t S, uint32_t B) { return ((r / FS) * S + r % S) % B; }

__device__ __forceinline__ f16x8 add8(const f16x8& a, const f16x8& v) {
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f16)((float)a[j] + (float)v[j]);
    return o;
}

// y[r, :] = x[r, :] + vec[j(r), :]; element i = (row r, chunk of 8 channels), n8 = rows * C / 8 of them
__global__ __launch_bounds__(256) void add_rowvec_interleaved_kernel(const f16* __restrict__ x, const f16* __restrict__ vec, uint32_t n8, uint32_t CH,
                                                                     uint32_t FS, uint32_t S, uint32_t B, f16* __restrict__ y) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n8; i += 4 * stride) {           // four independent 16-byte loads of x per thread before the first use
        f16x8 a[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = *(const f16x8*)(x + (i + u * stride) * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t e = (uint32_t)(i + u * stride), r = e / CH, c = e - r * CH;
            v[u] = *(const f16x8*)(vec + ((uint64_t)ctx_index(r, FS, S, B) * CH + c) * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) *(f16x8*)(y + (i + u * stride) * 8) = add8(a[u], v[u]);
    }
    for (; i < n8; i += stride) {
        const uint32_t e = (uint32_t)i, r = e / CH, c = e - r * CH;
        const f16x8 a = *(const f16x8*)(x + i * 8), v = *(const f16x8*)(vec + ((uint64_t)ctx_index(r, FS, S, B) * CH + c) * 8);
        *(f16x8*)(y + i * 8) = add8(a, v);
    }
}

// out[j, c] += sum over {r : j(r) = j} of dy[r, c].  Class j is {(b, s) : b S + s = j + k B, k = 0 .. S - 1} x all frames: exactly
// F S rows, enumerated t = f S + k -> q = j + k B, b = q / S, s = q % S, r = (b F + f) S + s.  grid (slabs over t, strips of 256
// channels, B): every row of dy is read by exactly one workgroup, as whole 16-byte chunks.  Written like colsum_kernel
// (norm_bwd.hip).  DET: out is the workspace, part[slab][j][C].
template <bool DET>
__global__ __launch_bounds__(256) void colsum_interleaved_kernel(const f16* __restrict__ dy, uint32_t F, uint32_t S, uint32_t B, int rows_per_slab,
                                                                 int C, float* __restrict__ out) {
    __shared__ float red[TY][256];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const uint32_t slab = blockIdx.x, strip = blockIdx.y, j = blockIdx.z;
    const int c = strip * 256 + tx * 8;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (c < C) {                                             // (C % 8 == 0: a chunk is inside the row or outside it)
        const uint32_t FS = F * S;
        const uint32_t t0 = slab * (uint32_t)rows_per_slab;
        uint32_t t1 = t0 + (uint32_t)rows_per_slab; if (t1 > FS) t1 = FS;
        const f16* base = dy + c;
        auto row = [&](uint32_t t) -> const f16x8* {
            const uint32_t f = t / S, k = t - f * S, q = j + k * B, b = q / S, sp = q - b * S;
            return (const f16x8*)(base + (uint64_t)((b * F + f) * S + sp) * C);
        };
        uint32_t t = t0 + ty;
        for (; t + 3 * TY < t1; t += 4 * TY) {               // four rows' loads in flight: one per iteration is a latency chain
            f16x8 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *row(t + u * TY);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] += (float)v[u][e];
        }
        for (; t < t1; t += TY) {
            const f16x8 v = *row(t);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[ty][tx * 8 + e] = s[e];
    __syncthreads();
    const int cc = strip * 256 + threadIdx.x;
    float a = 0.f;
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) a += red[yy][threadIdx.x];
    if (cc < C) {
        if constexpr (DET) out[((int64_t)slab * gridDim.z + j) * C + cc] = a;
        else atomicAdd(out + (int64_t)j * C + cc, a);
    }
}

inline bool sizes_ok(int32_t B, int32_t F, int32_t S, int32_t Cc) {
    return B > 0 && B < 65536 && F > 0 && S > 0 && Cc > 0 && Cc % 8 == 0 && (int64_t)B * F * S * (Cc / 8) < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int ptb_abi_version(void) { return PT_BATCH_ABI_VERSION; }

extern "C" int ptb_add_rowvec_interleaved_f16(const void* x, const void* vec, int32_t B, int32_t F, int32_t S, int32_t Cc, void* y, void* stream) {
    PT_CHECK(x && vec && y, "ptb_add_rowvec_interleaved_f16: null pointer");
    PT_CHECK(sizes_ok(B, F, S, Cc), "ptb_add_rowvec_interleaved_f16: bad sizes (B=%d F=%d S=%d C=%d: C %% 8 == 0, B F S C / 8 < 2^31)", B, F, S, Cc);
    const int64_t n8 = (int64_t)B * F * S * (Cc / 8);
    int64_t blocks = (n8 + 1023) / 1024;                     // four chunks per thread
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(add_rowvec_interleaved_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const f16*)x, (const f16*)vec,
                       (uint32_t)n8, (uint32_t)(Cc / 8), (uint32_t)(F * S), (uint32_t)S, (uint32_t)B, (f16*)y);
    PT_LAUNCH_CHECK("ptb_add_rowvec_interleaved_f16");
    return 0;
}

static int colsum_interleaved_launch(const char* who, bool det, const void* dy, int32_t B, int32_t F, int32_t S, int32_t Cc, float* out, float* ws,
                                     int64_t ws_floats, void* stream) {
    PT_CHECK(dy && out, "%s: null pointer", who);
    PT_CHECK(sizes_ok(B, F, S, Cc), "%s: bad sizes (B=%d F=%d S=%d C=%d: C %% 8 == 0, B F S C / 8 < 2^31)", who, B, F, S, Cc);
    const int strips = (Cc + 255) / 256;
    const int64_t FS = (int64_t)F * S;
    const int rps = slab_rows(FS, (int64_t)strips * B, TY);
    const int slabs = (int)((FS + rps - 1) / rps);
    const dim3 grid(slabs, strips, B);
    hipStream_t s = (hipStream_t)stream;
    if (det) {
        const int64_t n = (int64_t)B * Cc;
        PT_CHECK_WS(who, ws, ws_floats, slabs * n);
        hipLaunchKernelGGL(colsum_interleaved_kernel<true>, grid, dim3(256), 0, s, (const f16*)dy, (uint32_t)F, (uint32_t)S, (uint32_t)B, rps, Cc, ws);
        launch_fold<float>(s, fold_job(ws, n, slabs, out, 1));
    } else {
        hipLaunchKernelGGL(colsum_interleaved_kernel<false>, grid, dim3(256), 0, s, (const f16*)dy, (uint32_t)F, (uint32_t)S, (uint32_t)B, rps, Cc, out);
    }
    PT_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int ptb_colsum_interleaved_f16(const void* dy, int32_t B, int32_t F, int32_t S, int32_t Cc, float* out, void* stream) {
    return colsum_interleaved_launch("ptb_colsum_interleaved_f16", false, dy, B, F, S, Cc, out, nullptr, 0, stream);
}

extern "C" int64_t ptb_colsum_interleaved_ws_floats(int32_t B, int32_t F, int32_t S, int32_t Cc) {
    if (!sizes_ok(B, F, S, Cc)) return 0;
    const int64_t FS = (int64_t)F * S;
    const int rps = slab_rows(FS, (int64_t)((Cc + 255) / 256) * B, TY);
    return (FS + rps - 1) / rps * B * Cc;
}

extern "C" int ptb_colsum_interleaved_det_f16(const void* dy, int32_t B, int32_t F, int32_t S, int32_t Cc, float* out, float* ws, int64_t ws_floats,
                                              void* stream) {
    return colsum_interleaved_launch("ptb_colsum_interleaved_det_f16", true, dy, B, F, S, Cc, out, ws, ws_floats, stream);
}
