// Host side of the training kernels' launches (norm_bwd.hip, pointwise_bwd.hip, optim.hip, batch.hip): the grid rules, the
// deterministic workspace's check and the body of a pointwise entry point, each written once.
#pragma once
#include "pt_common.h"

namespace {

// grid of a grid-stride pass over n units, one per thread of a 256-thread block
inline unsigned ew_blocks(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 16384) b = 16384;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// rows per slab of a column reduction whose blocks own `ty` rows at a time: ~4096 blocks in total (`other_blocks`: the grid's
// other two dimensions), at least 64 rows per slab, a multiple of ty
inline int slab_rows(int64_t rows, int64_t other_blocks, int ty) {
    int64_t slabs = 4096 / (other_blocks > 0 ? other_blocks : 1);
    if (slabs < 1) slabs = 1;
    int64_t rps = (rows + slabs - 1) / slabs;
    if (rps < 64) rps = 64;
    return (int)((rps + ty - 1) / ty * ty);
}

// the float workspace of a deterministic reduction (include/posetraj_det.h): present, 4-byte aligned, `need` floats at least
#define PT_CHECK_WS(who, ws, ws_floats, need)                                                                                  \
    PT_CHECK((ws) && ((uintptr_t)(ws) & 3) == 0 && (ws_floats) >= (need), "%s: the workspace holds %lld floats, %lld needed", who, \
             (long long)((ws) ? (ws_floats) : 0), (long long)(need))

// what is left of a pointwise entry point after its PT_CHECK: the 256-thread kernel on ew_blocks(units) blocks, the launch's status
template <typename... P, typename... A>
inline int launch_ew(const char* who, void (*kernel)(P...), int64_t units, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(ew_blocks(units)), dim3(256), 0, (hipStream_t)stream, args...);
    PT_LAUNCH_CHECK(who);
    return 0;
}

}  // namespace
