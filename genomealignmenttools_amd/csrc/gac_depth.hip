// gac_depth.hip -- coverage depth of ranges (gac_depth_count; netSyntenic's
// qDup, kent/src/hg/mouseStuff/netSyntenic/netSyntenic.c:63-138): how many
// positions of each range lie under a summed depth of at least `threshold`.
// gfx950 only.
//
// The reference keeps a red-black tree of depth runs per sequence and edits it
// range by range.  Only the per-base sum matters, so here every range becomes
// two events, (seq << 32 | start, +delta) and (seq << 32 | end, -delta); the
// events are sorted by key, a scan of the signed deltas gives the depth after
// every event, the stretch to the next event of the same sequence counts when
// that depth reaches the threshold, a 64-bit scan of those lengths gives the
// covered length before every event, and a range's count is the difference of
// the two values at its own end and start events.  Events at one position are
// separated by stretches of length 0, so their order does not matter, and a
// range of length 0 has nothing between its events that is longer than 0.
// Every range adds +d and -d: the depth is back at 0 after the last event of a
// sequence, and the depth scan needs no segments.
//
// The kernels are element-wise over the 2n events (k_depth_out: the n
// ranges): one event per lane, grid-stride, 256-thread workgroups, coalesced
// loads and stores but for the gathers through the sorted order.  The sort and
// the two scans are the shared wrappers (dt_sort_pairs, dt_scan32, dt_scan64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kDepthThreads = 256;
constexpr int64_t kDepthMaxGrid = 2048;  // workgroups; the rest by grid stride

__device__ __forceinline__ int64_t depth_id() {
    return (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
}

__device__ __forceinline__ int64_t depth_stride() { return (int64_t)gridDim.x * kDepthThreads; }

// event e < n: the start of range e; event n + i: the end of range i
__global__ void __launch_bounds__(kDepthThreads)
    k_depth_events(DepthArgs a) {
    const int64_t n = a.n;
    for (int64_t e = depth_id(); e < 2 * n; e += depth_stride()) {
        const int64_t i = e < n ? e : e - n;
        const uint32_t pos = (uint32_t)(e < n ? a.start[i] : a.end[i]);
        a.key[e] = ((unsigned long long)(uint32_t)a.seq[i] << 32) | pos;
        a.val[e] = (int32_t)e;
    }
}

// per sorted position k: the signed delta of its event, and where the event went
__global__ void __launch_bounds__(kDepthThreads)
    k_depth_gather(DepthArgs a) {
    const int64_t n = a.n;
    for (int64_t k = depth_id(); k < 2 * n; k += depth_stride()) {
        const int32_t e = a.sval[k];
        const int32_t d = e < n ? (int32_t)a.delta[e] : -(int32_t)a.delta[e - n];
        a.sdelta[k] = d;
        a.where[e] = (int32_t)k;
    }
}

// per sorted position k: the length from event k to event k + 1 if both are
// of one sequence and the depth after event k reaches the threshold
__global__ void __launch_bounds__(kDepthThreads)
    k_depth_cover(DepthArgs a) {
    const int64_t m = 2 * a.n;
    for (int64_t k = depth_id(); k < m; k += depth_stride()) {
        long long len = 0;
        if (k + 1 < m) {
            const unsigned long long k0 = a.skey[k], k1 = a.skey[k + 1];
            const int32_t depth = a.excl[k] + a.sdelta[k];
            if ((k0 >> 32) == (k1 >> 32) && depth >= a.threshold) len = (long long)(k1 - k0);
        }
        a.len[k] = len;
    }
}

__global__ void __launch_bounds__(kDepthThreads)
    k_depth_out(DepthArgs a) {
    const int64_t n = a.n;
    for (int64_t i = depth_id(); i < n; i += depth_stride())
        a.count[i] = (int32_t)(a.before[a.where[n + i]] - a.before[a.where[i]]);
}

unsigned depth_grid(int64_t items) {
    const int64_t g = (items + kDepthThreads - 1) / kDepthThreads;
    return (unsigned)(g < 1 ? 1 : g > kDepthMaxGrid ? kDepthMaxGrid : g);
}

}  // namespace

hipError_t launch_depth_events(const DepthArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_events, dim3(depth_grid(2 * a.n)), dim3(kDepthThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_depth_gather(const DepthArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_gather, dim3(depth_grid(2 * a.n)), dim3(kDepthThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_depth_cover(const DepthArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_cover, dim3(depth_grid(2 * a.n)), dim3(kDepthThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_depth_out(const DepthArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_out, dim3(depth_grid(a.n)), dim3(kDepthThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace gac
