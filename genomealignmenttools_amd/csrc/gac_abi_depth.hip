// gac_abi_depth.hip -- libgachain's C ABI, coverage depth of ranges
// (gac_depth_count; the kernels and the method are in gac_depth.hip, the
// arguments' check is shared with the host twin, host/gac_depth.c).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>

#include "gac_ctx.h"
#include "gac_dp.h"

using namespace gac;

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int gac_depth_count(gac_ctx *c, int64_t n, const int32_t *seq, const int32_t *start,
                               const int32_t *end, const int8_t *delta, int32_t threshold,
                               int32_t *count) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    int32_t max_seq = 0;
    int rc = gac_depth_check(n, seq, start, end, delta, threshold, count, &max_seq);
    if (rc != GAC_OK || n == 0) return rc;
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t m = 2 * n;
    int end_bit = 32;  // the position, then the bits of the largest sequence id
    while (end_bit < 64 && ((int64_t)max_seq >> (end_bit - 32)) != 0) ++end_bit;

    // one allocation: the inputs, the event arrays, the sort and scan scratch
    size_t b_sort = 0, b_s32 = 0, b_s64 = 0;
    HIPCHK(dt_sort_pairs(nullptr, b_sort, nullptr, nullptr, nullptr, nullptr, m, end_bit, s));
    HIPCHK(dt_scan32(nullptr, b_s32, nullptr, nullptr, m, s));
    HIPCHK(dt_scan64(nullptr, b_s64, nullptr, nullptr, m, s));
    const size_t b_tmp = std::max(b_sort, std::max(b_s32, b_s64));
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += up256(bytes);
        return o;
    };
    const size_t o_seq = take((size_t)n * 4), o_start = take((size_t)n * 4), o_end = take((size_t)n * 4);
    const size_t o_delta = take((size_t)n), o_count = take((size_t)n * 4);
    const size_t o_key = take((size_t)m * 8), o_skey = take((size_t)m * 8);
    const size_t o_val = take((size_t)m * 4), o_sval = take((size_t)m * 4);
    const size_t o_sdelta = take((size_t)m * 4), o_excl = take((size_t)m * 4);
    const size_t o_where = take((size_t)m * 4), o_before = take((size_t)m * 8);
    const size_t o_tmp = take(b_tmp);
    char *d = nullptr;
    HIPCHK(hipMalloc(&d, off));

    DepthArgs a;
    a.n = n;
    a.threshold = threshold;
    a.seq = (const int32_t *)(d + o_seq);
    a.start = (const int32_t *)(d + o_start);
    a.end = (const int32_t *)(d + o_end);
    a.delta = (const int8_t *)(d + o_delta);
    a.key = (unsigned long long *)(d + o_key);
    a.val = (int32_t *)(d + o_val);
    a.skey = (const unsigned long long *)(d + o_skey);
    a.sval = (const int32_t *)(d + o_sval);
    a.sdelta = (int32_t *)(d + o_sdelta);
    a.where = (int32_t *)(d + o_where);
    a.excl = (const int32_t *)(d + o_excl);
    a.len = (long long *)(d + o_key);  // the unsorted keys are done with by then
    a.before = (const long long *)(d + o_before);
    a.count = (int32_t *)(d + o_count);

    hipError_t e = hipMemcpyAsync(d + o_seq, seq, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_start, start, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_end, end, (size_t)n * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_delta, delta, (size_t)n, hipMemcpyHostToDevice, s);
    {
        PROF_BEGIN(GAC_K_DEPTH);
        size_t b = b_tmp;
        if (e == hipSuccess) e = launch_depth_events(a, s);
        if (e == hipSuccess)
            e = dt_sort_pairs(d + o_tmp, b, a.key, (unsigned long long *)(d + o_skey), a.val,
                              (int32_t *)(d + o_sval), m, end_bit, s);
        if (e == hipSuccess) e = launch_depth_gather(a, s);
        b = b_tmp;
        if (e == hipSuccess) e = dt_scan32(d + o_tmp, b, a.sdelta, (int32_t *)(d + o_excl), m, s);
        if (e == hipSuccess) e = launch_depth_cover(a, s);
        b = b_tmp;
        if (e == hipSuccess) e = dt_scan64(d + o_tmp, b, a.len, (long long *)(d + o_before), m, s);
        if (e == hipSuccess) e = launch_depth_out(a, s);
        PROF_END(GAC_K_DEPTH);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(count, a.count, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // before the buffer goes, whatever e says
    if (e == hipSuccess) e = e2;
    hipFree(d);
    if (e != hipSuccess)
        return gac_fail(GAC_E_HIP, "gac_depth_count failed: %s", hipGetErrorString(e));
    return GAC_OK;
}
