// gac_abi_context.hip -- libgachain's C ABI (include/gachain.h), the context:
// gac_open / gac_close, the scoring setup, device memory and copies, the
// kernel profiler.  There is deliberately no host fallback: every entry point
// of gac_device.hip and the gac_abi_*.hip units runs HIP kernels on a gfx950 device or returns an
// error.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "gac_ctx.h"

using namespace gac;

// ----------------------------------------------------------------- context
extern "C" int gac_open(int device, gac_ctx **out) {
    gac_clear_error();
    if (!out) return gac_fail(GAC_E_ARG, "gac_open: NULL out");
    *out = nullptr;
    const bool timing = getenv("GAC_TIMING") != nullptr;
    auto t_now = [] {
        struct timespec ts;
        clock_gettime(CLOCK_MONOTONIC, &ts);
        return ts.tv_sec + 1e-9 * ts.tv_nsec;
    };
    double t_mark = t_now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const double t = t_now();
        fprintf(stderr, "[gac_open] %-28s %.3f s\n", what, t - t_mark);
        t_mark = t;
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    lap("hipGetDeviceCount (HIP init)");
    if (e != hipSuccess || n == 0)
        return gac_fail(GAC_E_HIP, "no HIP device available (%s); libgachain has no CPU fallback",
                        hipGetErrorString(e));
    if (device < 0 || device >= n)
        return gac_fail(GAC_E_ARG, "device %d out of range (%d devices)", device, n);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    lap("hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return gac_fail(GAC_E_HIP, "device %d is %s; libgachain is built for gfx950 only", device,
                        prop.gcnArchName);
    HIPCHK(hipSetDevice(device));
    lap("hipSetDevice");
    gac_ctx *c = new gac_ctx();
    c->device = device;
    snprintf(c->arch, sizeof(c->arch), "%s", prop.gcnArchName);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return gac_fail(GAC_E_HIP, "hipStreamCreate failed");
    }
    if (hipEventCreateWithFlags(&c->ws_ev, hipEventDisableTiming) != hipSuccess) {
        hipStreamDestroy(c->stream);
        delete c;
        return gac_fail(GAC_E_HIP, "hipEventCreate failed");
    }
    lap("hipStreamCreate");
    c->combine_grid = prop.multiProcessorCount * 8;  // k_fold_tiles: 32 waves per CU
    for (int sym = 0; sym < 2; ++sym)
        for (int l = 0; l < 2; ++l)
            c->tile_grid_sym[sym][l] = prop.multiProcessorCount * persistent_blocks_per_cu(l, sym);
    lap("occupancy (code object)");
    if (hipHostMalloc((void **)&c->h_stat, 64, hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_h_stat, c->h_stat, 0) != hipSuccess) {
        hipStreamDestroy(c->stream);
        delete c;
        return gac_fail(GAC_E_HIP, "hipHostMalloc failed");
    }
    if (hipHostMalloc((void **)&c->h_small_in, kSmallMax * sizeof(Range), hipHostMallocMapped) !=
            hipSuccess ||
        hipHostMalloc((void **)&c->h_small_out, kSmallMax * sizeof(SmallOut),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_small_in, c->h_small_in, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->d_small_out, c->h_small_out, 0) != hipSuccess) {
        gac_close(c);
        return gac_fail(GAC_E_HIP, "hipHostMalloc failed");
    }
    if (const char *v = getenv("GAC_SMALL_MAX")) {
        const int m = atoi(v);
        c->small_max = m < 0 ? 0 : (m > kSmallMax ? kSmallMax : m);
    }
    c->srv.on = true;  // (GAC_SMALL_SERVER=0: a launch per small batch)
    if (const char *v = getenv("GAC_SMALL_SERVER")) c->srv.on = v[0] != '0';
    if (const char *v = getenv("GAC_SRV_WGS")) {
        const int w = atoi(v);
        if (w >= 1 && w <= kSrvWaves / kWavesPerWG) c->srv.wgs = w;
    }
    if (const char *v = getenv("GAC_SMALL_SERVER_IDLE_US")) {
        const long long us = atoll(v);
        if (us > 0 && us <= 10000000) c->srv.idle = (uint64_t)us * 100;
    }
    lap("hipHostMalloc");
    *out = c;
    return GAC_OK;
}

extern "C" void gac_close(gac_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        srv_park(c);
        if (c->srv.launches && getenv("GAC_TIMING"))
            fprintf(stderr, "[gac_close] small-batch server: %lld requests, %lld launches\n",
                    (long long)c->srv.requests, (long long)c->srv.launches);
        if (c->srv.d_sync && getenv("GAC_SRV_TRACE")) {  // (the last grid's phase sums)
            SmallSync t;
            if (hipMemcpy(&t, c->srv.d_sync, sizeof(t), hipMemcpyDeviceToHost) == hipSuccess &&
                t.pad[15])
                fprintf(stderr, "[gac_close] server phases (us after the poll saw the request, "
                                "mean of %u): broadcast %.2f, all saw %.2f, "
                                "work %.2f, fenced %.2f, done %.2f; polls %.1f\n",
                        t.pad[15], 0.01 * t.pad[8] / t.pad[15], 0.01 * t.pad[9] / t.pad[15],
                        0.01 * t.pad[11] / t.pad[15],
                        0.01 * t.pad[12] / t.pad[15], 0.01 * t.pad[13] / t.pad[15],
                        (double)t.pad[14] / t.pad[15]);
        }
        srv_free(c);
    }
    hipStreamSynchronize(c->stream);
    {
        CTX_LOCK(c);
        for (gac_chainset *cs : c->sets) {
            free_set_memory(cs);
            cs->ctx = nullptr;
        }
        c->sets.clear();
    }
    axt_release(c);
    free_genome(c->g[0]);
    free_genome(c->g[1]);
    void *bufs[] = {c->d_small,  c->d_gap_tab, c->rdesc,    c->nblk,     c->goff, c->pb0, c->agg, c->plan_off, c->lbflag, c->gflat,
                    c->status,   c->tile_r0,  c->sum_head, c->sum_tail,
                    c->sup_head, c->sup_tail, c->sup_tail_r,
                    c->d_ranges, c->d_g,      c->d_l,      c->d_ali};
    for (void *p : bufs)
        if (p) hipFree(p);
    for (auto &p : c->prof_pending) {
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    for (auto ev : c->prof_free) hipEventDestroy(ev);
    if (c->h_stat) hipHostFree(c->h_stat);
    gac_gapcalc_free(c->gap_src);
    if (c->h_small_in) hipHostFree(c->h_small_in);
    if (c->h_small_out) hipHostFree(c->h_small_out);
    if (c->h_hq) hipHostFree(c->h_hq);
    if (c->h_pool) hipHostFree(c->h_pool);
    for (int k = 0; k < 2; ++k) {
        if (c->pin[k]) hipHostFree(c->pin[k]);
        if (c->pin_ev[k]) hipEventDestroy(c->pin_ev[k]);
    }
    if (c->ws_ev) hipEventDestroy(c->ws_ev);
    hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const char *gac_device_arch(gac_ctx *c) { return c ? c->arch : ""; }

// ----------------------------------------------------------------- scoring
extern "C" int gac_set_scoring(gac_ctx *c, const int32_t mat[16], const gac_gapcalc *g) {
    gac_clear_error();
    if (!c || !mat || !g) return gac_fail(GAC_E_ARG, "gac_set_scoring: NULL argument");
    CTX_LOCK(c);
    if (g->long_count < 2 || g->long_count > kMaxLong)
        return gac_fail(GAC_E_ARG, "gap table has %d long positions (2..%d supported)",
                        g->long_count, kMaxLong);
    if (g->small_size < 1 || g->small_size != g->long_pos[0])
        return gac_fail(GAC_E_ARG, "inconsistent gap table (smallSize %d)", g->small_size);
    HIPCHK(hipSetDevice(c->device));
    // the same setup again (a batch of jobs): tables, gap version and the
    // chain sets' per-block gaps stay valid
    if (c->scoring && memcmp(c->mat, mat, sizeof(c->mat)) == 0 && gac_gapcalc_same(c->gap_src, g))
        return GAC_OK;
    // the kernel multiplies basis coefficients (|c| <= 16 max|s|) by counts
    // <= 32 in 24 bits (v_mad_i32_i24) and sums 16 terms in int32
    for (int i = 0; i < 16; ++i)
        if (mat[i] <= -(1 << 17) || mat[i] >= (1 << 17))
            return gac_fail(GAC_E_ARG, "score matrix entry %d out of range (|s| < 2^17)", mat[i]);
    // f(S) = M[q][t] at t1,t0,d1,d0 = bits of S (q = t ^ d); Moebius transform
    // to the multilinear coefficients
    int32_t f[16];
    for (int S = 0; S < 16; ++S) {
        const int t = S >> 2, q = t ^ (S & 3);
        f[S] = mat[acgt_of_code(q) * 4 + acgt_of_code(t)];
    }
    for (int S = 0; S < 16; ++S) {
        int32_t cs = 0;
        for (int T = 0; T < 16; ++T)
            if ((T & S) == T) cs += (__builtin_popcount(S ^ T) & 1) ? -f[T] : f[T];
        c->coef[S] = cs;
    }
    c->sym = 1;
    for (int S = 8; S < 16; ++S)
        if (c->coef[S]) c->sym = 0;
    GapDev &d = c->gap;
    memset(&d, 0, sizeof(d));
    d.small_size = g->small_size;
    d.long_count = g->long_count;
    d.last_pos[0] = g->q_last_pos;
    d.last_pos[1] = g->t_last_pos;
    d.last_pos[2] = g->b_last_pos;
    d.last_val[0] = g->q_last_val;
    d.last_val[1] = g->t_last_val;
    d.last_val[2] = g->b_last_val;
    d.last_slope[0] = g->q_last_slope;
    d.last_slope[1] = g->t_last_slope;
    d.last_slope[2] = g->b_last_slope;
    for (int i = 0; i < g->long_count; ++i) {
        d.long_pos[i] = g->long_pos[i];
        d.long_val[0][i] = g->q_long[i];
        d.long_val[1][i] = g->t_long[i];
        d.long_val[2][i] = g->b_long[i];
    }
    std::vector<int32_t> small(3 * (size_t)g->small_size);
    memcpy(small.data(), g->q_small, g->small_size * 4);
    memcpy(small.data() + g->small_size, g->t_small, g->small_size * 4);
    memcpy(small.data() + 2 * g->small_size, g->b_small, g->small_size * 4);
    if (c->d_small) hipFree(c->d_small);
    c->d_small = nullptr;
    HIPCHK(hipMalloc(&c->d_small, small.size() * 4));
    HIPCHK(hipMemcpy(c->d_small, small.data(), small.size() * 4, hipMemcpyHostToDevice));
    // gap-cost table up to the last table position (everything beyond is the
    // slope branch); capped at GAC_GAP_TABLE_MAX entries per kind (default
    // 2^22) -- lengths past a capped table are evaluated in the kernel
    int64_t len = std::max(std::max(g->q_last_pos, g->t_last_pos), g->b_last_pos);
    int64_t cap = 1 << 22;
    if (const char *env = getenv("GAC_GAP_TABLE_MAX")) cap = std::max(1LL, atoll(env));
    len = std::max<int64_t>(g->small_size, std::min(len, cap));
    if (c->d_gap_tab) hipFree(c->d_gap_tab);
    c->d_gap_tab = nullptr;
    HIPCHK(hipMalloc(&c->d_gap_tab, 3 * len * 4));
    HIPCHK(launch_gap_table(d, c->d_small, (int)len, c->d_gap_tab, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->gap_len = (int)len;
    ++c->gap_version;
    memcpy(c->mat, mat, sizeof(c->mat));
    gac_gapcalc_free(c->gap_src);
    c->gap_src = gac_gapcalc_clone(g);
    c->scoring = true;
    return GAC_OK;
}

double gac::wall_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

// ----------------------------------------------------------------- memory
extern "C" int gac_dev_alloc(gac_ctx *c, size_t bytes, void **p) {
    if (!c || !p) return gac_fail(GAC_E_ARG, "NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(p, bytes ? bytes : 16));
    return GAC_OK;
}
extern "C" int gac_dev_free(gac_ctx *c, void *p) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    if (p) HIPCHK(hipFree(p));
    return GAC_OK;
}
extern "C" int gac_memcpy_h2d(gac_ctx *c, void *dst, const void *src, size_t n) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GAC_OK;
}
extern "C" int gac_memcpy_d2h(gac_ctx *c, void *dst, const void *src, size_t n) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GAC_OK;
}
extern "C" int gac_synchronize(gac_ctx *c) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    return GAC_OK;
}

// ----------------------------------------------------------------- profiling
extern "C" int gac_prof_enable(gac_ctx *c, int on) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    c->prof = on & GAC_PROF_ALL;
    return GAC_OK;
}

hipEvent_t gac::prof_event(gac_ctx *c) {
    if (!c->prof_free.empty()) {
        hipEvent_t e = c->prof_free.back();
        c->prof_free.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}

static int prof_fold(gac_ctx *c) {
    for (auto &p : c->prof_pending) {
        HIPCHK(hipEventSynchronize(p.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        c->prof_ms[p.kernel] += ms;
        c->prof_n[p.kernel] += 1;
        c->prof_free.push_back(p.a);
        c->prof_free.push_back(p.b);
    }
    c->prof_pending.clear();
    return GAC_OK;
}

extern "C" int gac_prof_read(gac_ctx *c, int k, double *ms, int64_t *n) {
    if (!c || k < 0 || k >= GAC_K_COUNT) return gac_fail(GAC_E_ARG, "bad argument");
    CTX_LOCK(c);
    int rc = prof_fold(c);
    if (rc != GAC_OK) return rc;
    if (ms) *ms = c->prof_ms[k];
    if (n) *n = c->prof_n[k];
    return GAC_OK;
}

extern "C" int gac_prof_reset(gac_ctx *c) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    int rc = prof_fold(c);
    if (rc != GAC_OK) return rc;
    for (int k = 0; k < GAC_K_COUNT; ++k) {
        c->prof_ms[k] = 0;
        c->prof_n[k] = 0;
    }
    return GAC_OK;
}
