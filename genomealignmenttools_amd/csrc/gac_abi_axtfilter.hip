// gac_abi_axtfilter.hip -- libgachain's C ABI, filterAxtIdentityEntropy's keep
// decision (gac_axt_filter: src/filterAxtIdentityEntropy.py:88-110 checkAxt,
// :41-69 getSeqIdent and getEntropy, :144-162 the column counts; the kernel and
// the method are in gac_axtfilter.hip, the arguments' check, the two host-made
// tables and the host twin in host/gac_axtfilter.c).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gac_ctx.h"

using namespace gac;

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int gac_axt_filter(gac_ctx *c, int64_t n, const char *text, int64_t text_bytes,
                              const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                              double min_ident, double min_entropy, int32_t window, uint8_t *keep,
                              gac_axtfilter_stats *st) {
    gac_clear_error();
    if (st) memset(st, 0, sizeof(*st));
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    // GAC_TIMING: where the call's time goes (the stream is synchronised after
    // every step then, so that a lap is that step's alone)
    const bool timing = getenv("GAC_TIMING") != nullptr;
    double t_lap = wall_s();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const double t = wall_s();
        fprintf(stderr, "[gac_axt_filter] %-24s %.3f s\n", what, t - t_lap);
        t_lap = t;
    };
    int rc = gac_axtf_check(n, text, text_bytes, t_off, q_off, len, window, keep);
    if (rc != GAC_OK || n == 0) return rc;
    if (window > GAC_AXTF_MAX_WINDOW) {  // the tile bound of the packed counters
        rc = gac_axt_filter_host(n, text, text_bytes, t_off, q_off, len, min_ident, min_entropy,
                                 window, 0, keep, st);
        if (rc == GAC_OK && st) st->fell_back = 1;
        return rc;
    }
    const int64_t W = window, CH = kAxtfTile - W;
    const int32_t m_min = gac_axtf_mmin(min_ident, window);
    double *term = gac_axtf_terms(window);
    if (!term) return gac_fail(GAC_E_ARG, "gac_axt_filter: out of memory");
    const size_t term_bytes = (size_t)(W * (W + 1) / 2) * sizeof(double);
    struct FreeTerm {
        double *p;
        ~FreeTerm() { free(p); }
    } free_term{term};
    lap("check + tables");

    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;

    int64_t budget = 0;
    HIPCHK(axt_batch_budget("GAC_AXTF_BATCH_BYTES", &budget));

    // the batches (gac_ctx.h); an entry shorter than the window has no chunk and is never kept
    AxtPlan plan;
    int64_t windows = 0;
    for (int64_t i = 0; i < n; ++i) {
        keep[i] = 0;
        if (len[i] >= W) windows += len[i] - W + 1;
    }
    axt_plan_batches(n, t_off, q_off, len, budget, [&](int64_t i) { return len[i] < W; }, plan);
    const std::vector<AxtBatch> &batches = plan.batches;
    const std::vector<int64_t> &host_idx = plan.host_idx;
    const int64_t n_dev = plan.n_dev, max_n = plan.max_n, max_bytes = plan.max_bytes;
    lap("batches");

    std::vector<uint32_t> flags((size_t)n_dev, 0u);
    if (n_dev > 0) {
        // one allocation: the batch's text, its records, the flags of every
        // uploaded entry of the call, the terms
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t o = off;
            off += up256(bytes);
            return o;
        };
        const size_t o_text = take((size_t)max_bytes + 256);
        const size_t o_ent = take((size_t)(max_n + 1) * sizeof(AxtfEntry));
        const size_t o_keep = take((size_t)n_dev * 4);
        const size_t o_term = take(term_bytes);
        char *d = nullptr;
        {
            const hipError_t e = hipMalloc(&d, off);
            if (e != hipSuccess)
                return gac_fail(GAC_E_HIP, "gac_axt_filter: %lld bytes of device memory: %s",
                                (long long)off, hipGetErrorString(e));
        }
        auto fail = [&](hipError_t e) {
            hipStreamSynchronize(s);  // before the buffers go
            hipFree(d);
            return gac_fail(GAC_E_HIP, "gac_axt_filter failed: %s", hipGetErrorString(e));
        };
        auto fail_rc = [&](int r) {
            hipStreamSynchronize(s);
            hipFree(d);
            return r;
        };
        hipError_t e = hipMemsetAsync(d + o_keep, 0, (size_t)n_dev * 4, s);
        if (e != hipSuccess) return fail(e);
        rc = upload_staged(c, d + o_term, term, term_bytes);
        if (rc != GAC_OK) return fail_rc(rc);
        lap("hipMalloc + terms");

        AxtfArgs a;
        memset(&a, 0, sizeof(a));
        a.text = (const uint8_t *)(d + o_text);
        a.ent = (const AxtfEntry *)(d + o_ent);
        a.window = window;
        a.m_min = m_min;
        a.term = (const double *)(d + o_term);
        a.ln2 = log(2.0);
        a.min_entropy = min_entropy;

        std::vector<AxtfEntry> ent;
        double up_s = 0, k_s = 0;
        int64_t up_bytes = 0, done = 0;
        size_t next_host = 0;
        for (const AxtBatch &b : batches) {
            // where the spans go in the batch's buffer, and the records against that
            const AxtSpans &sp = b.sp;
            const int64_t t_base = sp.t_base(), q_base = sp.q_base();
            ent.clear();
            int64_t chunks = 0;
            for (int64_t i = b.first; i < b.end; ++i) {
                const int64_t L = len[i];
                if (L < W) continue;
                if (next_host < host_idx.size() && host_idx[next_host] == i) {
                    ++next_host;
                    continue;
                }
                ent.push_back(AxtfEntry{t_base + (t_off[i] - sp.tlo), q_base + (q_off[i] - sp.qlo),
                                        len[i], 0, chunks});
                chunks += (L - W + 1 + CH - 1) / CH;
            }
            ent.push_back(AxtfEntry{0, 0, 0, 0, chunks});
            a.text_bytes = sp.bytes();
            a.n = b.n;
            a.keep = (uint32_t *)(d + o_keep) + done;

            const double t0 = timing ? wall_s() : 0;
            rc = axt_upload_spans(c, d + o_text, text, sp);
            if (rc == GAC_OK) rc = upload_staged(c, d + o_ent, ent.data(), ent.size() * sizeof(AxtfEntry));
            if (rc != GAC_OK) return fail_rc(rc);
            up_bytes += sp.bytes() + (int64_t)(ent.size() * sizeof(AxtfEntry));
            if (timing) {
                hipStreamSynchronize(s);
                up_s += wall_s() - t0;
            }
            const double t1 = timing ? wall_s() : 0;
            {
                PROF_BEGIN(GAC_K_AXTFILTER);
                e = launch_axt_filter(a, chunks, s);
                PROF_END(GAC_K_AXTFILTER);
            }
            if (e != hipSuccess) return fail(e);
            if (timing) {
                e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail(e);
                k_s += wall_s() - t1;
            }
            done += b.n;
        }
        if (timing) {
            fprintf(stderr, "[gac_axt_filter] %-24s %.3f s  (%lld bytes in %d batches: %.2f GB/s)\n",
                    "upload", up_s, (long long)up_bytes, (int)batches.size(),
                    up_s > 0 ? 1e-9 * (double)up_bytes / up_s : 0.0);
            fprintf(stderr, "[gac_axt_filter] %-24s %.3f s  (%.2f GB/s of uploaded text)\n", "kernels", k_s,
                    k_s > 0 ? 1e-9 * (double)up_bytes / k_s : 0.0);
            t_lap = wall_s();
        }
        e = hipMemcpyAsync(flags.data(), d + o_keep, (size_t)n_dev * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(e);
        hipFree(d);
        lap("download + hipFree");
    }

    // the flags back to their entries, in the order they were uploaded
    int64_t kept = 0;
    {
        int64_t k = 0;
        size_t next_host = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (len[i] < W) continue;
            if (next_host < host_idx.size() && host_idx[next_host] == i) {
                ++next_host;
                continue;
            }
            keep[i] = flags[(size_t)k++] != 0;
            kept += keep[i];
        }
    }
    if (!host_idx.empty()) {  // entries alone over the budget: the host twin decides them
        const size_t h = host_idx.size();
        std::vector<int64_t> ht(h), hq(h);
        std::vector<int32_t> hl(h);
        std::vector<uint8_t> hk(h);
        for (size_t k = 0; k < h; ++k)
            ht[k] = t_off[host_idx[k]], hq[k] = q_off[host_idx[k]], hl[k] = len[host_idx[k]];
        rc = gac_axt_filter_host((int64_t)h, text, text_bytes, ht.data(), hq.data(), hl.data(), min_ident,
                                 min_entropy, window, 0, hk.data(), nullptr);
        if (rc != GAC_OK) return rc;
        for (size_t k = 0; k < h; ++k) {
            keep[host_idx[k]] = hk[k];
            kept += hk[k];
        }
        lap("host twin (over budget)");
    }
    if (st) {
        st->kept = kept;
        st->windows = windows;
        st->host_entries = (int64_t)host_idx.size();
        st->batches = (int32_t)batches.size();
        st->fell_back = host_idx.empty() ? 0 : 2;
    }
    lap("flags");
    return GAC_OK;
}
