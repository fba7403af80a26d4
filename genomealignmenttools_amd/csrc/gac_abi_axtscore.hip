// gac_abi_axtscore.hip -- libgachain's C ABI, axtToMaf's scores
// (gac_axt_score: kent/src/lib/axt.c:196-229 axtScoreSym under :423-458
// axtScoreSchemeDefault; the kernels and the method are in gac_axtscore.hip,
// the arguments' check and the host twin in host/gac_axtscore.c, the batches
// in gac_ctx.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gac_ctx.h"
#include "gac_dp.h"

using namespace gac;

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

namespace {

// what a call holds until it returns
struct Held {
    hipStream_t s = nullptr;
    char *d = nullptr;
    ~Held() {
        if (d) {
            hipStreamSynchronize(s);  // before the buffer goes
            hipFree(d);
        }
    }
};

}  // namespace

extern "C" int gac_axt_score(gac_ctx *c, int64_t n, const char *text, int64_t text_bytes,
                             const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                             int32_t *score, gac_axtscore_stats *st) {
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
        fprintf(stderr, "[gac_axt_score] %-24s %.3f s\n", what, t - t_lap);
        t_lap = t;
    };
    int rc = gac_axtscore_check(n, text, text_bytes, t_off, q_off, len, score);
    if (rc != GAC_OK) return rc;
    if (n == 0) return GAC_OK;
    lap("check");

    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Held H;
    H.s = s;

    int64_t budget = 0;
    HIPCHK(axt_batch_budget("GAC_AXTSCORE_BATCH_BYTES", &budget));
    AxtPlan plan;
    axt_plan_batches(n, t_off, q_off, len, budget, [](int64_t) { return false; }, plan);
    const std::vector<int64_t> &host_idx = plan.host_idx;
    lap("batches");

    if (!host_idx.empty()) {  // entries alone over the budget: the host twin scores them
        const size_t h = host_idx.size();
        std::vector<int64_t> ht(h), hq(h);
        std::vector<int32_t> hl(h), hs(h);
        for (size_t k = 0; k < h; ++k)
            ht[k] = t_off[host_idx[k]], hq[k] = q_off[host_idx[k]], hl[k] = len[host_idx[k]];
        rc = gac_axt_score_host((int64_t)h, text, text_bytes, ht.data(), hq.data(), hl.data(), 0, hs.data(), nullptr);
        if (rc != GAC_OK) return rc;
        for (size_t k = 0; k < h; ++k) score[host_idx[k]] = hs[k];
        lap("host twin (over budget)");
    }

    if (plan.n_dev > 0) {
        // one allocation: the batch's text (and the words the kernel's aligned
        // loads may touch past it), its records, the chunk counts, their scan,
        // the scores
        size_t b_scan = 0;
        HIPCHK(dt_scan64(nullptr, b_scan, nullptr, nullptr, plan.max_n + 1, s));
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t o = off;
            off += up256(bytes);
            return o;
        };
        const size_t o_text = take((size_t)plan.max_bytes + 256);
        const size_t o_ent = take((size_t)plan.max_n * sizeof(AxtsEntry));
        const size_t o_nch = take((size_t)(plan.max_n + 1) * 8);
        const size_t o_ch0 = take((size_t)(plan.max_n + 1) * 8);
        const size_t o_score = take((size_t)plan.max_n * 4);
        const size_t o_tmp = take(b_scan);
        {
            const hipError_t e = hipMalloc(&H.d, off);
            if (e != hipSuccess) {
                H.d = nullptr;
                return gac_fail(GAC_E_HIP, "gac_axt_score: %lld bytes of device memory: %s", (long long)off,
                                hipGetErrorString(e));
            }
        }
        char *d = H.d;
        auto fail = [&](hipError_t e) { return gac_fail(GAC_E_HIP, "gac_axt_score failed: %s", hipGetErrorString(e)); };
        lap("hipMalloc");

        AxtsArgs a;
        memset(&a, 0, sizeof(a));
        a.text = (const uint8_t *)(d + o_text);
        a.ent = (const AxtsEntry *)(d + o_ent);
        a.nchunk = (long long *)(d + o_nch);
        a.chunk0 = (const long long *)(d + o_ch0);
        a.score = (uint32_t *)(d + o_score);

        std::vector<AxtsEntry> ent;
        std::vector<int32_t> tmp;
        double up_s = 0, k_s = 0, dn_s = 0;
        int64_t up_bytes = 0;
        size_t next_host = 0;  // into host_idx
        for (const AxtBatch &b : plan.batches) {
            while (next_host < host_idx.size() && host_idx[next_host] < b.first) ++next_host;
            const AxtSpans &sp = b.sp;
            const int64_t t_base = sp.t_base(), q_base = sp.q_base();
            const bool mixed = b.end - b.first != b.n;  // entries of the host twin among them
            ent.clear();
            long long want_chunks = 0;
            {
                size_t nh = next_host;
                for (int64_t i = b.first; i < b.end; ++i) {
                    if (nh < host_idx.size() && host_idx[nh] == i) {
                        ++nh;
                        continue;
                    }
                    ent.push_back(AxtsEntry{t_base + (t_off[i] - sp.tlo), q_base + (q_off[i] - sp.qlo), len[i], 0});
                    want_chunks += ((long long)len[i] + kAxtsChunk - 1) / kAxtsChunk;
                }
            }
            a.text_bytes = sp.bytes();
            a.n = b.n;

            const double t0 = timing ? wall_s() : 0;
            rc = axt_upload_spans(c, d + o_text, text, sp);
            if (rc == GAC_OK) rc = upload_staged(c, d + o_ent, ent.data(), ent.size() * sizeof(AxtsEntry));
            if (rc != GAC_OK) return rc;
            up_bytes += sp.bytes() + (int64_t)(ent.size() * sizeof(AxtsEntry));
            if (timing) {
                hipStreamSynchronize(s);
                up_s += wall_s() - t0;
            }
            const double t1 = timing ? wall_s() : 0;
            {
                long long chunks = 0;
                PROF_BEGIN(GAC_K_AXTSCORE);
                hipError_t e = hipMemsetAsync(a.nchunk + b.n, 0, 8, s);
                if (e == hipSuccess) e = hipMemsetAsync(a.score, 0, (size_t)b.n * 4, s);
                if (e == hipSuccess) e = launch_axt_score_chunks(a, s);
                size_t bytes = b_scan;
                if (e == hipSuccess) e = dt_scan64(d + o_tmp, bytes, a.nchunk, (long long *)(d + o_ch0), b.n + 1, s);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(&chunks, a.chunk0 + b.n, 8, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail(e);
                if (chunks != want_chunks)
                    return gac_fail(GAC_E_HIP, "gac_axt_score: %lld chunks for %lld entries, not %lld", chunks,
                                    (long long)b.n, want_chunks);
                e = launch_axt_score(a, chunks, s);
                PROF_END(GAC_K_AXTSCORE);
                if (e != hipSuccess) return fail(e);
            }
            if (timing) {
                const hipError_t e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail(e);
                k_s += wall_s() - t1;
            }
            const double t2 = timing ? wall_s() : 0;
            int32_t *dst = score + b.first;
            if (mixed) {
                tmp.resize((size_t)b.n);
                dst = tmp.data();
            }
            hipError_t e = hipMemcpyAsync(dst, a.score, (size_t)b.n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(e);
            if (mixed) {  // the host twin's entries keep the scores they have
                int64_t k = 0;
                for (int64_t i = b.first; i < b.end; ++i) {
                    if (next_host < host_idx.size() && host_idx[next_host] == i) {
                        ++next_host;
                        continue;
                    }
                    score[i] = tmp[(size_t)k++];
                }
            }
            if (timing) dn_s += wall_s() - t2;
        }
        if (timing) {
            fprintf(stderr, "[gac_axt_score] %-24s %.3f s  (%lld bytes in %d batches: %.2f GB/s)\n", "upload", up_s,
                    (long long)up_bytes, (int)plan.batches.size(), up_s > 0 ? 1e-9 * (double)up_bytes / up_s : 0.0);
            fprintf(stderr, "[gac_axt_score] %-24s %.3f s  (%.2f GB/s of uploaded text)\n", "kernels", k_s,
                    k_s > 0 ? 1e-9 * (double)up_bytes / k_s : 0.0);
            fprintf(stderr, "[gac_axt_score] %-24s %.3f s\n", "download", dn_s);
            t_lap = wall_s();
        }
    }
    if (st) {
        for (int64_t i = 0; i < n; ++i) st->columns += len[i];
        st->host_entries = (int64_t)host_idx.size();
        st->batches = (int32_t)plan.batches.size();
        st->fell_back = host_idx.empty() ? 0 : 2;
    }
    lap("result");
    return GAC_OK;
}
