// gac_abi_axtpsl.hip -- libgachain's C ABI, axtToPsl's conversion
// (gac_axt_psl: kent/src/lib/psl.c:1634-1806 trimAlignment, accumCounts and
// pslFromAlign's column loop; the kernels and the method are in
// gac_axtpsl.hip, the arguments' check, the result handle and the host twin in
// host/gac_axtpsl.c, the batches in gac_ctx.h).
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

static_assert(sizeof(gac_axtpsl_entry) == 64, "gac_axtpsl_entry layout");
static_assert(sizeof(gac_axtpsl_block) == 12, "gac_axtpsl_block layout");

namespace {

// what a call holds until it returns
struct Held {
    hipStream_t s = nullptr;
    char *d = nullptr, *d_blk = nullptr;
    gac_axtpsl_result *res = nullptr, *hres = nullptr;
    ~Held() {
        if (d || d_blk) hipStreamSynchronize(s);  // before the buffers go
        if (d) hipFree(d);
        if (d_blk) hipFree(d_blk);
        gac_axtpsl_free(res);
        gac_axtpsl_free(hres);
    }
};

}  // namespace

extern "C" int gac_axt_psl(gac_ctx *c, int64_t n, const char *text, int64_t text_bytes,
                           const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                           gac_axtpsl_result **out, gac_axtpsl_stats *st) {
    gac_clear_error();
    if (st) memset(st, 0, sizeof(*st));
    if (out) *out = nullptr;
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    // GAC_TIMING: where the call's time goes (the stream is synchronised after
    // every step then, so that a lap is that step's alone)
    const bool timing = getenv("GAC_TIMING") != nullptr;
    double t_lap = wall_s();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const double t = wall_s();
        fprintf(stderr, "[gac_axt_psl] %-24s %.3f s\n", what, t - t_lap);
        t_lap = t;
    };
    int rc = gac_axtpsl_check(n, text, text_bytes, t_off, q_off, len, out);
    if (rc != GAC_OK) return rc;
    Held H;
    H.res = gac_axtpsl_alloc(n, 0);
    if (!H.res) return gac_fail(GAC_E_ARG, "gac_axt_psl: out of memory");
    if (n == 0) {
        *out = H.res, H.res = nullptr;
        return GAC_OK;
    }
    lap("check");

    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    H.s = s;

    int64_t budget = 0;
    HIPCHK(axt_batch_budget("GAC_AXTPSL_BATCH_BYTES", &budget));
    AxtPlan plan;
    axt_plan_batches(n, t_off, q_off, len, budget, [](int64_t) { return false; }, plan);
    const std::vector<int64_t> &host_idx = plan.host_idx;
    lap("batches");

    if (!host_idx.empty()) {  // entries alone over the budget: the host twin converts them
        const size_t h = host_idx.size();
        std::vector<int64_t> ht(h), hq(h);
        std::vector<int32_t> hl(h);
        for (size_t k = 0; k < h; ++k)
            ht[k] = t_off[host_idx[k]], hq[k] = q_off[host_idx[k]], hl[k] = len[host_idx[k]];
        rc = gac_axt_psl_host((int64_t)h, text, text_bytes, ht.data(), hq.data(), hl.data(), 0, &H.hres,
                              nullptr);
        if (rc != GAC_OK) return rc;
        lap("host twin (over budget)");
    }

    // the result's blocks: grown as the batches' totals come in
    gac_axtpsl_entry *ent_out = H.res->entry;
    int64_t nb_all = 0, cap_all = 0;
    auto room = [&](int64_t more) {
        if (nb_all + more <= cap_all) return true;
        const int64_t cap = std::max<int64_t>(nb_all + more, cap_all + cap_all / 2);
        void *p = realloc(H.res->block, (size_t)std::max<int64_t>(cap, 1) * sizeof(gac_axtpsl_block));
        if (!p) return false;
        H.res->block = (gac_axtpsl_block *)p, cap_all = cap;
        return true;
    };
    size_t next_host = 0;  // into host_idx / H.hres
    // the entries before hi that the host twin converted and are not placed yet, into the result
    auto place_host = [&](int64_t hi) {
        for (; next_host < host_idx.size() && host_idx[next_host] < hi; ++next_host) {
            gac_axtpsl_entry e = H.hres->entry[next_host];
            if (!room(e.n_blocks)) return false;
            memcpy(H.res->block + nb_all, H.hres->block + e.block0, (size_t)e.n_blocks * sizeof(gac_axtpsl_block));
            e.block0 = nb_all;
            nb_all += e.n_blocks;
            ent_out[host_idx[next_host]] = e;
        }
        return true;
    };
    const char *oom = "gac_axt_psl: out of memory";

    if (plan.n_dev > 0) {
        // one allocation: the batch's text, its records, its results, the block
        // counts and their scan; the blocks in a buffer of their own, grown
        size_t b_scan = 0;
        HIPCHK(dt_scan64(nullptr, b_scan, nullptr, nullptr, plan.max_n + 1, s));
        size_t off = 0;
        auto take = [&](size_t bytes) {
            const size_t o = off;
            off += up256(bytes);
            return o;
        };
        const size_t o_text = take((size_t)plan.max_bytes + 256);
        const size_t o_ent = take((size_t)plan.max_n * sizeof(AxtpEntry));
        const size_t o_out = take((size_t)plan.max_n * sizeof(gac_axtpsl_entry));
        const size_t o_nblk = take((size_t)(plan.max_n + 1) * 8);
        const size_t o_boff = take((size_t)(plan.max_n + 1) * 8);
        const size_t o_tmp = take(b_scan);
        {
            const hipError_t e = hipMalloc(&H.d, off);
            if (e != hipSuccess)
                return gac_fail(GAC_E_HIP, "gac_axt_psl: %lld bytes of device memory: %s", (long long)off,
                                hipGetErrorString(e));
        }
        char *d = H.d;
        size_t cap_blk = 0;
        auto fail = [&](hipError_t e) { return gac_fail(GAC_E_HIP, "gac_axt_psl failed: %s", hipGetErrorString(e)); };
        lap("hipMalloc");

        AxtpArgs a;
        memset(&a, 0, sizeof(a));
        a.text = (const uint8_t *)(d + o_text);
        a.ent = (const AxtpEntry *)(d + o_ent);
        a.out = (gac_axtpsl_entry *)(d + o_out);
        a.nblk = (long long *)(d + o_nblk);
        a.boff = (const long long *)(d + o_boff);

        std::vector<AxtpEntry> ent;
        std::vector<gac_axtpsl_entry> tmp_ent;
        std::vector<gac_axtpsl_block> tmp_blk;
        double up_s = 0, k_s = 0, dn_s = 0;
        int64_t up_bytes = 0;
        for (const AxtBatch &b : plan.batches) {
            if (!place_host(b.first)) return gac_fail(GAC_E_ARG, "%s", oom);
            const AxtSpans &sp = b.sp;
            const int64_t t_base = sp.t_base(), q_base = sp.q_base();
            const bool mixed = b.end - b.first != b.n;  // entries of the host twin among them
            ent.clear();
            {
                size_t nh = next_host;
                for (int64_t i = b.first; i < b.end; ++i) {
                    if (nh < host_idx.size() && host_idx[nh] == i) {
                        ++nh;
                        continue;
                    }
                    ent.push_back(AxtpEntry{t_base + (t_off[i] - sp.tlo), q_base + (q_off[i] - sp.qlo), len[i], 0});
                }
            }
            a.text_bytes = sp.bytes();
            a.n = b.n;

            const double t0 = timing ? wall_s() : 0;
            rc = axt_upload_spans(c, d + o_text, text, sp);
            if (rc == GAC_OK) rc = upload_staged(c, d + o_ent, ent.data(), ent.size() * sizeof(AxtpEntry));
            if (rc != GAC_OK) return rc;
            up_bytes += sp.bytes() + (int64_t)(ent.size() * sizeof(AxtpEntry));
            if (timing) {
                hipStreamSynchronize(s);
                up_s += wall_s() - t0;
            }
            const double t1 = timing ? wall_s() : 0;
            long long nb = 0;
            {
                PROF_BEGIN(GAC_K_AXTPSL);
                hipError_t e = hipMemsetAsync(a.nblk + b.n, 0, 8, s);
                if (e == hipSuccess) e = launch_axt_psl_count(a, s);
                size_t bytes = b_scan;
                if (e == hipSuccess) e = dt_scan64(d + o_tmp, bytes, a.nblk, (long long *)(d + o_boff), b.n + 1, s);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(&nb, (const long long *)(d + o_boff) + b.n, 8, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail(e);
                if (nb < b.n) return gac_fail(GAC_E_HIP, "gac_axt_psl: %lld blocks for %lld entries", nb, (long long)b.n);
                if ((size_t)nb * sizeof(gac_axtpsl_block) > cap_blk) {
                    if (H.d_blk) hipFree(H.d_blk);
                    H.d_blk = nullptr;
                    cap_blk = up256((size_t)nb * sizeof(gac_axtpsl_block) * 5 / 4);
                    e = hipMalloc(&H.d_blk, cap_blk);
                    if (e != hipSuccess) {
                        H.d_blk = nullptr;
                        return gac_fail(GAC_E_HIP, "gac_axt_psl: %lld bytes of device memory: %s",
                                        (long long)cap_blk, hipGetErrorString(e));
                    }
                }
                a.blk = (gac_axtpsl_block *)H.d_blk;
                a.nb = nb;
                e = launch_axt_psl_emit(a, s);
                PROF_END(GAC_K_AXTPSL);
                if (e != hipSuccess) return fail(e);
            }
            if (timing) {
                const hipError_t e = hipStreamSynchronize(s);
                if (e != hipSuccess) return fail(e);
                k_s += wall_s() - t1;
            }
            const double t2 = timing ? wall_s() : 0;
            // (a batch with entries of the host twin among its own goes through copies, and
            // asks for room entry by entry: the host's blocks lie between the device's)
            gac_axtpsl_entry *he = ent_out + b.first;
            gac_axtpsl_block *hb = nullptr;
            if (mixed) {
                tmp_ent.resize((size_t)b.n), tmp_blk.resize((size_t)nb);
                he = tmp_ent.data(), hb = tmp_blk.data();
            } else {
                if (!room(nb)) return gac_fail(GAC_E_ARG, "%s", oom);
                hb = H.res->block + nb_all;
            }
            hipError_t e = hipMemcpyAsync(he, d + o_out, (size_t)b.n * sizeof(gac_axtpsl_entry), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess)
                e = hipMemcpyAsync(hb, H.d_blk, (size_t)nb * sizeof(gac_axtpsl_block), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return fail(e);
            if (!mixed) {
                for (int64_t k = 0; k < b.n; ++k) he[k].block0 += nb_all;
                nb_all += nb;
            } else {
                int64_t k = 0;
                for (int64_t i = b.first; i < b.end; ++i) {
                    if (next_host < host_idx.size() && host_idx[next_host] == i) {
                        if (!place_host(i + 1)) return gac_fail(GAC_E_ARG, "%s", oom);
                        continue;
                    }
                    gac_axtpsl_entry r = tmp_ent[(size_t)k++];
                    if (r.block0 < 0 || r.n_blocks < 1 || r.block0 + r.n_blocks > nb)
                        return gac_fail(GAC_E_HIP, "gac_axt_psl: entry %lld: blocks outside the batch's", (long long)i);
                    if (!room(r.n_blocks)) return gac_fail(GAC_E_ARG, "%s", oom);
                    memcpy(H.res->block + nb_all, tmp_blk.data() + r.block0, (size_t)r.n_blocks * sizeof(gac_axtpsl_block));
                    r.block0 = nb_all;
                    nb_all += r.n_blocks;
                    ent_out[i] = r;
                }
            }
            if (timing) dn_s += wall_s() - t2;
        }
        if (timing) {
            fprintf(stderr, "[gac_axt_psl] %-24s %.3f s  (%lld bytes in %d batches: %.2f GB/s)\n", "upload", up_s,
                    (long long)up_bytes, (int)plan.batches.size(), up_s > 0 ? 1e-9 * (double)up_bytes / up_s : 0.0);
            fprintf(stderr, "[gac_axt_psl] %-24s %.3f s  (%.2f GB/s of uploaded text)\n", "kernels", k_s,
                    k_s > 0 ? 1e-9 * (double)up_bytes / k_s : 0.0);
            fprintf(stderr, "[gac_axt_psl] %-24s %.3f s  (%lld blocks)\n", "download", dn_s, (long long)nb_all);
            t_lap = wall_s();
        }
    }
    if (!place_host(n)) return gac_fail(GAC_E_ARG, "%s", oom);
    H.res->n_blocks = nb_all;
    if (st) {
        st->blocks = nb_all;
        for (int64_t i = 0; i < n; ++i) st->columns += len[i];
        st->host_entries = (int64_t)host_idx.size();
        st->batches = (int32_t)plan.batches.size();
        st->fell_back = host_idx.empty() ? 0 : 2;
    }
    *out = H.res, H.res = nullptr;
    lap("result");
    return GAC_OK;
}
