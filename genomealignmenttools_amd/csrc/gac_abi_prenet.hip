// gac_abi_prenet.hip -- libgachain's C ABI, chainPreNet's keep decision
// (gac_prenet_keep; the kernels and the method are in gac_prenet.hip, the
// arguments' check and the sequential pass are the host twin's,
// host/gac_prenet.c).
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

// the sequences of one side that counted chains name, in groups of at most
// `cap` words: largest first, each into the first group with room
struct SideGroups {
    std::vector<int32_t> group;  // per sequence, -1 = unused
    std::vector<int64_t> base;   // its first word in its group
    std::vector<int64_t> words;  // per group
    bool too_large = false;      // a sequence alone is over cap
};

SideGroups group_side(int64_t n, const int32_t *seq, const int32_t *other, int32_t n_seq,
                      const int32_t *sizes, int64_t cap) {
    SideGroups g;
    g.group.assign((size_t)std::max(n_seq, 1), -1);
    g.base.assign((size_t)std::max(n_seq, 1), 0);
    std::vector<int32_t> used;
    for (int64_t i = 0; i < n; ++i)
        if (seq[i] >= 0 && other[i] >= 0 && g.group[seq[i]] < 0) {
            g.group[seq[i]] = 0;
            used.push_back(seq[i]);
        }
    std::sort(used.begin(), used.end(), [&](int32_t x, int32_t y) {
        return sizes[x] != sizes[y] ? sizes[x] > sizes[y] : x < y;
    });
    for (int32_t s : used) {
        const int64_t z = sizes[s];
        if (z > cap) {
            g.too_large = true;
            return g;
        }
        size_t k = 0;
        while (k < g.words.size() && g.words[k] + z > cap) ++k;
        if (k == g.words.size()) g.words.push_back(0);
        g.group[s] = (int32_t)k;
        g.base[s] = g.words[k];
        g.words[k] += z;
    }
    return g;
}

}  // namespace

extern "C" int gac_prenet_keep(gac_ctx *c, int64_t n, const int64_t *blk_off, const int32_t *t_seq,
                               const int32_t *q_seq, int64_t n_blocks, const int32_t *blk_t,
                               const int32_t *blk_q, const int32_t *blk_size, int32_t n_tseq,
                               const int32_t *t_sizes, int32_t n_qseq, const int32_t *q_sizes,
                               int32_t pad, int32_t max_rounds, uint8_t *keep,
                               gac_prenet_stats *stats) {
    gac_clear_error();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    // GAC_TIMING: where the call's time goes
    const bool timing = getenv("GAC_TIMING") != nullptr;
    double t_lap = wall_s();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const double t = wall_s();
        fprintf(stderr, "[gac_prenet_keep] %-24s %.3f s\n", what, t - t_lap);
        t_lap = t;
    };
    int rc = gac_prenet_check(n, blk_off, t_seq, q_seq, n_blocks, blk_t, blk_q, blk_size, n_tseq,
                              t_sizes, n_qseq, q_sizes, pad, keep);
    if (rc != GAC_OK || n == 0) return rc;
    lap("check");
    if (max_rounds <= 0) max_rounds = GAC_PRENET_MAX_ROUNDS;
    auto host = [&](int why) {
        int r = gac_prenet_keep_host(n, blk_off, t_seq, q_seq, n_blocks, blk_t, blk_q, blk_size,
                                     n_tseq, t_sizes, n_qseq, q_sizes, pad, keep, nullptr);
        if (r == GAC_OK && stats) {
            stats->fell_back = why;
            stats->kept = 0;
            for (int64_t i = 0; i < n; ++i) stats->kept += keep[i];
        }
        return r;
    };
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t nb = n_blocks;
    const int32_t nseq[2] = {n_tseq, n_qseq};
    const int32_t *sizes[2] = {t_sizes, q_sizes};

    // one allocation for everything but the per-base words
    size_t b_scan = 0;
    HIPCHK(dt_scan64(nullptr, b_scan, nullptr, nullptr, nb + 1, s));
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += up256(bytes);
        return o;
    };
    const size_t o_boff = take((size_t)(n + 1) * 8);
    const size_t o_seq[2] = {take((size_t)n * 4), take((size_t)n * 4)};
    const size_t o_state = take((size_t)n), o_open = take((size_t)n), o_keep = take((size_t)n);
    const size_t o_bstart[2] = {take((size_t)nb * 4), take((size_t)nb * 4)};
    const size_t o_bsize = take((size_t)nb * 4), o_bchain = take((size_t)nb * 4);
    const size_t o_len = take((size_t)(nb + 1) * 8), o_off = take((size_t)(nb + 1) * 8);
    const size_t o_badr = take((size_t)nb * 8);
    size_t o_ssize[2], o_sgroup[2], o_sbase[2];
    for (int sd = 0; sd < 2; ++sd) {
        const size_t m = (size_t)std::max(nseq[sd], 1);
        o_ssize[sd] = take(m * 4), o_sgroup[sd] = take(m * 4), o_sbase[sd] = take(m * 8);
    }
    const size_t o_counts = take(16), o_tmp = take(b_scan);
    char *d = nullptr;
    HIPCHK(hipMalloc(&d, off));

    // the budget of the per-base words, then the groups that fit it
    int64_t budget = 0;
    if (const char *v = getenv("GAC_PRENET_FC_BYTES")) budget = atoll(v);
    if (budget <= 0) {
        size_t free_b = 0, total_b = 0;
        const hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess) {
            hipFree(d);
            return gac_fail(GAC_E_HIP, "hipMemGetInfo failed: %s", hipGetErrorString(e));
        }
        budget = (int64_t)(free_b / 4 * 3);
    }
    const int64_t cap = std::max<int64_t>(budget / 4, 1);
    SideGroups G[2] = {group_side(n, t_seq, q_seq, n_tseq, t_sizes, cap),
                       group_side(n, q_seq, t_seq, n_qseq, q_sizes, cap)};
    if (G[0].too_large || G[1].too_large) {
        hipFree(d);
        return host(GAC_PRENET_FELL_MEMORY);
    }
    int64_t fc_words = 1;
    for (int sd = 0; sd < 2; ++sd)
        for (int64_t w : G[sd].words) fc_words = std::max(fc_words, w);
    uint32_t *fc = nullptr;
    {
        const hipError_t e = hipMalloc(&fc, (size_t)fc_words * 4);
        if (e != hipSuccess) {
            hipFree(d);
            return gac_fail(GAC_E_HIP, "gac_prenet_keep: %lld bytes of per-base words: %s",
                            (long long)fc_words * 4, hipGetErrorString(e));
        }
    }

    lap("groups + hipMalloc");
    PrenetArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.nb = nb;
    a.pad = pad;
    a.boff = (const int64_t *)(d + o_boff);
    a.bsize = (const int32_t *)(d + o_bsize);
    a.bchain = (int32_t *)(d + o_bchain);
    for (int sd = 0; sd < 2; ++sd) {
        a.seq[sd] = (const int32_t *)(d + o_seq[sd]);
        a.bstart[sd] = (const int32_t *)(d + o_bstart[sd]);
        a.ssize[sd] = (const int32_t *)(d + o_ssize[sd]);
        a.sgroup[sd] = (const int32_t *)(d + o_sgroup[sd]);
        a.sbase[sd] = (const int64_t *)(d + o_sbase[sd]);
    }
    a.state = (uint8_t *)(d + o_state);
    a.open = (uint8_t *)(d + o_open);
    a.len = (long long *)(d + o_len);
    a.off = (const long long *)(d + o_off);
    a.badr = (long long *)(d + o_badr);
    a.fc = fc;
    a.counts = (unsigned long long *)(d + o_counts);

    auto fail = [&](hipError_t e) {
        hipStreamSynchronize(s);  // before the buffers go
        hipFree(fc);
        hipFree(d);
        return gac_fail(GAC_E_HIP, "gac_prenet_keep failed: %s", hipGetErrorString(e));
    };
    auto up = [&](size_t o, const void *src, size_t bytes) {
        return bytes ? upload_staged(c, d + o, src, bytes) : GAC_OK;
    };
    rc = up(o_boff, blk_off, (size_t)(n + 1) * 8);
    if (rc == GAC_OK) rc = up(o_seq[0], t_seq, (size_t)n * 4);
    if (rc == GAC_OK) rc = up(o_seq[1], q_seq, (size_t)n * 4);
    if (rc == GAC_OK) rc = up(o_bstart[0], blk_t, (size_t)nb * 4);
    if (rc == GAC_OK) rc = up(o_bstart[1], blk_q, (size_t)nb * 4);
    if (rc == GAC_OK) rc = up(o_bsize, blk_size, (size_t)nb * 4);
    for (int sd = 0; sd < 2 && rc == GAC_OK; ++sd) {
        rc = up(o_ssize[sd], sizes[sd], (size_t)nseq[sd] * 4);
        if (rc == GAC_OK) rc = up(o_sgroup[sd], G[sd].group.data(), (size_t)nseq[sd] * 4);
        if (rc == GAC_OK) rc = up(o_sbase[sd], G[sd].base.data(), (size_t)nseq[sd] * 8);
    }
    if (rc != GAC_OK) {
        hipStreamSynchronize(s);
        hipFree(fc);
        hipFree(d);
        return rc;
    }

    if (timing) hipStreamSynchronize(s);
    lap("upload");
    int rounds = 0, passes = 0;
    unsigned long long counts[2] = {(unsigned long long)n, 0};
    hipError_t e = hipSuccess;
    {
        PROF_BEGIN(GAC_K_PRENET);
        e = launch_prenet_setup(a, s);
        while (e == hipSuccess && counts[0] > 0 && rounds < max_rounds) {
            for (int pass = 1; pass <= 2 && e == hipSuccess; ++pass) {
                a.with_undecided = pass == 1;
                for (int sd = 0; sd < 2 && e == hipSuccess; ++sd)
                    for (size_t g = 0; g < G[sd].words.size() && e == hipSuccess; ++g) {
                        a.side = sd;
                        a.group = (int32_t)g;
                        e = hipMemsetAsync(fc, 0xff, (size_t)std::max<int64_t>(G[sd].words[g], 1) * 4, s);
                        size_t b = b_scan;
                        if (e == hipSuccess) e = launch_prenet_len(a, true, s);
                        if (e == hipSuccess)
                            e = dt_scan64(d + o_tmp, b, a.len, (long long *)(d + o_off), nb + 1, s);
                        if (e == hipSuccess) e = launch_prenet_mark(a, s);
                        b = b_scan;
                        if (e == hipSuccess) e = launch_prenet_len(a, false, s);
                        if (e == hipSuccess)
                            e = dt_scan64(d + o_tmp, b, a.len, (long long *)(d + o_off), nb + 1, s);
                        if (e == hipSuccess) e = launch_prenet_check(a, s);
                    }
                if (e == hipSuccess && pass == 2) e = hipMemsetAsync(a.counts, 0, 16, s);
                if (e == hipSuccess) e = launch_prenet_decide(a, pass, s);
                ++passes;
            }
            // the round's counts: all that comes back before the flags
            if (e == hipSuccess) e = hipMemcpyAsync(counts, a.counts, 16, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            ++rounds;
        }
        PROF_END(GAC_K_PRENET);
    }
    if (e != hipSuccess) return fail(e);
    lap("rounds");
    if (stats) {
        stats->rounds = rounds;
        stats->passes = passes;
        stats->groups[0] = (int32_t)G[0].words.size();
        stats->groups[1] = (int32_t)G[1].words.size();
        stats->kept = (int64_t)counts[1];
    }
    if (counts[0] > 0) {  // max_rounds reached: the host's sequential pass decides
        hipStreamSynchronize(s);
        hipFree(fc);
        hipFree(d);
        return host(GAC_PRENET_FELL_ROUNDS);
    }
    e = launch_prenet_flags(a, (uint8_t *)(d + o_keep), s);
    if (e == hipSuccess) e = hipMemcpyAsync(keep, d + o_keep, (size_t)n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(e);
    hipFree(fc);
    hipFree(d);
    lap("flags + hipFree");
    return GAC_OK;
}
