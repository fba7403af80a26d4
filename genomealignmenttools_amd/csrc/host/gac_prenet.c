/* gac_prenet.c -- chainPreNet's keep decision on the host: the argument check
 * gac_prenet_keep shares, and gac_prenet_keep_host, the reference's own pass
 * (kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c:104-137): chain by chain,
 * one bitmap per named sequence and side, a chain kept when a base of one of
 * its blocks is still clear, a kept chain setting its padded blocks
 * (chainPreNet -host, and the device call's fallbacks). */
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

int gac_prenet_check(int64_t n, const int64_t *blk_off, const int32_t *t_seq, const int32_t *q_seq,
                     int64_t n_blocks, const int32_t *blk_t, const int32_t *blk_q,
                     const int32_t *blk_size, int32_t n_tseq, const int32_t *t_sizes,
                     int32_t n_qseq, const int32_t *q_sizes, int32_t pad, const uint8_t *keep) {
    if (n < 0 || n_blocks < 0 || pad < 0 || n_tseq < 0 || n_qseq < 0)
        return gac_fail(GAC_E_ARG, "gac_prenet_keep: bad argument (n %lld, blocks %lld, pad %d)",
                        (long long)n, (long long)n_blocks, pad);
    if (n > GAC_PRENET_MAX_ITEMS || n_blocks > GAC_PRENET_MAX_ITEMS)
        return gac_fail(GAC_E_ARG, "gac_prenet_keep: %lld chains, %lld blocks, at most %d a call",
                        (long long)n, (long long)n_blocks, GAC_PRENET_MAX_ITEMS);
    if (n == 0)
        return GAC_OK;
    if (!blk_off || !t_seq || !q_seq || !keep || (n_blocks > 0 && (!blk_t || !blk_q || !blk_size)) ||
        (n_tseq > 0 && !t_sizes) || (n_qseq > 0 && !q_sizes))
        return gac_fail(GAC_E_ARG, "gac_prenet_keep: NULL buffer");
    if (blk_off[0] != 0 || blk_off[n] != n_blocks)
        return gac_fail(GAC_E_ARG, "gac_prenet_keep: block offsets run from %lld to %lld, not 0 to %lld",
                        (long long)blk_off[0], (long long)blk_off[n], (long long)n_blocks);
    for (int32_t s = 0; s < n_tseq; ++s)
        if (t_sizes[s] < 0)
            return gac_fail(GAC_E_ARG, "gac_prenet_keep: target sequence %d of size %d", s, t_sizes[s]);
    for (int32_t s = 0; s < n_qseq; ++s)
        if (q_sizes[s] < 0)
            return gac_fail(GAC_E_ARG, "gac_prenet_keep: query sequence %d of size %d", s, q_sizes[s]);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t b0 = blk_off[i], b1 = blk_off[i + 1];
        if (b1 < b0 || b1 > n_blocks)
            return gac_fail(GAC_E_ARG, "gac_prenet_keep: chain %lld: blocks [%lld, %lld)", (long long)i,
                            (long long)b0, (long long)b1);
        const int32_t ts = t_seq[i], qs = q_seq[i];
        if (ts < -1 || ts >= n_tseq || qs < -1 || qs >= n_qseq)
            return gac_fail(GAC_E_ARG, "gac_prenet_keep: chain %lld: sequences %d, %d", (long long)i, ts,
                            qs);
        if (ts < 0 || qs < 0)
            continue; /* skipped: its blocks are not read */
        const int64_t tz = t_sizes[ts], qz = q_sizes[qs];
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t z = blk_size[b];
            if (z < 0 || blk_t[b] < 0 || blk_q[b] < 0 || blk_t[b] + z > tz || blk_q[b] + z > qz)
                return gac_fail(GAC_E_ARG,
                                "gac_prenet_keep: chain %lld block %lld: target %d, query %d, size %d "
                                "outside sequences of %lld and %lld bases",
                                (long long)i, (long long)(b - b0), blk_t[b], blk_q[b], blk_size[b],
                                (long long)tz, (long long)qz);
        }
    }
    return GAC_OK;
}

/* bits [s, e) of a bitmap of 64-bit words */
static int all_set(const uint64_t *w, int64_t s, int64_t e) {
    if (s >= e)
        return 1;
    const int64_t w0 = s >> 6, w1 = (e - 1) >> 6;
    const uint64_t m0 = ~(uint64_t)0 << (s & 63), m1 = ~(uint64_t)0 >> (63 - ((e - 1) & 63));
    if (w0 == w1)
        return (w[w0] & m0 & m1) == (m0 & m1);
    if ((w[w0] & m0) != m0 || (w[w1] & m1) != m1)
        return 0;
    for (int64_t k = w0 + 1; k < w1; ++k)
        if (w[k] != ~(uint64_t)0)
            return 0;
    return 1;
}

static void set_range(uint64_t *w, int64_t s, int64_t e) {
    if (s >= e)
        return;
    const int64_t w0 = s >> 6, w1 = (e - 1) >> 6;
    const uint64_t m0 = ~(uint64_t)0 << (s & 63), m1 = ~(uint64_t)0 >> (63 - ((e - 1) & 63));
    if (w0 == w1) {
        w[w0] |= m0 & m1;
        return;
    }
    w[w0] |= m0;
    for (int64_t k = w0 + 1; k < w1; ++k)
        w[k] = ~(uint64_t)0;
    w[w1] |= m1;
}

/* setWithPad (:88-96) */
static void set_padded(uint64_t *w, int64_t s, int64_t e, int64_t pad, int64_t size) {
    s -= pad;
    if (s < 0)
        s = 0;
    e += pad;
    if (e > size)
        e = size;
    set_range(w, s, e);
}

static void free_maps(uint64_t **m, int32_t n) {
    for (int32_t s = 0; m && s < n; ++s)
        free(m[s]);
    free(m);
}

int gac_prenet_keep_host(int64_t n, const int64_t *blk_off, const int32_t *t_seq,
                         const int32_t *q_seq, int64_t n_blocks, const int32_t *blk_t,
                         const int32_t *blk_q, const int32_t *blk_size, int32_t n_tseq,
                         const int32_t *t_sizes, int32_t n_qseq, const int32_t *q_sizes,
                         int32_t pad, uint8_t *keep, gac_prenet_stats *stats) {
    gac_clear_error();
    if (stats)
        memset(stats, 0, sizeof(*stats));
    int rc = gac_prenet_check(n, blk_off, t_seq, q_seq, n_blocks, blk_t, blk_q, blk_size, n_tseq,
                              t_sizes, n_qseq, q_sizes, pad, keep);
    if (rc != GAC_OK || n == 0)
        return rc;
    /* a bitmap per sequence that a counted chain names, made at its first use */
    uint64_t **tm = calloc((size_t)(n_tseq ? n_tseq : 1), sizeof(*tm));
    uint64_t **qm = calloc((size_t)(n_qseq ? n_qseq : 1), sizeof(*qm));
    int oom = !tm || !qm;
    int64_t kept = 0;
    for (int64_t i = 0; i < n && !oom; ++i) {
        keep[i] = 0;
        const int32_t ts = t_seq[i], qs = q_seq[i];
        if (ts < 0 || qs < 0)
            continue;
        if (!tm[ts] && !(tm[ts] = calloc((size_t)(t_sizes[ts] / 64 + 1), 8)))
            oom = 1;
        if (!oom && !qm[qs] && !(qm[qs] = calloc((size_t)(q_sizes[qs] / 64 + 1), 8)))
            oom = 1;
        if (oom)
            break;
        uint64_t *tw = tm[ts], *qw = qm[qs];
        int open = 0;
        for (int64_t b = blk_off[i]; b < blk_off[i + 1] && !open; ++b) {
            const int64_t z = blk_size[b];
            open = !all_set(qw, blk_q[b], blk_q[b] + z) || !all_set(tw, blk_t[b], blk_t[b] + z);
        }
        if (!open)
            continue;
        for (int64_t b = blk_off[i]; b < blk_off[i + 1]; ++b) {
            const int64_t z = blk_size[b];
            set_padded(qw, blk_q[b], blk_q[b] + z, pad, q_sizes[qs]);
            set_padded(tw, blk_t[b], blk_t[b] + z, pad, t_sizes[ts]);
        }
        keep[i] = 1;
        ++kept;
    }
    free_maps(tm, n_tseq);
    free_maps(qm, n_qseq);
    if (oom)
        return gac_fail(GAC_E_ARG, "gac_prenet_keep_host: out of memory");
    if (stats)
        stats->kept = kept;
    return GAC_OK;
}
