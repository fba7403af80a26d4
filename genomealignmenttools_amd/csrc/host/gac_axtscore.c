/* gac_axtscore.c -- axtToMaf's scores on the host: the argument check
 * gac_axt_score shares, and gac_axt_score_host (kent/src/lib/axt.c:196-229
 * axtScoreSym under :423-458 axtScoreSchemeDefault), one pass an entry,
 * threaded over slices of entries (axtToMaf -host, and the device call's
 * fallback).
 *
 * A character's class comes from a 256-byte table: a c g t in either case 0-3,
 * '-' 5, anything else 4 (bytes >= 0x80 among them: the reference indexes its
 * matrix with a negative char there).  The sum is kept in 64 bits and narrowed,
 * which is the reference's int sum modulo 2^32. */
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

int gac_axtscore_check(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                       const int64_t *q_off, const int32_t *len, const int32_t *score) {
    if (n < 0 || text_bytes < 0)
        return gac_fail(GAC_E_ARG, "gac_axt_score: bad argument (n %lld, text bytes %lld)", (long long)n,
                        (long long)text_bytes);
    if (n == 0)
        return GAC_OK;
    if (!text || !t_off || !q_off || !len || !score)
        return gac_fail(GAC_E_ARG, "gac_axt_score: NULL buffer");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = len[i];
        if (L < 0 || t_off[i] < 0 || q_off[i] < 0 || t_off[i] > text_bytes - L || q_off[i] > text_bytes - L)
            return gac_fail(GAC_E_ARG,
                            "gac_axt_score: entry %lld: rows of %d columns at %lld and %lld outside "
                            "%lld bytes of text",
                            (long long)i, len[i], (long long)t_off[i], (long long)q_off[i],
                            (long long)text_bytes);
    }
    return GAC_OK;
}

#define AXTSCORE_SLICE 256 /* entries a thread takes at a time */
#define AXTSCORE_GAP 5
#define AXTSCORE_GAP_OPEN 400
#define AXTSCORE_GAP_EXTEND 30

typedef struct axtscore_job {
    int64_t n, nslices;
    const char *text;
    const int64_t *t_off, *q_off;
    const int32_t *len;
    int32_t *score;
    _Atomic int64_t next, columns;
} axtscore_job;

static uint8_t k_class[256];
/* by class: a c g t other; the dash's row and column are never read */
static const int16_t k_matrix[6][6] = {
    {91, -114, -31, -123, 0, 0},
    {-114, 100, -125, -31, 0, 0},
    {-31, -125, 100, -114, 0, 0},
    {-123, -31, -114, 91, 0, 0},
    {0, 0, 0, 0, 0, 0},
    {0, 0, 0, 0, 0, 0},
};

static void axtscore_tables(void) {
    uint8_t v[256];
    memset(v, 4, sizeof(v));
    v['a'] = v['A'] = 0;
    v['c'] = v['C'] = 1;
    v['g'] = v['G'] = 2;
    v['t'] = v['T'] = 3;
    v['-'] = AXTSCORE_GAP;
    memcpy(k_class, v, sizeof(v)); /* (every byte gets its final value at once) */
}

static int32_t axtscore_entry(const uint8_t *t, const uint8_t *q, int32_t n) {
    int64_t sum = 0;
    int last_gap = 0;
    for (int32_t j = 0; j < n; ++j) {
        const unsigned tc = k_class[t[j]], qc = k_class[q[j]];
        if (tc == AXTSCORE_GAP || qc == AXTSCORE_GAP) {
            sum -= last_gap ? AXTSCORE_GAP_EXTEND : AXTSCORE_GAP_OPEN + AXTSCORE_GAP_EXTEND;
            last_gap = 1;
        } else {
            sum += k_matrix[tc][qc];
            last_gap = 0;
        }
    }
    return (int32_t)(uint32_t)(uint64_t)sum;
}

static void *axtscore_thread(void *arg) {
    axtscore_job *J = arg;
    int64_t columns = 0;
    for (int64_t s; (s = atomic_fetch_add(&J->next, 1)) < J->nslices;) {
        const int64_t lo = s * AXTSCORE_SLICE, hi = lo + AXTSCORE_SLICE < J->n ? lo + AXTSCORE_SLICE : J->n;
        for (int64_t i = lo; i < hi; ++i) {
            J->score[i] = axtscore_entry((const uint8_t *)J->text + J->t_off[i],
                                         (const uint8_t *)J->text + J->q_off[i], J->len[i]);
            columns += J->len[i];
        }
    }
    atomic_fetch_add(&J->columns, columns);
    return NULL;
}

int gac_axt_score_host(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                       const int64_t *q_off, const int32_t *len, int nthreads, int32_t *score,
                       gac_axtscore_stats *st) {
    gac_clear_error();
    if (st)
        memset(st, 0, sizeof(*st));
    int rc = gac_axtscore_check(n, text, text_bytes, t_off, q_off, len, score);
    if (rc != GAC_OK)
        return rc;
    if (n == 0)
        return GAC_OK;
    static _Atomic int tables;
    if (!atomic_load(&tables)) { /* (every writer writes the same bytes) */
        axtscore_tables();
        atomic_store(&tables, 1);
    }
    axtscore_job J;
    memset(&J, 0, sizeof(J));
    J.n = n, J.text = text, J.t_off = t_off, J.q_off = q_off, J.len = len, J.score = score;
    J.nslices = (n + AXTSCORE_SLICE - 1) / AXTSCORE_SLICE;
    atomic_init(&J.next, 0);
    atomic_init(&J.columns, 0);
    int nt = nthreads > 0 ? nthreads : gac_host_threads();
    if (nt > 64)
        nt = 64;
    while (nt > 1 && n / nt < AXTSCORE_SLICE)
        nt /= 2;
    if (nt < 1)
        nt = 1;
    gac_run_threads(nt, axtscore_thread, &J);
    if (st) {
        st->columns = atomic_load(&J.columns);
        st->host_entries = n;
    }
    return GAC_OK;
}
