/* gac_axtpsl.c -- axtToPsl's conversion on the host: the argument check
 * gac_axt_psl shares, the result handle, and gac_axt_psl_host
 * (kent/src/lib/psl.c:1634-1665 trimAlignment, :1680-1714 accumCounts,
 * :1716-1806 pslFromAlign's column loop), one sequential pass an entry,
 * threaded over entries (axtToPsl -host, and the device call's fallback).
 *
 * A thread takes slices of consecutive entries and keeps each slice's blocks
 * in a buffer of its own; when every slice is done the slices' first blocks
 * are a prefix sum, and the threads copy the buffers to their places. */
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

int gac_axtpsl_check(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                     const int64_t *q_off, const int32_t *len, gac_axtpsl_result *const *out) {
    if (n < 0 || text_bytes < 0)
        return gac_fail(GAC_E_ARG, "gac_axt_psl: bad argument (n %lld, text bytes %lld)", (long long)n,
                        (long long)text_bytes);
    if (!out)
        return gac_fail(GAC_E_ARG, "gac_axt_psl: NULL result pointer");
    if (n == 0)
        return GAC_OK;
    if (!text || !t_off || !q_off || !len)
        return gac_fail(GAC_E_ARG, "gac_axt_psl: NULL buffer");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = len[i];
        if (L < 0 || t_off[i] < 0 || q_off[i] < 0 || t_off[i] > text_bytes - L || q_off[i] > text_bytes - L)
            return gac_fail(GAC_E_ARG,
                            "gac_axt_psl: entry %lld: rows of %d columns at %lld and %lld outside "
                            "%lld bytes of text",
                            (long long)i, len[i], (long long)t_off[i], (long long)q_off[i],
                            (long long)text_bytes);
    }
    return GAC_OK;
}

gac_axtpsl_result *gac_axtpsl_alloc(int64_t n, int64_t n_blocks) {
    gac_axtpsl_result *r = calloc(1, sizeof(*r));
    if (!r)
        return NULL;
    r->n = n, r->n_blocks = n_blocks;
    r->entry = malloc((size_t)(n ? n : 1) * sizeof(gac_axtpsl_entry));
    r->block = malloc((size_t)(n_blocks ? n_blocks : 1) * sizeof(gac_axtpsl_block));
    if (!r->entry || !r->block) {
        gac_axtpsl_free(r);
        return NULL;
    }
    return r;
}

void gac_axtpsl_free(gac_axtpsl_result *r) {
    if (!r)
        return;
    free(r->entry);
    free(r->block);
    free(r);
}

#define AXTPSL_SLICE 256 /* entries a thread takes at a time */

typedef struct axtpsl_slice {
    gac_axtpsl_block *v;
    int64_t n, cap, first;
} axtpsl_slice;

typedef struct axtpsl_job {
    int64_t n, nslices;
    const char *text;
    const int64_t *t_off, *q_off;
    const int32_t *len;
    gac_axtpsl_entry *entry;
    gac_axtpsl_block *block; /* the copy phase's target */
    axtpsl_slice *slice;
    _Atomic int64_t next, columns;
    _Atomic int failed;
} axtpsl_job;

static uint8_t k_del[256], k_upper[256];
static void axtpsl_tables(void) {
    for (int c = 0; c < 256; ++c) {
        k_del[c] = c == '-' || c == '.' || c == '=' || c == '_';
        k_upper[c] = (uint8_t)(c >= 'a' && c <= 'z' ? c - 32 : c);
    }
}

static int slice_push(axtpsl_slice *S, int32_t q_adv, int32_t t_adv, int32_t size) {
    if (S->n == S->cap) {
        const int64_t cap = S->cap ? S->cap * 2 : 1024;
        gac_axtpsl_block *v = realloc(S->v, (size_t)cap * sizeof(*v));
        if (!v)
            return 0;
        S->v = v, S->cap = cap;
    }
    S->v[S->n++] = (gac_axtpsl_block){q_adv, t_adv, size};
    return 1;
}

/* block0 is left relative to the slice's first block */
static int axtpsl_entry(const axtpsl_job *J, int64_t i, axtpsl_slice *S) {
    const uint8_t *t = (const uint8_t *)J->text + J->t_off[i], *q = (const uint8_t *)J->text + J->q_off[i];
    int32_t lo = 0, n = J->len[i];
    gac_axtpsl_entry e;
    memset(&e, 0, sizeof(e));
    while (n > 0 && (k_del[q[lo]] || k_del[t[lo]])) { /* trimAlignment */
        if (!k_del[q[lo]])
            ++e.q_head;
        else if (!k_del[t[lo]])
            ++e.t_head;
        ++lo, --n;
    }
    while (n > 0 && (k_del[q[lo + n - 1]] || k_del[t[lo + n - 1]])) {
        if (!k_del[q[lo + n - 1]])
            ++e.q_tail;
        else if (!k_del[t[lo + n - 1]])
            ++e.t_tail;
        --n;
    }
    e.cols = n;
    e.block0 = S->n;
    int32_t qs = 0, ts = 0, qe = 0, te = 0;
    int either = 0, prev_qd = 0, prev_td = 0;
    for (int32_t j = lo; j < lo + n; ++j) {
        const uint8_t qc = q[j], tc = t[j];
        const int qd = k_del[qc], td = k_del[tc];
        if (qd && td)
            continue;
        if (qd || td) {
            if (!either) {
                if (!slice_push(S, qs, ts, qe - qs))
                    return 0;
                either = 1;
            }
            qe += !qd, te += !td;
            if (qd) {
                ++e.t_base_insert;
                e.t_num_insert += !prev_qd;
            } else {
                ++e.q_base_insert;
                e.q_num_insert += !prev_td;
            }
        } else {
            if (either)
                qs = qe, ts = te, either = 0;
            ++qe, ++te;
            if (qc == 'N' || tc == 'N')
                ++e.n_count;
            else if (k_upper[qc] == k_upper[tc]) {
                if (k_upper[qc] != qc || k_upper[tc] != tc)
                    ++e.rep_match;
                else
                    ++e.match;
            } else
                ++e.mis_match;
        }
        prev_qd = qd, prev_td = td;
    }
    if (!slice_push(S, qs, ts, qe - qs))
        return 0;
    e.n_blocks = (int32_t)(S->n - e.block0);
    J->entry[i] = e;
    return 1;
}

static void *axtpsl_thread(void *arg) {
    axtpsl_job *J = arg;
    int64_t columns = 0;
    for (int64_t s; (s = atomic_fetch_add(&J->next, 1)) < J->nslices && !atomic_load(&J->failed);) {
        const int64_t lo = s * AXTPSL_SLICE, hi = lo + AXTPSL_SLICE < J->n ? lo + AXTPSL_SLICE : J->n;
        for (int64_t i = lo; i < hi; ++i) {
            if (!axtpsl_entry(J, i, &J->slice[s])) {
                atomic_store(&J->failed, 1);
                return NULL;
            }
            columns += J->len[i];
        }
    }
    atomic_fetch_add(&J->columns, columns);
    return NULL;
}

static void *axtpsl_copy_thread(void *arg) {
    axtpsl_job *J = arg;
    for (int64_t s; (s = atomic_fetch_add(&J->next, 1)) < J->nslices;) {
        const axtpsl_slice *S = &J->slice[s];
        if (S->n)
            memcpy(J->block + S->first, S->v, (size_t)S->n * sizeof(*S->v));
        const int64_t lo = s * AXTPSL_SLICE, hi = lo + AXTPSL_SLICE < J->n ? lo + AXTPSL_SLICE : J->n;
        for (int64_t i = lo; i < hi; ++i)
            J->entry[i].block0 += S->first;
    }
    return NULL;
}

int gac_axt_psl_host(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                     const int64_t *q_off, const int32_t *len, int nthreads,
                     gac_axtpsl_result **out, gac_axtpsl_stats *st) {
    gac_clear_error();
    if (st)
        memset(st, 0, sizeof(*st));
    if (out)
        *out = NULL;
    int rc = gac_axtpsl_check(n, text, text_bytes, t_off, q_off, len, out);
    if (rc != GAC_OK)
        return rc;
    static _Atomic int tables;
    if (!atomic_load(&tables)) { /* (every writer writes the same bytes) */
        axtpsl_tables();
        atomic_store(&tables, 1);
    }
    axtpsl_job J;
    memset(&J, 0, sizeof(J));
    J.n = n, J.text = text, J.t_off = t_off, J.q_off = q_off, J.len = len;
    J.nslices = (n + AXTPSL_SLICE - 1) / AXTPSL_SLICE;
    J.entry = malloc((size_t)(n ? n : 1) * sizeof(gac_axtpsl_entry));
    J.slice = calloc((size_t)(J.nslices ? J.nslices : 1), sizeof(axtpsl_slice));
    gac_axtpsl_result *r = calloc(1, sizeof(*r));
    if (!J.entry || !J.slice || !r) {
        free(J.entry), free(J.slice), free(r);
        return gac_fail(GAC_E_ARG, "gac_axt_psl_host: out of memory");
    }
    atomic_init(&J.next, 0);
    atomic_init(&J.columns, 0);
    atomic_init(&J.failed, 0);
    int nt = nthreads > 0 ? nthreads : gac_host_threads();
    if (nt > 64)
        nt = 64;
    while (nt > 1 && n / nt < AXTPSL_SLICE)
        nt /= 2;
    if (nt < 1)
        nt = 1;
    gac_run_threads(nt, axtpsl_thread, &J);
    int64_t nb = 0;
    for (int64_t s = 0; s < J.nslices; ++s) {
        J.slice[s].first = nb;
        nb += J.slice[s].n;
    }
    if (!atomic_load(&J.failed))
        J.block = malloc((size_t)(nb ? nb : 1) * sizeof(gac_axtpsl_block));
    if (J.block) {
        atomic_store(&J.next, 0);
        gac_run_threads(nt, axtpsl_copy_thread, &J);
    }
    for (int64_t s = 0; s < J.nslices; ++s)
        free(J.slice[s].v);
    free(J.slice);
    if (!J.block) {
        free(J.entry), free(r);
        return gac_fail(GAC_E_ARG, "gac_axt_psl_host: out of memory");
    }
    r->n = n, r->n_blocks = nb, r->entry = J.entry, r->block = J.block;
    *out = r;
    if (st) {
        st->blocks = nb;
        st->columns = atomic_load(&J.columns);
        st->host_entries = n;
    }
    return GAC_OK;
}
