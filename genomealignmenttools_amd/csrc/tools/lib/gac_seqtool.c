/* gac_seqtool.c -- the host-only part of the sequence tools' front end
 * (gac_seqtool.h): argument checks, the kept-chain set, the batch plan. */
#include "gac_seqtool.h"

#include <stdlib.h>
#include <string.h>

#include "host/gac_host.h"

void gs_check_twobits(const char *t2bit, const char *q2bit, const char *noun) {
    if (!gt_file_exists(t2bit))
        gt_abort("ERROR: target %s %s does not exist\n", noun, t2bit);
    if (!gt_file_exists(q2bit))
        gt_abort("ERROR: query %s %s does not exist\n", noun, q2bit);
    if (!gac_is_twobit_file(t2bit))
        gt_abort("ERROR: only 2bit files are supported, not %s\n", t2bit);
    if (!gac_is_twobit_file(q2bit))
        gt_abort("ERROR: only 2bit files are supported, not %s\n", q2bit);
}

void gs_check_frag(const char *name, int64_t start, int64_t end, int32_t seq_size) {
    if (end == 0)
        end = seq_size;
    if (end > seq_size)
        gt_abort("twoBitReadSeqFrag in %s end (%d) >= seqSize (%d)", name, (int)end, seq_size);
    if (end - start < 1 || start < 0)
        gt_abort("twoBitReadSeqFrag in %s start (%d) >= end (%d)", name, (int)start, (int)end);
}

void *gs_alloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p)
        gt_abort("Out of memory (%zu bytes)", n);
    return p;
}

size_t *gs_name_lens(const gt_names *t) {
    size_t *len = gs_alloc((size_t)t->n * sizeof(*len));
    for (int32_t i = 0; i < t->n; ++i)
        len[i] = strlen(t->names[i]);
    return len;
}

void gs_subset_build(const gs_env *e, const uint8_t *keep, const int32_t *tname,
                     const int32_t *qname, const int32_t *tmap, const int32_t *qmap,
                     gs_chain_check check, int check_gaps, gs_subset *s) {
    const gt_chains *c = e->c;
    int64_t nc = 0, nb = 0;
    for (int64_t i = 0; i < c->n; ++i)
        if (keep[i]) {
            ++nc;
            nb += c->blk_off[i + 1] - c->blk_off[i];
        }
    s->nc = nc;
    s->nb = nb;
    s->sel = gs_alloc((size_t)nc * 8), s->boff = gs_alloc((size_t)(nc + 1) * 8);
    s->tseq = gs_alloc((size_t)nc * 4), s->qseq = gs_alloc((size_t)nc * 4);
    s->strand = gs_alloc((size_t)nc), s->bs = gs_alloc((size_t)nb * 4);
    s->bt = gs_alloc((size_t)nb * 4), s->bq = gs_alloc((size_t)nb * 4);
    int64_t k = 0, b = 0;
    s->boff[0] = 0;
    for (int64_t i = 0; i < c->n; ++i) {
        if (!keep[i])
            continue;
        const int32_t ts = tmap[tname[i]], qs = qmap[qname[i]];
        check(e, i, ts, qs);
        s->sel[k] = i;
        s->tseq[k] = ts;
        s->qseq[k] = qs;
        s->strand[k] = c->qstrand[i];
        const int64_t j0 = c->blk_off[i], n = c->blk_off[i + 1] - j0;
        if (check_gaps)
            /* a negative gap is undefined in the reference (assert / negative
             * memset): refused here, before anything runs on it */
            for (int64_t j = j0 + 1; j < j0 + n; ++j)
                if (c->bt[j] < c->bt[j - 1] + c->bs[j - 1] || c->bq[j] < c->bq[j - 1] + c->bs[j - 1])
                    gt_abort("chain %d: blocks overlap (negative gap before block %lld)", c->id[i],
                             (long long)(j - j0));
        if (n) {
            memcpy(s->bt + b, c->bt + j0, (size_t)n * 4);
            memcpy(s->bq + b, c->bq + j0, (size_t)n * 4);
            memcpy(s->bs + b, c->bs + j0, (size_t)n * 4);
        }
        b += n;
        s->boff[++k] = b;
    }
    s->d = (gac_chainset_desc){nc, s->tseq, s->qseq, s->strand, s->boff, nb, s->bt, s->bq, s->bs};
}

int64_t gs_axt_budget(void) {
    const char *e = getenv("GAC_AXT_BUDGET");
    return e && atoll(e) > 0 ? atoll(e) : 64ll << 20;
}

void gs_axt_plan_make(const int64_t *sym, int64_t n, int64_t budget, gs_axt_plan *P) {
    int64_t bcap = 16;
    P->budget = P->cap = budget;
    P->nbatch = 0;
    P->off = gs_alloc((size_t)n * 8);
    P->lo = gs_alloc((size_t)bcap * 8), P->bytes = gs_alloc((size_t)bcap * 8);
    for (int64_t p = 0; p < n;) {
        if (P->nbatch + 1 >= bcap) {
            bcap *= 2;
            P->lo = realloc(P->lo, (size_t)bcap * 8);
            P->bytes = realloc(P->bytes, (size_t)bcap * 8);
            if (!P->lo || !P->bytes)
                gt_abort("Out of memory");
        }
        int64_t used = 0;
        P->lo[P->nbatch] = p;
        do {
            const int64_t size = 2 * sym[p] + 3;
            if (size > P->cap)
                P->cap = size;
            P->off[p++] = used;
            used += size;
        } while (p < n && used + 2 * sym[p] + 3 <= budget);
        P->bytes[P->nbatch++] = used;
    }
    P->lo[P->nbatch] = n;
    P->job_bytes[0] = !P->nbatch ? 0 : P->nbatch > 1 || P->cap > budget ? P->cap : P->bytes[0];
    P->job_bytes[1] = P->nbatch > 1 ? P->cap : 0;
}
