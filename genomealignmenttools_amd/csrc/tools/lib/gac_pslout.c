/* gac_pslout.c -- see gac_pslout.h */
#include "gac_pslout.h"

#include <stdlib.h>
#include <string.h>

/* v in decimal and one separator; u32: as "%u" of the 32-bit value, else "%d" */
static inline char *put(char *p, int64_t v, int u32, char sep) {
    p = gt_put_int(p, u32 ? (int64_t)(uint32_t)v : (int64_t)(int32_t)(uint32_t)v);
    p[-1] = sep;
    return p;
}

/* one of the three block lists: every element and a comma, then `end` */
static char *put_list(FILE *f, char *buf, size_t cap, char *p, const int32_t *v, int64_t n,
                      int u32, char end) {
    for (int64_t b = 0; b < n; ++b) {
        if ((size_t)(p - buf) > cap - 32) {
            fwrite(buf, 1, (size_t)(p - buf), f);
            p = buf;
        }
        p = put(p, v[b], u32, ',');
    }
    *p++ = end;
    return p;
}

void gt_write_psl(FILE *f, const gt_chains *c, int64_t i, const int64_t counts[4], int basic) {
    gt_write_psl_ex(f, c, i, counts, basic, !basic, 0);
}

void gt_write_psl_ex(FILE *f, const gt_chains *c, int64_t i, const int64_t counts[4], int basic,
                     int ins_ne, char t_strand) {
    const int64_t b0 = c->blk_off[i], nb = c->blk_off[i + 1] - b0;
    const int32_t *bt = c->bt + b0, *bq = c->bq + b0, *bs = c->bs + b0;
    uint32_t qn = 0, qb = 0, tn = 0, tb = 0; /* the reference's ints: 32-bit sums */
    for (int64_t b = 0; b + 1 < nb; ++b) {
        const int32_t dq = bq[b + 1] - (bq[b] + bs[b]), dt = bt[b + 1] - (bt[b] + bs[b]);
        if (ins_ne ? dq != 0 : dq > 0) {
            ++qn;
            qb += (uint32_t)dq;
        }
        if (ins_ne ? dt != 0 : dt > 0) {
            ++tn;
            tb += (uint32_t)dt;
        }
    }
    const char *tname = c->tnames.names[c->tname[i]], *qname = c->qnames.names[c->qname[i]];
    const size_t tl = strlen(tname), ql = strlen(qname);
    const size_t cap = 1 << 14, need = tl + ql + 512;
    char small[1 << 14], *buf = need <= cap ? small : malloc(need), *p = buf;
    if (!buf)
        gt_abort("Out of memory");
    for (int k = 0; k < 4; ++k)
        p = put(p, counts[k], basic, '\t');
    p = put(p, qn, basic, '\t');
    p = put(p, qb, 0, '\t');
    p = put(p, tn, basic, '\t');
    p = put(p, tb, 0, '\t');
    *p++ = c->qstrand[i] ? '-' : '+';
    if (t_strand)
        *p++ = t_strand;
    *p++ = '\t';
    memcpy(p, qname, ql);
    p += ql;
    *p++ = '\t';
    p = put(p, c->qsize[i], basic, '\t');
    p = put(p, c->qstrand[i] ? (int64_t)c->qsize[i] - c->qend[i] : c->qstart[i], basic, '\t');
    p = put(p, c->qstrand[i] ? (int64_t)c->qsize[i] - c->qstart[i] : c->qend[i], basic, '\t');
    memcpy(p, tname, tl);
    p += tl;
    *p++ = '\t';
    p = put(p, c->tsize[i], basic, '\t');
    p = put(p, c->tstart[i], basic, '\t');
    p = put(p, c->tend[i], basic, '\t');
    p = put(p, nb, basic, '\t');
    if (buf != small) { /* a long name: the lists go through the small buffer */
        fwrite(buf, 1, (size_t)(p - buf), f);
        free(buf);
        buf = p = small;
    }
    p = put_list(f, buf, cap, p, bs, nb, basic, '\t');
    p = put_list(f, buf, cap, p, bq, nb, basic, '\t');
    p = put_list(f, buf, cap, p, bt, nb, basic, '\n');
    fwrite(buf, 1, (size_t)(p - buf), f);
}

int gt_put_psl_align(gac_obuf *o, const gt_psl_align *a, const gac_axtpsl_entry *e,
                     const gac_axtpsl_block *blk) {
    const int minus = a->strand == '-';
    const uint32_t qsize = (uint32_t)a->qsize;
    uint32_t qstart = (uint32_t)a->qstart, qend = (uint32_t)a->qend;
    uint32_t tstart = (uint32_t)a->tstart, tend = (uint32_t)a->tend;
    if (minus) { /* reverseIntRange */
        const uint32_t s = qstart;
        qstart = qsize - qend, qend = qsize - s;
    }
    qstart += (uint32_t)e->q_head, tstart += (uint32_t)e->t_head; /* trimAlignment */
    qend -= (uint32_t)e->q_tail, tend -= (uint32_t)e->t_tail;
    if (qstart == qend || tstart == tend)
        return 0;
    const uint32_t qs = minus ? qsize - qend : qstart, ts = tstart;
    const int64_t nb = e->n_blocks;
    char *p = gac_obuf_reserve(o, a->qname_len + a->tname_len + 16 * 12 + 8 + (size_t)nb * 36);
    if (!p)
        gt_abort("Out of memory");
    char *const p0 = p;
    p = put(p, e->match, 1, '\t');
    p = put(p, e->mis_match, 1, '\t');
    p = put(p, e->rep_match, 1, '\t');
    p = put(p, e->n_count, 1, '\t');
    p = put(p, e->q_num_insert, 1, '\t');
    p = put(p, e->q_base_insert, 0, '\t');
    p = put(p, e->t_num_insert, 1, '\t');
    p = put(p, e->t_base_insert, 0, '\t');
    *p++ = a->strand;
    *p++ = '\t';
    memcpy(p, a->qname, a->qname_len);
    p += a->qname_len;
    *p++ = '\t';
    p = put(p, qsize, 1, '\t');
    p = put(p, qstart, 1, '\t');
    p = put(p, qend, 1, '\t');
    memcpy(p, a->tname, a->tname_len);
    p += a->tname_len;
    *p++ = '\t';
    p = put(p, (uint32_t)a->tsize, 1, '\t');
    p = put(p, tstart, 1, '\t');
    p = put(p, tend, 1, '\t');
    p = put(p, nb, 1, '\t');
    for (int64_t b = 0; b < nb; ++b)
        p = put(p, (uint32_t)blk[b].size, 1, ',');
    *p++ = '\t';
    for (int64_t b = 0; b < nb; ++b)
        p = put(p, qs + (uint32_t)blk[b].q_adv, 1, ',');
    *p++ = '\t';
    for (int64_t b = 0; b < nb; ++b)
        p = put(p, ts + (uint32_t)blk[b].t_adv, 1, ',');
    *p++ = '\n';
    o->n += (size_t)(p - p0);
    return 1;
}
