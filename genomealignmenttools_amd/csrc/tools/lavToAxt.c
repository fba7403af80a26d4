/* lavToAxt -- blastz / lastz .lav to axt, with the sequence (drop-in for
 * kent/src/hg/mouseStuff/lavToAxt/lavToAxt.c + kent/src/hg/lib/lav.c).
 *
 * Same command line (optionHash: any option is accepted), options and output
 * bytes.  The file is read stanza by stanza and every block list is checked
 * where the reference would abort on it, in file order: sequence names, the
 * fragment ranges (twoBitReadSeqFrag's), "Gaps in both strand".  A negative
 * gap, undefined in the reference, is refused.  A block list is one chain
 * with single-sided gaps and becomes one record with the lav's score.
 *
 * -dropSelf (breakUpIfOnDiagonal, :370-422): for a self alignment the blocks
 * whose target range meets their own query range are removed, the lists
 * before and after them become records of their own, and when anything was
 * removed every list of the alignment is rescored as axtScoreSym does under
 * -scoreScheme (default: blastz): the matrix over the ungapped columns, minus
 * O + E L per gap run of L columns, in int arithmetic.
 *
 * Two paths give the same bytes:
 *   -host    (and always with -fa / -tfa) rows are built from fragments of the
 *            mmapped .2bit (or the fasta text) on host threads, and scored
 *            from the rows.
 *   -device  both .2bit files' named sequences go to the GPU with the
 *            soft-mask plane, the block lists are uploaded as chains, one
 *            piece each, and rendered in batches by the render jobs
 *            chainToAxt uses (gs_axt_open / gs_axt_next); the rescored lists'
 *            ungapped-column sums come from gac_axt_pair_counts.
 * Without either option the host path runs.
 *
 * The reference flips '-' coordinates with the lav's qSize, not the .2bit
 * sequence's size: the engine's coordinates are shifted by (sequence size -
 * lav qSize), the lav's are printed. */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_lav.h"
#include "gac_seqtool.h"
#include "gachain.h"
#include "host/gac_host.h"

static void usage(void) {
    gt_abort("lavToAxt - Convert blastz lav file to an axt file (which includes sequence)\n"
             "usage:\n"
             "   lavToAxt in.lav tNibDir qNibDir out.axt\n"
             "Where tNibDir/qNibDir are either directories full of nib files, or a single\n"
             "twoBit file\n"
             "options:\n"
             "   -fa  qNibDir is interpreted as a fasta file of multiple dna seq instead of directory of nibs\n"
             "   -tfa tNibDir is interpreted as a fasta file of multiple dna seq instead of directory of nibs\n"
             "   -dropSelf  drops alignment blocks on the diagonal for self alignments\n"
             "   -scoreScheme=fileName Read the scoring matrix from a blastz-format file.\n"
             "                (only used in conjunction with -dropSelf, to rescore \n"
             "                alignments when blocks are dropped)\n\n");
}

/* ------------------------------------------------------- sequence sources */
typedef struct seq_src {
    const char *path;
    int is_fa;
    gac_twobit tb;
    gt_names names;  /* 2bit: the file's names in file order */
    char **fa_name;  /* fasta: in file order (the first of equal names wins) */
    char **fa_dna;
    int32_t *fa_size;
    int32_t n_fa;
    char *fa_buf;
} seq_src;

/* faReadAllMixed (fa.c:430-494): the first word after '>' names a record, its
 * letters and dashes are kept with their case */
static void fa_read(seq_src *s) {
    size_t len = 0;
    char *buf = s->fa_buf = gt_slurp(s->path, &len);
    int32_t cap = 0, line_no = 0;
    char *w = buf, *cur = buf; /* the kept letters are packed in place */
    while (*cur) {
        char *line = cur, *nl = strchr(cur, '\n');
        if (nl) {
            *nl = 0;
            cur = nl + 1;
        } else {
            cur += strlen(cur);
        }
        ++line_no;
        if (line[0] == '>') {
            char *nm = line + 1;
            while (*nm && isspace((unsigned char)*nm))
                ++nm;
            char *e = nm;
            while (*e && !isspace((unsigned char)*e))
                ++e;
            if (e == nm)
                gt_abort("Expecting sequence name after '>' line %d of %s", line_no, s->path);
            if (s->n_fa == cap) {
                cap = cap ? 2 * cap : 64;
                s->fa_name = realloc(s->fa_name, (size_t)cap * sizeof(char *));
                s->fa_dna = realloc(s->fa_dna, (size_t)cap * sizeof(char *));
                s->fa_size = realloc(s->fa_size, (size_t)cap * 4);
                if (!s->fa_name || !s->fa_dna || !s->fa_size)
                    gt_abort("Out of memory");
            }
            char *name = malloc((size_t)(e - nm) + 1);
            if (!name)
                gt_abort("Out of memory");
            memcpy(name, nm, (size_t)(e - nm));
            name[e - nm] = 0;
            if (strlen(name) > 511) /* (the reference's name buffer) */
                name[511] = 0;
            s->fa_name[s->n_fa] = name;
            s->fa_dna[s->n_fa] = w;
            s->fa_size[s->n_fa++] = 0;
            continue;
        }
        if (!s->n_fa)
            gt_abort("Expecting '>' line %d of %s", line_no, s->path);
        for (const char *p = line; *p; ++p)
            if (isalpha((unsigned char)*p) || *p == '-')
                *w++ = *p;
        s->fa_size[s->n_fa - 1] = (int32_t)(w - s->fa_dna[s->n_fa - 1]);
    }
}

static void src_open(seq_src *s, const char *path, int is_fa, const char *side) {
    memset(s, 0, sizeof(*s));
    s->path = path;
    s->is_fa = is_fa;
    if (is_fa) {
        fa_read(s);
        return;
    }
    if (!gt_file_exists(path))
        gt_abort("ERROR: %s 2bit file or nib directory %s does not exist\n", side, path);
    if (!gac_is_twobit_file(path))
        gt_abort("ERROR: only 2bit files are supported, not %s\n", path);
    gt_check(gac_twobit_open(path, &s->tb));
    for (uint32_t i = 0; i < s->tb.seq_count; ++i)
        gt_names_add(&s->names, s->tb.seqs[i].name, strlen(s->tb.seqs[i].name));
}

static int32_t src_find(const seq_src *s, const char *name) {
    if (!s->is_fa)
        return gt_names_find(&s->names, name);
    for (int32_t i = 0; i < s->n_fa; ++i)
        if (!strcmp(s->fa_name[i], name))
            return i;
    return -1;
}

static int32_t src_size(const seq_src *s, int32_t i) {
    return s->is_fa ? s->fa_size[i] : (int32_t)s->tb.seqs[i].size;
}

/* runs [starts[r], starts[r] + sizes[r]) (ascending, disjoint) cut to
 * [start, end): fn over each part */
static void over_runs(const gac_twobit *tb, const uint8_t *starts, const uint8_t *sizes,
                      uint32_t count, int64_t start, int64_t end, char *out, int lower) {
    uint32_t lo = 0, hi = count; /* the first run that ends after start */
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int64_t e = (int64_t)gac_twobit_u32(tb, starts + 4 * (size_t)mid) +
                          gac_twobit_u32(tb, sizes + 4 * (size_t)mid);
        if (e > start)
            hi = mid;
        else
            lo = mid + 1;
    }
    for (uint32_t r = lo; r < count; ++r) {
        const int64_t a = gac_twobit_u32(tb, starts + 4 * (size_t)r);
        if (a >= end)
            break;
        const int64_t b = a + gac_twobit_u32(tb, sizes + 4 * (size_t)r);
        const int64_t x = a > start ? a : start, y = b < end ? b : end;
        for (int64_t i = x; i < y; ++i)
            out[i - start] = lower ? (char)tolower((unsigned char)out[i - start]) : 'N';
    }
}

/* [start, end) of sequence i as twoBitReadSeqFrag gives it (upper case, N
 * runs, then the mask runs lower-cased), or as the fasta text has it */
static void src_fetch(const seq_src *s, int32_t i, int64_t start, int64_t end, char *out) {
    if (s->is_fa) {
        memcpy(out, s->fa_dna[i] + start, (size_t)(end - start));
        return;
    }
    const gac_twobit_seq *q = &s->tb.seqs[i];
    for (int64_t p = start; p < end; ++p)
        out[p - start] = "TCAG"[(q->packed[p >> 2] >> (6 - 2 * (p & 3))) & 3];
    over_runs(&s->tb, q->n_starts_raw, q->n_sizes_raw, q->n_count, start, end, out, 0);
    over_runs(&s->tb, q->m_starts_raw, q->m_sizes_raw, q->m_count, start, end, out, 1);
}

/* reverseComplement with kent's ntCompTable (dnautil.c:401-447): a byte it
 * does not know becomes 0 */
static char g_comp[256];
static void comp_init(void) {
    static const char from[] = " -=acgtun.ACGTUNRYMKSWVHDBXryswmkvhdbx()";
    static const char to[] = " -=tgcaan.TGCAANYRKMSWBDHVNyrswkmbdhvn)(";
    for (size_t i = 0; from[i]; ++i)
        g_comp[(unsigned char)from[i]] = to[i];
}

static void rev_comp(char *s, int64_t n) {
    for (int64_t i = 0, j = n - 1; i <= j; ++i, --j) {
        const char a = g_comp[(unsigned char)s[i]], b = g_comp[(unsigned char)s[j]];
        s[i] = b;
        s[j] = a;
    }
}

/* ------------------------------------------------------------ the records */
typedef struct rec {
    int32_t tn, qn;     /* name table indices */
    int32_t tseq, qseq; /* sequence indices in the two sources */
    int32_t q_size;     /* the lav's, which flips '-' coordinates */
    int32_t t_start, t_end, q_start, q_end;
    int32_t score;
    uint8_t is_rc, rescore;
    int32_t nb;
    int64_t b0, sym;
    char *pre; /* 'd' stanza header lines that go before this record */
} rec;

typedef struct job {
    rec *r;
    int64_t n, cap;
    int32_t *bt, *bq, *bs; /* bq: the lav's strand coordinates */
    int64_t nblk, bcap;
    gt_names tnames, qnames;
    seq_src T, Q;
    int32_t mat[16], gap_open, gap_extend;
    int32_t by_char[256][256]; /* the scheme as axtScoreSym indexes it */
    char *pending;             /* header lines met since the last record */
    char *tail;                /* ... after the last one */
} job;

static void text_append(char **dst, const char *s, size_t n) {
    const size_t have = *dst ? strlen(*dst) : 0;
    *dst = realloc(*dst, have + n + 1);
    if (!*dst)
        gt_abort("Out of memory");
    memcpy(*dst + have, s, n);
    (*dst)[have + n] = 0;
}

/* What axtScoreSym subtracts for the gap runs of a block list: a zero-length
 * block leaves the runs on its two sides one run. */
static int32_t gap_terms(const job *J, const rec *r) {
    uint32_t cost = 0;
    int in_gap = 0;
    for (int64_t b = r->b0; b < r->b0 + r->nb; ++b) {
        if (b > r->b0) {
            const int64_t g = ((int64_t)J->bt[b] - (J->bt[b - 1] + J->bs[b - 1])) +
                              ((int64_t)J->bq[b] - (J->bq[b - 1] + J->bs[b - 1]));
            if (g > 0) {
                cost += (uint32_t)J->gap_extend * (uint32_t)g + (in_gap ? 0u : (uint32_t)J->gap_open);
                in_gap = 1;
            }
        }
        if (J->bs[b] > 0)
            in_gap = 0;
    }
    return (int32_t)cost;
}

/* outputBlocks' checks (:165-290) on one block list, then the list is kept */
static void add_list(job *J, const gl_reader *R, const gl_block *b, int64_t n, int rescore) {
    if (n == 0)
        return;
    const char *tname = R->t_name ? R->t_name : "(null)", *qname = R->q_name ? R->q_name : "(null)";
    int32_t qs = 0x3fffffff, qe = 0, ts = 0x3fffffff, te = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (qs > b[i].q_start) qs = b[i].q_start;
        if (qe < b[i].q_end) qe = b[i].q_end;
        if (ts > b[i].t_start) ts = b[i].t_start;
        if (te < b[i].t_end) te = b[i].t_end;
    }
    /* the query first, a reverse-complement stanza flipped with the lav's qSize */
    const int32_t qi = src_find(&J->Q, qname);
    if (qi < 0) {
        if (J->Q.is_fa)
            gt_abort("sequence not found %s\n\n", qname);
        gt_abort("%s is not in %s", qname, J->Q.path);
    }
    const int64_t fq0 = R->is_rc ? (int64_t)R->q_size - qe : qs;
    const int64_t fq1 = R->is_rc ? (int64_t)R->q_size - qs : qe;
    if (J->Q.is_fa) {
        if (fq0 < 0 || fq1 > src_size(&J->Q, qi) || fq0 > fq1)
            gt_abort("%s:%lld-%lld is outside the %d bases of %s in %s", qname, (long long)fq0,
                     (long long)fq1, src_size(&J->Q, qi), qname, J->Q.path);
    } else {
        gs_check_frag(qname, fq0, fq1, src_size(&J->Q, qi));
    }
    const int32_t ti = src_find(&J->T, tname);
    if (ti < 0) {
        if (J->T.is_fa)
            gt_abort("sequence not found %s\n\n", tname);
        gt_abort("%s is not in %s", tname, J->T.path);
    }
    if (J->T.is_fa) {
        if (ts < 0 || te > src_size(&J->T, ti) || ts > te)
            gt_abort("%s:%d-%d is outside the %d bases of %s in %s", tname, ts, te,
                     src_size(&J->T, ti), tname, J->T.path);
    } else {
        gs_check_frag(tname, ts, te, src_size(&J->T, ti));
    }
    int64_t sym = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (i > 0) {
            const int64_t qg = (int64_t)b[i].q_start - b[i - 1].q_end;
            const int64_t tg = (int64_t)b[i].t_start - b[i - 1].t_end;
            if (qg != 0 && tg != 0)
                gt_abort("Gaps in both strand on alignment ending line %d of %s", R->line, R->path);
            if (qg < 0 || tg < 0) /* undefined in the reference (a negative append) */
                gt_abort("negative gap before block %lld (dt %lld, dq %lld) of the alignment ending "
                         "line %d of %s", (long long)i, (long long)tg, (long long)qg, R->line, R->path);
            sym += qg + tg;
        }
        if (b[i].t_end < b[i].t_start)
            gt_abort("negative block size in the alignment ending line %d of %s", R->line, R->path);
        sym += b[i].t_end - b[i].t_start;
    }
    if (J->n == J->cap) {
        J->cap = J->cap ? 2 * J->cap : 1024;
        J->r = realloc(J->r, (size_t)J->cap * sizeof(rec));
        if (!J->r)
            gt_abort("Out of memory");
    }
    if (J->nblk + n > J->bcap) {
        J->bcap = 2 * (J->nblk + n) + 1024;
        J->bt = realloc(J->bt, (size_t)J->bcap * 4), J->bq = realloc(J->bq, (size_t)J->bcap * 4);
        J->bs = realloc(J->bs, (size_t)J->bcap * 4);
        if (!J->bt || !J->bq || !J->bs)
            gt_abort("Out of memory");
    }
    rec *r = &J->r[J->n++];
    memset(r, 0, sizeof(*r));
    r->tn = gt_names_add(&J->tnames, tname, strlen(tname));
    r->qn = gt_names_add(&J->qnames, qname, strlen(qname));
    r->tseq = ti, r->qseq = qi;
    r->q_size = R->q_size;
    r->t_start = ts, r->t_end = te, r->q_start = qs, r->q_end = qe;
    r->score = R->score;
    r->is_rc = (uint8_t)R->is_rc;
    r->rescore = (uint8_t)rescore;
    r->nb = (int32_t)n;
    r->b0 = J->nblk;
    r->sym = sym;
    r->pre = J->pending;
    J->pending = NULL;
    for (int64_t i = 0; i < n; ++i) {
        J->bt[J->nblk] = b[i].t_start;
        J->bq[J->nblk] = b[i].q_start;
        J->bs[J->nblk++] = b[i].t_end - b[i].t_start;
    }
}

/* breakUpIfOnDiagonal (:370-422) and the loop over its lists (:462-477) */
static void add_drop_self(job *J, const gl_reader *R) {
    enum { MAX_LISTS = 256 };
    int64_t lo[MAX_LISTS], hi[MAX_LISTS];
    int idx = 0, broken = 0;
    const int64_t n = R->nb;
    lo[0] = 0, hi[0] = n;
    if (R->q_name && R->t_name && !strcmp(R->q_name, R->t_name)) {
        int64_t head = 0; /* the first block of the list being built */
        for (int64_t i = 0; i < n; ++i) {
            const gl_block *b = &R->blk[i];
            int32_t qs = b->q_start, qe = b->q_end;
            if (R->is_rc) {
                const int32_t s = qs;
                qs = R->q_size - qe, qe = R->q_size - s;
            }
            const int32_t s = b->t_start > qs ? b->t_start : qs, e = b->t_end < qe ? b->t_end : qe;
            if (e - s > 0) {
                broken = 1;
                if (i != head) {
                    lo[idx] = head, hi[idx] = i;
                    if (++idx >= MAX_LISTS)
                        gt_abort("breakUpIfOnDiagonal: Too many fragmented block lists!");
                }
                head = i + 1;
            }
        }
        if (head >= n)
            --idx;
        else
            lo[idx] = head, hi[idx] = n;
    }
    for (int k = 0; k <= idx; ++k) {
        int64_t m = hi[k] - lo[k];
        /* (only a self alignment's lists are frayed again, :415-418; the
         * stanza's own ends were trimmed by the reader) */
        const gl_block *b = R->blk + lo[k];
        if (R->q_name && R->t_name && !strcmp(R->q_name, R->t_name))
            b = gl_remove_frayed((gl_block *)b, &m);
        add_list(J, R, b, m, broken);
    }
}

/* -------------------------------------------------------------- host path */
enum { HOST_RUN = 32 }; /* records per run of the parallel writer */

static void put_head(gac_obuf *o, const job *J, int64_t k, int32_t score) {
    const rec *r = &J->r[k];
    const char *tn = J->tnames.names[r->tn], *qn = J->qnames.names[r->qn];
    const size_t tl = strlen(tn), ql = strlen(qn);
    char *p = gac_obuf_reserve(o, tl + ql + 128), *h = p;
    h = gt_put_int(h, k);
    h = gt_put_str(h, tn, tl);
    h = gt_put_int(h, (int64_t)r->t_start + 1);
    h = gt_put_int(h, r->t_end);
    h = gt_put_str(h, qn, ql);
    h = gt_put_int(h, (int64_t)r->q_start + 1);
    h = gt_put_int(h, r->q_end);
    *h++ = r->is_rc ? '-' : '+';
    *h++ = ' ';
    h = gt_put_int(h, score);
    h[-1] = '\n';
    o->n += (size_t)(h - p);
}

static void host_run(gac_obuf *o, int64_t run, void *arg) {
    const job *J = arg;
    const int64_t k1 = (run + 1) * HOST_RUN < J->n ? (run + 1) * HOST_RUN : J->n;
    char *tf = NULL, *qf = NULL;
    int64_t tcap = 0, qcap = 0;
    for (int64_t k = run * HOST_RUN; k < k1; ++k) {
        const rec *r = &J->r[k];
        if (r->pre) {
            const size_t n = strlen(r->pre);
            memcpy(gac_obuf_reserve(o, n), r->pre, n);
            o->n += n;
        }
        const int64_t tl = (int64_t)r->t_end - r->t_start, ql = (int64_t)r->q_end - r->q_start;
        if (tl > tcap) {
            free(tf);
            tf = gs_alloc((size_t)(tcap = tl + tl / 2 + 64));
        }
        if (ql > qcap) {
            free(qf);
            qf = gs_alloc((size_t)(qcap = ql + ql / 2 + 64));
        }
        src_fetch(&J->T, r->tseq, r->t_start, r->t_end, tf);
        if (r->is_rc) {
            src_fetch(&J->Q, r->qseq, (int64_t)r->q_size - r->q_end, (int64_t)r->q_size - r->q_start, qf);
            rev_comp(qf, ql);
        } else {
            src_fetch(&J->Q, r->qseq, r->q_start, r->q_end, qf);
        }
        /* the rows in scratch space behind the header's place, so that the
         * header can carry the new score */
        const size_t sym = (size_t)r->sym;
        char *rows = gs_alloc(2 * sym + 3), *ts = rows, *qs = rows + sym + 1;
        int64_t c = 0;
        for (int64_t b = r->b0; b < r->b0 + r->nb; ++b) {
            const int64_t bt = J->bt[b] - r->t_start, bq = J->bq[b] - r->q_start, z = J->bs[b];
            if (b > r->b0) {
                const int64_t pt = J->bt[b - 1] + J->bs[b - 1] - r->t_start;
                const int64_t pq = J->bq[b - 1] + J->bs[b - 1] - r->q_start;
                const int64_t qg = bq - pq, tg = bt - pt;
                if (qg > 0) {
                    memset(ts + c, '-', (size_t)qg);
                    memcpy(qs + c, qf + pq, (size_t)qg);
                    c += qg;
                }
                if (tg > 0) {
                    memset(qs + c, '-', (size_t)tg);
                    memcpy(ts + c, tf + pt, (size_t)tg);
                    c += tg;
                }
            }
            memcpy(ts + c, tf + bt, (size_t)z);
            memcpy(qs + c, qf + bq, (size_t)z);
            c += z;
        }
        ts[sym] = '\n';
        qs[sym] = '\n';
        qs[sym + 1] = '\n';
        int32_t score = r->score;
        if (r->rescore) { /* axtScoreSym (axt.c:196-229) */
            uint32_t sc = 0;
            int last_gap = 0;
            for (size_t i = 0; i < sym; ++i) {
                const unsigned char q = (unsigned char)qs[i], t = (unsigned char)ts[i];
                if (q == '-' || t == '-') {
                    sc -= last_gap ? (uint32_t)J->gap_extend : (uint32_t)(J->gap_open + J->gap_extend);
                    last_gap = 1;
                } else {
                    sc += (uint32_t)J->by_char[q][t];
                    last_gap = 0;
                }
            }
            score = (int32_t)sc;
        }
        put_head(o, J, k, score);
        memcpy(gac_obuf_reserve(o, 2 * sym + 3), rows, 2 * sym + 3);
        o->n += 2 * sym + 3;
        free(rows);
    }
    free(tf);
    free(qf);
}

/* ------------------------------------------------------------ device path */
static void device_path(job *J, gt_device *dev, FILE *out) {
    const int64_t n = J->n;
    gac_ctx *ctx = gt_device_join(dev);
    gt_stage("device open (rest)");
    /* only the sequences the lav names */
    seq_src *src[2] = {&J->T, &J->Q};
    int32_t *dmap[2];
    for (int side = 0; side < 2; ++side) {
        const uint32_t ns = src[side]->tb.seq_count;
        uint8_t *keep = calloc(ns ? ns : 1, 1);
        if (!keep)
            gt_abort("Out of memory");
        for (int64_t k = 0; k < n; ++k)
            keep[side ? J->r[k].qseq : J->r[k].tseq] = 1;
        gac_twobit tb;
        gt_check(gac_twobit_open(src[side]->path, &tb));
        gt_check(gac_genome_load_twobit_keep(ctx, side, &tb, keep));
        dmap[side] = gs_alloc((size_t)ns * 4);
        for (uint32_t i = 0; i < ns; ++i)
            dmap[side][i] = keep[i] ? gac_genome_seq_index(ctx, side, src[side]->tb.seqs[i].name) : -1;
        free(keep);
    }
    gt_stage("2bit genomes to HBM");
    /* the block lists as chains of their own; '-' query coordinates move by
     * (sequence size - lav qSize) for the engine, the lav's are printed */
    gs_subset s, sp;
    memset(&s, 0, sizeof(s));
    s.nc = n, s.nb = J->nblk;
    s.sel = gs_alloc((size_t)n * 8), s.boff = gs_alloc((size_t)(n + 1) * 8);
    s.tseq = gs_alloc((size_t)n * 4), s.qseq = gs_alloc((size_t)n * 4);
    s.strand = gs_alloc((size_t)n);
    s.bt = J->bt, s.bs = J->bs, s.bq = gs_alloc((size_t)J->nblk * 4);
    gac_window *pc = gs_alloc((size_t)n * sizeof(*pc));
    int64_t *sym = gs_alloc((size_t)n * 8);
    int32_t *score = gs_alloc((size_t)n * 4);
    int64_t n_re = 0;
    for (int64_t k = 0; k < n; ++k) {
        const rec *r = &J->r[k];
        s.sel[k] = k;
        s.boff[k] = r->b0;
        s.tseq[k] = dmap[0][r->tseq], s.qseq[k] = dmap[1][r->qseq];
        s.strand[k] = r->is_rc;
        const int32_t shift = r->is_rc ? src_size(&J->Q, r->qseq) - r->q_size : 0;
        for (int64_t b = r->b0; b < r->b0 + r->nb; ++b)
            s.bq[b] = J->bq[b] + shift;
        pc[k] = (gac_window){(int32_t)k, r->t_start, r->t_end, 0, r->nb};
        sym[k] = r->sym;
        score[k] = r->score;
        n_re += r->rescore;
    }
    s.boff[n] = J->nblk;
    s.d = (gac_chainset_desc){n, s.tseq, s.qseq, s.strand, s.boff, s.nb, s.bt, s.bq, s.bs};
    sp = s;
    sp.bq = J->bq;
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &s.d, &cs));
    gt_stage("chains to HBM");
    if (n_re) { /* -dropSelf: the lists of the broken alignments under the scheme */
        gac_window *rp = gs_alloc((size_t)n_re * sizeof(*rp));
        int64_t *pairs = gs_alloc((size_t)n_re * 16 * 8), *ncols = gs_alloc((size_t)n_re * 8);
        int64_t m = 0;
        for (int64_t k = 0; k < n; ++k)
            if (J->r[k].rescore)
                rp[m++] = pc[k];
        gt_check(gac_axt_pair_counts(ctx, cs, rp, n_re, pairs, ncols));
        m = 0;
        for (int64_t k = 0; k < n; ++k) {
            if (!J->r[k].rescore)
                continue;
            uint32_t sc = 0; /* the reference's int arithmetic wraps */
            for (int i = 0; i < 16; ++i)
                sc += (uint32_t)J->mat[i] * (uint32_t)pairs[m * 16 + i];
            score[k] = (int32_t)(sc - (uint32_t)gap_terms(J, &J->r[k]));
            ++m;
        }
        free(rp);
        free(pairs);
        free(ncols);
        gt_stage("GPU pair counts");
    }
    gs_axt_run run;
    gs_axt_open(&run, ctx, cs, pc, sym, n, 0);
    gt_verbose(2, "%lld records in %lld batches of at most %lld text bytes\n", (long long)n,
               (long long)run.plan.nbatch, (long long)run.plan.budget);
    char head[GS_AXT_HEAD];
    size_t *tlen = gs_name_lens(&J->tnames), *qlen = gs_name_lens(&J->qnames);
    int64_t lo, hi;
    const char *text;
    while (gs_axt_next(&run, &lo, &hi, &text))
        for (int64_t p = lo; p < hi; ++p) {
            const rec *r = &J->r[p];
            if (r->pre)
                fputs(r->pre, out);
            const size_t hn = gs_axt_head(head, p, &pc[p], &sp, J->tnames.names[r->tn], tlen[r->tn],
                                          J->qnames.names[r->qn], qlen[r->qn], score[p]);
            fwrite(head, 1, hn, out);
            fwrite(text + run.plan.off[p], 1, (size_t)(2 * sym[p] + 3), out);
        }
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[lavToAxt] %lld batches: submit (checks + enqueue) %.3f s, wait for "
                        "render + copy %.3f s, header lines + fwrite %.3f s\n",
                (long long)run.plan.nbatch, run.t_submit, run.t_wait, run.t_write);
    gt_stage("render + write output");
    gs_axt_close(&run);
    gt_device_close_async(dev, ctx, cs);
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options_hash(&argc, argv);
    if (argc != 5)
        usage();
    const int q_fa = gt_opt_exists("fa"), t_fa = gt_opt_exists("tfa");
    const int drop_self = gt_opt_exists("dropSelf");
    const int want_device = gt_opt_exists("device");
    if (want_device && gt_opt_exists("host"))
        gt_abort("-host and -device exclude each other");
    if (want_device && (q_fa || t_fa))
        gt_abort("-device needs both sides as .2bit files (not -fa / -tfa)");
    const int device = want_device;
    static job J;
    comp_init();
    /* the reference's order: the query's fasta, the target's, the scheme */
    if (q_fa)
        src_open(&J.Q, argv[3], 1, "query");
    src_open(&J.T, argv[2], t_fa, "target");
    if (!q_fa)
        src_open(&J.Q, argv[3], 0, "query");
    gt_check(gac_scheme_read(gt_opt_str("scoreScheme", NULL), J.mat, &J.gap_open, &J.gap_extend, NULL));
    static const char acgt[] = "acgt";
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { /* propagateCase (axt.c) */
            const int v = J.mat[i * 4 + j], q = acgt[i], t = acgt[j];
            J.by_char[q][t] = J.by_char[q][toupper(t)] = v;
            J.by_char[toupper(q)][t] = J.by_char[toupper(q)][toupper(t)] = v;
        }
    gt_device dev;
    if (device) {
        gt_device_on_open(gs_softmask_both);
        gt_device_start_bare(&dev);
    }
    FILE *out = gt_must_open(argv[4], "w");
    setvbuf(out, NULL, _IOFBF, 1 << 20);
    gt_stage("options + setup");

    /* header lines of 'd' stanzas are collected in memory and go before the
     * next record, where the reference's sequential writes put them */
    char *hdr = NULL;
    size_t hdr_len = 0;
    FILE *hf = open_memstream(&hdr, &hdr_len);
    if (!hf)
        gt_abort("Out of memory");
    gl_reader R;
    gl_open(&R, argv[1], hf, 0, NULL);
    for (;;) {
        const int more = gl_next(&R);
        fflush(hf);
        if (hdr_len) {
            text_append(&J.pending, hdr, hdr_len);
            fclose(hf);
            free(hdr);
            hdr = NULL;
            if (!(hf = open_memstream(&hdr, &hdr_len)))
                gt_abort("Out of memory");
            R.out = hf;
        }
        if (!more)
            break;
        if (drop_self)
            add_drop_self(&J, &R);
        else
            add_list(&J, &R, R.blk, R.nb, 0);
    }
    J.tail = J.pending;
    J.pending = NULL;
    gt_stage("read lav + checks");

    if (device) {
        device_path(&J, &dev, out);
    } else {
        if (gac_par_output_buf(out, (J.n + HOST_RUN - 1) / HOST_RUN, host_run, &J) != 0)
            gt_abort("writing %s failed", argv[4]);
        gt_stage("rows + write output (host)");
    }
    if (J.tail)
        fputs(J.tail, out);
    gt_careful_close(out, argv[4]);
    if (device) {
        gt_device_close_join(&dev);
        gt_stage("device close (rest)");
    }
    gt_exit_ok();
}
