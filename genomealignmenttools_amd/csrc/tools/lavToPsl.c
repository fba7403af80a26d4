/* lavToPsl -- blastz / lastz .lav to PSL (drop-in for
 * kent/src/hg/mouseStuff/lavToPsl/lavToPsl.c; host only, no sequence is read).
 *
 * Same command line (optionHash: any option is accepted) and output bytes.
 * Per 'a' stanza one pslTabOut line: match = the sum over the blocks of
 * round(0.01 * percentId * bases) (:50-53), misMatch the other bases,
 * repMatch = nCount = 0, inserts counted where two blocks do not abut
 * (:57-66), the query span flipped by the lav's qSize for a reverse-complement
 * stanza, strand '+' / '-' followed by the first character of -target-strand.
 * Zero-length blocks are dropped while reading (:160-164), then
 * removeFrayedEnds.  -bed: bedFromPsl + bedTabOutN(12) (basicBed.c:713-763,
 * 518-618) with pslCalcMilliBad's arithmetic (psl.c:754-785).  -scoreFile: one
 * line per 's' line of an 'a' stanza, whether the stanza gives a record or
 * not.  A lastz 'd' stanza's header lines go into the output where it occurs
 * (lav.c:106-130). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_lav.h"
#include "gac_pslout.h"

static void usage(void) {
    gt_abort("lavToPsl - Convert blastz lav to psl format\n"
             "usage:\n"
             "   lavToPsl in.lav out.psl\n"
             "options:\n"
             "   -target-strand=c set the target strand to c (default is no strand)\n"
             "   -bed output bed instead of psl\n"
             "   -scoreFile=filename  output lav scores to side file, such that\n"
             "                        each psl line in out.psl is matched by a score line.\n\n");
}

static const char *or_null(const char *s) { return s ? s : "(null)"; }

/* bedFromPsl + bedTabOutN(12) of the record */
static void write_bed(FILE *f, const gl_reader *r, uint32_t match, uint32_t mis, uint32_t q_num,
                      char t_strand) {
    const gl_block *b = r->blk;
    const int64_t nb = r->nb;
    const uint32_t q0 = (uint32_t)b[0].q_start, q1 = (uint32_t)b[nb - 1].q_end;
    const uint32_t qsize = (uint32_t)r->q_size, tsize = (uint32_t)r->t_size;
    const uint32_t qstart = r->is_rc ? qsize - q1 : q0, qend = r->is_rc ? qsize - q0 : q1;
    const uint32_t tstart = (uint32_t)b[0].t_start, tend = (uint32_t)b[nb - 1].t_end;
    if (qstart >= qend || qend > qsize || tstart >= tend || tend > tsize)
        gt_abort("mangled psl format for %s", or_null(r->q_name));
    /* pslIsProtein (psl.c:743-752) on the last block */
    const uint32_t last_t = (uint32_t)b[nb - 1].t_start;
    const uint32_t last_z = (uint32_t)(b[nb - 1].t_end - b[nb - 1].t_start);
    const int protein = (t_strand == '+' && tend == last_t + 3 * last_z) ||
                        (t_strand == '-' && tstart == tsize - (last_t + 3 * last_z));
    /* pslCalcMilliBad(psl, TRUE) */
    const int size_mul = protein ? 3 : 1;
    const int q_ali = size_mul * (int)(qend - qstart), t_ali = (int)(tend - tstart);
    const int ali = q_ali < t_ali ? q_ali : t_ali;
    int milli_bad = 0;
    if (ali > 0) {
        int size_dif = q_ali - t_ali;
        if (size_dif < 0)
            size_dif = 0;
        const int insert_factor = (int)q_num;
        const int total = size_mul * (int)(match + 0 + mis);
        if (total != 0)
            milli_bad = (int)((1000 * ((mis * (uint32_t)size_mul + (uint32_t)insert_factor) +
                                       round(3 * log(1 + size_dif)))) /
                              total);
    }
    int score = 1000 - 2 * milli_bad;
    if (score < 0)
        score = 0;
    char strand = r->is_rc ? '-' : '+';
    int32_t *sizes = malloc((size_t)nb * 4), *starts = malloc((size_t)nb * 4);
    if (!sizes || !starts)
        gt_abort("Out of memory");
    for (int64_t i = 0; i < nb; ++i) {
        sizes[i] = (protein ? 3 : 1) * (b[i].t_end - b[i].t_start);
        starts[i] = b[i].t_start;
    }
    if (t_strand == '-') { /* a minus target strand is switched to plus */
        for (int64_t i = 0; i < nb / 2; ++i) {
            int32_t x = sizes[i];
            sizes[i] = sizes[nb - 1 - i], sizes[nb - 1 - i] = x;
            x = starts[i];
            starts[i] = starts[nb - 1 - i], starts[nb - 1 - i] = x;
        }
        for (int64_t i = 0; i < nb; ++i)
            starts[i] = (int32_t)tsize - starts[i] - sizes[i];
        strand = strand == '-' ? '+' : '-';
    }
    fprintf(f, "%s\t%u\t%u\t%s\t%d\t%c\t%u\t%u\t%u\t%d\t", or_null(r->t_name), tstart, tend,
            or_null(r->q_name), score, strand, tstart, tend, 0u, (int)nb);
    for (int64_t i = 0; i < nb; ++i)
        fprintf(f, "%d,", sizes[i]);
    fputc('\t', f);
    for (int64_t i = 0; i < nb; ++i)
        fprintf(f, "%d,", (int32_t)((uint32_t)starts[i] - tstart));
    fputc('\n', f);
    free(sizes);
    free(starts);
}

int main(int argc, char *argv[]) {
    gt_options_hash(&argc, argv);
    if (argc != 3)
        usage();
    const char t_strand = gt_opt_str("target-strand", "")[0];
    const char *score_path = gt_opt_str("scoreFile", NULL);
    const int bed = gt_opt_exists("bed");
    FILE *out = gt_must_open(argv[2], "w");
    FILE *ff = score_path ? gt_must_open(score_path, "w") : NULL;
    setvbuf(out, NULL, _IOFBF, 1 << 20);
    gl_reader r;
    gl_open(&r, argv[1], out, 1, ff);
    int32_t *bt = NULL, *bq = NULL, *bs = NULL;
    int64_t cap = 0;
    while (gl_next(&r)) {
        const int64_t nb = r.nb;
        if (nb == 0)
            continue;
        if (nb > cap) {
            cap = nb + nb / 2 + 64;
            bt = realloc(bt, (size_t)cap * 4), bq = realloc(bq, (size_t)cap * 4);
            bs = realloc(bs, (size_t)cap * 4);
            if (!bt || !bq || !bs)
                gt_abort("Out of memory");
        }
        /* the reference's ints: 32-bit sums */
        uint32_t match = 0, mis = 0, q_num = 0;
        for (int64_t i = 0; i < nb; ++i) {
            const gl_block *b = &r.blk[i];
            const double scale = 0.01 * b->pct;
            const int bases = b->q_end - b->q_start;
            const int one = (int)round(scale * bases);
            match += (uint32_t)one;
            mis += (uint32_t)(bases - one);
            if (i > 0 && b->q_start != b[-1].q_end)
                ++q_num;
            bt[i] = b->t_start;
            bq[i] = b->q_start;
            bs[i] = b->t_end - b->t_start;
        }
        if (bed) {
            write_bed(out, &r, match, mis, q_num, t_strand);
            continue;
        }
        char *tn = (char *)or_null(r.t_name), *qn = (char *)or_null(r.q_name);
        int32_t zero = 0, tsize = r.t_size, qsize = r.q_size;
        int32_t tstart = r.blk[0].t_start, tend = r.blk[nb - 1].t_end;
        int32_t qstart = r.blk[0].q_start, qend = r.blk[nb - 1].q_end;
        uint8_t strand = (uint8_t)r.is_rc;
        int64_t off[2] = {0, nb};
        gt_chains c;
        memset(&c, 0, sizeof(c));
        c.n = 1;
        c.tname = c.qname = &zero;
        c.tnames.names = &tn, c.tnames.n = 1;
        c.qnames.names = &qn, c.qnames.n = 1;
        c.tsize = &tsize, c.tstart = &tstart, c.tend = &tend;
        c.qsize = &qsize, c.qstart = &qstart, c.qend = &qend;
        c.qstrand = &strand;
        c.blk_off = off;
        c.nb = nb;
        c.bt = bt, c.bq = bq, c.bs = bs;
        const int64_t counts[4] = {match, mis, 0, 0};
        gt_write_psl_ex(out, &c, 0, counts, 1, 1, t_strand);
    }
    gt_careful_close(out, argv[2]);
    if (ff)
        gt_careful_close(ff, score_path);
    gl_close(&r);
    free(bt);
    free(bq);
    free(bs);
    gt_exit_ok();
}
