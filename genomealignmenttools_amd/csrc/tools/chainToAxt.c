/* chainToAxt -- chains back to alignment text (axt or bed), on an MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c
 * (+ kent/src/lib/chainToAxt.c, axtWrite / axtScoreSym of kent/src/lib/axt.c):
 * same command line, options and output.  Both genomes are loaded with the
 * soft-mask plane; the chains at or above -minScore (:138) are uploaded, cut
 * into pieces on the host (gac_axt_split, lib chainToAxt.c:105-121), and one
 * GPU call (gac_axt_measure) gives every piece its score, identity counts and
 * column count (axt.c:196-229, chainToAxt.c:69-89).  The pieces that pass
 * -minId are rendered in batches of at most GAC_AXT_BUDGET bytes of text
 * (default 64 MiB; a piece larger than that is a batch of its own) by two
 * render jobs used in turn (gac_axt_job): while the host writes the header
 * lines and rows of batch k, batch k + 1 is rendered and copied into the other
 * pinned buffer.  No more than two batches of text exist at any time.
 *
 * -maxChain is accepted and has no effect, as in the reference (the tool
 * passes BIGNUM to the library, :108).  A '-' query is flipped inside the
 * .2bit sequence (loadSeqStrand uses nibTwoGetSize, :58), which is what the
 * engine does, so strand coordinates are uploaded as they are. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "gac_tool.h"
#include "gachain.h"
#include "host/gac_host.h"

#define BIGNUM 0x3fffffff

static const gt_spec k_opts[] = {
    {"maxGap", GT_INT}, {"maxChain", GT_INT}, {"minScore", GT_DOUBLE},
    {"minId", GT_DOUBLE}, {"bed", GT_BOOL},   {NULL, 0},
};

static void usage(int max_gap, int max_chain) {
    gt_abort("chainToAxt - Convert from chain to axt file\n"
             "usage:\n"
             "   chainToAxt in.chain tNibDirOr2bit qNibDirOr2bit out.axt\n"
             "options:\n"
             "   -maxGap=maximum gap sized allowed without breaking, default %d\n"
             "   -maxChain=maximum chain size allowed without breaking, default %d\n"
             "   -minScore=minimum score of chain\n"
             "   -minId=minimum percentage ID within blocks\n"
             "   -bed  Output bed instead of axt\n",
             max_gap, max_chain);
}

/* the range check of twoBitReadSeqFragExt (kent/src/lib/twoBit.c:744-751) for
 * the fragment nibTwoCacheSeqPartExt asks for (nibTwo.c) */
static void check_frag(const char *name, int64_t start, int64_t end, int32_t seq_size) {
    if (end == 0)
        end = seq_size;
    if (end > seq_size)
        gt_abort("twoBitReadSeqFrag in %s end (%d) >= seqSize (%d)", name, (int)end, seq_size);
    if (end - start < 1 || start < 0)
        gt_abort("twoBitReadSeqFrag in %s start (%d) >= end (%d)", name, (int)start, (int)end);
}

static int want_softmask(gac_ctx *ctx) {
    const int rc = gac_genome_want_softmask(ctx, GAC_T);
    return rc != GAC_OK ? rc : gac_genome_want_softmask(ctx, GAC_Q);
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static size_t *name_lens(const gt_names *t) {
    size_t *len = malloc((size_t)(t->n ? t->n : 1) * sizeof(*len));
    if (!len)
        gt_abort("Out of memory");
    for (int32_t i = 0; i < t->n; ++i)
        len[i] = strlen(t->names[i]);
    return len;
}

static void *must_alloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p)
        gt_abort("Out of memory (%zu bytes)", n);
    return p;
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options(&argc, argv, k_opts);
    const int max_gap = gt_opt_int("maxGap", 100);
    const int max_chain = gt_opt_int("maxChain", BIGNUM); /* read, never used (:108) */
    /* optionFloat returns float */
    const double min_ratio = (double)(float)gt_opt_double("minId", 0.0) / 100.0;
    const double min_score = (double)(float)gt_opt_double("minScore", 0);
    const int bed = gt_opt_exists("bed");
    if (argc != 5)
        usage(max_gap, max_chain);
    const char *t2bit = argv[2], *q2bit = argv[3];
    if (!gt_file_exists(t2bit))
        gt_abort("ERROR: target 2bit file or nib directory %s does not exist\n", t2bit);
    if (!gt_file_exists(q2bit))
        gt_abort("ERROR: query 2bit file or nib directory %s does not exist\n", q2bit);
    if (!gac_is_twobit_file(t2bit))
        gt_abort("ERROR: only 2bit files are supported, not %s\n", t2bit);
    if (!gac_is_twobit_file(q2bit))
        gt_abort("ERROR: only 2bit files are supported, not %s\n", q2bit);
    int64_t budget = 64ll << 20;
    if (getenv("GAC_AXT_BUDGET") && atoll(getenv("GAC_AXT_BUDGET")) > 0)
        budget = atoll(getenv("GAC_AXT_BUDGET"));

    gt_device dev;
    gt_device_on_open(want_softmask);
    gt_stage("options + setup");
    gt_device_start(&dev, t2bit, q2bit, NULL, NULL);
    gt_chains c;
    gt_read_chains(argv[1], &c, -HUGE_VAL, 0);
    gt_stage("read chains");
    FILE *out = gt_must_open(argv[4], "w");
    setvbuf(out, NULL, _IOFBF, 1 << 20);
    gac_ctx *ctx = gt_device_join(&dev);
    gt_stage("device open + 2bit genomes (rest)");

    /* the chains at or above -minScore (:138), as a set of their own */
    int64_t nc = 0, nb = 0;
    for (int64_t i = 0; i < c.n; ++i)
        if (c.score[i] >= min_score) {
            ++nc;
            nb += c.blk_off[i + 1] - c.blk_off[i];
        }
    int64_t *sel = must_alloc((size_t)nc * 8), *boff = must_alloc((size_t)(nc + 1) * 8);
    int32_t *tseq = must_alloc((size_t)nc * 4), *qseq = must_alloc((size_t)nc * 4);
    uint8_t *strand = must_alloc((size_t)nc);
    int32_t *bt = must_alloc((size_t)nb * 4), *bq = must_alloc((size_t)nb * 4);
    int32_t *bs = must_alloc((size_t)nb * 4);
    int32_t *tmap = gt_seq_map(ctx, GAC_T, &c.tnames), *qmap = gt_seq_map(ctx, GAC_Q, &c.qnames);
    int64_t k = 0, b = 0;
    boff[0] = 0;
    for (int64_t i = 0; i < c.n; ++i) {
        if (!(c.score[i] >= min_score))
            continue;
        const char *tn = c.tnames.names[c.tname[i]], *qn = c.qnames.names[c.qname[i]];
        const int32_t ts = tmap[c.tname[i]], qs = qmap[c.qname[i]];
        if (ts < 0)
            gt_abort("%s is not in %s", tn, t2bit);
        if (qs < 0)
            gt_abort("%s is not in %s", qn, q2bit);
        /* loadSeqStrand (:48-67): the query first, '-' flipped with the .2bit size */
        const int32_t S = gac_genome_seq_size(ctx, GAC_Q, qs);
        if (c.qstrand[i])
            check_frag(qn, (int64_t)S - c.qend[i], (int64_t)S - c.qstart[i], S);
        else
            check_frag(qn, c.qstart[i], c.qend[i], S);
        check_frag(tn, c.tstart[i], c.tend[i], gac_genome_seq_size(ctx, GAC_T, ts));
        sel[k] = i;
        tseq[k] = ts;
        qseq[k] = qs;
        strand[k] = c.qstrand[i];
        for (int64_t j = c.blk_off[i]; j < c.blk_off[i + 1]; ++j, ++b) {
            /* a negative gap is undefined in the reference (assert / negative
             * memset): refused here, before anything runs on it */
            if (j > c.blk_off[i] && (c.bt[j] < c.bt[j - 1] + c.bs[j - 1] || c.bq[j] < c.bq[j - 1] + c.bs[j - 1]))
                gt_abort("chain %d: blocks overlap (negative gap before block %lld)", c.id[i],
                         (long long)(j - c.blk_off[i]));
            bt[b] = c.bt[j];
            bq[b] = c.bq[j];
            bs[b] = c.bs[j];
        }
        boff[++k] = b;
    }
    free(tmap);
    free(qmap);
    gac_chainset_desc d = {nc, tseq, qseq, strand, boff, nb, bt, bq, bs};
    gac_window *pc = NULL;
    int64_t np = 0;
    gt_check(gac_axt_split(&d, max_gap, &pc, &np));
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &d, &cs));
    gt_stage("chains to HBM");
    int32_t *score = must_alloc((size_t)np * 4);
    int64_t *match = must_alloc((size_t)np * 8), *ali = must_alloc((size_t)np * 8);
    int64_t *sym = must_alloc((size_t)np * 8);
    gt_check(gac_axt_measure(ctx, cs, pc, np, score, match, ali, sym));
    gt_stage("GPU measure");

    /* the pieces written (:113-114), compacted in place with their results */
    int64_t nw = 0;
    double *ratio = must_alloc((size_t)np * 8);
    for (int64_t p = 0; p < np; ++p) {
        const double r = match[p] == 0 ? 0.0 : (double)match[p] / (double)ali[p];
        if (!(min_ratio <= r))
            continue;
        pc[nw] = pc[p];
        score[nw] = score[p];
        sym[nw] = sym[p];
        ratio[nw++] = r;
    }
    if (bed) { /* bedWriteAxt (:91-100): no rows, no record number */
        for (int64_t p = 0; p < nw; ++p) {
            const int64_t i = sel[pc[p].chain];
            fprintf(out, "%s\t%d\t%d\t%s\t%d\t%c\n", c.tnames.names[c.tname[i]], pc[p].t_start,
                    pc[p].t_end, c.qnames.names[c.qname[i]], (int)(ratio[p] * 1000),
                    c.qstrand[i] ? '-' : '+');
        }
        gt_stage("write output");
    } else {
        int64_t cap = budget;
        for (int64_t p = 0; p < nw; ++p)
            if (2 * sym[p] + 3 > cap)
                cap = 2 * sym[p] + 3;
        gac_axt_job *job[2] = {NULL, NULL};
        int64_t *off = must_alloc((size_t)nw * 8);
        /* batches [lo[k], lo[k + 1]) of at most `budget` bytes */
        int64_t nbatch = 0, bcap = 16, *lo = must_alloc(16 * 8), *bytes = must_alloc(16 * 8);
        for (int64_t p = 0; p < nw;) {
            if (nbatch + 1 >= bcap) {
                bcap *= 2;
                lo = realloc(lo, (size_t)bcap * 8);
                bytes = realloc(bytes, (size_t)bcap * 8);
                if (!lo || !bytes)
                    gt_abort("Out of memory");
            }
            int64_t used = 0;
            lo[nbatch] = p;
            do {
                off[p] = used;
                used += 2 * sym[p] + 3;
                ++p;
            } while (p < nw && used + 2 * sym[p] + 3 <= budget);
            bytes[nbatch++] = used;
        }
        lo[nbatch] = nw;
        if (nbatch) {
            gt_check(gac_axt_job_open(ctx, nbatch > 1 || cap > budget ? cap : bytes[0], &job[0]));
            if (nbatch > 1)
                gt_check(gac_axt_job_open(ctx, cap, &job[1]));
            gt_check(gac_axt_job_submit(job[0], cs, pc + lo[0], lo[1] - lo[0], off + lo[0], bytes[0]));
        }
        gt_verbose(2, "%lld pieces in %lld batches of at most %lld text bytes\n", (long long)nw,
                   (long long)nbatch, (long long)budget);
        char head[2 * 1024];
        size_t *tlen = name_lens(&c.tnames), *qlen = name_lens(&c.qnames);
        double t_submit = 0, t_wait = 0, t_write = 0, t0 = now_s(), t1;
        for (int64_t kb = 0; kb < nbatch; ++kb) {
            if (kb + 1 < nbatch) /* the next batch renders while this one is written */
                gt_check(gac_axt_job_submit(job[(kb + 1) & 1], cs, pc + lo[kb + 1],
                                            lo[kb + 2] - lo[kb + 1], off + lo[kb + 1], bytes[kb + 1]));
            t_submit += (t1 = now_s()) - t0;
            const char *text = NULL;
            gt_check(gac_axt_job_wait(job[kb & 1], &text, NULL));
            t_wait += (t0 = now_s()) - t1;
            for (int64_t p = lo[kb]; p < lo[kb + 1]; ++p) { /* axtWrite (axt.c:101-114) */
                const int64_t i = sel[pc[p].chain];
                const int64_t b0 = boff[pc[p].chain] + pc[p].first_block, b1 = b0 + pc[p].n_blocks - 1;
                /* "%d %s %d %d %s %d %d %c %d\n" (56 M lines on a whole genome:
                 * printf's format parsing was most of the tool's time) */
                const int32_t tn = c.tname[i], qn = c.qname[i];
                if (tlen[tn] + qlen[qn] + 128 > sizeof head)
                    gt_abort("sequence names too long for an axt header line");
                char *h = gt_put_int(head, p);
                h = gt_put_str(h, c.tnames.names[tn], tlen[tn]);
                h = gt_put_int(h, (int64_t)pc[p].t_start + 1);
                h = gt_put_int(h, pc[p].t_end);
                h = gt_put_str(h, c.qnames.names[qn], qlen[qn]);
                h = gt_put_int(h, (int64_t)bq[b0] + 1);
                h = gt_put_int(h, (int64_t)bq[b1] + bs[b1]);
                *h++ = c.qstrand[i] ? '-' : '+';
                *h++ = ' ';
                h = gt_put_int(h, score[p]);
                h[-1] = '\n';
                fwrite(head, 1, (size_t)(h - head), out);
                fwrite(text + off[p], 1, (size_t)(2 * sym[p] + 3), out);
            }
            t_write += (t1 = now_s()) - t0;
            t0 = t1;
        }
        if (getenv("GAC_TIMING"))
            fprintf(stderr, "[chainToAxt] %lld batches: submit (checks + enqueue) %.3f s, wait for "
                            "render + copy %.3f s, header lines + fwrite %.3f s\n",
                    (long long)nbatch, t_submit, t_wait, t_write);
        gt_stage("render + write output");
        gac_axt_job_close(job[0]);
        gac_axt_job_close(job[1]);
    }
    gt_device_close_async(&dev, ctx, cs); /* overlaps closing the output */
    gt_careful_close(out, argv[4]);
    gac_axt_free(pc);
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
