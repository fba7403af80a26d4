/* chainToPsl -- convert chains to PSL with match counts, on an MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c:
 * same command line and output.  The reference loads both genomes one byte
 * per base and reverse-complements the whole query sequence in place, twice,
 * for every '-' chain (:55-56, :183-184); here the genomes are the resident
 * bit planes (the target with its soft-mask plane: repMatch is decided by the
 * target's case alone, :110-123), every chain is uploaded as one set with its
 * own strand coordinates, and one batched GPU call (gac_chain_psl_counts)
 * counts match / misMatch / repMatch / nCount per aligned base (:106-131).
 * The insert counts (:81-93) and the text (:130-176) are made on the host, one
 * line per chain in input order; '#' lines are skipped.  tSizes and qSizes
 * are never opened, as there. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_pslout.h"
#include "gac_seqtool.h"
#include "gachain.h"

static void usage(void) {
    gt_abort("chainToPsl - Convert chain file to psl format\n"
             "usage:\n"
             "   chainToPsl in.chain tSizes qSizes target.lst query.lst out.psl\n"
             "Where tSizes and qSizes are tab-delimited files with\n"
             "       <seqName><size>\n"
             "columns.\n"
             "The target and query lists can either be fasta files, nib files, 2bit files\n"
             "or a list of fasta, 2bit and/or nib files one per line\n");
}

typedef struct out_ctx {
    const gt_chains *c;
    const int64_t *counts;
} out_ctx;

static void write_one(FILE *f, int64_t i, void *arg) {
    const out_ctx *o = arg;
    gt_write_psl(f, o->c, i, o->counts + 4 * i, 0);
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options_hash(&argc, argv); /* optionHash (:219): any option is accepted */
    if (argc != 7)
        usage();
    const char *t2bit = argv[4], *q2bit = argv[5];
    gs_check_twobits(t2bit, q2bit, "file");

    /* device open + genome upload beside the parse */
    gt_device dev;
    /* the target side with the soft-mask plane; the query's case is never read */
    gt_device_on_open(gs_softmask_target);
    gt_stage("options + setup");
    gt_device_start(&dev, t2bit, q2bit, NULL, NULL);
    gt_verbose(1, "Scanning %s\n", t2bit);
    gt_verbose(1, "Scanning %s\n", q2bit);
    gt_verbose(1, "Converting %s\n", argv[1]);
    gt_chains c;
    gt_read_chains(argv[1], &c, -HUGE_VAL, 0);
    gt_stage("read chains");
    FILE *out = gt_must_open(argv[6], "w");
    gac_ctx *ctx = gt_device_join(&dev);
    gt_stage("device open + 2bit genomes (rest)");

    const size_t n1 = (size_t)(c.n ? c.n : 1);
    int32_t *tseq = malloc(n1 * 4), *qseq = malloc(n1 * 4);
    int64_t *counts = malloc(n1 * 4 * 8);
    if (!tseq || !qseq || !counts)
        gt_abort("Out of memory");
    int32_t *tmap = gt_seq_map(ctx, GAC_T, &c.tnames), *qmap = gt_seq_map(ctx, GAC_Q, &c.qnames);
    for (int64_t i = 0; i < c.n; ++i) {
        const char *tn = c.tnames.names[c.tname[i]], *qn = c.qnames.names[c.qname[i]];
        const int32_t ts = tmap[c.tname[i]], qs = qmap[c.qname[i]];
        if (ts < 0) /* hashMustFindVal (:206-207), the target first */
            gt_abort("hashMustFindVal: '%s' not found", tn);
        if (qs < 0)
            gt_abort("hashMustFindVal: '%s' not found", qn);
        /* The reference indexes dna[] with the block coordinates unchecked
         * (:103-104; '-': the whole sequence reversed with its own size, so
         * strand position p is forward base size - 1 - p): a block outside
         * its sequence is undefined there and refused here. */
        const int64_t T = gac_genome_seq_size(ctx, GAC_T, ts), S = gac_genome_seq_size(ctx, GAC_Q, qs);
        for (int64_t j = c.blk_off[i]; j < c.blk_off[i + 1]; ++j) {
            if (c.bt[j] < 0 || (int64_t)c.bt[j] + c.bs[j] > T)
                gt_abort("chain block %d-%d is outside target sequence %s of %d bases", c.bt[j],
                         c.bt[j] + c.bs[j], tn, (int)T);
            if (c.bq[j] < 0 || (int64_t)c.bq[j] + c.bs[j] > S)
                gt_abort("chain block %d-%d (%c strand) is outside query sequence %s of %d bases",
                         c.bq[j], c.bq[j] + c.bs[j], c.qstrand[i] ? '-' : '+', qn, (int)S);
        }
        tseq[i] = ts;
        qseq[i] = qs;
    }
    free(tmap);
    free(qmap);
    /* block query coordinates as the file has them: the engine flips a '-'
     * chain with the .2bit size, which is the reference's qSeq->size (:56) */
    gac_chainset_desc d = {c.n, tseq, qseq, c.qstrand, c.blk_off, c.nb, c.bt, c.bq, c.bs};
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &d, &cs));
    gt_stage("chains to HBM");
    gt_check(gac_chain_psl_counts(ctx, cs, counts));
    gt_stage("GPU psl counts");
    gt_device_close_async(&dev, ctx, cs); /* overlaps writing the output */

    out_ctx oc = {&c, counts};
    gt_par_write(out, c.n, write_one, &oc);
    gt_careful_close(out, argv[6]);
    gt_stage("write output");
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
