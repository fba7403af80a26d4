/* chainToAxt -- chains back to alignment text (axt or bed), on an MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c
 * (+ kent/src/lib/chainToAxt.c, axtWrite / axtScoreSym of kent/src/lib/axt.c):
 * same command line, options and output.  Both genomes are loaded with the
 * soft-mask plane; the chains at or above -minScore (:138) are uploaded, cut
 * into pieces on the host (gac_axt_split, lib chainToAxt.c:105-121), and one
 * GPU call (gac_axt_measure) gives every piece its score, identity counts and
 * column count (axt.c:196-229, chainToAxt.c:69-89).  The pieces that pass
 * -minId are rendered in batches of at most gs_axt_budget() bytes of text
 * (default 64 MiB; a piece larger than that is a batch of its own) by two
 * render jobs used in turn (gs_axt_run): while the host writes the header
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

#include "gac_seqtool.h"
#include "gachain.h"

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

/* the per-chain aborts, in the reference's order */
static void check_chain(const gs_env *k, int64_t i, int32_t ts, int32_t qs) {
    const gt_chains *c = k->c;
    const char *tn = c->tnames.names[c->tname[i]], *qn = c->qnames.names[c->qname[i]];
    if (ts < 0)
        gt_abort("%s is not in %s", tn, k->t2bit);
    if (qs < 0)
        gt_abort("%s is not in %s", qn, k->q2bit);
    /* loadSeqStrand (:48-67): the query first, '-' flipped with the .2bit size */
    const int32_t S = gac_genome_seq_size(k->ctx, GAC_Q, qs);
    if (c->qstrand[i])
        gs_check_frag(qn, (int64_t)S - c->qend[i], (int64_t)S - c->qstart[i], S);
    else
        gs_check_frag(qn, c->qstart[i], c->qend[i], S);
    gs_check_frag(tn, c->tstart[i], c->tend[i], gac_genome_seq_size(k->ctx, GAC_T, ts));
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
    gs_check_twobits(t2bit, q2bit, "2bit file or nib directory");

    gt_device dev;
    gt_device_on_open(gs_softmask_both);
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
    uint8_t *keep = gs_alloc((size_t)c.n);
    for (int64_t i = 0; i < c.n; ++i)
        keep[i] = c.score[i] >= min_score;
    int32_t *tmap = gt_seq_map(ctx, GAC_T, &c.tnames), *qmap = gt_seq_map(ctx, GAC_Q, &c.qnames);
    const gs_env env = {&c, ctx, t2bit, q2bit};
    gs_subset s;
    gs_subset_build(&env, keep, c.tname, c.qname, tmap, qmap, check_chain, 1, &s);
    free(tmap);
    free(qmap);
    free(keep);
    gac_window *pc = NULL;
    int64_t np = 0;
    gt_check(gac_axt_split(&s.d, max_gap, &pc, &np));
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &s.d, &cs));
    gt_stage("chains to HBM");
    int32_t *score = gs_alloc((size_t)np * 4);
    int64_t *match = gs_alloc((size_t)np * 8), *ali = gs_alloc((size_t)np * 8);
    int64_t *sym = gs_alloc((size_t)np * 8);
    gt_check(gac_axt_measure(ctx, cs, pc, np, score, match, ali, sym));
    gt_stage("GPU measure");

    /* the pieces written (:113-114), compacted in place with their results */
    int64_t nw = 0;
    double *ratio = gs_alloc((size_t)np * 8);
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
            const int64_t i = s.sel[pc[p].chain];
            fprintf(out, "%s\t%d\t%d\t%s\t%d\t%c\n", c.tnames.names[c.tname[i]], pc[p].t_start,
                    pc[p].t_end, c.qnames.names[c.qname[i]], (int)(ratio[p] * 1000),
                    c.qstrand[i] ? '-' : '+');
        }
        gt_stage("write output");
    } else {
        gs_axt_run run;
        gs_axt_open(&run, ctx, cs, pc, sym, nw, 0);
        gt_verbose(2, "%lld pieces in %lld batches of at most %lld text bytes\n", (long long)nw,
                   (long long)run.plan.nbatch, (long long)run.plan.budget);
        char head[GS_AXT_HEAD];
        size_t *tlen = gs_name_lens(&c.tnames), *qlen = gs_name_lens(&c.qnames);
        int64_t lo, hi;
        const char *text;
        while (gs_axt_next(&run, &lo, &hi, &text))
            for (int64_t p = lo; p < hi; ++p) { /* axtWrite (axt.c:101-114) */
                const int64_t i = s.sel[pc[p].chain];
                const int32_t tn = c.tname[i], qn = c.qname[i];
                const size_t n = gs_axt_head(head, p, &pc[p], &s, c.tnames.names[tn], tlen[tn],
                                             c.qnames.names[qn], qlen[qn], score[p]);
                fwrite(head, 1, n, out);
                fwrite(text + run.plan.off[p], 1, (size_t)(2 * sym[p] + 3), out);
            }
        if (getenv("GAC_TIMING"))
            fprintf(stderr, "[chainToAxt] %lld batches: submit (checks + enqueue) %.3f s, wait for "
                            "render + copy %.3f s, header lines + fwrite %.3f s\n",
                    (long long)run.plan.nbatch, run.t_submit, run.t_wait, run.t_write);
        gt_stage("render + write output");
        gs_axt_close(&run);
    }
    gt_device_close_async(&dev, ctx, cs); /* overlaps closing the output */
    gt_careful_close(out, argv[4]);
    gac_axt_free(pc);
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
