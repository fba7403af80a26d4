/* chainAntiRepeat -- drop chains that are mostly repeats or degenerate DNA,
 * on an MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/chainAntiRepeat/
 * chainAntiRepeat.c: same command line, options and output.  Both genomes
 * are loaded with the soft-mask plane; the chains scoring under
 * -noCheckScore (:138) are uploaded and one batched GPU call
 * (gac_chain_composition) counts what degeneracyFilter and repeatFilter
 * count per aligned base (:53-66, :102-114); the two decisions are taken on
 * the host (gac_antirepeat_pass, :66-91, :115-116) and the survivors and
 * the '#' lines are written in input order (:128, :162-165). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_seqtool.h"
#include "gachain.h"

static const gt_spec k_opts[] = {
    {"minScore", GT_INT},
    {"noCheckScore", GT_INT},
    {NULL, 0},
};

static void usage(void) {
    gt_abort(
        "chainAntiRepeat - Get rid of chains that are primarily the results of repeats and degenerate DNA\n"
        "usage:\n"
        "   chainAntiRepeat tNibDir qNibDir inChain outChain\n"
        "options:\n"
        "   -minScore=N - minimum score (after repeat stuff) to pass\n"
        "   -noCheckScore=N - score that will pass without checks (speed tweak)\n");
}

/* the per-chain aborts, in the reference's order: the target is fetched
 * first (:141-149) */
static void check_chain(const gs_env *k, int64_t i, int32_t ts, int32_t qs) {
    const gt_chains *c = k->c;
    const char *tn = c->tnames.names[c->tname[i]], *qn = c->qnames.names[c->qname[i]];
    if (ts < 0)
        gt_abort("%s is not in %s", tn, k->t2bit);
    gs_check_frag(tn, c->tstart[i], c->tend[i], gac_genome_seq_size(k->ctx, GAC_T, ts));
    if (qs < 0)
        gt_abort("%s is not in %s", qn, k->q2bit);
    const int32_t S = gac_genome_seq_size(k->ctx, GAC_Q, qs);
    /* a '-' query is fetched at [qSize - qEnd, qSize - qStart) with the
     * header's qSize (:144-149) */
    if (c->qstrand[i])
        gs_check_frag(qn, (int64_t)c->qsize[i] - c->qend[i], (int64_t)c->qsize[i] - c->qstart[i], S);
    else
        gs_check_frag(qn, c->qstart[i], c->qend[i], S);
}

/* output items in input order: a '#' line (chain < 0: meta index in k) or a
 * surviving chain */
typedef struct out_item {
    int64_t chain, k;
} out_item;

typedef struct out_ctx {
    const gt_chains *c;
    const out_item *it;
    const int32_t *id;
} out_ctx;

static void write_one(FILE *f, int64_t i, void *arg) {
    const out_ctx *o = arg;
    const out_item *it = &o->it[i];
    if (it->chain < 0)
        fprintf(f, "%s\n", o->c->meta[it->k]);
    else
        gt_write_chain(f, o->c, it->chain, o->c->score[it->chain], o->id[it->chain]);
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options(&argc, argv, k_opts);
    if (argc != 5)
        usage();
    const int min_score = gt_opt_int("minScore", 5000);
    const int no_check = gt_opt_int("noCheckScore", 200000);
    const char *t2bit = argv[1], *q2bit = argv[2];
    gs_check_twobits(t2bit, q2bit, "2bit file or nib directory");

    /* device open + genome upload (with the soft-mask plane) beside the parse */
    gt_device dev;
    gt_device_on_open(gs_softmask_both);
    gt_stage("options + setup");
    gt_device_start(&dev, t2bit, q2bit, NULL, NULL);

    /* chainRead gives an id-less header chainIdNext when it is read, and
     * chainWrite gives an id of 0 the next one when it is written
     * (chain.c:180-204): both in stream order, replayed below */
    gt_defer_chain_ids(1);
    gt_chains c;
    gt_read_chains(argv[3], &c, -HUGE_VAL, 1);
    gt_stage("read chains");
    FILE *out = gt_must_open(argv[4], "w");
    gac_ctx *ctx = gt_device_join(&dev);
    gt_stage("device open + 2bit genomes (rest)");

    /* the checked chains (:138, double against int), as a set of their own */
    uint8_t *keep = gs_alloc((size_t)c.n);
    for (int64_t i = 0; i < c.n; ++i)
        keep[i] = c.score[i] < no_check;
    int32_t *tmap = gt_seq_map(ctx, GAC_T, &c.tnames), *qmap = gt_seq_map(ctx, GAC_Q, &c.qnames);
    const gs_env env = {&c, ctx, t2bit, q2bit};
    gs_subset s;
    gs_subset_build(&env, keep, c.tname, c.qname, tmap, qmap, check_chain, 0, &s);
    free(tmap);
    free(qmap);
    free(keep);
    /* the engine flips a '-' query with the .2bit size S, the reference with
     * the header's qSize: the same bases lie at strand coordinates shifted by
     * S - qSize */
    for (int64_t k = 0; k < s.nc; ++k) {
        const int64_t i = s.sel[k];
        const int64_t shift = (int64_t)gac_genome_seq_size(ctx, GAC_Q, s.qseq[k]) - c.qsize[i];
        if (c.qstrand[i] && shift)
            for (int64_t b = s.boff[k]; b < s.boff[k + 1]; ++b)
                s.bq[b] = (int32_t)(s.bq[b] + shift);
    }
    const int64_t nc = s.nc, *sel = s.sel;
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &s.d, &cs));
    gt_stage("chains to HBM");
    int64_t *match = malloc((size_t)(nc ? nc : 1) * 4 * 8), *rep = malloc((size_t)(nc ? nc : 1) * 8);
    int64_t *total = malloc((size_t)(nc ? nc : 1) * 8);
    gt_check(gac_chain_composition(ctx, cs, match, rep, total));
    gt_stage("GPU composition");
    gt_device_close_async(&dev, ctx, cs); /* overlaps writing the output */

    uint8_t *pass = malloc((size_t)(c.n ? c.n : 1));
    memset(pass, 1, (size_t)(c.n ? c.n : 1));
    for (int64_t j = 0; j < nc; ++j)
        pass[sel[j]] = (uint8_t)gac_antirepeat_pass(c.score[sel[j]], match + 4 * j, rep[j], total[j],
                                                    min_score);
    /* items and ids in stream order */
    out_item *it = malloc((size_t)(c.n + c.n_meta + 1) * sizeof(out_item));
    int32_t *id = malloc((size_t)(c.n ? c.n : 1) * 4);
    int64_t ni = 0;
    int32_t m = 0;
    for (int64_t i = 0; i <= c.n; ++i) {
        for (; m < c.n_meta && c.meta_at[m] <= i; ++m)
            it[ni++] = (out_item){-1, m};
        if (i == c.n)
            break;
        id[i] = c.id[i] == INT32_MIN ? gt_next_chain_id() : c.id[i];
        if (!pass[i])
            continue;
        if (id[i] == 0)
            id[i] = gt_next_chain_id();
        it[ni++] = (out_item){i, 0};
    }
    out_ctx oc = {&c, it, id};
    gt_par_write(out, ni, write_one, &oc);
    gt_careful_close(out, argv[4]);
    gt_stage("write output");
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
