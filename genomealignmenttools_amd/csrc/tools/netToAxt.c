/* netToAxt -- the fills of a net back to alignment text, on an MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/netToAxt/netToAxt.c
 * (+ chainSubsetOnT / chainSwap of kent/src/lib/chain.c, chainToAxt() of
 * kent/src/lib/chainToAxt.c, axtWrite / axtScoreSym of kent/src/lib/axt.c):
 * same command line, options and output.
 *
 * The host parses the net and lists the sub-chain ranges (chain, tStart, tEnd)
 * in the reference's order (rConvert / convertFill / splitWrite, :107-169);
 * it never walks a chain's blocks for them.  The chains the nets use are
 * uploaded (swapped first with -qChain, chain.c:348-390), one device call
 * (gac_axt_cut) turns the ranges into clipped pieces, one (gac_axt_measure_clip)
 * gives every piece its score and column count, and the pieces are rendered in
 * batches of at most gs_axt_budget() bytes of text (default 64 MiB) by two
 * render jobs used in turn (gs_axt_run, lib/gac_seqtool.h), as in chainToAxt.
 *
 * '#' lines of the net are copied to the output where the reference's reader
 * emits them (lineFileSetMetaDataOutput, :204): chainNetRead reads on to the
 * next "net" line, so every '#' line between net k's "net" line and the next
 * one (and, for the first net, before it) precedes net k's records.
 *
 * A '-' query is flipped inside the .2bit sequence (:92-97), which is what the
 * engine does; -qChain's swap reverses with the chain header's sizes. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_netfile.h"
#include "gac_seqtool.h"
#include "gachain.h"

static const gt_spec k_opts[] = {
    {"qChain", GT_BOOL}, {"maxGap", GT_INT}, {"gapOut", GT_STRING}, {"noSplit", GT_BOOL}, {NULL, 0},
};

static void usage(int max_gap) {
    gt_abort("netToAxt - Convert net (and chain) to axt.\n"
             "usage:\n"
             "   netToAxt in.net in.chain target.2bit query.2bit out.axt\n"
             "note:\n"
             "   directories full of .nib files (an older format)\n"
             "   may also be used in place of target.2bit and query.2bit.\n"
             "options:\n"
             "   -qChain - net is with respect to the q side of chains.\n"
             "   -maxGap=N - maximum size of gap before breaking. Default %d\n"
             "   -gapOut=gap.tab - Output gap sizes to file\n"
             "   -noSplit - Don't split chain when there is an insertion of another chain\n",
             max_gap);
}

/* the per-chain abort: a name the .2bit lacks (-qChain: the sides swapped) */
typedef struct net_env {
    gs_env e;
    int q_chain;
} net_env;

static void check_chain(const gs_env *e, int64_t i, int32_t ts, int32_t qs) {
    const gt_chains *c = e->c;
    const char *tn = c->tnames.names[c->tname[i]], *qn = c->qnames.names[c->qname[i]];
    const int swap = ((const net_env *)e)->q_chain;
    if (ts < 0)
        gt_abort("%s is not in %s", swap ? qn : tn, e->t2bit);
    if (qs < 0)
        gt_abort("%s is not in %s", swap ? tn : qn, e->q2bit);
}

/* ---- chain ids ---- */
typedef struct id_ix {
    int32_t id;
    int64_t ix;
} id_ix;

static int cmp_id(const void *a, const void *b) {
    const id_ix *x = a, *y = b;
    return x->id < y->id ? -1 : x->id > y->id ? 1 : x->ix < y->ix ? -1 : x->ix > y->ix;
}

static int64_t find_id(const id_ix *tab, int64_t n, int32_t id) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tab[mid].id < id)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && tab[lo].id == id ? tab[lo].ix : -1;
}

/* ---- ranges ---- */
typedef struct ranges {
    gac_range *r; /* chain: index into the chain file, then into the uploaded set */
    int64_t n, cap;
} ranges;

static void push_range(ranges *R, int64_t chain, int32_t s, int32_t e) {
    if (R->n == R->cap) {
        R->cap = R->cap ? R->cap * 2 : 1024;
        R->r = realloc(R->r, (size_t)R->cap * sizeof(*R->r));
        if (!R->r)
            gt_abort("Out of memory");
    }
    R->r[R->n++] = (gac_range){(int32_t)chain, s, e};
}

typedef struct lister {
    const gt_netset *ns;
    const id_ix *ids;
    int64_t n_ids;
    int split;
    ranges *R;
} lister;

/* rConvert (:154-169): a fill's own ranges (convertFill / splitWrite,
 * :119-152), then its children's */
static void list_fills(const lister *L, int32_t f) {
    for (; f >= 0; f = L->ns->fills[f].next) {
        const gt_fill *fill = &L->ns->fills[f];
        if (fill->chain_id) {
            const int64_t c = find_id(L->ids, L->n_ids, fill->chain_id);
            if (c < 0) /* chainLookup -> hashMustFindVal of the id in hex */
                gt_abort("hashMustFindVal: '%x' not found", (unsigned)fill->chain_id);
            int32_t s = fill->tstart;
            if (L->split) /* nextGapWithInsert: a child gap that has children of its own */
                for (int32_t g = fill->child; g >= 0; g = L->ns->fills[g].next) {
                    const gt_fill *gap = &L->ns->fills[g];
                    if (gap->child < 0)
                        continue;
                    push_range(L->R, c, s, gap->tstart);
                    s = gap->tstart + gap->tsize;
                }
            push_range(L->R, c, s, fill->tstart + fill->tsize);
        }
        if (fill->child >= 0)
            list_fills(L, fill->child);
    }
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options(&argc, argv, k_opts);
    const int q_chain = gt_opt_exists("qChain");
    const int max_gap = gt_opt_int("maxGap", 100);
    const int split = !gt_opt_exists("noSplit");
    const char *gap_name = gt_opt_str("gapOut", NULL);
    if (argc != 6)
        usage(max_gap);
    const char *t2bit = argv[3], *q2bit = argv[4];
    gs_check_twobits(t2bit, q2bit, "2bit file or nib directory");

    gt_device dev;
    gt_device_on_open(gs_softmask_both);
    gt_stage("options + setup");
    gt_device_start(&dev, t2bit, q2bit, NULL, NULL);

    /* the net (findUsedIds reads all of it first, :192), its '#' lines by net */
    gt_lines nl;
    gt_lines_read(argv[1], &nl);
    gt_netset ns;
    gt_net_parse(&nl, argv[1], &ns);
    int64_t n_meta = 0;
    for (int64_t i = 0; i < nl.n; ++i)
        n_meta += nl.line[i][0] == '#';
    const char **meta = gs_alloc((size_t)n_meta * sizeof(*meta));
    /* meta[meta_off[k] .. meta_off[k + 1]): the lines the read of net k emits */
    int64_t *meta_off = gs_alloc((size_t)(ns.n + 2) * 8);
    {
        int64_t k = 0, m = 0;
        int32_t seen = 0;
        meta_off[0] = 0;
        for (int64_t i = 0; i < nl.n; ++i) {
            if (strncmp(nl.line[i], "net ", 4) == 0 && ++seen > 1)
                meta_off[++k] = m;
            if (nl.line[i][0] == '#')
                meta[m++] = nl.line[i];
        }
        while (k < ns.n)
            meta_off[++k] = m;
    }
    gt_stage("read net");

    gt_chains c;
    gt_read_chains(argv[2], &c, -HUGE_VAL, 0);
    /* chainReadUsedSwap with bits NULL (:205, chain.c:421-429): every chain goes
     * into the hash, so a duplicate id anywhere aborts */
    id_ix *ids = gs_alloc((size_t)c.n * sizeof(*ids));
    for (int64_t i = 0; i < c.n; ++i)
        ids[i] = (id_ix){c.id[i], i};
    qsort(ids, (size_t)c.n, sizeof(*ids), cmp_id);
    for (int64_t i = 1; i < c.n; ++i)
        if (ids[i].id == ids[i - 1].id)
            gt_abort("Duplicate chain %d (chains %lld and %lld) of %s", ids[i].id,
                     (long long)ids[i - 1].ix + 1, (long long)ids[i].ix + 1, argv[2]);
    gt_stage("read chains");
    FILE *out = gt_must_open(argv[5], "w");
    setvbuf(out, NULL, _IOFBF, 1 << 20);
    FILE *gap_out = gap_name ? gt_must_open(gap_name, "w") : NULL;
    gac_ctx *ctx = gt_device_join(&dev);
    gt_stage("device open + 2bit genomes (rest)");

    /* the ranges, net by net; net_r0[k]: the first range of net k */
    ranges R = {NULL, 0, 0};
    int64_t *net_r0 = gs_alloc((size_t)(ns.n + 1) * 8);
    lister L = {&ns, ids, c.n, split, &R};
    for (int32_t k = 0; k < ns.n; ++k) {
        const gt_net1 *net = &ns.nets[k];
        net_r0[k] = R.n;
        gt_verbose(1, "Processing %s\n", net->name);
        const int32_t ts = gac_genome_seq_index(ctx, GAC_T, net->name);
        if (ts < 0)
            gt_abort("%s is not in %s", net->name, t2bit);
        if (gac_genome_seq_size(ctx, GAC_T, ts) != net->size)
            gt_abort("Size mismatch on %s.  Net/nib out of sync or possibly nib dirs swapped?",
                     net->name);
        list_fills(&L, net->first);
        /* the reference takes the target text from the net's sequence whatever
         * the chain says: a chain of another sequence is refused here */
        for (int64_t r = net_r0[k]; r < R.n; ++r) {
            const int64_t i = R.r[r].chain;
            const char *tn = q_chain ? c.qnames.names[c.qname[i]] : c.tnames.names[c.tname[i]];
            if (strcmp(tn, net->name) != 0)
                gt_abort("chain %d is on %s, but a fill of net %s names it", c.id[i], tn, net->name);
        }
    }
    net_r0[ns.n] = R.n;

    /* the chains the nets use, as a set of their own (swapped with -qChain) */
    uint8_t *keep = gs_alloc((size_t)c.n);
    memset(keep, 0, (size_t)c.n);
    for (int64_t r = 0; r < R.n; ++r)
        keep[R.r[r].chain] = 1;
    /* after the swap the chain's target is its file's query and the other way round */
    const gt_names *tnames = q_chain ? &c.qnames : &c.tnames, *qnames = q_chain ? &c.tnames : &c.qnames;
    const int32_t *tname = q_chain ? c.qname : c.tname, *qname = q_chain ? c.tname : c.qname;
    int32_t *tmap = gt_seq_map(ctx, GAC_T, tnames), *qmap = gt_seq_map(ctx, GAC_Q, qnames);
    const net_env env = {{&c, ctx, t2bit, q2bit}, q_chain};
    gs_subset s;
    gs_subset_build(&env.e, keep, tname, qname, tmap, qmap, check_chain, 1, &s);
    free(tmap);
    free(qmap);
    free(keep);
    int64_t *slot = gs_alloc((size_t)c.n * 8); /* the set's chain of a chain of the file */
    for (int64_t k = 0; k < s.nc; ++k)
        slot[s.sel[k]] = k;
    for (int64_t r = 0; r < R.n; ++r)
        R.r[r].chain = (int32_t)slot[R.r[r].chain];
    free(slot);
    /* chainSwap (chain.c:348-390): the sides change places; for '-' both are
     * reversed with the header's sizes and the block order is reversed */
    for (int64_t k = 0; q_chain && k < s.nc; ++k) {
        const int64_t i = s.sel[k], b = s.boff[k], n = s.boff[k + 1] - b, j0 = c.blk_off[i];
        const int rev = c.qstrand[i];
        for (int64_t j = 0; j < n; ++j) {
            const int64_t o = rev ? j0 + n - 1 - j : j0 + j; /* the block that comes here */
            s.bt[b + j] = rev ? c.qsize[i] - (c.bq[o] + c.bs[o]) : c.bq[o];
            s.bq[b + j] = rev ? c.tsize[i] - (c.bt[o] + c.bs[o]) : c.bt[o];
            s.bs[b + j] = c.bs[o];
        }
    }
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &s.d, &cs));
    gt_stage("chains to HBM");

    gac_window *pc = NULL;
    int64_t *first = NULL, np = 0;
    gt_check(gac_axt_cut(ctx, cs, R.r, R.n, max_gap, &pc, &first, &np));
    for (int64_t r = 0; r < R.n; ++r)
        if (first[r] == first[r + 1]) /* writeChainPart (:88-89) */
            gt_abort("null subchain in chain ID %d\n", c.id[s.sel[R.r[r].chain]]);
    gt_stage("GPU cut");
    if (gap_out) { /* writeGaps (:49-59): the inner gaps of every sub-chain; a clip changes none */
        for (int64_t r = 0; r < R.n; ++r) {
            const gac_window *f = &pc[first[r]], *l = &pc[first[r + 1] - 1];
            const int64_t b0 = s.boff[f->chain] + f->first_block;
            const int64_t b1 = s.boff[l->chain] + l->first_block + l->n_blocks;
            for (int64_t j = b0 + 1; j < b1; ++j)
                fprintf(gap_out, "%d\t%d\n", s.bt[j] - (s.bt[j - 1] + s.bs[j - 1]),
                        s.bq[j] - (s.bq[j - 1] + s.bs[j - 1]));
        }
        gt_careful_close(gap_out, gap_name);
        gt_stage("write -gapOut");
    }
    int32_t *score = gs_alloc((size_t)np * 4);
    int64_t *match = gs_alloc((size_t)np * 8), *ali = gs_alloc((size_t)np * 8);
    int64_t *sym = gs_alloc((size_t)np * 8);
    gt_check(gac_axt_measure_clip(ctx, cs, pc, np, score, match, ali, sym));
    gt_stage("GPU measure");

    /* every piece is written */
    gs_axt_run run;
    gs_axt_open(&run, ctx, cs, pc, sym, np, 1);
    gt_verbose(2, "%lld ranges, %lld pieces in %lld batches of at most %lld text bytes\n",
               (long long)R.n, (long long)np, (long long)run.plan.nbatch, (long long)run.plan.budget);
    char head[GS_AXT_HEAD];
    size_t *tlen = gs_name_lens(tnames), *qlen = gs_name_lens(qnames);
    int32_t net = 0; /* the next net whose '#' lines are due: before its first record */
    int64_t lo, hi;
    const char *text;
    while (gs_axt_next(&run, &lo, &hi, &text))
        for (int64_t p = lo; p < hi; ++p) { /* axtWrite (axt.c:101-114) */
            for (; net < ns.n && first[net_r0[net]] <= p; ++net)
                for (int64_t m = meta_off[net]; m < meta_off[net + 1]; ++m)
                    fprintf(out, "%s\n", meta[m]);
            const int64_t i = s.sel[pc[p].chain];
            const int32_t tn = tname[i], qn = qname[i];
            const size_t n = gs_axt_head(head, p, &pc[p], &s, tnames->names[tn], tlen[tn],
                                         qnames->names[qn], qlen[qn], score[p]);
            fwrite(head, 1, n, out);
            fwrite(text + run.plan.off[p], 1, (size_t)(2 * sym[p] + 3), out);
        }
    for (; net < ns.n; ++net) /* nets without a record, and whatever follows the last */
        for (int64_t m = meta_off[net]; m < meta_off[net + 1]; ++m)
            fprintf(out, "%s\n", meta[m]);
    if (!ns.n) /* a net file of comments only */
        for (int64_t m = 0; m < n_meta; ++m)
            fprintf(out, "%s\n", meta[m]);
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[netToAxt] %lld ranges, %lld pieces, %lld batches: submit (checks + enqueue) "
                        "%.3f s, wait for render + copy %.3f s, header lines + fwrite %.3f s\n",
                (long long)R.n, (long long)np, (long long)run.plan.nbatch, run.t_submit, run.t_wait,
                run.t_write);
    gt_stage("render + write output");
    gs_axt_close(&run);
    gt_device_close_async(&dev, ctx, cs); /* overlaps closing the output */
    gt_careful_close(out, argv[5]);
    gac_axt_free(pc);
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
