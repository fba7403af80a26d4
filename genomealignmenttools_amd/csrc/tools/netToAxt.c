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
 * batches of at most GAC_AXT_BUDGET bytes of text (default 64 MiB) by two
 * render jobs used in turn, as in chainToAxt.
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
#include <time.h>

#include "gac_netfile.h"
#include "gac_tool.h"
#include "gachain.h"
#include "host/gac_host.h"

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

static int want_softmask(gac_ctx *ctx) {
    const int rc = gac_genome_want_softmask(ctx, GAC_T);
    return rc != GAC_OK ? rc : gac_genome_want_softmask(ctx, GAC_Q);
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

static void *must_alloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p)
        gt_abort("Out of memory (%zu bytes)", n);
    return p;
}

static size_t *name_lens(const gt_names *t) {
    size_t *len = must_alloc((size_t)t->n * sizeof(*len));
    for (int32_t i = 0; i < t->n; ++i)
        len[i] = strlen(t->names[i]);
    return len;
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

    /* the net (findUsedIds reads all of it first, :192), its '#' lines by net */
    gt_lines nl;
    gt_lines_read(argv[1], &nl);
    gt_netset ns;
    gt_net_parse(&nl, argv[1], &ns);
    int64_t n_meta = 0;
    for (int64_t i = 0; i < nl.n; ++i)
        n_meta += nl.line[i][0] == '#';
    const char **meta = must_alloc((size_t)n_meta * sizeof(*meta));
    /* meta[meta_off[k] .. meta_off[k + 1]): the lines the read of net k emits */
    int64_t *meta_off = must_alloc((size_t)(ns.n + 2) * 8);
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
    id_ix *ids = must_alloc((size_t)c.n * sizeof(*ids));
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
    int64_t *net_r0 = must_alloc((size_t)(ns.n + 1) * 8);
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
    int64_t *slot = must_alloc((size_t)c.n * 8);
    memset(slot, 0xff, (size_t)c.n * 8);
    int64_t nc = 0, nb = 0;
    for (int64_t r = 0; r < R.n; ++r)
        if (slot[R.r[r].chain] < 0)
            slot[R.r[r].chain] = 0;
    for (int64_t i = 0; i < c.n; ++i)
        if (slot[i] == 0) {
            slot[i] = nc++;
            nb += c.blk_off[i + 1] - c.blk_off[i];
        }
    for (int64_t r = 0; r < R.n; ++r)
        R.r[r].chain = (int32_t)slot[R.r[r].chain];
    int64_t *sel = must_alloc((size_t)nc * 8), *boff = must_alloc((size_t)(nc + 1) * 8);
    int32_t *tseq = must_alloc((size_t)nc * 4), *qseq = must_alloc((size_t)nc * 4);
    uint8_t *strand = must_alloc((size_t)nc);
    int32_t *bt = must_alloc((size_t)nb * 4), *bq = must_alloc((size_t)nb * 4);
    int32_t *bs = must_alloc((size_t)nb * 4);
    /* after the swap the chain's target is its file's query and the other way round */
    const gt_names *tnames = q_chain ? &c.qnames : &c.tnames, *qnames = q_chain ? &c.tnames : &c.qnames;
    const int32_t *tname = q_chain ? c.qname : c.tname, *qname = q_chain ? c.tname : c.qname;
    int32_t *tmap = gt_seq_map(ctx, GAC_T, tnames), *qmap = gt_seq_map(ctx, GAC_Q, qnames);
    int64_t k = 0, b = 0;
    boff[0] = 0;
    for (int64_t i = 0; i < c.n; ++i) {
        if (slot[i] < 0)
            continue;
        if (tmap[tname[i]] < 0)
            gt_abort("%s is not in %s", tnames->names[tname[i]], t2bit);
        if (qmap[qname[i]] < 0)
            gt_abort("%s is not in %s", qnames->names[qname[i]], q2bit);
        sel[k] = i;
        tseq[k] = tmap[tname[i]];
        qseq[k] = qmap[qname[i]];
        strand[k] = c.qstrand[i];
        const int64_t j0 = c.blk_off[i], j1 = c.blk_off[i + 1];
        /* chainSwap (chain.c:348-390): for '-' both sides are reversed with the
         * header's sizes and the block order is reversed */
        const int rev = q_chain && c.qstrand[i];
        const int32_t new_tsize = c.qsize[i], new_qsize = c.tsize[i];
        for (int64_t j = j0; j < j1; ++j, ++b) {
            /* a negative gap is undefined in the reference (assert / negative
             * memset): refused here, before anything runs on it */
            if (j > j0 && (c.bt[j] < c.bt[j - 1] + c.bs[j - 1] || c.bq[j] < c.bq[j - 1] + c.bs[j - 1]))
                gt_abort("chain %d: blocks overlap (negative gap before block %lld)", c.id[i],
                         (long long)(j - j0));
            if (!q_chain) {
                bt[b] = c.bt[j];
                bq[b] = c.bq[j];
                bs[b] = c.bs[j];
            } else if (!rev) {
                bt[b] = c.bq[j];
                bq[b] = c.bt[j];
                bs[b] = c.bs[j];
            } else {
                const int64_t o = j1 - 1 - (j - j0); /* the block that comes here */
                bt[b] = new_tsize - (c.bq[o] + c.bs[o]);
                bq[b] = new_qsize - (c.bt[o] + c.bs[o]);
                bs[b] = c.bs[o];
            }
        }
        boff[++k] = b;
    }
    free(tmap);
    free(qmap);
    gac_chainset_desc d = {nc, tseq, qseq, strand, boff, nb, bt, bq, bs};
    gac_chainset *cs = NULL;
    gt_check(gac_chains_upload(ctx, &d, &cs));
    gt_stage("chains to HBM");

    gac_window *pc = NULL;
    int64_t *first = NULL, np = 0;
    gt_check(gac_axt_cut(ctx, cs, R.r, R.n, max_gap, &pc, &first, &np));
    for (int64_t r = 0; r < R.n; ++r)
        if (first[r] == first[r + 1]) /* writeChainPart (:88-89) */
            gt_abort("null subchain in chain ID %d\n", c.id[sel[R.r[r].chain]]);
    gt_stage("GPU cut");
    if (gap_out) { /* writeGaps (:49-59): the inner gaps of every sub-chain; a clip changes none */
        for (int64_t r = 0; r < R.n; ++r) {
            const gac_window *f = &pc[first[r]], *l = &pc[first[r + 1] - 1];
            const int64_t b0 = boff[f->chain] + f->first_block;
            const int64_t b1 = boff[l->chain] + l->first_block + l->n_blocks;
            for (int64_t j = b0 + 1; j < b1; ++j)
                fprintf(gap_out, "%d\t%d\n", bt[j] - (bt[j - 1] + bs[j - 1]),
                        bq[j] - (bq[j - 1] + bs[j - 1]));
        }
        gt_careful_close(gap_out, gap_name);
        gt_stage("write -gapOut");
    }
    int32_t *score = must_alloc((size_t)np * 4);
    int64_t *match = must_alloc((size_t)np * 8), *ali = must_alloc((size_t)np * 8);
    int64_t *sym = must_alloc((size_t)np * 8);
    gt_check(gac_axt_measure_clip(ctx, cs, pc, np, score, match, ali, sym));
    gt_stage("GPU measure");

    /* batches [lo[k], lo[k + 1]) of at most `budget` bytes; every piece is written */
    int64_t cap = budget;
    for (int64_t p = 0; p < np; ++p)
        if (2 * sym[p] + 3 > cap)
            cap = 2 * sym[p] + 3;
    gac_axt_job *job[2] = {NULL, NULL};
    int64_t *off = must_alloc((size_t)np * 8);
    int64_t nbatch = 0, bcap = 16, *lo = must_alloc(16 * 8), *bytes = must_alloc(16 * 8);
    for (int64_t p = 0; p < np;) {
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
        } while (p < np && used + 2 * sym[p] + 3 <= budget);
        bytes[nbatch++] = used;
    }
    lo[nbatch] = np;
    if (nbatch) {
        gt_check(gac_axt_job_open(ctx, nbatch > 1 || cap > budget ? cap : bytes[0], &job[0]));
        if (nbatch > 1)
            gt_check(gac_axt_job_open(ctx, cap, &job[1]));
        gt_check(gac_axt_job_submit_clip(job[0], cs, pc + lo[0], lo[1] - lo[0], off + lo[0], bytes[0]));
    }
    gt_verbose(2, "%lld ranges, %lld pieces in %lld batches of at most %lld text bytes\n",
               (long long)R.n, (long long)np, (long long)nbatch, (long long)budget);
    char head[2 * 1024];
    size_t *tlen = name_lens(tnames), *qlen = name_lens(qnames);
    double t_submit = 0, t_wait = 0, t_write = 0, t0 = now_s(), t1;
    int32_t net = 0; /* the next net whose '#' lines are due: before its first record */
    for (int64_t kb = 0; kb < nbatch; ++kb) {
        if (kb + 1 < nbatch) /* the next batch renders while this one is written */
            gt_check(gac_axt_job_submit_clip(job[(kb + 1) & 1], cs, pc + lo[kb + 1],
                                             lo[kb + 2] - lo[kb + 1], off + lo[kb + 1], bytes[kb + 1]));
        t_submit += (t1 = now_s()) - t0;
        const char *text = NULL;
        gt_check(gac_axt_job_wait(job[kb & 1], &text, NULL));
        t_wait += (t0 = now_s()) - t1;
        for (int64_t p = lo[kb]; p < lo[kb + 1]; ++p) { /* axtWrite (axt.c:101-114) */
            for (; net < ns.n && first[net_r0[net]] <= p; ++net)
                for (int64_t m = meta_off[net]; m < meta_off[net + 1]; ++m)
                    fprintf(out, "%s\n", meta[m]);
            const int64_t i = sel[pc[p].chain];
            const int64_t b0 = boff[pc[p].chain] + pc[p].first_block, b1 = b0 + pc[p].n_blocks - 1;
            const int32_t tn = tname[i], qn = qname[i];
            if (tlen[tn] + qlen[qn] + 128 > sizeof head)
                gt_abort("sequence names too long for an axt header line");
            /* the query follows the clip (chain.c:513-522) */
            const int64_t qs = (int64_t)bq[b0] + (pc[p].t_start - bt[b0]);
            const int64_t qe = (int64_t)bq[b1] + bs[b1] - ((int64_t)bt[b1] + bs[b1] - pc[p].t_end);
            char *h = gt_put_int(head, p);
            h = gt_put_str(h, tnames->names[tn], tlen[tn]);
            h = gt_put_int(h, (int64_t)pc[p].t_start + 1);
            h = gt_put_int(h, pc[p].t_end);
            h = gt_put_str(h, qnames->names[qn], qlen[qn]);
            h = gt_put_int(h, qs + 1);
            h = gt_put_int(h, qe);
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
    for (; net < ns.n; ++net) /* nets without a record, and whatever follows the last */
        for (int64_t m = meta_off[net]; m < meta_off[net + 1]; ++m)
            fprintf(out, "%s\n", meta[m]);
    if (!ns.n) /* a net file of comments only */
        for (int64_t m = 0; m < n_meta; ++m)
            fprintf(out, "%s\n", meta[m]);
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[netToAxt] %lld ranges, %lld pieces, %lld batches: submit (checks + enqueue) "
                        "%.3f s, wait for render + copy %.3f s, header lines + fwrite %.3f s\n",
                (long long)R.n, (long long)np, (long long)nbatch, t_submit, t_wait, t_write);
    gt_stage("render + write output");
    gac_axt_job_close(job[0]);
    gac_axt_job_close(job[1]);
    gt_device_close_async(&dev, ctx, cs); /* overlaps closing the output */
    gt_careful_close(out, argv[5]);
    gac_axt_free(pc);
    gt_chains_drop_pages(&c);
    gt_device_close_join(&dev);
    gt_stage("device close (rest)");
    gt_exit_ok();
}
