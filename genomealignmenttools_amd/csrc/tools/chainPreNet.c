/* chainPreNet -- remove chains that don't have a chance of being netted, on an
 * MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c:
 * same command line, options and output; "stdin" and "stdout" are accepted as
 * file names.
 *
 * The reference walks the chains in file order (best score first) with one
 * bitmap per chromosome and side: a chain is written when a base of one of
 * its blocks is still clear, and a written chain sets its blocks, padded by
 * -pad.  Here the file is parsed by all host threads, the whole decision is
 * one call (gac_prenet_keep: per-base first cover on the device, in rounds;
 * DESIGN.md 7.13), and the kept chains and the '#' lines are written in input
 * order by all host threads.  Query coordinates are used as they stand in the
 * file, for '-' chains too, as the reference uses them (:115-116).
 *
 * What the reference checks chain by chain while it reads (:157-168) is
 * checked in the same order after the parse: the score order, then the query
 * and the target name in their sizes files.  A malformed chain anywhere in
 * the file is reported first, and nothing is written before an abort.  A
 * block outside its sequence as the sizes file has it is refused (the
 * reference writes outside its bitmap).
 *
 * One extension: -host takes the decision on the CPU (gac_prenet_keep_host,
 * the reference's own pass) and never opens a device.  Without it the device
 * is opened while the file is read and parsed; no device is an error.
 * -verbose=2 reports the rounds, passes and sequence groups of the device
 * call. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_tool.h"
#include "gachain.h"

static const gt_spec k_opts[] = {
    {"dots", GT_INT}, {"pad", GT_INT}, {"inclHap", GT_BOOL}, {"host", GT_BOOL}, {NULL, 0},
};

static void usage(int pad) {
    gt_abort("chainPreNet - Remove chains that don't have a chance of being netted\n"
             "usage:\n"
             "   chainPreNet in.chain target.sizes query.sizes out.chain\n"
             "options:\n"
             "   -dots=N - output a dot every so often\n"
             "   -pad=N - extra to pad around blocks to decrease trash\n"
             "            (default %d)\n"
             "   -inclHap - include query sequences name in the form *_hap*|*_alt*.\n"
             "              Normally these are excluded from nets as being haplotype\n"
             "              pseudochromosomes\n"
             "   -host - decide on the CPU; no GPU is opened\n",
             pad);
}

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

/* lf->lineIx after chainRead of chain i (0-based): the line of its last block.
 * Only the abort for a file out of order needs it, so the file is read again
 * then; 0 when it cannot be (stdin). */
static long long last_line_of_chain(const char *path, int64_t i) {
    if (strcmp(path, "stdin") == 0)
        return 0;
    size_t len;
    char *buf = gt_slurp(path, &len);
    long long line = 0, found = 0;
    int64_t heads = 0;
    for (char *p = buf, *end = buf + len; p < end && !found;) {
        char *nl = memchr(p, '\n', (size_t)(end - p));
        char *e = nl ? nl : end;
        ++line;
        const char *w = p;
        while (w < e && (*w == ' ' || *w == '\t' || *w == '\r'))
            ++w;
        if (w < e && *w != '#') {
            if (e - w >= 5 && memcmp(w, "chain", 5) == 0) {
                ++heads;
            } else if (heads == i + 1) { /* a block line of chain i: its last has one word */
                const char *q = w;
                while (q < e && *q != ' ' && *q != '\t' && *q != '\r')
                    ++q;
                while (q < e && (*q == ' ' || *q == '\t' || *q == '\r'))
                    ++q;
                if (q == e)
                    found = line;
            }
        }
        p = e + 1;
    }
    free(buf);
    return found;
}

/* output items in input order: a '#' line (chain < 0: meta index in k) or a
 * kept chain */
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
    const int dots = gt_opt_int("dots", 0);
    const int pad = gt_opt_int("pad", 1);
    const int incl_hap = gt_opt_exists("inclHap");
    const int host = gt_opt_exists("host");
    if (argc != 5)
        usage(pad); /* (the reference prints the option's value as the default) */
    gt_device dev;
    if (!host)
        gt_device_start_bare(&dev);
    gt_sizes tsz, qsz;
    gt_read_sizes(argv[2], &tsz);
    gt_read_sizes(argv[3], &qsz);
    gt_stage("options + setup");

    /* chainRead gives an id-less header chainIdNext when it is read, and
     * chainWrite gives an id of 0 the next one when it is written
     * (chain.c:180-204): both in stream order, replayed below */
    gt_defer_chain_ids(1);
    gt_chains c;
    gt_read_chains(argv[1], &c, -HUGE_VAL, 1);
    FILE *out = gt_must_open(argv[4], "w");
    gt_stage("read + parse chains");

    /* the reading loop's checks (:155-168), chain by chain */
    int32_t *tmap = must_alloc((size_t)c.tnames.n * 4), *qmap = must_alloc((size_t)c.qnames.n * 4);
    uint8_t *hap = must_alloc((size_t)c.qnames.n);
    for (int32_t k = 0; k < c.tnames.n; ++k)
        tmap[k] = gt_names_find(&tsz.names, c.tnames.names[k]);
    for (int32_t k = 0; k < c.qnames.n; ++k) {
        const char *name = c.qnames.names[k];
        qmap[k] = gt_names_find(&qsz.names, name);
        hap[k] = strstr(name, "_hap") != NULL || strstr(name, "_alt") != NULL; /* common.c:3711 */
    }
    int32_t *tseq = must_alloc((size_t)c.n * 4), *qseq = must_alloc((size_t)c.n * 4);
    double last_score = 9e99;
    int dot_mod = 0;
    for (int64_t i = 0; i < c.n; ++i) {
        if (dots > 0 && --dot_mod <= 0) {
            dot_mod = dots;
            putc('.', stdout);
            fflush(stdout);
        }
        if (c.score[i] > last_score) {
            const long long line = last_line_of_chain(argv[1], i);
            if (line)
                gt_abort("%s not sorted by score line %lld", argv[1], line);
            gt_abort("%s not sorted by score chain %lld", argv[1], (long long)i + 1);
        }
        last_score = c.score[i];
        if (qmap[c.qname[i]] < 0)
            gt_abort("hashMustFindVal: '%s' not found", c.qnames.names[c.qname[i]]);
        if (tmap[c.tname[i]] < 0)
            gt_abort("hashMustFindVal: '%s' not found", c.tnames.names[c.tname[i]]);
        const int skip = !incl_hap && hap[c.qname[i]];
        tseq[i] = skip ? -1 : tmap[c.tname[i]];
        qseq[i] = skip ? -1 : qmap[c.qname[i]];
    }
    free(tmap);
    free(qmap);
    free(hap);
    gt_stage("order + names");

    uint8_t *keep = must_alloc((size_t)c.n);
    gac_prenet_stats st;
    gac_ctx *ctx = NULL;
    char what[128];
    if (host) {
        gt_check(gac_prenet_keep_host(c.n, c.blk_off, tseq, qseq, c.nb, c.bt, c.bq, c.bs, tsz.names.n,
                                      tsz.size, qsz.names.n, qsz.size, pad, keep, &st));
        snprintf(what, sizeof(what), "keep (host): %lld of %lld", (long long)st.kept, (long long)c.n);
        gt_stage(what);
    } else {
        ctx = gt_device_join(&dev);
        gt_stage("device open (rest)");
        gt_check(gac_prenet_keep(ctx, c.n, c.blk_off, tseq, qseq, c.nb, c.bt, c.bq, c.bs, tsz.names.n,
                                 tsz.size, qsz.names.n, qsz.size, pad, 0, keep, &st));
        snprintf(what, sizeof(what), "keep (GPU): %d rounds, %d passes, groups %d + %d%s", st.rounds,
                 st.passes, st.groups[0], st.groups[1],
                 st.fell_back == GAC_PRENET_FELL_ROUNDS   ? ", finished on the host (rounds)"
                 : st.fell_back == GAC_PRENET_FELL_MEMORY ? ", on the host (memory)"
                                                          : "");
        gt_stage(what);
        gt_device_close_async(&dev, ctx, NULL); /* overlaps the writing */
    }
    free(tseq);
    free(qseq);

    /* items and ids in stream order */
    out_item *it = must_alloc((size_t)(c.n + c.n_meta + 1) * sizeof(out_item));
    int32_t *id = must_alloc((size_t)c.n * 4);
    int64_t ni = 0;
    int32_t m = 0;
    for (int64_t i = 0; i <= c.n; ++i) {
        for (; m < c.n_meta && c.meta_at[m] <= i; ++m)
            it[ni++] = (out_item){-1, m};
        if (i == c.n)
            break;
        id[i] = c.id[i] == INT32_MIN ? gt_next_chain_id() : c.id[i];
        if (!keep[i])
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
    if (!host) {
        gt_device_close_join(&dev);
        gt_stage("device close (rest)");
    }
    gt_exit_ok();
}
