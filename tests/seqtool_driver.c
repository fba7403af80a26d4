/* Test driver for tools/lib/gac_seqtool.c (tests/test_seqtool_cpu.py): the
 * batch planner and the chain subset builder, without a device.
 *
 *   seqtool_driver plan BUDGET < sym values
 *   seqtool_driver subset IN.CHAIN MIN_SCORE CHECK_GAPS [MISSING_TNAME]
 *
 * subset keeps the chains scoring at least MIN_SCORE, with identity name maps
 * (sequence index = index in the file's name table); MISSING_TNAME is absent
 * from the target map, which the per-chain callback aborts on as the tools do. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_seqtool.h"

static void put64(const char *tag, const int64_t *v, int64_t n) {
    printf("%s", tag);
    for (int64_t i = 0; i < n; ++i)
        printf(" %lld", (long long)v[i]);
    printf("\n");
}

static void put32(const char *tag, const int32_t *v, int64_t n) {
    printf("%s", tag);
    for (int64_t i = 0; i < n; ++i)
        printf(" %d", v[i]);
    printf("\n");
}

static int plan(int64_t budget) {
    int64_t n = 0, cap = 64, *sym = gs_alloc((size_t)cap * 8);
    long long v;
    while (scanf("%lld", &v) == 1) {
        if (n == cap && !(sym = realloc(sym, (size_t)(cap *= 2) * 8)))
            gt_abort("Out of memory");
        sym[n++] = v;
    }
    gs_axt_plan P;
    gs_axt_plan_make(sym, n, budget, &P);
    printf("nbatch %lld\ncap %lld\njobs %lld %lld\n", (long long)P.nbatch, (long long)P.cap,
           (long long)P.job_bytes[0], (long long)P.job_bytes[1]);
    put64("lo", P.lo, P.nbatch + 1);
    put64("bytes", P.bytes, P.nbatch);
    put64("off", P.off, n);
    return 0;
}

static void check_chain(const gs_env *e, int64_t i, int32_t ts, int32_t qs) {
    if (ts < 0)
        gt_abort("%s is not in %s", e->c->tnames.names[e->c->tname[i]], e->t2bit);
    if (qs < 0)
        gt_abort("%s is not in %s", e->c->qnames.names[e->c->qname[i]], e->q2bit);
}

static int32_t *identity(const gt_names *t, const char *missing) {
    int32_t *map = gs_alloc((size_t)t->n * 4);
    for (int32_t i = 0; i < t->n; ++i)
        map[i] = missing && !strcmp(t->names[i], missing) ? -1 : i;
    return map;
}

static int subset(const char *path, double min_score, int check_gaps, const char *missing) {
    gt_chains c;
    gt_read_chains(path, &c, -HUGE_VAL, 0);
    uint8_t *keep = gs_alloc((size_t)c.n);
    for (int64_t i = 0; i < c.n; ++i)
        keep[i] = c.score[i] >= min_score;
    int32_t *tmap = identity(&c.tnames, missing), *qmap = identity(&c.qnames, NULL);
    const gs_env env = {&c, NULL, "t.2bit", "q.2bit"};
    gs_subset s;
    gs_subset_build(&env, keep, c.tname, c.qname, tmap, qmap, check_chain, check_gaps, &s);
    const gac_chainset_desc *d = &s.d;
    printf("desc %d\n", d->n_chains == s.nc && d->n_blocks == s.nb && d->t_seq == s.tseq &&
                            d->q_seq == s.qseq && d->q_strand == s.strand && d->blk_off == s.boff &&
                            d->blk_t == s.bt && d->blk_q == s.bq && d->blk_size == s.bs);
    put64("sel", s.sel, s.nc);
    put64("boff", s.boff, s.nc + 1);
    put32("tseq", s.tseq, s.nc);
    put32("qseq", s.qseq, s.nc);
    printf("strand");
    for (int64_t k = 0; k < s.nc; ++k)
        printf(" %d", s.strand[k]);
    printf("\n");
    put32("bt", s.bt, s.nb);
    put32("bq", s.bq, s.nb);
    put32("bs", s.bs, s.nb);
    return 0;
}

int main(int argc, char *argv[]) {
    if (argc == 3 && !strcmp(argv[1], "plan"))
        return plan(atoll(argv[2]));
    if ((argc == 5 || argc == 6) && !strcmp(argv[1], "subset"))
        return subset(argv[2], atof(argv[3]), atoi(argv[4]), argc == 6 ? argv[5] : NULL);
    fprintf(stderr, "usage: seqtool_driver plan BUDGET | subset IN.CHAIN MIN_SCORE CHECK_GAPS [NAME]\n");
    return 2;
}
