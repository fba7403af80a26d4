/* chainToPslBasic -- convert chains to PSL without reading sequence (drop-in
 * for kent/src/hg/mouseStuff/chainToPslBasic/chainToPslBasic.c; host only).
 *
 * Same command line and output bytes: per chain one pslTabOut line
 * (kent/src/lib/psl.c:175-254) with match = the sum of the block sizes,
 * misMatch = repMatch = nCount = 0, and inserts counted where the next block
 * starts after the previous one ends (pslAddBlock, :28-50).  optionInit with
 * an empty spec (:91): an unknown option aborts.  '#' lines are skipped.  The
 * file is parsed on all threads (gt_read_chains) and the text formatted on
 * all threads (gt_par_write), with the line writer chainToPsl uses. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "gac_pslout.h"
#include "gac_tool.h"

static const gt_spec k_opts[] = {
    {NULL, 0},
};

static void usage(void) {
    gt_abort("chainToPslBasic - Basic conversion chain file to psl format\n"
             "usage:\n"
             "   chainToPsl in.chain out.psl\n"
             "If you need match and mismatch stats updated, pipe output through pslRecalcMatch\n");
}

static void write_one(FILE *f, int64_t i, void *arg) {
    const gt_chains *c = arg;
    uint32_t match = 0; /* unsigned match (psl.h) */
    for (int64_t b = c->blk_off[i]; b < c->blk_off[i + 1]; ++b)
        match += (uint32_t)c->bs[b];
    const int64_t counts[4] = {match, 0, 0, 0};
    gt_write_psl(f, c, i, counts, 1);
}

int main(int argc, char *argv[]) {
    gt_options(&argc, argv, k_opts);
    if (argc != 3)
        usage();
    gt_chains c;
    gt_read_chains(argv[1], &c, -HUGE_VAL, 0);
    FILE *out = gt_must_open(argv[2], "w");
    gt_par_write(out, c.n, write_one, &c);
    gt_careful_close(out, argv[2]);
    gt_exit_ok();
}
