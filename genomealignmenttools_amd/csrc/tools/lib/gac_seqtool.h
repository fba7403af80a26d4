/* gac_seqtool.h -- the front end shared by the tools on sequence-backed chains
 * (scoreChain, chainAntiRepeat, chainToAxt, netToAxt, chainToPsl; DESIGN.md
 * §7.10).  gac_seqtool.c is host only; gac_seqtool_dev.c holds what calls
 * device-only entry points and is left out of the CPU stand-in builds. */
#ifndef GAC_SEQTOOL_H
#define GAC_SEQTOOL_H

#include "gac_tool.h"

/* Both files exist (the target first), then both are .2bit files; else the
 * tools' aborts.  noun: "2bit file or nib directory", or chainToPsl's "file". */
void gs_check_twobits(const char *t2bit, const char *q2bit, const char *noun);
/* for gt_device_on_open: the soft-mask plane of both sides / of the target */
int gs_softmask_both(gac_ctx *ctx);
int gs_softmask_target(gac_ctx *ctx);
/* the range check of twoBitReadSeqFragExt (kent/src/lib/twoBit.c:744-751) for
 * the fragment nibTwoCacheSeqPartExt asks for (nibTwo.c:74-77) */
void gs_check_frag(const char *name, int64_t start, int64_t end, int32_t seq_size);
void *gs_alloc(size_t n); /* malloc (of at least one byte) or abort */
size_t *gs_name_lens(const gt_names *t); /* strlen of every name */

/* ---- the kept chains as a set of their own: chain k is chain sel[k] of the
 * file, with its blocks (a tool transforms bt/bq/bs in place afterwards) ---- */
typedef struct gs_subset {
    int64_t nc, nb, *sel, *boff; /* sel: nc, boff: nc + 1 */
    int32_t *tseq, *qseq, *bt, *bq, *bs;
    uint8_t *strand;
    gac_chainset_desc d;
} gs_subset;
typedef struct gs_env { /* what a tool's per-chain checks read */
    const gt_chains *c;
    gac_ctx *ctx;
    const char *t2bit, *q2bit;
} gs_env;
/* A tool's aborts for kept chain i, in that tool's order: a name the .2bit
 * lacks (tseq or qseq < 0), fragment checks.  It runs before the chain's blocks
 * are copied, so of a file's defects the first in file order wins. */
typedef void (*gs_chain_check)(const gs_env *e, int64_t i, int32_t tseq, int32_t qseq);
/* keep[i] != 0: chain i is kept.  tname / qname: per chain, the name index on
 * the set's target / query side (c's own, or swapped for netToAxt -qChain)
 * into the tables tmap / qmap come from (gt_seq_map).  check_gaps: "chain %d:
 * blocks overlap (negative gap before block %lld)" is an abort. */
void gs_subset_build(const gs_env *e, const uint8_t *keep, const int32_t *tname,
                     const int32_t *qname, const int32_t *tmap, const int32_t *qmap,
                     gs_chain_check check, int check_gaps, gs_subset *s);

/* ---- axt text in batches (chainToAxt, netToAxt) ----
 * Piece p takes 2 * sym[p] + 3 bytes.  Batch k, pieces [lo[k], lo[k + 1]) and
 * bytes[k] of text, takes pieces while they fit the budget (an exact fit does)
 * and at least one; off[p] is the piece's offset in its batch's text; cap =
 * max(budget, largest piece).  job_bytes: what the two render jobs are opened
 * with (0: not opened): bytes[0] when that is all there is, else cap. */
typedef struct gs_axt_plan {
    int64_t budget, cap, nbatch, *lo, *bytes, *off, job_bytes[2];
} gs_axt_plan;
/* GAC_AXT_BUDGET (bytes of text per batch) when it is positive, else 64 MiB */
int64_t gs_axt_budget(void);
void gs_axt_plan_make(const int64_t *sym, int64_t n, int64_t budget, gs_axt_plan *P);

/* The batches through two render jobs used in turn: open plans them and
 * submits batch 0; next submits batch k + 1, waits for batch k and hands out
 * its pieces [*lo, *hi) and their text, or returns 0 after the last.  The
 * caller writes the batch between two calls: those seconds are t_write, the
 * submits' t_submit, the waits' t_wait.  clip: the _clip entry points. */
typedef struct gs_axt_run {
    gs_axt_plan plan;
    const gac_chainset *cs;
    const gac_window *pc;
    int clip;
    gac_axt_job *job[2];
    int64_t k; /* the batch the next call hands out */
    double t_submit, t_wait, t_write, t0;
} gs_axt_run;
void gs_axt_open(gs_axt_run *R, gac_ctx *ctx, const gac_chainset *cs, const gac_window *pc,
                 const int64_t *sym, int64_t n, int clip);
int gs_axt_next(gs_axt_run *R, int64_t *lo, int64_t *hi, const char **text);
void gs_axt_close(gs_axt_run *R);

/* axtWrite's header line (kent/src/lib/axt.c:101-114), "%d %s %d %d %s %d %d
 * %c %d\n", of piece w (record p) of set s; returns its length.  (56 M lines on
 * a whole genome: printf's format parsing was most of the tool's time.)  The
 * query span follows the clip of t_start / t_end (chain.c:513-522): for a piece
 * of gac_axt_split, whose span is its blocks', that is the blocks' span. */
enum { GS_AXT_HEAD = 2 * 1024 };
static inline size_t gs_axt_head(char *head, int64_t p, const gac_window *w, const gs_subset *s,
                                 const char *tn, size_t tlen, const char *qn, size_t qlen,
                                 int32_t score) {
    if (tlen + qlen + 128 > GS_AXT_HEAD)
        gt_abort("sequence names too long for an axt header line");
    const int64_t b0 = s->boff[w->chain] + w->first_block, b1 = b0 + w->n_blocks - 1;
    const int64_t qs = (int64_t)s->bq[b0] + (w->t_start - s->bt[b0]);
    const int64_t qe = (int64_t)s->bq[b1] - ((int64_t)s->bt[b1] - w->t_end);
    char *h = gt_put_int(head, p);
    h = gt_put_str(h, tn, tlen);
    h = gt_put_int(h, (int64_t)w->t_start + 1);
    h = gt_put_int(h, w->t_end);
    h = gt_put_str(h, qn, qlen);
    h = gt_put_int(h, qs + 1);
    h = gt_put_int(h, qe);
    *h++ = s->strand[w->chain] ? '-' : '+';
    *h++ = ' ';
    h = gt_put_int(h, score);
    h[-1] = '\n';
    return (size_t)(h - head);
}
#endif
