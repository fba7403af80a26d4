/* gac_seqtool_dev.c -- the part of the sequence tools' front end that calls
 * device-only entry points (gac_seqtool.h): the soft-mask request and the
 * batch iterator over two render jobs.  Not in the CPU stand-in builds. */
#include "gac_seqtool.h"

int gs_softmask_target(gac_ctx *ctx) { return gac_genome_want_softmask(ctx, GAC_T); }

int gs_softmask_both(gac_ctx *ctx) {
    const int rc = gac_genome_want_softmask(ctx, GAC_T);
    return rc != GAC_OK ? rc : gac_genome_want_softmask(ctx, GAC_Q);
}

static void submit(gs_axt_run *R, int64_t k) {
    const gs_axt_plan *P = &R->plan;
    const int64_t lo = P->lo[k];
    gt_check((R->clip ? gac_axt_job_submit_clip : gac_axt_job_submit)(
        R->job[k & 1], R->cs, R->pc + lo, P->lo[k + 1] - lo, P->off + lo, P->bytes[k]));
}

void gs_axt_open(gs_axt_run *R, gac_ctx *ctx, const gac_chainset *cs, const gac_window *pc,
                 const int64_t *sym, int64_t n, int clip) {
    *R = (gs_axt_run){.cs = cs, .pc = pc, .clip = clip};
    gs_axt_plan *P = &R->plan;
    gs_axt_plan_make(sym, n, gs_axt_budget(), P);
    for (int j = 0; j < 2; ++j)
        if (P->job_bytes[j])
            gt_check(gac_axt_job_open(ctx, P->job_bytes[j], &R->job[j]));
    if (P->nbatch)
        submit(R, 0);
}

int gs_axt_next(gs_axt_run *R, int64_t *lo, int64_t *hi, const char **text) {
    const gs_axt_plan *P = &R->plan;
    double t1 = gt_now_s();
    if (R->k) /* the caller wrote batch k - 1 */
        R->t_write += t1 - R->t0;
    R->t0 = t1;
    if (R->k == P->nbatch)
        return 0;
    if (R->k + 1 < P->nbatch) /* the next batch renders while this one is written */
        submit(R, R->k + 1);
    R->t_submit += (t1 = gt_now_s()) - R->t0;
    gt_check(gac_axt_job_wait(R->job[R->k & 1], text, NULL));
    R->t_wait += (R->t0 = gt_now_s()) - t1;
    *lo = P->lo[R->k];
    *hi = P->lo[R->k + 1];
    ++R->k;
    return 1;
}

void gs_axt_close(gs_axt_run *R) {
    gac_axt_job_close(R->job[0]);
    gac_axt_job_close(R->job[1]);
}
