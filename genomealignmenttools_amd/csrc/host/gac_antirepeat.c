/* gac_antirepeat.c -- host half of chainAntiRepeat: the pass/drop decision
 * from a chain's match composition (no device needed), and the soft-mask
 * runs of a .2bit sequence as the host reader keeps them. */
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

/* degeneracyFilter then repeatFilter of
 * kent/src/hg/mouseStuff/chainAntiRepeat/chainAntiRepeat.c:40-117, in the
 * reference's operation order (doubles; the build has -ffp-contract=off).
 * match[] by .2bit code T, C, A, G = ntVal 0..3 (counts[0..3], :61-66). */
int gac_antirepeat_pass(double score, const int64_t match[4], int64_t rep, int64_t total,
                        int min_score) {
    const int64_t *counts = match;
    const double okBest2 = 0.80;
    const double maxOverOk = 1.0 - okBest2;
    const int64_t totalMatches = counts[0] + counts[1] + counts[2] + counts[3];
    int64_t best2 = counts[0] + counts[1], sum2;
    sum2 = counts[0] + counts[2];
    if (best2 < sum2) best2 = sum2;
    sum2 = counts[0] + counts[3];
    if (best2 < sum2) best2 = sum2;
    sum2 = counts[1] + counts[2];
    if (best2 < sum2) best2 = sum2;
    sum2 = counts[1] + counts[3];
    if (best2 < sum2) best2 = sum2;
    sum2 = counts[2] + counts[3];
    if (best2 < sum2) best2 = sum2;
    /* totalMatches == 0: NaN, neither comparison below holds -> dropped */
    const double observedBest2 = (double)best2 / (double)totalMatches;
    const double overOk = observedBest2 - okBest2;
    if (!(overOk <= 0)) {
        const double adjustFactor = 1.01 - overOk / maxOverOk;
        const double adjustedScore = score * adjustFactor;
        if (!(adjustedScore >= min_score))
            return 0;
    }
    /* repeatFilter (:94-117): int operands promoted as in the reference */
    const double adjusted = (score * 2.0 * (double)(total - rep) / (double)total);
    return adjusted >= min_score ? 1 : 0;
}

int gac_twobit_mask_runs(const char *path, const char *name, int32_t cap, int32_t *starts,
                         int32_t *sizes, int32_t *count) {
    gac_clear_error();
    if (!path || !name || !count || cap < 0 || (cap > 0 && (!starts || !sizes)))
        return gac_fail(GAC_E_ARG, "gac_twobit_mask_runs: bad argument");
    gac_twobit tb;
    int rc = gac_twobit_open(path, &tb);
    if (rc != GAC_OK)
        return rc;
    rc = gac_fail(GAC_E_ARG, "%s is not in %s", name, path);
    for (uint32_t i = 0; i < tb.seq_count; ++i) {
        const gac_twobit_seq *s = &tb.seqs[i];
        if (strcmp(s->name, name) != 0)
            continue;
        *count = (int32_t)s->m_count;
        for (uint32_t k = 0; k < s->m_count && (int32_t)k < cap; ++k) {
            starts[k] = (int32_t)gac_twobit_u32(&tb, s->m_starts_raw + 4 * k);
            sizes[k] = (int32_t)gac_twobit_u32(&tb, s->m_sizes_raw + 4 * k);
        }
        gac_clear_error();
        rc = GAC_OK;
        break;
    }
    gac_twobit_close(&tb);
    return rc;
}
