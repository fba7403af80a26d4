/* gac_axtsplit.c -- host half of chainToAxt: where a chain is cut into
 * pieces that become one axt record each (no device needed). */
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

/* chainToAxt's break rule (kent/src/lib/chainToAxt.c:105-121) with maxChain =
 * BIGNUM, as the tool always calls it (kent/src/hg/mouseStuff/chainToAxt/
 * chainToAxt.c:108): a piece ends before block b when the gap to the previous
 * block a is double-sided or longer than max_gap on either side. */
int gac_axt_split(const gac_chainset_desc *d, int32_t max_gap, gac_window **pieces, int64_t *n) {
    gac_clear_error();
    if (!d || !pieces || !n)
        return gac_fail(GAC_E_ARG, "gac_axt_split: NULL argument");
    *pieces = NULL;
    *n = 0;
    if (d->n_chains < 0 || d->n_blocks < 0 || !d->blk_off ||
        (d->n_blocks && (!d->blk_t || !d->blk_q || !d->blk_size)))
        return gac_fail(GAC_E_ARG, "gac_axt_split: incomplete chain set descriptor");
    if (d->n_chains > INT32_MAX)
        return gac_fail(GAC_E_ARG, "gac_axt_split: more than 2^31 - 1 chains");
    int64_t cap = d->n_chains + 16, k = 0;
    gac_window *w = malloc((size_t)cap * sizeof(*w));
    if (!w)
        return gac_fail(GAC_E_ARG, "gac_axt_split: out of memory");
    for (int64_t c = 0; c < d->n_chains; ++c) {
        const int64_t b0 = d->blk_off[c], b1 = d->blk_off[c + 1];
        if (b0 < 0 || b1 < b0 || b1 > d->n_blocks || b1 - b0 > INT32_MAX) {
            free(w);
            return gac_fail(GAC_E_ARG, "chain %lld: bad block offsets", (long long)c);
        }
        int64_t start = b0;
        for (int64_t b = b0; b <= b1; ++b) {
            int cut = b == b1 && b1 > b0;
            if (b > b0 && b < b1) {
                const int64_t dq = (int64_t)d->blk_q[b] - ((int64_t)d->blk_q[b - 1] + d->blk_size[b - 1]);
                const int64_t dt = (int64_t)d->blk_t[b] - ((int64_t)d->blk_t[b - 1] + d->blk_size[b - 1]);
                if (dq < 0 || dt < 0) { /* the reference asserts or memsets a negative length */
                    free(w);
                    return gac_fail(GAC_E_FORMAT,
                                    "chain %lld: negative gap before block %lld (dt %lld, dq %lld)",
                                    (long long)c, (long long)(b - b0), (long long)dt, (long long)dq);
                }
                cut = (dq > 0 && dt > 0) || dt > max_gap || dq > max_gap;
            }
            if (!cut)
                continue;
            if (k == cap) {
                cap += cap / 2;
                gac_window *nw = realloc(w, (size_t)cap * sizeof(*w));
                if (!nw) {
                    free(w);
                    return gac_fail(GAC_E_ARG, "gac_axt_split: out of memory");
                }
                w = nw;
            }
            w[k].chain = (int32_t)c;
            w[k].t_start = d->blk_t[start];
            w[k].t_end = d->blk_t[b - 1] + d->blk_size[b - 1];
            w[k].first_block = (int32_t)(start - b0);
            w[k].n_blocks = (int32_t)(b - start);
            ++k;
            start = b;
        }
    }
    *pieces = w;
    *n = k;
    return GAC_OK;
}

void gac_axt_free(gac_window *pieces) { free(pieces); }
