/* gac_axtpairs.c -- gac_axt_pair_counts on the host (no device): per piece
 * the 16 letter-pair counts of its ungapped columns and the columns with an
 * N, read base by base from two .2bit files.  The plain twin the device
 * kernel (k_axt_pairs) is tested against; lavToAxt's host path scores its
 * rows directly. */
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

/* .2bit code (T=0 C=1 A=2 G=3) to the A, C, G, T index of gac_scheme_read */
static const int k_acgt[4] = {3, 1, 0, 2};

/* codes[0, len) = the codes of [start, start + len) of s, 4 under an N run */
static void seq_codes(const gac_twobit *tb, const gac_twobit_seq *s, int64_t start, int64_t len,
                      uint8_t *codes) {
    for (int64_t i = 0; i < len; ++i) {
        const int64_t p = start + i;
        codes[i] = (s->packed[p >> 2] >> (6 - 2 * (p & 3))) & 3;
    }
    for (uint32_t r = 0; r < s->n_count; ++r) {
        const int64_t a = gac_twobit_u32(tb, s->n_starts_raw + 4 * (size_t)r);
        const int64_t b = a + gac_twobit_u32(tb, s->n_sizes_raw + 4 * (size_t)r);
        const int64_t lo = a > start ? a : start, hi = b < start + len ? b : start + len;
        if (lo < hi)
            memset(codes + (lo - start), 4, (size_t)(hi - lo));
    }
}

int gac_axt_pair_counts_twobit(const gac_twobit *t, const gac_twobit *q, const gac_chainset_desc *d,
                               const gac_window *pieces, int64_t n, int64_t *pairs,
                               int64_t *n_cols) {
    if (!t || !q || !d || n < 0 || (n > 0 && (!pieces || !pairs || !n_cols)))
        return gac_fail(GAC_E_ARG, "gac_axt_pair_counts_host: bad argument");
    uint8_t *tc = NULL, *qc = NULL;
    int64_t cap = 0;
    for (int64_t p = 0; p < n; ++p) {
        const gac_window *w = &pieces[p];
        memset(pairs + p * 16, 0, 16 * sizeof(*pairs));
        n_cols[p] = 0;
        if (w->chain < 0 || w->chain >= d->n_chains || w->first_block < 0 || w->n_blocks < 0 ||
            (int64_t)w->first_block + w->n_blocks > d->blk_off[w->chain + 1] - d->blk_off[w->chain]) {
            free(tc);
            free(qc);
            return gac_fail(GAC_E_ARG, "gac_axt: a piece's blocks lie outside its chain (or its "
                                       "chain index is out of range)");
        }
        const int32_t ts = d->t_seq[w->chain], qs = d->q_seq[w->chain];
        if (ts < 0 || (uint32_t)ts >= t->seq_count || qs < 0 || (uint32_t)qs >= q->seq_count) {
            free(tc);
            free(qc);
            return gac_fail(GAC_E_ARG, "chain %d: sequence index out of range", (int)w->chain);
        }
        const gac_twobit_seq *T = &t->seqs[ts], *Q = &q->seqs[qs];
        const int minus = d->q_strand[w->chain] != 0;
        const int64_t b0 = d->blk_off[w->chain] + w->first_block;
        for (int64_t b = b0; b < b0 + w->n_blocks; ++b) {
            const int64_t bt = d->blk_t[b], bq = d->blk_q[b], z = d->blk_size[b];
            int bad = z < 0 || bt < 0 || bq < 0 || bt + z > (int64_t)T->size || bq + z > (int64_t)Q->size;
            if (!bad && b > b0) {
                const int64_t dt = bt - ((int64_t)d->blk_t[b - 1] + d->blk_size[b - 1]);
                const int64_t dq = bq - ((int64_t)d->blk_q[b - 1] + d->blk_size[b - 1]);
                if (dt < 0 || dq < 0 || (dt > 0 && dq > 0)) {
                    free(tc);
                    free(qc);
                    return gac_fail(GAC_E_ARG, "gac_axt: a piece holds a negative or double-sided "
                                               "gap (cut chains with gac_axt_split)");
                }
            }
            if (bad) {
                free(tc);
                free(qc);
                return gac_fail(GAC_E_ARG, "chain %d block %lld outside its sequences", (int)w->chain,
                                (long long)(b - d->blk_off[w->chain]));
            }
            if (z > cap) {
                cap = z + z / 2 + 64;
                free(tc);
                free(qc);
                tc = malloc((size_t)cap);
                qc = malloc((size_t)cap);
                if (!tc || !qc) {
                    free(tc);
                    free(qc);
                    return gac_fail(GAC_E_ARG, "gac_axt_pair_counts_host: out of memory");
                }
            }
            seq_codes(t, T, bt, z, tc);
            /* '-': strand base i is the complement of forward base size - 1 - (bq + i) */
            seq_codes(q, Q, minus ? (int64_t)Q->size - bq - z : bq, z, qc);
            for (int64_t i = 0; i < z; ++i) {
                const int a = tc[i];
                int c = minus ? qc[z - 1 - i] : qc[i];
                if (a == 4 || c == 4) {
                    ++n_cols[p];
                    continue;
                }
                if (minus)
                    c ^= 2;
                ++pairs[p * 16 + k_acgt[c] * 4 + k_acgt[a]];
            }
        }
    }
    free(tc);
    free(qc);
    return GAC_OK;
}

int gac_axt_pair_counts_host(const char *t_2bit, const char *q_2bit, const gac_chainset_desc *d,
                             const gac_window *pieces, int64_t n, int64_t *pairs, int64_t *n_cols) {
    gac_clear_error();
    if (!t_2bit || !q_2bit)
        return gac_fail(GAC_E_ARG, "gac_axt_pair_counts_host: bad argument");
    gac_twobit t, q;
    int rc = gac_twobit_open(t_2bit, &t);
    if (rc != GAC_OK)
        return rc;
    rc = gac_twobit_open(q_2bit, &q);
    if (rc == GAC_OK) {
        rc = gac_axt_pair_counts_twobit(&t, &q, d, pieces, n, pairs, n_cols);
        gac_twobit_close(&q);
    }
    gac_twobit_close(&t);
    return rc;
}
