/* gac_axtfilter.c -- filterAxtIdentityEntropy's keep decision on the host: the
 * argument check and the two tables gac_axt_filter shares (the smallest match
 * count that reaches minSeqIdent, the p*log(p) terms), and
 * gac_axt_filter_host (src/filterAxtIdentityEntropy.py:32-69 getNum,
 * getSeqIdent, getEntropy; :88-110 checkAxt; :144-162 the column counts) with
 * running window counts, threaded over entries
 * (filterAxtIdentityEntropy.py -host, and the device call's fallbacks).
 *
 * An entry passes iff a window start s with target[s] != '-' and s + W <= L
 * has 100.0 * m / W >= minSeqIdent and H >= minEntropy over [s, s + W): the
 * script's inner loop over longer windows only runs after that first window
 * passed and never takes the pass back.  Every libm call is made here, on the
 * host, in the script's own expression and order; the window test itself is
 * integer compares, double subtractions in a, c, g, t order and one division. */
#include <math.h>
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

int gac_axtf_check(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                   const int64_t *q_off, const int32_t *len, int32_t window, const uint8_t *keep) {
    if (window < 1)
        return gac_fail(GAC_E_ARG, "gac_axt_filter: window size %d, must be at least 1", window);
    if (n < 0 || text_bytes < 0)
        return gac_fail(GAC_E_ARG, "gac_axt_filter: bad argument (n %lld, text bytes %lld)", (long long)n,
                        (long long)text_bytes);
    if (n == 0)
        return GAC_OK;
    if (!text || !t_off || !q_off || !len || !keep)
        return gac_fail(GAC_E_ARG, "gac_axt_filter: NULL buffer");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t L = len[i];
        if (L < 0 || t_off[i] < 0 || q_off[i] < 0 || t_off[i] > text_bytes - L || q_off[i] > text_bytes - L)
            return gac_fail(GAC_E_ARG,
                            "gac_axt_filter: entry %lld: rows of %d columns at %lld and %lld outside "
                            "%lld bytes of text",
                            (long long)i, len[i], (long long)t_off[i], (long long)q_off[i],
                            (long long)text_bytes);
    }
    return GAC_OK;
}

/* getSeqIdent's test (:42, :102) turned round: the smallest m in 0..W with
 * 100.0 * m / W >= min_ident in the script's own doubles, W + 1 if none (the
 * quotient ascends with m, so the first hit is the threshold) */
int32_t gac_axtf_mmin(double min_ident, int32_t window) {
    for (int32_t m = 0; m <= window; ++m)
        if (100.0 * (double)m / (double)window >= min_ident)
            return m;
    return window + 1;
}

/* getEntropy's terms (:54-67): term[n (n - 1) / 2 + k - 1] = p * log(p), p =
 * k / n, 1 <= k <= n <= window */
double *gac_axtf_terms(int32_t window) {
    const size_t W = (size_t)window;
    double *t = malloc((W * (W + 1) / 2 + 1) * sizeof(double));
    if (!t)
        return NULL;
    size_t at = 0;
    for (int32_t n = 1; n <= window; ++n)
        for (int32_t k = 1; k <= n; ++k) {
            const double p = (double)k / (double)n;
            t[at++] = p * log(p);
        }
    return t;
}

typedef struct axtf_job {
    int64_t n;
    const char *text;
    const int64_t *t_off, *q_off;
    const int32_t *len;
    int32_t W, m_min;
    double min_entropy, ln2;
    const double *term; /* NULL: a window too large for the table, the terms computed in place */
    uint8_t *keep;
    _Atomic int64_t next, kept, windows;
} axtf_job;

static inline double axtf_term(const axtf_job *J, int32_t n, int32_t k) {
    if (J->term)
        return J->term[(size_t)n * (size_t)(n - 1) / 2 + (size_t)(k - 1)];
    const double p = (double)k / (double)n;
    return p * log(p);
}

/* column class: 0..3 = a c g t (target, lower-cased), 4 = anything else */
static uint8_t k_class[256], k_lower[256];
static void axtf_tables(void) {
    for (int c = 0; c < 256; ++c) {
        k_lower[c] = (uint8_t)(c >= 'A' && c <= 'Z' ? c + 32 : c);
        k_class[c] = 4;
    }
    k_class['a'] = k_class['A'] = 0;
    k_class['c'] = k_class['C'] = 1;
    k_class['g'] = k_class['G'] = 2;
    k_class['t'] = k_class['T'] = 3;
}

static int axtf_entry(const axtf_job *J, int64_t i) {
    const int32_t L = J->len[i], W = J->W;
    if (L < W)
        return 0;
    const uint8_t *t = (const uint8_t *)J->text + J->t_off[i], *q = (const uint8_t *)J->text + J->q_off[i];
    int32_t cnt[5] = {0, 0, 0, 0, 0}, m = 0;
    for (int32_t j = 0; j < W - 1; ++j) {
        ++cnt[k_class[t[j]]];
        m += k_lower[t[j]] == k_lower[q[j]];
    }
    for (int32_t s = 0; s + W <= L; ++s) {
        const int32_t j = s + W - 1;
        ++cnt[k_class[t[j]]];
        m += k_lower[t[j]] == k_lower[q[j]];
        if (t[s] != '-' && m >= J->m_min) {
            const int32_t n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            double H = 0.0;
            if (n != 0) {
                double e = 0.0;
                for (int b = 0; b < 4; ++b)
                    if (cnt[b] != 0)
                        e -= axtf_term(J, n, cnt[b]);
                H = e / J->ln2;
            }
            if (H >= J->min_entropy)
                return 1;
        }
        --cnt[k_class[t[s]]];
        m -= k_lower[t[s]] == k_lower[q[s]];
    }
    return 0;
}

#define AXTF_SLICE 256 /* entries a thread takes at a time */

static void *axtf_thread(void *arg) {
    axtf_job *J = arg;
    int64_t kept = 0, windows = 0;
    for (int64_t lo; (lo = atomic_fetch_add(&J->next, AXTF_SLICE)) < J->n;) {
        const int64_t hi = lo + AXTF_SLICE < J->n ? lo + AXTF_SLICE : J->n;
        for (int64_t i = lo; i < hi; ++i) {
            J->keep[i] = (uint8_t)axtf_entry(J, i);
            kept += J->keep[i];
            if (J->len[i] >= J->W)
                windows += J->len[i] - J->W + 1;
        }
    }
    atomic_fetch_add(&J->kept, kept);
    atomic_fetch_add(&J->windows, windows);
    return NULL;
}

#define AXTF_HOST_TABLE_MAX 2048 /* 16.8 MB of terms; a larger window computes them in place */

int gac_axt_filter_host(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                        const int64_t *q_off, const int32_t *len, double min_ident, double min_entropy,
                        int32_t window, int nthreads, uint8_t *keep, gac_axtfilter_stats *st) {
    gac_clear_error();
    if (st)
        memset(st, 0, sizeof(*st));
    int rc = gac_axtf_check(n, text, text_bytes, t_off, q_off, len, window, keep);
    if (rc != GAC_OK || n == 0)
        return rc;
    static _Atomic int tables;
    if (!atomic_load(&tables)) { /* (every writer writes the same bytes) */
        axtf_tables();
        atomic_store(&tables, 1);
    }
    axtf_job J;
    memset(&J, 0, sizeof(J));
    J.n = n, J.text = text, J.t_off = t_off, J.q_off = q_off, J.len = len, J.keep = keep;
    J.W = window;
    J.m_min = gac_axtf_mmin(min_ident, window);
    J.min_entropy = min_entropy;
    J.ln2 = log(2.0);
    double *term = NULL;
    if (window <= AXTF_HOST_TABLE_MAX && !(term = gac_axtf_terms(window)))
        return gac_fail(GAC_E_ARG, "gac_axt_filter_host: out of memory");
    J.term = term;
    atomic_init(&J.next, 0);
    atomic_init(&J.kept, 0);
    atomic_init(&J.windows, 0);
    int nt = nthreads > 0 ? nthreads : gac_host_threads();
    if (nt > 64)
        nt = 64;
    while (nt > 1 && n / nt < AXTF_SLICE)
        nt /= 2;
    if (nt < 1)
        nt = 1;
    gac_run_threads(nt, axtf_thread, &J);
    free(term);
    if (st) {
        st->kept = atomic_load(&J.kept);
        st->windows = atomic_load(&J.windows);
        st->host_entries = n;
    }
    return GAC_OK;
}
