/* gac_depth.c -- coverage depth of ranges on the host: the argument check
 * gac_depth_count shares, and gac_depth_count_host, the same result by a
 * threaded sort of the 2n range ends and one sweep over them (netSyntenic
 * -host; the method is described in gac_depth.hip). */
#include <limits.h>
#include <stdatomic.h>
#include <stdlib.h>
#include <string.h>

#include "gac_host.h"
#include "gachain.h"

int gac_depth_check(int64_t n, const int32_t *seq, const int32_t *start, const int32_t *end,
                    const int8_t *delta, int32_t threshold, const int32_t *count,
                    int32_t *max_seq) {
    if (n < 0 || threshold < 1)
        return gac_fail(GAC_E_ARG, "gac_depth_count: bad argument (n %lld, threshold %d)",
                        (long long)n, threshold);
    if (n > INT32_MAX / 2) /* the sort and scan wrappers take int counts of 2n events */
        return gac_fail(GAC_E_ARG, "gac_depth_count: %lld ranges, at most %d a call", (long long)n,
                        INT32_MAX / 2);
    if (n > 0 && (!seq || !start || !end || !delta || !count))
        return gac_fail(GAC_E_ARG, "gac_depth_count: NULL buffer");
    int32_t top = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (seq[i] < 0 || start[i] < 0 || end[i] < start[i])
            return gac_fail(GAC_E_ARG, "gac_depth_count: range %lld: sequence %d [%d, %d)",
                            (long long)i, seq[i], start[i], end[i]);
        if (seq[i] > top)
            top = seq[i];
    }
    if (max_seq)
        *max_seq = top;
    return GAC_OK;
}

typedef struct depth_ev {
    uint64_t key; /* (seq << 32) | position */
    uint32_t id;  /* < n: start of range id; else end of range id - n */
} depth_ev;

static int cmp_ev(const void *a, const void *b) {
    const uint64_t x = ((const depth_ev *)a)->key, y = ((const depth_ev *)b)->key;
    return x < y ? -1 : x > y;
}

/* sort: `parts` equal slices sorted on their own, then merged pairwise in
 * rounds (each merge on one thread, slices doubling) between two buffers */
typedef struct depth_sort {
    depth_ev *a, *b;
    int64_t m, per; /* per: the slice length of this round */
    int round;      /* 0: sort slices of a; else merge pairs of slices a -> b */
    _Atomic int64_t next;
} depth_sort;

static void *depth_sort_thread(void *arg) {
    depth_sort *S = arg;
    for (;;) {
        const int64_t k = atomic_fetch_add(&S->next, 1);
        if (S->round == 0) {
            const int64_t lo = k * S->per;
            if (lo >= S->m)
                return NULL;
            const int64_t hi = lo + S->per < S->m ? lo + S->per : S->m;
            qsort(S->a + lo, (size_t)(hi - lo), sizeof(depth_ev), cmp_ev);
            continue;
        }
        const int64_t lo = k * 2 * S->per;
        if (lo >= S->m)
            return NULL;
        const int64_t mid = lo + S->per < S->m ? lo + S->per : S->m;
        const int64_t hi = mid + S->per < S->m ? mid + S->per : S->m;
        const depth_ev *x = S->a + lo, *xe = S->a + mid, *y = S->a + mid, *ye = S->a + hi;
        depth_ev *o = S->b + lo;
        while (x < xe && y < ye)
            *o++ = y->key < x->key ? *y++ : *x++;
        while (x < xe)
            *o++ = *x++;
        while (y < ye)
            *o++ = *y++;
    }
}

int gac_depth_count_host(int64_t n, const int32_t *seq, const int32_t *start, const int32_t *end,
                         const int8_t *delta, int32_t threshold, int32_t *count) {
    gac_clear_error();
    int rc = gac_depth_check(n, seq, start, end, delta, threshold, count, NULL);
    if (rc != GAC_OK || n == 0)
        return rc;
    const int64_t m = 2 * n;
    depth_ev *ev = malloc((size_t)m * sizeof(depth_ev)), *ev2 = malloc((size_t)m * sizeof(depth_ev));
    int64_t *before = malloc((size_t)m * sizeof(int64_t)); /* by event id */
    if (!ev || !ev2 || !before) {
        free(ev);
        free(ev2);
        free(before);
        return gac_fail(GAC_E_ARG, "gac_depth_count_host: out of memory (%lld ranges)", (long long)n);
    }
    for (int64_t i = 0; i < n; ++i) {
        ev[i].key = ((uint64_t)(uint32_t)seq[i] << 32) | (uint32_t)start[i];
        ev[i].id = (uint32_t)i;
        ev[n + i].key = ((uint64_t)(uint32_t)seq[i] << 32) | (uint32_t)end[i];
        ev[n + i].id = (uint32_t)(n + i);
    }
    int nt = gac_host_threads();
    if (nt < 1)
        nt = 1;
    while (nt > 1 && m / nt < 4096) /* small inputs: fewer, larger slices */
        nt /= 2;
    depth_sort S = {ev, ev2, m, (m + nt - 1) / nt, 0, 0};
    atomic_init(&S.next, 0);
    gac_run_threads(nt, depth_sort_thread, &S);
    for (S.round = 1; S.per < m; S.per *= 2) {
        atomic_init(&S.next, 0);
        const int64_t pairs = (m + 2 * S.per - 1) / (2 * S.per);
        gac_run_threads(pairs < nt ? (int)pairs : nt, depth_sort_thread, &S);
        depth_ev *t = S.a;
        S.a = S.b;
        S.b = t;
    }
    const depth_ev *s = S.a;
    /* sweep: the covered length before every event */
    int64_t acc = 0;
    int32_t depth = 0;
    for (int64_t k = 0; k < m; ++k) {
        const uint32_t id = s[k].id;
        before[id] = acc;
        depth += (int64_t)id < n ? (int32_t)delta[id] : -(int32_t)delta[id - n];
        if (k + 1 < m && (s[k].key >> 32) == (s[k + 1].key >> 32) && depth >= threshold)
            acc += (int64_t)(s[k + 1].key - s[k].key);
    }
    for (int64_t i = 0; i < n; ++i)
        count[i] = (int32_t)(before[n + i] - before[i]);
    free(ev);
    free(ev2);
    free(before);
    return GAC_OK;
}
