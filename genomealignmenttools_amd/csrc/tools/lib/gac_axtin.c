/* gac_axtin.c -- the shared axt reader (gac_axtin.h): lineFile's lines split on
 * all threads, axtRead's records, their headers parsed on all threads, sizes
 * files.  (A NUL byte inside a line ends the line for the reference; here it
 * is a byte like any other.) */
#define _GNU_SOURCE
#include <limits.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_axtin.h"

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

/* isspace in the C locale */
static inline int is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

/* ---- lines, as lineFileNext returns them */
typedef struct line_part {
    const char *buf;
    int64_t lo, hi; /* line starts */
    char sep;
    int dos;
    gt_axt_line *v;
    int64_t n, cap;
    int64_t too_long; /* offset of a line over INT32_MAX bytes, or -1 */
} line_part;

static void *line_thread(void *arg) {
    line_part *P = arg;
    const char *buf = P->buf;
    for (int64_t i = P->lo; i < P->hi;) {
        const char *nl = memchr(buf + i, P->sep, (size_t)(P->hi - i));
        int64_t e = nl ? nl - buf : P->hi;
        const int64_t next = nl ? e + 1 : P->hi;
        if (P->dos && nl && e > i && buf[e - 1] == '\r')
            --e;
        if (e - i > INT32_MAX) {
            P->too_long = i;
            return NULL;
        }
        if (P->n == P->cap) {
            P->cap = P->cap ? P->cap * 2 : 4096;
            P->v = realloc(P->v, (size_t)P->cap * sizeof(gt_axt_line));
            if (!P->v)
                gt_abort("Out of memory");
        }
        P->v[P->n++] = (gt_axt_line){i, (int32_t)(e - i), 0};
        i = next;
    }
    return NULL;
}

gt_axt_line *gt_axt_lines(const char *buf, int64_t size, int64_t *n_out) {
    /* determineNlType (linefile.c:425): the first line end decides */
    char sep = '\n';
    int dos = 0;
    for (int64_t i = 0; i < size; ++i) {
        if (buf[i] == '\n')
            break;
        if (buf[i] == '\r') {
            if (i + 1 < size && buf[i + 1] == '\n')
                dos = 1;
            else
                sep = '\r';
            break;
        }
    }
    int nt = gt_threads();
    if (nt > 64)
        nt = 64;
    while (nt > 1 && size / nt < (1 << 20))
        nt /= 2;
    line_part part[64];
    for (int k = 0; k < nt; ++k) {
        int64_t lo = size / nt * k;
        while (lo > 0 && lo < size && buf[lo - 1] != sep)
            ++lo;
        part[k] = (line_part){buf, lo, size, sep, dos, NULL, 0, 0, -1};
        if (k)
            part[k - 1].hi = lo;
    }
    gt_parallel(nt, line_thread, part, sizeof(line_part));
    int64_t n = 0;
    for (int k = 0; k < nt; ++k) {
        if (part[k].too_long >= 0)
            gt_abort("a line of more than %d bytes at offset %lld", INT32_MAX, (long long)part[k].too_long);
        n += part[k].n;
    }
    gt_axt_line *v = must_alloc((size_t)n * sizeof(gt_axt_line));
    n = 0;
    for (int k = 0; k < nt; ++k) {
        if (part[k].n)
            memcpy(v + n, part[k].v, (size_t)part[k].n * sizeof(gt_axt_line));
        n += part[k].n;
        free(part[k].v);
    }
    *n_out = n;
    return v;
}

int gt_axt_chop(const char *p, int32_t len, gt_axt_word *w, int max) {
    int n = 0;
    for (int32_t i = 0; n < max;) {
        while (i < len && is_space((unsigned char)p[i]))
            ++i;
        if (i == len)
            break;
        const int32_t a = i;
        while (i < len && !is_space((unsigned char)p[i]))
            ++i;
        w[n++] = (gt_axt_word){p + a, i - a};
    }
    return n;
}

/* lineFileNeedNum (linefile.c:1015): a '-' or a digit first, then atoi */
int gt_axt_need_num(gt_axt_word w, int32_t *v) {
    const unsigned char c = (unsigned char)w.p[0];
    if (c != '-' && !(c >= '0' && c <= '9'))
        return 0;
    uint32_t u = 0;
    for (int32_t i = c == '-'; i < w.len && w.p[i] >= '0' && w.p[i] <= '9'; ++i)
        u = u * 10u + (uint32_t)(w.p[i] - '0');
    *v = (int32_t)(c == '-' ? 0u - u : u);
    return 1;
}

/* lineFileChopNext's line test: not a '#' line and not blank */
int gt_axt_has_words(const char *buf, gt_axt_line ln) {
    if (ln.len > 0 && buf[ln.off] == '#')
        return 0;
    for (int32_t i = 0; i < ln.len; ++i)
        if (!is_space((unsigned char)buf[ln.off + i]))
            return 1;
    return 0;
}

/* ---- sizes: readSizes (axtToPsl.c:29-45) */
void gt_axt_read_sizes(const char *path, gt_axt_sizes *S) {
    memset(S, 0, sizeof(*S));
    size_t bytes;
    char *buf = gt_slurp(path, &bytes);
    int64_t nl;
    gt_axt_line *v = gt_axt_lines(buf, (int64_t)bytes, &nl);
    for (int64_t k = 0; k < nl; ++k) {
        if (!gt_axt_has_words(buf, v[k]))
            continue;
        gt_axt_word w[2];
        const int wc = gt_axt_chop(buf + v[k].off, v[k].len, w, 2);
        if (wc < 2)
            gt_abort("Expecting 2 words line %lld of %s got %d", (long long)k + 1, path, wc);
        int32_t size;
        if (!gt_axt_need_num(w[1], &size))
            gt_abort("Expecting number field 2 line %lld of %s, got %.*s", (long long)k + 1, path, w[1].len,
                     w[1].p);
        const int32_t id = gt_names_add(&S->names, w[0].p, (size_t)w[0].len);
        if (id >= S->cap) {
            S->cap = S->cap ? S->cap * 2 : 64;
            S->size = realloc(S->size, (size_t)S->cap * sizeof(int32_t));
            if (!S->size)
                gt_abort("Out of memory");
        }
        S->size[id] = size; /* hashAdd puts the newest first: the last line of a name counts */
    }
    free(v);
    free(buf);
}

void gt_axt_free_sizes(gt_axt_sizes *S) {
    gt_names_free(&S->names);
    free(S->size);
}

int32_t gt_axt_find_name(const gt_axt_sizes *S, gt_axt_word w) {
    char small[256], *s = w.len < (int32_t)sizeof(small) ? small : must_alloc((size_t)w.len + 1);
    memcpy(s, w.p, (size_t)w.len);
    s[w.len] = 0;
    const int32_t id = gt_names_find(&S->names, s);
    if (s != small)
        free(s);
    return id;
}

/* ---- records */
void gt_axt_group(const char *buf, const gt_axt_line *v, int64_t nl, const char *path, gt_axt_records *R) {
    const int64_t cap = nl / 3 + 1;
    int64_t n = 0;
    R->h_off = must_alloc((size_t)cap * 8), R->t_off = must_alloc((size_t)cap * 8);
    R->q_off = must_alloc((size_t)cap * 8);
    R->h_len = must_alloc((size_t)cap * 4), R->len = must_alloc((size_t)cap * 4);
    R->line0 = must_alloc((size_t)(cap + 1) * 8);
    int64_t first = 0; /* the first line read for the next record */
    for (int64_t k = 0; k < nl;) {
        if (!gt_axt_has_words(buf, v[k])) {
            ++k;
            continue;
        }
        if (k + 2 >= nl)
            gt_abort("Unexpected end of file in %s", path);
        if (v[k + 1].len != v[k + 2].len)
            gt_abort("Symbol count %d != %d inconsistent between sequences line %lld and prev line of %s",
                     v[k + 1].len, v[k + 2].len, (long long)k + 3, path);
        R->h_off[n] = v[k].off, R->h_len[n] = v[k].len;
        R->t_off[n] = v[k + 1].off, R->q_off[n] = v[k + 2].off, R->len[n] = v[k + 1].len;
        R->line0[n] = first;
        ++n;
        k += 4; /* the line after the rows is taken, whatever it holds */
        first = k < nl ? k : nl;
    }
    R->line0[n] = first;
    R->n = n;
    R->tname = must_alloc((size_t)n * 4), R->qname = must_alloc((size_t)n * 4);
    R->tstart = must_alloc((size_t)n * 4), R->tend = must_alloc((size_t)n * 4);
    R->qstart = must_alloc((size_t)n * 4), R->qend = must_alloc((size_t)n * 4);
    R->score = must_alloc((size_t)n * 4);
    R->tn_off = must_alloc((size_t)n * 8), R->qn_off = must_alloc((size_t)n * 8);
    R->tn_len = must_alloc((size_t)n * 4), R->qn_len = must_alloc((size_t)n * 4);
    R->strand = must_alloc((size_t)n);
}

void gt_axt_free_records(gt_axt_records *R) {
    free(R->h_off), free(R->t_off), free(R->q_off), free(R->h_len), free(R->len), free(R->line0);
    free(R->tname), free(R->qname), free(R->tstart), free(R->tend), free(R->qstart), free(R->qend), free(R->score);
    free(R->tn_off), free(R->qn_off), free(R->tn_len), free(R->qn_len), free(R->strand);
}

/* the headers on all threads; the first bad record in file order is reported */
typedef struct head_job {
    const char *buf;
    gt_axt_records *R;
    const gt_axt_sizes *T, *Q;
    _Atomic int64_t next, bad; /* bad: the lowest failing record, or INT64_MAX */
} head_job;

enum { HEAD_OK, HEAD_WORDS, HEAD_NUMBER, HEAD_QNAME, HEAD_TNAME };

static int parse_head(const head_job *J, int64_t i, int *field) {
    gt_axt_records *R = J->R;
    gt_axt_word w[10];
    const int wc = gt_axt_chop(J->buf + R->h_off[i], R->h_len[i], w, 10);
    *field = wc;
    if (wc < 8)
        return HEAD_WORDS;
    static const int k_num[4] = {5, 6, 2, 3}; /* axtRead's order */
    int32_t v[4], score = 0;
    for (int k = 0; k < 4; ++k)
        if (!gt_axt_need_num(w[k_num[k]], &v[k])) {
            *field = k_num[k] + 1;
            return HEAD_NUMBER;
        }
    if (wc > 8 && !gt_axt_need_num(w[8], &score)) {
        *field = 9;
        return HEAD_NUMBER;
    }
    R->qstart[i] = (int32_t)((uint32_t)v[0] - 1u), R->qend[i] = v[1];
    R->tstart[i] = (int32_t)((uint32_t)v[2] - 1u), R->tend[i] = v[3];
    R->score[i] = score;
    R->strand[i] = w[7].p[0];
    R->tn_off[i] = w[1].p - J->buf, R->tn_len[i] = w[1].len;
    R->qn_off[i] = w[4].p - J->buf, R->qn_len[i] = w[4].len;
    R->qname[i] = R->tname[i] = -1;
    if (J->Q && (R->qname[i] = gt_axt_find_name(J->Q, w[4])) < 0)
        return HEAD_QNAME;
    if (J->T && (R->tname[i] = gt_axt_find_name(J->T, w[1])) < 0)
        return HEAD_TNAME;
    return HEAD_OK;
}

static void *head_thread(void *arg) {
    head_job *J = arg;
    for (int64_t lo; (lo = atomic_fetch_add(&J->next, 1024)) < J->R->n;) {
        const int64_t hi = lo + 1024 < J->R->n ? lo + 1024 : J->R->n;
        for (int64_t i = lo; i < hi; ++i) {
            int field;
            if (parse_head(J, i, &field) != HEAD_OK) {
                int64_t b = atomic_load(&J->bad);
                while (i < b && !atomic_compare_exchange_weak(&J->bad, &b, i))
                    ;
                return NULL;
            }
        }
    }
    return NULL;
}

void gt_axt_parse_heads(const char *buf, gt_axt_records *R, const gt_axt_sizes *T, const gt_axt_sizes *Q, const char *path) {
    head_job J = {buf, R, T, Q, 0, INT64_MAX};
    int nt = gt_threads();
    while (nt > 1 && R->n / nt < 1024)
        nt /= 2;
    /* (gt_parallel hands thread i args + i * stride: stride 0 is the one job) */
    gt_parallel(nt, head_thread, &J, 0);
    const int64_t bad = atomic_load(&J.bad);
    if (bad == INT64_MAX)
        return;
    int field;
    const int why = parse_head(&J, bad, &field);
    const int hl = R->h_len[bad] > 200 ? 200 : R->h_len[bad];
    const char *h = buf + R->h_off[bad];
    switch (why) {
    case HEAD_WORDS:
        gt_abort("Expecting at least 8 words record %lld of %s got %d", (long long)bad + 1, path, field);
    case HEAD_NUMBER:
        gt_abort("Expecting number field %d record %lld of %s, got '%.*s'", field, (long long)bad + 1, path, hl, h);
    case HEAD_QNAME:
        gt_abort("%.*s not found in the query sizes (record %lld of %s)", R->qn_len[bad], buf + R->qn_off[bad],
                 (long long)bad + 1, path);
    default:
        gt_abort("%.*s not found in the target sizes (record %lld of %s)", R->tn_len[bad], buf + R->tn_off[bad],
                 (long long)bad + 1, path);
    }
}
