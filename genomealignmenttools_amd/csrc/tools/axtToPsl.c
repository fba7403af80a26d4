/* axtToPsl -- native drop-in for the reference's
 * kent/src/hg/mouseStuff/axtToPsl/axtToPsl.c, the step patchChain.perl puts
 * between lastz (or the filter behind it) and axtChain -psl
 * (patchChain.perl:210,215,243,248): every axt record as one PSL line.
 *
 *   axtToPsl in.axt tSizes qSizes out.psl
 *
 * Reading is axtRead's (kent/src/lib/axt.c:52-92) over lineFile's lines: the
 * first '\n' or '\r' of a file decides whether its lines end with '\n', with
 * '\r\n' or with '\r'.  A record is the next line that does not start with '#'
 * and has a word -- at least 8 words, the 3rd, 4th, 6th, 7th and, if there is
 * one, the 9th starting with '-' or a digit and read as atoi reads them, the
 * strand the first character of the 8th -- then two lines as they are, target
 * row and query row, of equal length, then one more line, whatever it holds.
 * A sizes file is lineFileRow's with two columns; the last line of a name
 * counts, as with kent's hashAdd and hashFindVal.  (A NUL byte inside a line
 * ends the line for the reference; here it is a byte like any other.)
 *
 * The conversion is pslFromAlign's (kent/src/lib/psl.c:1716-1806):
 * gac_axt_psl or gac_axt_psl_host give the counts, the trim
 * and the blocks of the rows, and the reference's own arithmetic puts the
 * header's coordinates on them -- qStart / qEnd flipped to the plus strand for
 * '-', moved by the trim in those coordinates (so that on '-' leading
 * query-only columns move the wrong end, as there), nothing written when
 * qStart == qEnd or tStart == tEnd afterwards, the blocks from the flipped-back
 * qStart.  The lines are pslTabOut's.
 *
 * Where the reference aborts -- a header of fewer than 8 words, a word that is
 * no number, rows of unequal length, a file that ends inside a record, a name
 * missing from a sizes file, a sizes line of one word -- this tool aborts with
 * a message and status 255 before it writes a line (the reference has written
 * the records before the bad one by then).  Another number of arguments
 * prints the reference's usage and exits 255; any option is accepted, as
 * optionHash does.  Extensions:
 *   -host, -device   force the path.  By default a regular input file of 2 GiB
 *                    or more takes the device path and everything else
 *                    (smaller files, stdin) the host path: the sweep of
 *                    scripts/axtpsl_profile.sh.  The device
 *                    is opened only if a job takes the device path.
 *   -jobs=FILE       run every line of FILE (the four arguments, white space
 *                    between them, no quoting; blank and '#' lines skipped) in
 *                    this process, with one device context for all of them.
 *   -verbose=2       stage laps.
 *
 * The line index is this tool's own: filterAxtIdentityEntropy.py reads as
 * Python does (every line end at once, lines stripped, '#' lines dropped
 * wherever they stand), and a reader that did both would share the thread
 * split and nothing else. */
#define _GNU_SOURCE
#include <limits.h>
#include <stdatomic.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "gac_pslout.h"
#include "gac_tool.h"
#include "gachain.h"
#include "host/gac_host.h"

/* Inputs of at least this many bytes take the device path by default; < 0:
 * none does.  From the sweep of scripts/axtpsl_profile.sh: the
 * device path, its bring-up included, took 5.28, 1.82, 1.05, 0.73 and 0.81 of
 * the host path's time at 67 MB, 268 MB, 1.07 GB, 2.15 GB and 4.29 GB; 2 GiB is
 * the smallest size at which it took at most 0.8. */
static const int64_t k_device_min_bytes = 2048ll << 20;

static void usage(void) {
    gt_abort("axtToPsl - Convert axt to psl format\n"
             "usage:\n"
             "   axtToPsl in.axt tSizes qSizes out.psl\n"
             "Where tSizes and qSizes are tab-delimited files with\n"
             "       <seqName><size>\n"
             "columns.\n"
             "options:\n"
             "   -xxx=XXX\n");
}

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

/* isspace in the C locale */
static inline int is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13); }

/* ---- lines, as lineFileNext returns them */
typedef struct line {
    int64_t off;
    int32_t len, pad;
} line;

typedef struct line_part {
    const char *buf;
    int64_t lo, hi; /* line starts */
    char sep;
    int dos;
    line *v;
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
            P->v = realloc(P->v, (size_t)P->cap * sizeof(line));
            if (!P->v)
                gt_abort("Out of memory");
        }
        P->v[P->n++] = (line){i, (int32_t)(e - i), 0};
        i = next;
    }
    return NULL;
}

static line *read_lines(const char *buf, int64_t size, int64_t *n_out) {
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
    line *v = must_alloc((size_t)n * sizeof(line));
    n = 0;
    for (int k = 0; k < nt; ++k) {
        if (part[k].n)
            memcpy(v + n, part[k].v, (size_t)part[k].n * sizeof(line));
        n += part[k].n;
        free(part[k].v);
    }
    *n_out = n;
    return v;
}

/* chopByWhite (common.c:2029): up to max words of a line; returns the count */
typedef struct word {
    const char *p;
    int32_t len;
} word;

static int chop_white(const char *p, int32_t len, word *w, int max) {
    int n = 0;
    for (int32_t i = 0; n < max;) {
        while (i < len && is_space((unsigned char)p[i]))
            ++i;
        if (i == len)
            break;
        const int32_t a = i;
        while (i < len && !is_space((unsigned char)p[i]))
            ++i;
        w[n++] = (word){p + a, i - a};
    }
    return n;
}

/* lineFileNeedNum (linefile.c:1015): a '-' or a digit first, then atoi */
static int need_num(word w, int32_t *v) {
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
static int has_words(const char *buf, line ln) {
    if (ln.len > 0 && buf[ln.off] == '#')
        return 0;
    for (int32_t i = 0; i < ln.len; ++i)
        if (!is_space((unsigned char)buf[ln.off + i]))
            return 1;
    return 0;
}

/* ---- sizes: readSizes (axtToPsl.c:29-45) */
typedef struct sizes {
    gt_names names;
    int32_t *size;
    int32_t cap;
} sizes;

static void read_sizes(const char *path, sizes *S) {
    memset(S, 0, sizeof(*S));
    size_t bytes;
    char *buf = gt_slurp(path, &bytes);
    int64_t nl;
    line *v = read_lines(buf, (int64_t)bytes, &nl);
    for (int64_t k = 0; k < nl; ++k) {
        if (!has_words(buf, v[k]))
            continue;
        word w[2];
        const int wc = chop_white(buf + v[k].off, v[k].len, w, 2);
        if (wc < 2)
            gt_abort("Expecting 2 words line %lld of %s got %d", (long long)k + 1, path, wc);
        int32_t size;
        if (!need_num(w[1], &size))
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

static void free_sizes(sizes *S) {
    gt_names_free(&S->names);
    free(S->size);
}

static int32_t find_name(const sizes *S, word w) {
    char small[256], *s = w.len < (int32_t)sizeof(small) ? small : must_alloc((size_t)w.len + 1);
    memcpy(s, w.p, (size_t)w.len);
    s[w.len] = 0;
    const int32_t id = gt_names_find(&S->names, s);
    if (s != small)
        free(s);
    return id;
}

/* ---- records */
typedef struct records {
    int64_t n;
    int64_t *h_off, *t_off, *q_off;
    int32_t *h_len, *len;
    /* from the headers, on all threads */
    int32_t *tname, *qname; /* index into the sizes' names */
    int32_t *tstart, *tend, *qstart, *qend;
    int64_t *tn_off, *qn_off; /* the names in the text */
    int32_t *tn_len, *qn_len;
    char *strand;
} records;

static void group_records(const char *buf, const line *v, int64_t nl, const char *path, records *R) {
    const int64_t cap = nl / 3 + 1;
    int64_t n = 0;
    R->h_off = must_alloc((size_t)cap * 8), R->t_off = must_alloc((size_t)cap * 8);
    R->q_off = must_alloc((size_t)cap * 8);
    R->h_len = must_alloc((size_t)cap * 4), R->len = must_alloc((size_t)cap * 4);
    for (int64_t k = 0; k < nl;) {
        if (!has_words(buf, v[k])) {
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
        ++n;
        k += 4; /* the line after the rows is taken, whatever it holds */
    }
    R->n = n;
    R->tname = must_alloc((size_t)n * 4), R->qname = must_alloc((size_t)n * 4);
    R->tstart = must_alloc((size_t)n * 4), R->tend = must_alloc((size_t)n * 4);
    R->qstart = must_alloc((size_t)n * 4), R->qend = must_alloc((size_t)n * 4);
    R->tn_off = must_alloc((size_t)n * 8), R->qn_off = must_alloc((size_t)n * 8);
    R->tn_len = must_alloc((size_t)n * 4), R->qn_len = must_alloc((size_t)n * 4);
    R->strand = must_alloc((size_t)n);
}

static void free_records(records *R) {
    free(R->h_off), free(R->t_off), free(R->q_off), free(R->h_len), free(R->len);
    free(R->tname), free(R->qname), free(R->tstart), free(R->tend), free(R->qstart), free(R->qend);
    free(R->tn_off), free(R->qn_off), free(R->tn_len), free(R->qn_len), free(R->strand);
}

/* the headers on all threads; the first bad record in file order is reported */
typedef struct head_job {
    const char *buf;
    records *R;
    const sizes *T, *Q;
    _Atomic int64_t next, bad; /* bad: the lowest failing record, or INT64_MAX */
} head_job;

enum { HEAD_OK, HEAD_WORDS, HEAD_NUMBER, HEAD_QNAME, HEAD_TNAME };

static int parse_head(const head_job *J, int64_t i, int *field) {
    records *R = J->R;
    word w[10];
    const int wc = chop_white(J->buf + R->h_off[i], R->h_len[i], w, 10);
    *field = wc;
    if (wc < 8)
        return HEAD_WORDS;
    static const int k_num[4] = {5, 6, 2, 3}; /* axtRead's order */
    int32_t v[4], score;
    for (int k = 0; k < 4; ++k)
        if (!need_num(w[k_num[k]], &v[k])) {
            *field = k_num[k] + 1;
            return HEAD_NUMBER;
        }
    if (wc > 8 && !need_num(w[8], &score)) {
        *field = 9;
        return HEAD_NUMBER;
    }
    R->qstart[i] = (int32_t)((uint32_t)v[0] - 1u), R->qend[i] = v[1];
    R->tstart[i] = (int32_t)((uint32_t)v[2] - 1u), R->tend[i] = v[3];
    R->strand[i] = w[7].p[0];
    R->tn_off[i] = w[1].p - J->buf, R->tn_len[i] = w[1].len;
    R->qn_off[i] = w[4].p - J->buf, R->qn_len[i] = w[4].len;
    if ((R->qname[i] = find_name(J->Q, w[4])) < 0)
        return HEAD_QNAME;
    if ((R->tname[i] = find_name(J->T, w[1])) < 0)
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

static void parse_heads(const char *buf, records *R, const sizes *T, const sizes *Q, const char *path) {
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

/* ---- output: pslTabOut of every record that is not empty after the trim, in runs */
typedef struct out_ctx {
    const char *buf;
    const records *R;
    const sizes *T, *Q;
    const gac_axtpsl_result *res;
    int64_t per;
} out_ctx;

static void write_run(gac_obuf *o, int64_t r, void *arg) {
    const out_ctx *C = arg;
    const records *R = C->R;
    const int64_t a = r * C->per, b = a + C->per < R->n ? a + C->per : R->n;
    for (int64_t i = a; i < b; ++i) {
        const gac_axtpsl_entry *e = &C->res->entry[i];
        gt_psl_align A;
        A.strand = R->strand[i];
        A.qname = C->buf + R->qn_off[i], A.qname_len = (size_t)R->qn_len[i];
        A.tname = C->buf + R->tn_off[i], A.tname_len = (size_t)R->tn_len[i];
        A.qsize = C->Q->size[R->qname[i]], A.tsize = C->T->size[R->tname[i]];
        A.qstart = R->qstart[i], A.qend = R->qend[i], A.tstart = R->tstart[i], A.tend = R->tend[i];
        gt_put_psl_align(o, &A, e, C->res->block + e->block0);
    }
}

/* ---- one run of the tool */
typedef struct job {
    const char *in, *tsizes, *qsizes, *out;
    int device;
} job;

static int64_t file_bytes(const char *path) {
    struct stat st;
    return stat(path, &st) == 0 && S_ISREG(st.st_mode) ? (int64_t)st.st_size : -1;
}

static void set_job(char *const *argv, int force, job *J) {
    J->in = argv[0], J->tsizes = argv[1], J->qsizes = argv[2], J->out = argv[3];
    const int64_t bytes = file_bytes(J->in);
    J->device = force ? force > 0 : k_device_min_bytes >= 0 && bytes >= k_device_min_bytes;
}

/* last: no job after this one uses the device, which is then closed under the writing */
static void run_job(const job *J, gt_device *dev, gac_ctx **ctx, int last) {
    sizes T, Q;
    read_sizes(J->tsizes, &T);
    read_sizes(J->qsizes, &Q);
    size_t size;
    char *buf = gt_slurp(J->in, &size);
    gt_stage("read input");
    int64_t nl;
    line *v = read_lines(buf, (int64_t)size, &nl);
    records R;
    memset(&R, 0, sizeof(R));
    group_records(buf, v, nl, J->in, &R);
    free(v);
    parse_heads(buf, &R, &T, &Q, J->in);
    gt_stage("parse");

    gac_axtpsl_result *res = NULL;
    gac_axtpsl_stats st;
    char what[160];
    if (J->device) {
        if (!*ctx) {
            *ctx = gt_device_join(dev);
            gt_stage("device open (rest)");
        }
        gt_check(gac_axt_psl(*ctx, R.n, buf, (int64_t)size, R.t_off, R.q_off, R.len, &res, &st));
        snprintf(what, sizeof(what), "convert (GPU): %lld records, %lld blocks, %d batches%s", (long long)R.n,
                 (long long)st.blocks, st.batches,
                 st.fell_back == 2 ? ", some records on the host (over the batch bytes)" : "");
    } else {
        gt_check(gac_axt_psl_host(R.n, buf, (int64_t)size, R.t_off, R.q_off, R.len, gt_threads(), &res, &st));
        snprintf(what, sizeof(what), "convert (host): %lld records, %lld blocks", (long long)R.n,
                 (long long)st.blocks);
    }
    gt_stage(what);
    if (last && *ctx) {
        gt_device_close_async(dev, *ctx, NULL);
        *ctx = NULL;
    }

    FILE *out = gt_must_open(J->out, "w"); /* (every record is checked by now) */
    out_ctx C = {buf, &R, &T, &Q, res, 64};
    if (gac_par_output_buf(out, (R.n + C.per - 1) / C.per, write_run, &C) != 0)
        gt_abort("write error on %s", J->out);
    gt_careful_close(out, J->out);
    gac_axtpsl_free(res);
    free_records(&R);
    free(buf);
    free_sizes(&T);
    free_sizes(&Q);
    gt_stage("write output");
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options_hash(&argc, argv);
    const char *jobs_file = gt_opt_str("jobs", NULL);
    if (gt_opt_exists("host") && gt_opt_exists("device"))
        gt_abort("-host and -device exclude each other");
    const int force = gt_opt_exists("host") ? -1 : gt_opt_exists("device") ? 1 : 0;
    if (jobs_file ? argc != 1 : argc != 5)
        usage();

    job *J = NULL;
    int64_t nj = 0;
    if (!jobs_file) {
        J = must_alloc(sizeof(job));
        set_job(argv + 1, force, &J[nj++]);
    } else {
        size_t len;
        char *text = gt_slurp(jobs_file, &len); /* (the jobs point into it) */
        int64_t cap = 0;
        for (char *ln = text, *nl; ln && *ln; ln = nl ? nl + 1 : NULL) {
            nl = strchr(ln, '\n');
            if (nl)
                *nl = 0;
            char *w[8];
            const int wc = gac_chop_white(ln, w, 7);
            if (wc == 0 || w[0][0] == '#')
                continue;
            if (wc != 4)
                gt_abort("%s: job %lld: four arguments expected (in.axt tSizes qSizes out.psl)", jobs_file,
                         (long long)nj + 1);
            if (nj == cap) {
                cap = cap ? cap * 2 : 64;
                J = realloc(J, (size_t)cap * sizeof(job));
                if (!J)
                    gt_abort("Out of memory");
            }
            set_job(w, force, &J[nj++]);
        }
    }
    int any_device = 0;
    for (int64_t k = 0; k < nj; ++k)
        any_device |= J[k].device;
    gt_device dev;
    gac_ctx *ctx = NULL;
    if (any_device)
        gt_device_start_bare(&dev); /* opens while the first input is read and parsed */
    gt_stage("options + setup");
    int64_t last_device = -1;
    for (int64_t k = 0; k < nj; ++k)
        if (J[k].device)
            last_device = k;
    for (int64_t k = 0; k < nj; ++k)
        run_job(&J[k], &dev, &ctx, k >= last_device);
    if (nj > 1)
        gt_verbose(2, "%lld jobs%s\n", (long long)nj, any_device ? " in one device context" : "");
    if (any_device) {
        gt_device_close_join(&dev);
        gt_stage("device close (rest)");
    }
    gt_exit_ok();
}
