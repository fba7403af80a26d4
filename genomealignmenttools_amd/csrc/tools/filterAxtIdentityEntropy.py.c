/* filterAxtIdentityEntropy.py -- native drop-in for the reference's
 * src/filterAxtIdentityEntropy.py, the step patchChain.perl puts behind every
 * lastz call (patchChain.perl:209,242): write the axt entries that have a
 * window of windowSize columns with enough identity and enough entropy.  The
 * binary keeps the script's name, so a job that runs it through $PATH picks it
 * up unchanged.
 *
 *   filterAxtIdentityEntropy.py input.axt minSeqIdent minEntropy windowSize output.axt
 *
 * Reading follows the script (:183-196), not axtRead: every line is read
 * ('\n', '\r\n' and a lone '\r' end one, as Python's text mode has it); lines
 * starting with '#' are dropped wherever they stand; then, repeatedly, lines
 * that are empty after stripping white space are skipped and three lines are
 * taken, each stripped: header, target row, query row.  The header needs five
 * words, the third an integer (:125-128); nothing else of it is used.  The
 * query row's length L counts; a longer target row is written whole.  Where
 * the script dies with status 1 -- a target row shorter than L, a truncated
 * last entry, a bad header, windowSize 0 -- this tool aborts with a message
 * and status 255 before it writes an entry; windowSize < 1 is refused before
 * the input is read.  Another number of arguments prints the usage line on
 * stdout and exits 1, as there.  An argument that parses as a number is a
 * positional argument also when it starts with '-' (a negative threshold).
 *
 * The decision is gac_axt_filter (windows on the device: DESIGN.md 7.14) or
 * gac_axt_filter_host (running counts on all host threads); both give the
 * script's flags bit for bit.  Extensions:
 *   -host, -device   force the path.  The default takes the host path: the
 *                    device path, its bring-up included, took between 3.4 and
 *                    0.96 of the host path's time on inputs of 67 MB to 4 GB,
 *                    never the 0.8 asked of it.  The device
 *                    is opened only if a job takes the device path.
 *   -jobs=FILE       run every line of FILE (the five arguments, white space
 *                    between them, no quoting; blank and '#' lines skipped) in
 *                    this process, with one device context for all of them.
 *   -verbose=2       stage laps. */
#define _GNU_SOURCE
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "gac_tool.h"
#include "gachain.h"
#include "host/gac_host.h"

/* Inputs of at least this many bytes take the device path by default; < 0:
 * none does.  From the sweep of scripts/axtfilter_profile.sh. */
static const int64_t k_device_min_bytes = -1;

static const gt_spec k_opts[] = {
    {"host", GT_BOOL}, {"device", GT_BOOL}, {"jobs", GT_STRING}, {NULL, 0},
};

static void usage(void) {
    printf("usage: filterAxtIdentityEntropy.py input.axt minSeqIdent minEntropy windowSize output.axt\n"
           "options: -host | -device (where the windows are tested), -jobs=FILE (one run per line)\n");
    exit(1);
}

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

static int is_number(const char *s) {
    char *end;
    if (!*s)
        return 0;
    strtod(s, &end);
    return *end == 0;
}

/* white space of Python's str.strip() among the bytes */
static inline int is_space(unsigned char c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

/* ---- lines: the stripped extent of every line that does not start with '#' */
typedef struct line {
    int64_t off;
    int32_t len, pad;
} line;

typedef struct line_part {
    const char *buf;
    int64_t size, lo, hi; /* line starts */
    line *v;
    int64_t n, cap;
    int64_t too_long; /* offset of a line over INT32_MAX bytes, or -1 */
} line_part;

static int is_line_start(const char *buf, int64_t size, int64_t i) {
    return i == 0 || buf[i - 1] == '\n' || (buf[i - 1] == '\r' && (i == size || buf[i] != '\n'));
}

static void *line_thread(void *arg) {
    line_part *P = arg;
    const char *buf = P->buf;
    for (int64_t i = P->lo; i < P->hi;) {
        const char *nl = memchr(buf + i, '\n', (size_t)(P->hi - i));
        int64_t e = nl ? nl - buf : P->hi, next = nl ? e + 1 : P->hi;
        const char *cr = memchr(buf + i, '\r', (size_t)(e - i));
        if (cr) {
            e = cr - buf;
            next = e + 1 < P->size && buf[e + 1] == '\n' ? e + 2 : e + 1;
        }
        if (!(e > i && buf[i] == '#')) {
            int64_t a = i, b = e;
            while (a < b && is_space((unsigned char)buf[a]))
                ++a;
            while (b > a && is_space((unsigned char)buf[b - 1]))
                --b;
            if (b - a > INT32_MAX) {
                P->too_long = a;
                return NULL;
            }
            if (P->n == P->cap) {
                P->cap = P->cap ? P->cap * 2 : 4096;
                P->v = realloc(P->v, (size_t)P->cap * sizeof(line));
                if (!P->v)
                    gt_abort("Out of memory");
            }
            P->v[P->n++] = (line){a, (int32_t)(b - a), 0};
        }
        i = next;
    }
    return NULL;
}

static line *read_lines(const char *buf, int64_t size, int64_t *n_out) {
    int nt = gt_threads();
    if (nt > 64)
        nt = 64;
    while (nt > 1 && size / nt < (1 << 20))
        nt /= 2;
    line_part part[64];
    for (int k = 0; k < nt; ++k) {
        int64_t lo = size / nt * k;
        while (lo < size && !is_line_start(buf, size, lo))
            ++lo;
        part[k] = (line_part){buf, size, lo, size, NULL, 0, 0, -1};
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

/* the script's info.split() and int(splitted[2]) (:125-128): at least five
 * words, the third a decimal integer with an optional sign */
static int header_ok(const char *p, int32_t len) {
    int words = 0, third_ok = 0;
    for (int32_t i = 0; i < len;) {
        while (i < len && is_space((unsigned char)p[i]))
            ++i;
        if (i == len)
            break;
        int32_t a = i;
        while (i < len && !is_space((unsigned char)p[i]))
            ++i;
        if (++words == 3) {
            int32_t k = a;
            if (k < i && (p[k] == '+' || p[k] == '-'))
                ++k;
            third_ok = k < i;
            for (; k < i; ++k)
                if (p[k] < '0' || p[k] > '9')
                    third_ok = 0;
        }
        if (words == 5)
            break;
    }
    return words >= 5 && third_ok;
}

typedef struct entries {
    int64_t n;
    int64_t *h_off, *t_off, *q_off;
    int32_t *h_len, *t_len, *len;
} entries;

static void group_entries(const char *buf, const line *v, int64_t nl, const char *path, entries *E) {
    int64_t cap = nl / 3 + 1, n = 0;
    E->h_off = must_alloc((size_t)cap * 8), E->t_off = must_alloc((size_t)cap * 8);
    E->q_off = must_alloc((size_t)cap * 8);
    E->h_len = must_alloc((size_t)cap * 4), E->t_len = must_alloc((size_t)cap * 4);
    E->len = must_alloc((size_t)cap * 4);
    for (int64_t k = 0; k < nl;) {
        if (v[k].len == 0) {
            ++k;
            continue;
        }
        if (k + 2 >= nl)
            gt_abort("%s: entry %lld is cut short: a header, a target row and a query row expected", path,
                     (long long)n + 1);
        if (!header_ok(buf + v[k].off, v[k].len))
            gt_abort("%s: entry %lld: the header needs five words, the third an integer, got '%.*s'", path,
                     (long long)n + 1, v[k].len > 200 ? 200 : v[k].len, buf + v[k].off);
        if (v[k + 1].len < v[k + 2].len)
            gt_abort("%s: entry %lld: a target row of %d columns, shorter than the query row's %d", path,
                     (long long)n + 1, v[k + 1].len, v[k + 2].len);
        E->h_off[n] = v[k].off, E->h_len[n] = v[k].len;
        E->t_off[n] = v[k + 1].off, E->t_len[n] = v[k + 1].len;
        E->q_off[n] = v[k + 2].off, E->len[n] = v[k + 2].len;
        ++n;
        k += 3;
    }
    E->n = n;
}

static void free_entries(entries *E) {
    free(E->h_off), free(E->t_off), free(E->q_off), free(E->h_len), free(E->t_len), free(E->len);
}

/* ---- output: info \n target \n query \n \n (:109) of the kept entries, in runs */
typedef struct out_ctx {
    const char *buf;
    const entries *E;
    const int64_t *kept; /* entry of every kept one */
    int64_t n, per;
} out_ctx;

static void write_run(gac_obuf *o, int64_t r, void *arg) {
    const out_ctx *C = arg;
    const entries *E = C->E;
    const int64_t a = r * C->per, b = a + C->per < C->n ? a + C->per : C->n;
    size_t bytes = 0;
    for (int64_t k = a; k < b; ++k) {
        const int64_t i = C->kept[k];
        bytes += (size_t)E->h_len[i] + (size_t)E->t_len[i] + (size_t)E->len[i] + 4;
    }
    char *p = gac_obuf_reserve(o, bytes);
    if (!p)
        return;
    for (int64_t k = a; k < b; ++k) {
        const int64_t i = C->kept[k];
        memcpy(p, C->buf + E->h_off[i], (size_t)E->h_len[i]), p += E->h_len[i], *p++ = '\n';
        memcpy(p, C->buf + E->t_off[i], (size_t)E->t_len[i]), p += E->t_len[i], *p++ = '\n';
        memcpy(p, C->buf + E->q_off[i], (size_t)E->len[i]), p += E->len[i], *p++ = '\n';
        *p++ = '\n';
    }
    o->n += bytes;
}

/* ---- one run of the script */
typedef struct job {
    const char *in, *out;
    double min_ident, min_entropy;
    int32_t window;
    int device;
} job;

static int64_t file_bytes(const char *path) {
    struct stat st;
    return stat(path, &st) == 0 && S_ISREG(st.st_mode) ? (int64_t)st.st_size : -1;
}

/* argv: the five positional arguments */
static void parse_job(char *const *argv, int force, job *J) {
    char *end;
    J->in = argv[0], J->out = argv[4];
    J->min_ident = strtod(argv[1], &end);
    if (!*argv[1] || *end)
        gt_abort("minSeqIdent: '%s' is not a number", argv[1]);
    J->min_entropy = strtod(argv[2], &end);
    if (!*argv[2] || *end)
        gt_abort("minEntropy: '%s' is not a number", argv[2]);
    const long w = strtol(argv[3], &end, 10);
    if (!*argv[3] || *end)
        gt_abort("windowSize: '%s' is not an integer", argv[3]);
    if (w < 1 || w > INT32_MAX)
        gt_abort("windowSize %ld: at least 1 (no window of that size can be tested)", w);
    J->window = (int32_t)w;
    const int64_t bytes = file_bytes(J->in);
    J->device = force ? force > 0 : k_device_min_bytes >= 0 && bytes >= k_device_min_bytes;
}

/* last: no job after this one uses the device, which is then closed under the writing */
static void run_job(const job *J, gt_device *dev, gac_ctx **ctx, int last) {
    size_t size;
    char *buf = gt_slurp(J->in, &size);
    FILE *out = gt_must_open(J->out, "w");
    gt_stage("read input");
    int64_t nl;
    line *v = read_lines(buf, (int64_t)size, &nl);
    entries E;
    group_entries(buf, v, nl, J->in, &E);
    free(v);
    gt_stage("parse");

    uint8_t *keep = must_alloc((size_t)E.n);
    gac_axtfilter_stats st;
    char what[160];
    if (J->device) {
        if (!*ctx) {
            *ctx = gt_device_join(dev);
            gt_stage("device open (rest)");
        }
        gt_check(gac_axt_filter(*ctx, E.n, buf, (int64_t)size, E.t_off, E.q_off, E.len, J->min_ident,
                                J->min_entropy, J->window, keep, &st));
        snprintf(what, sizeof(what), "filter (GPU): %lld of %lld kept, %d batches%s", (long long)st.kept,
                 (long long)E.n, st.batches,
                 st.fell_back == 1   ? ", on the host (window over the device's)"
                 : st.fell_back == 2 ? ", some entries on the host (over the batch bytes)"
                                     : "");
    } else {
        gt_check(gac_axt_filter_host(E.n, buf, (int64_t)size, E.t_off, E.q_off, E.len, J->min_ident,
                                     J->min_entropy, J->window, gt_threads(), keep, &st));
        snprintf(what, sizeof(what), "filter (host): %lld of %lld kept", (long long)st.kept, (long long)E.n);
    }
    gt_stage(what);
    if (last && *ctx) {
        gt_device_close_async(dev, *ctx, NULL);
        *ctx = NULL;
    }

    int64_t *kept = must_alloc((size_t)st.kept * 8), nk = 0;
    for (int64_t i = 0; i < E.n; ++i)
        if (keep[i])
            kept[nk++] = i;
    out_ctx C = {buf, &E, kept, nk, 64};
    if (gac_par_output_buf(out, (nk + C.per - 1) / C.per, write_run, &C) != 0)
        gt_abort("write error on %s", J->out);
    gt_careful_close(out, J->out);
    free(kept);
    free(keep);
    free_entries(&E);
    free(buf);
    gt_stage("write output");
}

int main(int argc, char *argv[]) {
    gt_stage("");
    /* options apart from the positional arguments: a word that parses as a
     * number is positional, whatever it starts with */
    char **pos = must_alloc((size_t)(argc + 1) * sizeof(char *));
    char **opt = must_alloc((size_t)(argc + 1) * sizeof(char *));
    int npos = 0, nopt = 1;
    opt[0] = argv[0];
    for (int i = 1; i < argc; ++i) {
        if (argv[i][0] == '-' && argv[i][1] && !is_number(argv[i]))
            opt[nopt++] = argv[i];
        else
            pos[npos++] = argv[i];
    }
    opt[nopt] = NULL;
    gt_options(&nopt, opt, k_opts);
    const char *jobs_file = gt_opt_str("jobs", NULL);
    if (gt_opt_exists("host") && gt_opt_exists("device"))
        gt_abort("-host and -device exclude each other");
    const int force = gt_opt_exists("host") ? -1 : gt_opt_exists("device") ? 1 : 0;
    if (jobs_file ? npos != 0 : npos != 5)
        usage();

    job *J = NULL;
    int64_t nj = 0;
    if (!jobs_file) {
        J = must_alloc(sizeof(job));
        parse_job(pos, force, &J[nj++]);
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
            if (wc != 5)
                gt_abort("%s: job %lld: five arguments expected (input.axt minSeqIdent minEntropy "
                         "windowSize output.axt)", jobs_file, (long long)nj + 1);
            if (nj == cap) {
                cap = cap ? cap * 2 : 64;
                J = realloc(J, (size_t)cap * sizeof(job));
                if (!J)
                    gt_abort("Out of memory");
            }
            parse_job(w, force, &J[nj++]);
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
