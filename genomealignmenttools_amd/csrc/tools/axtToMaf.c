/* axtToMaf -- native drop-in for the reference's
 * kent/src/hg/mouseStuff/axtToMaf/axtToMaf.c, the last step from a net to a
 * MAF (netToAxt ... | axtSort | axtToMaf): every axt record as one MAF block.
 *
 *   axtToMaf in.axt tSizes qSizes out.maf [-qPrefix= -tPrefix= -tSplit -score -scoreZero]
 *
 * Reading is axtRead's over lineFile's lines (tools/lib/gac_axtin.c, shared
 * with axtToPsl and axtSort); the 9th word of a header is the score, 0 without
 * one.  The sizes files are loadIntHash's: two columns, the last line of a
 * name counts, a name that is missing aborts.
 *
 * The output is mafWrite's (kent/src/lib/maf.c:281-361): the line
 * "##maf version=1 scoring=blastz", then for every record "a score=%f", the
 * target's "s" line, the query's "s" line and a blank line; the name, start,
 * size and source size columns are as wide as the wider of the record's two
 * values (digitsBaseTen counts a minus sign), and a prefixed name equal to "."
 * becomes "defaultName".  Every input line that starts with '#' -- wherever it
 * stands, a record's rows and fourth line included -- is copied to the output
 * before the block of the record it was read for, those after the last record
 * at the end (lineFileSetMetaDataOutput); with -tSplit they go nowhere.
 *
 * -score replaces every record's score by axtScoreDnaDefault of its rows,
 * -scoreZero those that are 0: one gac_axt_score or
 * gac_axt_score_host call over just those records.  Without either option no
 * scoring call is made and no device is opened.
 *
 * -tSplit makes out a directory with one <tName>.maf per run of equal target
 * names and aborts with the reference's message when a name comes back.
 *
 * Where the reference aborts -- a bad header, rows of unequal length, a file
 * that ends inside a record, a missing name, a prefixed name of 256 bytes or
 * more, an unsorted input under -tSplit -- this tool aborts with a message and
 * status 255 before it writes anything (the reference has written the records
 * before the bad one by then).  Another number of arguments prints the
 * reference's usage and exits 255.  Extensions:
 *   -host, -device   force the scoring path.  The default is the host path at
 *                    every size: see k_device_min_bytes.
 *   -jobs=FILE       run every line of FILE (the four arguments, white space
 *                    between them, no quoting; blank and '#' lines skipped)
 *                    with this command line's options in this process, with
 *                    one device context for all of them.
 *   -verbose=2       stage laps. */
#define _GNU_SOURCE
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "gac_axtin.h"
#include "gac_tool.h"
#include "gachain.h"
#include "host/gac_host.h"

/* Inputs of at least this many bytes take the device path for -score and
 * -scoreZero by default; < 0: none does.  The project's rule: the smallest
 * size at which the device path, its bring-up included, takes at most 0.8 of
 * the host path's time (scripts/axtmaf_profile.sh). */
static const int64_t k_device_min_bytes = -1;

static const gt_spec k_opts[] = {
    {"qPrefix", GT_STRING}, {"tPrefix", GT_STRING}, {"tSplit", GT_BOOL}, {"score", GT_BOOL},
    {"scoreZero", GT_BOOL}, {"host", GT_BOOL},      {"device", GT_BOOL}, {"jobs", GT_STRING},
    {NULL, 0},
};

static void usage(void) {
    gt_abort("axtToMaf - Convert from axt to maf format\n"
             "usage:\n"
             "   axtToMaf in.axt tSizes qSizes out.maf\n"
             "Where tSizes and qSizes is a file that contains\n"
             "the sizes of the target and query sequences.\n"
             "Very often this with be a chrom.sizes file\n"
             "Options:\n"
             "    -qPrefix=XX. - add XX. to start of query sequence name in maf\n"
             "    -tPrefex=YY. - add YY. to start of target sequence name in maf\n"
             "    -tSplit Create a separate maf file for each target sequence.\n"
             "            In this case output is a dir rather than a file\n"
             "            In this case in.maf must be sorted by target.\n"
             "    -score       - recalculate score \n"
             "    -scoreZero   - recalculate score if zero \n");
}

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

typedef struct opts {
    const char *q_prefix, *t_prefix;
    size_t q_prefix_len, t_prefix_len;
    int t_split, score, score_zero;
} opts;

/* digitsBaseTen (obscure.c:53) */
static int digits(int32_t x) {
    int n = 1;
    uint32_t u = (uint32_t)x;
    if (x < 0)
        n = 2, u = 0u - u;
    for (; u >= 10; u /= 10)
        ++n;
    return n;
}

/* ---- output */
typedef struct out_ctx {
    const char *buf;
    const gt_axt_line *v;
    int64_t nl;
    const gt_axt_records *R;
    const gt_axt_sizes *T, *Q;
    const opts *O;
    const int32_t *score;
    int64_t first, end; /* the records of this file */
    int64_t per;
    int meta; /* copy the '#' lines */
} out_ctx;

static void put_bytes(gac_obuf *o, const char *p, size_t n) {
    memcpy(gac_obuf_reserve(o, n), p, n);
    o->n += n;
}

static void put_meta(gac_obuf *o, const out_ctx *C, int64_t lo, int64_t hi) {
    for (int64_t k = lo; k < hi; ++k)
        if (C->v[k].len > 0 && C->buf[C->v[k].off] == '#') {
            put_bytes(o, C->buf + C->v[k].off, (size_t)C->v[k].len);
            put_bytes(o, "\n", 1);
        }
}

/* a component's name: the prefix and the name, "defaultName" for "." */
static int src_name(char *dst, const char *prefix, size_t plen, const char *name, size_t nlen) {
    memcpy(dst, prefix, plen);
    memcpy(dst + plen, name, nlen);
    size_t n = plen + nlen;
    if (n == 1 && dst[0] == '.') {
        memcpy(dst, "defaultName", 11);
        n = 11;
    }
    dst[n] = 0;
    return (int)n;
}

static void put_record(gac_obuf *o, const out_ctx *C, int64_t i) {
    const gt_axt_records *R = C->R;
    char tn[256], qn[256];
    const int tl = src_name(tn, C->O->t_prefix, C->O->t_prefix_len, C->buf + R->tn_off[i], (size_t)R->tn_len[i]);
    const int ql = src_name(qn, C->O->q_prefix, C->O->q_prefix_len, C->buf + R->qn_off[i], (size_t)R->qn_len[i]);
    const int32_t tstart = R->tstart[i], qstart = R->qstart[i];
    const int32_t tsize = (int32_t)((uint32_t)R->tend[i] - (uint32_t)tstart);
    const int32_t qsize = (int32_t)((uint32_t)R->qend[i] - (uint32_t)qstart);
    const int32_t tsrc = C->T->size[R->tname[i]], qsrc = C->Q->size[R->qname[i]];
    const int w_src = tl > ql ? tl : ql;
    const int w_start = digits(tstart) > digits(qstart) ? digits(tstart) : digits(qstart);
    const int w_size = digits(tsize) > digits(qsize) ? digits(tsize) : digits(qsize);
    const int w_srcsize = digits(tsrc) > digits(qsrc) ? digits(tsrc) : digits(qsrc);
    const size_t L = (size_t)R->len[i];
    gac_obuf_printf(o, "a score=%f\ns %-*s %*d %*d + %*d ", (double)C->score[i], w_src, tn, w_start, tstart, w_size,
                    tsize, w_srcsize, tsrc);
    put_bytes(o, C->buf + R->t_off[i], L);
    gac_obuf_printf(o, "\ns %-*s %*d %*d %c %*d ", w_src, qn, w_start, qstart, w_size, qsize, R->strand[i],
                    w_srcsize, qsrc);
    put_bytes(o, C->buf + R->q_off[i], L);
    put_bytes(o, "\n\n", 2);
}

/* run r: records [first + r * per, ...); the first run starts the file and the
 * last one ends it */
static void write_run(gac_obuf *o, int64_t r, void *arg) {
    const out_ctx *C = arg;
    const gt_axt_records *R = C->R;
    const int64_t a = C->first + r * C->per, b = a + C->per < C->end ? a + C->per : C->end;
    if (r == 0)
        put_bytes(o, "##maf version=1 scoring=blastz\n", 31);
    for (int64_t i = a; i < b; ++i) {
        if (C->meta) /* what was read for this record, its own lines included */
            put_meta(o, C, R->line0[i], R->line0[i + 1]);
        put_record(o, C, i);
    }
    if (C->meta && b == C->end) /* the lines after the last record */
        put_meta(o, C, R->line0[R->n], C->nl);
}

static void write_file(const char *path, out_ctx *C) {
    FILE *out = gt_must_open(path, "w");
    const int64_t n = C->end - C->first;
    if (n == 0) {
        gac_obuf o = {NULL, 0, 0};
        put_bytes(&o, "##maf version=1 scoring=blastz\n", 31);
        if (C->meta)
            put_meta(&o, C, 0, C->nl);
        if (fwrite(o.p, 1, o.n, out) != o.n)
            gt_abort("write error on %s", path);
        free(o.p);
    } else if (gac_par_output_buf(out, (n + C->per - 1) / C->per, write_run, C) != 0)
        gt_abort("write error on %s", path);
    gt_careful_close(out, path);
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

static void set_job(char *const *argv, int force, const opts *O, job *J) {
    J->in = argv[0], J->tsizes = argv[1], J->qsizes = argv[2], J->out = argv[3];
    const int64_t bytes = file_bytes(J->in);
    J->device = force ? force > 0 : k_device_min_bytes >= 0 && bytes >= k_device_min_bytes;
    if (!O->score && !O->score_zero)
        J->device = 0; /* nothing to score */
}

static int same_name(const char *buf, const gt_axt_records *R, int64_t a, int64_t b) {
    return R->tn_len[a] == R->tn_len[b] && memcmp(buf + R->tn_off[a], buf + R->tn_off[b], (size_t)R->tn_len[a]) == 0;
}

/* last: no job after this one uses the device, which is then closed under the writing */
static void run_job(const job *J, const opts *O, gt_device *dev, gac_ctx **ctx, int last) {
    gt_axt_sizes T, Q;
    gt_axt_read_sizes(J->tsizes, &T);
    gt_axt_read_sizes(J->qsizes, &Q);
    size_t size;
    char *buf = gt_slurp(J->in, &size);
    gt_stage("read input");
    int64_t nl;
    gt_axt_line *v = gt_axt_lines(buf, (int64_t)size, &nl);
    gt_axt_records R;
    memset(&R, 0, sizeof(R));
    gt_axt_group(buf, v, nl, J->in, &R);
    gt_axt_parse_heads(buf, &R, &T, &Q, J->in);
    for (int64_t i = 0; i < R.n; ++i) /* safef(srcName, 256, ...) */
        if (O->q_prefix_len + (size_t)R.qn_len[i] >= 256 || O->t_prefix_len + (size_t)R.tn_len[i] >= 256)
            gt_abort("buffer overflow, size 256, format: %%s%%s (record %lld of %s)", (long long)i + 1, J->in);
    /* -tSplit: the runs of equal target names; a name that comes back aborts */
    int64_t *run0 = NULL, nruns = 0;
    if (O->t_split) {
        run0 = must_alloc((size_t)(R.n + 1) * 8);
        gt_names seen;
        memset(&seen, 0, sizeof(seen));
        for (int64_t i = 0; i < R.n; ++i) {
            if (i > 0 && same_name(buf, &R, i - 1, i))
                continue;
            const int32_t before = seen.n;
            if (gt_names_add(&seen, buf + R.tn_off[i], (size_t)R.tn_len[i]) < before)
                gt_abort("%s isn't sorted, which is necessary when -tSplit option is used", J->in);
            if (strlen(J->out) + (size_t)R.tn_len[i] + 6 > 512)
                gt_abort("buffer overflow, size 512, format: %%s/%%s.maf");
            run0[nruns++] = i;
        }
        run0[nruns] = R.n;
        gt_names_free(&seen);
    }
    gt_stage("parse");

    /* the scores: the headers', or the rows' for the records the options name */
    int32_t *score = R.score;
    if (O->score || O->score_zero) {
        int64_t m = 0;
        int64_t *idx = must_alloc((size_t)R.n * 8);
        for (int64_t i = 0; i < R.n; ++i)
            if (O->score || R.score[i] == 0)
                idx[m++] = i;
        int64_t *t_off = R.t_off, *q_off = R.q_off;
        int32_t *len = R.len, *sc = score;
        if (m != R.n) {
            t_off = must_alloc((size_t)m * 8), q_off = must_alloc((size_t)m * 8);
            len = must_alloc((size_t)m * 4), sc = must_alloc((size_t)m * 4);
            for (int64_t k = 0; k < m; ++k)
                t_off[k] = R.t_off[idx[k]], q_off[k] = R.q_off[idx[k]], len[k] = R.len[idx[k]];
        }
        gac_axtscore_stats st;
        char what[160];
        if (J->device) {
            if (!*ctx) {
                *ctx = gt_device_join(dev);
                gt_stage("device open (rest)");
            }
            gt_check(gac_axt_score(*ctx, m, buf, (int64_t)size, t_off, q_off, len, sc, &st));
            snprintf(what, sizeof(what), "score (GPU): %lld of %lld records, %lld columns, %d batches%s", (long long)m,
                     (long long)R.n, (long long)st.columns, st.batches,
                     st.fell_back == 2 ? ", some records on the host (over the batch bytes)" : "");
        } else {
            gt_check(gac_axt_score_host(m, buf, (int64_t)size, t_off, q_off, len, gt_threads(), sc, &st));
            snprintf(what, sizeof(what), "score (host): %lld of %lld records, %lld columns", (long long)m,
                     (long long)R.n, (long long)st.columns);
        }
        if (m != R.n) {
            for (int64_t k = 0; k < m; ++k)
                score[idx[k]] = sc[k];
            free(t_off), free(q_off), free(len), free(sc);
        }
        free(idx);
        gt_stage(what);
    }
    if (last && *ctx) {
        gt_device_close_async(dev, *ctx, NULL);
        *ctx = NULL;
    }

    /* (every record is checked by now) */
    out_ctx C = {buf, v, nl, &R, &T, &Q, O, score, 0, R.n, 64, !O->t_split};
    if (!O->t_split) {
        write_file(J->out, &C);
    } else {
        if (mkdir(J->out, 0777) != 0 && errno != EEXIST) /* makeDir (osunix.c) */
            gt_abort("Couldn't make directory %s", J->out);
        for (int64_t r = 0; r < nruns; ++r) {
            char path[600];
            snprintf(path, sizeof(path), "%s/%.*s.maf", J->out, R.tn_len[run0[r]], buf + R.tn_off[run0[r]]);
            C.first = run0[r], C.end = run0[r + 1];
            write_file(path, &C);
        }
        free(run0);
    }
    free(v);
    gt_axt_free_records(&R);
    free(buf);
    gt_axt_free_sizes(&T);
    gt_axt_free_sizes(&Q);
    gt_stage("write output");
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options(&argc, argv, k_opts);
    const char *jobs_file = gt_opt_str("jobs", NULL);
    if (gt_opt_exists("host") && gt_opt_exists("device"))
        gt_abort("-host and -device exclude each other");
    const int force = gt_opt_exists("host") ? -1 : gt_opt_exists("device") ? 1 : 0;
    if (jobs_file ? argc != 1 : argc != 5)
        usage();
    opts O;
    O.q_prefix = gt_opt_str("qPrefix", ""), O.t_prefix = gt_opt_str("tPrefix", "");
    O.q_prefix_len = strlen(O.q_prefix), O.t_prefix_len = strlen(O.t_prefix);
    O.t_split = gt_opt_exists("tSplit"), O.score = gt_opt_exists("score"), O.score_zero = gt_opt_exists("scoreZero");

    job *J = NULL;
    int64_t nj = 0;
    if (!jobs_file) {
        J = must_alloc(sizeof(job));
        set_job(argv + 1, force, &O, &J[nj++]);
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
                gt_abort("%s: job %lld: four arguments expected (in.axt tSizes qSizes out.maf)", jobs_file,
                         (long long)nj + 1);
            if (nj == cap) {
                cap = cap ? cap * 2 : 64;
                J = realloc(J, (size_t)cap * sizeof(job));
                if (!J)
                    gt_abort("Out of memory");
            }
            set_job(w, force, &O, &J[nj++]);
        }
    }
    int any_device = 0;
    int64_t last_device = -1;
    for (int64_t k = 0; k < nj; ++k)
        if (J[k].device)
            any_device = 1, last_device = k;
    gt_device dev;
    gac_ctx *ctx = NULL;
    if (any_device)
        gt_device_start_bare(&dev); /* opens while the first input is read and parsed */
    gt_stage("options + setup");
    for (int64_t k = 0; k < nj; ++k)
        run_job(&J[k], &O, &dev, &ctx, k >= last_device);
    if (nj > 1)
        gt_verbose(2, "%lld jobs%s\n", (long long)nj, any_device ? " in one device context" : "");
    if (any_device) {
        gt_device_close_join(&dev);
        gt_stage("device close (rest)");
    }
    gt_exit_ok();
}
