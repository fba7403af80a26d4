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
 * The reader is tools/lib/gac_axtin.c, shared with axtToMaf and axtSort.  It is
 * not the filter's: filterAxtIdentityEntropy.py reads as
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

#include "gac_axtin.h"
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

/* ---- output: pslTabOut of every record that is not empty after the trim, in runs */
typedef struct out_ctx {
    const char *buf;
    const gt_axt_records *R;
    const gt_axt_sizes *T, *Q;
    const gac_axtpsl_result *res;
    int64_t per;
} out_ctx;

static void write_run(gac_obuf *o, int64_t r, void *arg) {
    const out_ctx *C = arg;
    const gt_axt_records *R = C->R;
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
    free(v);
    gt_axt_parse_heads(buf, &R, &T, &Q, J->in);
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
    gt_axt_free_records(&R);
    free(buf);
    gt_axt_free_sizes(&T);
    gt_axt_free_sizes(&Q);
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
