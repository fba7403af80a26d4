/* netSyntenic -- add synteny info (qDup, type, qOver, qFar) to a net, on an
 * MI355X.
 *
 * Drop-in for the reference's kent/src/hg/mouseStuff/netSyntenic/netSyntenic.c
 * (+ chainNetRead / chainNetWrite of kent/src/hg/lib/chainNet.c:86-264): same
 * command line and output; "stdin" and "stdout" are accepted as file names.
 *
 * The reference adds every fill's query range to (and takes every gap's from)
 * a red-black tree of depth runs per query sequence, one range at a time, and
 * then asks the tree for each fill's bases under a depth of two or more.  Here
 * that is one call on all ranges at once (gac_depth_count: sort the range
 * ends, scan the depth, scan the covered lengths), while reading, typing and
 * writing the lines is per-line work for all host threads (lib/gac_netfile.c).
 *
 * '#' lines that start in column 0 go first, in input order: the reference's
 * reader copies them as it meets them, and it reads every net before it writes
 * one (:281-303).  Its "memory usage" line on stderr is not reproduced.
 *
 * One extension: -host counts the depth on the CPU (gac_depth_count_host) and
 * never opens a device.  Without it the device is opened while the file is
 * read and parsed; no device is an error.
 *
 * A record whose query range is negative is refused (the reference hands it
 * to its tree as it is). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_netfile.h"
#include "gac_tool.h"
#include "gachain.h"

static const gt_spec k_opts[] = {{"host", GT_BOOL}, {NULL, 0}};

static void usage(void) {
    gt_abort("netSyntenic - Add synteny info to net.\n"
             "usage:\n"
             "   netSyntenic in.net out.net\n"
             "options:\n"
             "   -xxx=XXX\n"
             "   -host - count the coverage depth on the CPU; no GPU is opened\n");
}

static void *must_alloc(size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p)
        gt_abort("Out of memory");
    return p;
}

int main(int argc, char *argv[]) {
    gt_stage("");
    gt_options(&argc, argv, k_opts);
    if (argc != 3)
        usage();
    const int host = gt_opt_exists("host");
    gt_device dev;
    if (!host)
        gt_device_start_bare(&dev);
    FILE *out = gt_must_open(argv[2], "w"); /* (before the input is read, as there) */
    gt_stage("options + setup");

    gt_lines nl;
    gt_lines_read(argv[1], &nl);
    gt_nnetset ns;
    gt_nnet_parse(&nl, argv[1], &ns);
    gt_stage("read + parse net");

    /* rCalcDupes (:184-209): every record of the trees, fills +1, gaps -1 */
    const int64_t n = ns.n_order;
    int32_t *seq = must_alloc((size_t)n * 4), *start = must_alloc((size_t)n * 4);
    int32_t *end = must_alloc((size_t)n * 4), *qdup = must_alloc((size_t)n * 4);
    int8_t *delta = must_alloc((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const gt_nfill *f = &ns.fills[ns.order[k]];
        const int64_t e = (int64_t)f->qstart + f->qsize;
        if (f->qstart < 0 || f->qsize < 0 || e > INT32_MAX)
            gt_abort("Query range %d size %d out of bounds line %d of %s", f->qstart, f->qsize,
                     ns.order[k] + 1, argv[1]);
        seq[k] = f->qname;
        start[k] = f->qstart;
        end[k] = (int32_t)e;
        delta[k] = f->chain_id ? 1 : -1;
    }
    gt_stage("depth rows");
    gac_ctx *ctx = NULL;
    if (host) {
        gt_check(gac_depth_count_host(n, seq, start, end, delta, 2, qdup));
        gt_stage("depth count (host)");
    } else {
        ctx = gt_device_join(&dev);
        gt_stage("device open (rest)");
        gt_check(gac_depth_count(ctx, n, seq, start, end, delta, 2, qdup));
        gt_stage("depth count (GPU)");
        gt_device_close_async(&dev, ctx, NULL); /* overlaps the writing */
    }
    free(seq);
    free(start);
    free(end);
    free(delta);

    setvbuf(out, NULL, _IOFBF, 1 << 20);
    for (int64_t i = 0; i < nl.n; ++i)
        if (nl.line[i][0] == '#')
            fprintf(out, "%s\n", nl.line[i]);
    gt_nnet_write_typed(out, &ns, qdup);
    gt_careful_close(out, argv[2]);
    gt_stage("format + write");
    if (!host) {
        gt_device_close_join(&dev);
        gt_stage("device close (rest)");
    }
    gt_exit_ok();
}
