/* axtSort -- sort axt files (drop-in for kent/src/hg/mouseStuff/axtSort).
 *
 *   axtSort in.axt out.axt [-query] [-byScore]
 *
 * Same command line and output bytes as the reference (axtSort.c:24-57): every
 * record is read (axtRead, kent/src/lib/axt.c:52-92; the shared reader of
 * tools/lib/gac_axtin.c), the list is reversed by slAddHead and slSort'ed --
 * a stable merge sort -- with axtCmpTarget (strcmp of tName, then tStart),
 * with -query axtCmpQuery (qName, qStart), with -byScore, which wins over
 * -query, axtCmpScore (score, descending) (axt.c:122-152); so records that
 * compare equal come out in the reverse of their input order.  Any option is
 * accepted, as optionHash does.  Every input line that starts with '#' comes
 * first, in input order (lineFileSetMetaDataOutput writes them while the file
 * is read); then axtWrite's records (axt.c:101-120): the running number from
 * 0, the score always written (0 for a header of 8 words), a blank line after
 * each.
 *
 * The reference compares starts and scores by the sign of an int difference;
 * here they are compared as numbers, which is the same wherever that
 * difference fits an int (beyond it the reference's subtraction overflows).
 *
 * The records stay in the input buffer: an index is sorted by the keys, with
 * the input position as the last key, and the text is formatted on all
 * threads (gac_par_output_buf).  Where the reference aborts, this tool aborts
 * with status 255 before it writes anything. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gac_axtin.h"
#include "gac_tool.h"
#include "host/gac_host.h"

static void usage(void) {
    gt_abort("axtSort - Sort axt files\n"
             "usage:\n"
             "   axtSort in.axt out.axt\n"
             "options:\n"
             "   -query - Sort by query position, not target\n"
             "   -byScore - Sort by score\n");
}

enum { BY_TARGET, BY_QUERY, BY_SCORE };

typedef struct sort_ctx {
    const char *buf;
    const gt_axt_records *R;
    int mode;
} sort_ctx;

static const sort_ctx *g_sc;

/* strcmp of two names that are slices of the input */
static int cmp_name(const char *a, int32_t al, const char *b, int32_t bl) {
    const int d = memcmp(a, b, (size_t)(al < bl ? al : bl));
    return d ? d : (al > bl) - (al < bl);
}

/* axtCmpTarget / axtCmpQuery / axtCmpScore, then the list position (slSort is
 * stable, and slAddHead put later records first) */
static int cmp_axt(const void *va, const void *vb) {
    const int64_t a = *(const int64_t *)va, b = *(const int64_t *)vb;
    const gt_axt_records *R = g_sc->R;
    const char *buf = g_sc->buf;
    int d;
    if (g_sc->mode == BY_SCORE) {
        d = (R->score[b] > R->score[a]) - (R->score[b] < R->score[a]);
    } else if (g_sc->mode == BY_TARGET) {
        d = cmp_name(buf + R->tn_off[a], R->tn_len[a], buf + R->tn_off[b], R->tn_len[b]);
        if (d == 0)
            d = (R->tstart[a] > R->tstart[b]) - (R->tstart[a] < R->tstart[b]);
    } else {
        d = cmp_name(buf + R->qn_off[a], R->qn_len[a], buf + R->qn_off[b], R->qn_len[b]);
        if (d == 0)
            d = (R->qstart[a] > R->qstart[b]) - (R->qstart[a] < R->qstart[b]);
    }
    if (d)
        return d;
    return (a < b) - (a > b);
}

typedef struct out_ctx {
    const char *buf;
    const gt_axt_line *v;
    int64_t nl;
    const gt_axt_records *R;
    const int64_t *ord;
    int64_t per;
} out_ctx;

static void put_bytes(gac_obuf *o, const char *p, size_t n) {
    memcpy(gac_obuf_reserve(o, n), p, n);
    o->n += n;
}

static void put_meta(gac_obuf *o, const out_ctx *C) {
    for (int64_t k = 0; k < C->nl; ++k)
        if (C->v[k].len > 0 && C->buf[C->v[k].off] == '#') {
            put_bytes(o, C->buf + C->v[k].off, (size_t)C->v[k].len);
            put_bytes(o, "\n", 1);
        }
}

static void write_run(gac_obuf *o, int64_t r, void *arg) {
    const out_ctx *C = arg;
    const gt_axt_records *R = C->R;
    const int64_t a = r * C->per, b = a + C->per < R->n ? a + C->per : R->n;
    if (r == 0)
        put_meta(o, C);
    for (int64_t k = a; k < b; ++k) {
        const int64_t i = C->ord[k];
        gac_obuf_printf(o, "%d %.*s %d %d %.*s %d %d %c %d\n", (int)k, R->tn_len[i], C->buf + R->tn_off[i],
                        (int32_t)((uint32_t)R->tstart[i] + 1u), R->tend[i], R->qn_len[i], C->buf + R->qn_off[i],
                        (int32_t)((uint32_t)R->qstart[i] + 1u), R->qend[i], R->strand[i], R->score[i]);
        put_bytes(o, C->buf + R->t_off[i], (size_t)R->len[i]);
        put_bytes(o, "\n", 1);
        put_bytes(o, C->buf + R->q_off[i], (size_t)R->len[i]);
        put_bytes(o, "\n\n", 2);
    }
}

int main(int argc, char *argv[]) {
    gt_options_hash(&argc, argv);
    if (argc != 3)
        usage();
    const char *in = argv[1], *out = argv[2];
    const int mode = gt_opt_exists("byScore") ? BY_SCORE : gt_opt_exists("query") ? BY_QUERY : BY_TARGET;
    size_t size;
    char *buf = gt_slurp(in, &size);
    int64_t nl;
    gt_axt_line *v = gt_axt_lines(buf, (int64_t)size, &nl);
    gt_axt_records R;
    memset(&R, 0, sizeof(R));
    gt_axt_group(buf, v, nl, in, &R);
    gt_axt_parse_heads(buf, &R, NULL, NULL, in);
    int64_t *ord = malloc((size_t)(R.n ? R.n : 1) * 8);
    if (!ord)
        gt_abort("Out of memory");
    for (int64_t k = 0; k < R.n; ++k)
        ord[k] = k;
    sort_ctx sc = {buf, &R, mode};
    g_sc = &sc;
    qsort(ord, (size_t)R.n, 8, cmp_axt);

    FILE *f = gt_must_open(out, "w"); /* (every record is checked by now) */
    out_ctx C = {buf, v, nl, &R, ord, 64};
    if (R.n == 0) {
        gac_obuf o = {NULL, 0, 0};
        put_meta(&o, &C);
        if (o.n && fwrite(o.p, 1, o.n, f) != o.n)
            gt_abort("write error on %s", out);
        free(o.p);
    } else if (gac_par_output_buf(f, (R.n + C.per - 1) / C.per, write_run, &C) != 0)
        gt_abort("write error on %s", out);
    gt_careful_close(f, out);
    free(ord);
    free(v);
    gt_axt_free_records(&R);
    free(buf);
    gt_exit_ok();
}
