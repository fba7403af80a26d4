/* gac_axtin.h -- the axt reader axtToPsl, axtToMaf and axtSort share: lines
 * as lineFileNext returns them, records as axtRead groups them
 * (kent/src/lib/axt.c:52-92), their headers on all threads, and two-column
 * sizes files with kent's duplicate-name rule.  Everything stays in the
 * slurped input: a record is offsets into it. */
#ifndef GAC_AXTIN_H
#define GAC_AXTIN_H

#include <stdint.h>

#include "gac_tool.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lines: the first '\n' or '\r' of a file decides whether its lines end
 * with '\n', with '\r\n' or with '\r' (determineNlType, linefile.c:425) */
typedef struct gt_axt_line {
    int64_t off;
    int32_t len, pad;
} gt_axt_line;
gt_axt_line *gt_axt_lines(const char *buf, int64_t size, int64_t *n_out);

/* chopByWhite (common.c:2029): up to max words of a line; returns the count */
typedef struct gt_axt_word {
    const char *p;
    int32_t len;
} gt_axt_word;
int gt_axt_chop(const char *p, int32_t len, gt_axt_word *w, int max);
/* lineFileNeedNum (linefile.c:1015): a '-' or a digit first, then atoi */
int gt_axt_need_num(gt_axt_word w, int32_t *v);
/* lineFileChopNext's line test: not a '#' line and not blank */
int gt_axt_has_words(const char *buf, gt_axt_line ln);

/* ---- sizes: lineFileRow with two columns; hashAdd puts the newest first, so
 * the last line of a name counts */
typedef struct gt_axt_sizes {
    gt_names names;
    int32_t *size;
    int32_t cap;
} gt_axt_sizes;
void gt_axt_read_sizes(const char *path, gt_axt_sizes *S);
void gt_axt_free_sizes(gt_axt_sizes *S);
int32_t gt_axt_find_name(const gt_axt_sizes *S, gt_axt_word w); /* index or -1 */

/* ---- records */
typedef struct gt_axt_records {
    int64_t n;
    int64_t *h_off, *t_off, *q_off;
    int32_t *h_len, *len;
    /* [n + 1] line0[i]: the first line read for record i, so that record i
     * took lines [line0[i], line0[i + 1]) -- the blank and '#' lines before its
     * header, the header, the rows and the line after them -- and line0[n] is
     * the first line after the last record */
    int64_t *line0;
    /* from the headers, on all threads */
    int32_t *tname, *qname; /* index into the sizes' names (-1 without sizes) */
    int32_t *tstart, *tend, *qstart, *qend;
    int32_t *score;           /* the 9th word, 0 without one */
    int64_t *tn_off, *qn_off; /* the names in the text */
    int32_t *tn_len, *qn_len;
    char *strand;
} gt_axt_records;
/* aborts on a file that ends inside a record or on rows of unequal length */
void gt_axt_group(const char *buf, const gt_axt_line *v, int64_t nl, const char *path, gt_axt_records *R);
/* aborts on the first bad header in file order: fewer than 8 words, a word that
 * is no number, a name missing from T or Q (NULL: names are not looked up) */
void gt_axt_parse_heads(const char *buf, gt_axt_records *R, const gt_axt_sizes *T, const gt_axt_sizes *Q,
                        const char *path);
void gt_axt_free_records(gt_axt_records *R);

#ifdef __cplusplus
}
#endif
#endif
