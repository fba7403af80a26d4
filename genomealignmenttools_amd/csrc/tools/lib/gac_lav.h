/* gac_lav.h -- the .lav reader shared by lavToAxt and lavToPsl
 * (kent/src/hg/lib/lav.c and the two tools' parseA / parseInto* loops,
 * kent/src/hg/mouseStuff/lavToAxt/lavToAxt.c:320-368,425-488,
 * lavToPsl/lavToPsl.c:126-219).  Host only. */
#ifndef GAC_LAV_H
#define GAC_LAV_H

#include "gac_tool.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gl_block {
    int32_t t_start, t_end, q_start, q_end, pct; /* zero-based half-open; percentId */
} gl_block;

/* A pull reader: gl_next reads up to the end of the next 'a' stanza.  What
 * the stanzas before it set (names, sizes, isRc) is in the reader; a 'd'
 * stanza's header lines are written to `out` as they are met. */
typedef struct gl_reader {
    const char *path;
    char *buf, *cur;
    int line; /* lines read so far (lf->lineIx) */
    FILE *out;
    /* lavToPsl: zero-length blocks are dropped while reading, a missing score
     * is no error, the 's' line takes exactly two words, and every 's' line
     * is echoed to score_file (may be NULL) */
    int psl;
    FILE *score_file;
    /* state */
    char *t_name, *q_name; /* NULL before the first 'h' stanza */
    int32_t t_size, q_size;
    int is_rc;
    /* the stanza gl_next returned: blocks [0, nb) after removeFrayedEnds */
    gl_block *blk;
    int64_t nb, cap;
    gl_block *blk_base;
    int32_t score;
} gl_reader;

/* opens path (".gz" and "stdin" as gt_slurp) and checks the "#:lav" header */
void gl_open(gl_reader *r, const char *path, FILE *out, int psl, FILE *score_file);
int gl_next(gl_reader *r); /* 1: an 'a' stanza (maybe without blocks); 0: end of file */
void gl_close(gl_reader *r);

/* removeFrayedEnds (lav.c:132-163) on blocks [0, *n): a zero-length first
 * block and then a zero-length last block are dropped, each once; returns the
 * new first block */
gl_block *gl_remove_frayed(gl_block *b, int64_t *n);

#ifdef __cplusplus
}
#endif
#endif
