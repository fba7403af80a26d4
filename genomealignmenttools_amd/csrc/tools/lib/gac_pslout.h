/* gac_pslout.h -- the PSL line of a chain, shared by chainToPsl and
 * chainToPslBasic (kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c:130-176 and
 * pslTabOut, kent/src/lib/psl.c:175-254: the same 21 tab-separated columns),
 * and the PSL line of an alignment's rows (axtToPsl). */
#ifndef GAC_PSLOUT_H
#define GAC_PSLOUT_H

#include "gac_tool.h"
#include "host/gac_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One line for chain i of c: counts[4] = match, misMatch, repMatch, nCount;
 * the insert columns are counted here over adjacent blocks, where the next
 * block's start differs from the previous block's end (chainToPsl.c:81-93)
 * or, with basic, where it is greater (chainToPslBasic.c:36-48).  basic also
 * prints the unsigned columns as pslOutput does ("%u"); chainToPsl prints
 * every number "%d".  For '-' qStart / qEnd are flipped with the header's
 * qSize; qStarts are the chain's own strand coordinates. */
void gt_write_psl(FILE *f, const gt_chains *c, int64_t i, const int64_t counts[4], int basic);
/* The same with the two rules apart (lavToPsl prints as pslTabOut does, basic,
 * but counts an insert wherever two blocks do not abut, ins_ne), and with a
 * target strand character after the query's (0: none). */
void gt_write_psl_ex(FILE *f, const gt_chains *c, int64_t i, const int64_t counts[4], int basic,
                     int ins_ne, char t_strand);

/* An axt record's header for gt_put_psl_align: the strand character, the
 * names as they stand in the text, the sizes, and the coordinates as axtRead
 * leaves them (starts zero-based, the query's on its own strand). */
typedef struct gt_psl_align {
    char strand;
    const char *qname, *tname;
    size_t qname_len, tname_len;
    int32_t qsize, tsize, qstart, qend, tstart, tend;
} gt_psl_align;

/* pslTabOut of pslFromAlign's psl (kent/src/lib/psl.c:1716-1806), appended to
 * o, from what gac_axt_psl returns for the record's rows (e, and blk = its
 * blocks) with the reference's arithmetic: qStart / qEnd flipped to the plus
 * strand for '-' (axtToPsl.c:74), moved by the trim in those coordinates,
 * nothing appended (and 0 returned) when qStart == qEnd or tStart == tEnd
 * after it, qStarts from the flipped-back qStart.  The numbers are the
 * reference's 32-bit ints, printed "%u" except the two base-insert columns. */
int gt_put_psl_align(gac_obuf *o, const gt_psl_align *a, const gac_axtpsl_entry *e,
                     const gac_axtpsl_block *blk);

#ifdef __cplusplus
}
#endif
#endif
