/* gac_pslout.h -- the PSL line of a chain, shared by chainToPsl and
 * chainToPslBasic (kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c:130-176 and
 * pslTabOut, kent/src/lib/psl.c:175-254: the same 21 tab-separated columns). */
#ifndef GAC_PSLOUT_H
#define GAC_PSLOUT_H

#include "gac_tool.h"

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

#ifdef __cplusplus
}
#endif
#endif
