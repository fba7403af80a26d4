/* gachain.h -- C ABI of libgachain, the MI355X-native chain-scoring engine.
 *
 * This is the drop-in boundary for the reference's chain-scoring hot path
 * (hillerlab/GenomeAlignmentTools: scoreChain, chainNet -rescore,
 * chainCleaner suspect rescoring).  The reference is single-threaded C whose
 * tools call the kent library one chain / one sub-chain at a time; this ABI
 * is the batch, struct-of-arrays replacement for those calls.  Plain C types
 * only: no torch, no HIP types in any signature.  Every entry point returns
 * GAC_OK (0) or a negative GAC_E* code; gac_last_error() gives the message.
 * There is NO CPU fallback: if the HIP runtime or an MI355X (gfx950) device
 * is unavailable, gac_open() fails and every call on a NULL context fails.
 *
 * Reference interfaces replaced (paths relative to the reference root):
 *   gac_score_ranges      <- chainSubsetOnT      kent/src/lib/chain.c:471-558
 *   (gac_score_windows: the same, windows known -- chainFastSubsetOnT :489-558)
 *                          + chainCalcScore       kent/src/lib/chainConnect.c:24-40
 *                          + chainScoreBlock      kent/src/lib/chainConnect.c:14-22
 *                          + gapCalcCost          kent/src/lib/gapCalc.c:298-331
 *                          + chainCalcScoreLocal  src/scoreChain/scoreChain.c:176-198
 *                                                 (= src/chainCleaner/chainCleaner.c:531-551)
 *                          + chainBaseCountSubT   src/chainNet/chainNet.c:773-782
 *                          (one call scores a whole batch of (chain, tStart, tEnd)
 *                           sub-chains; a range covering the chain is the full chain)
 *   gac_set_scoring       <- axtScoreSchemeDefault / axtScoreSchemeReadLf
 *                                                 kent/src/lib/axt.c:423-458,692-819
 *                          + gapCalcFromFile      kent/src/lib/gapCalc.c:233-255
 *   gac_genome_load_2bit  <- twoBitOpen + twoBitReadSeqFrag(tbf, name, 0, 0)
 *                                                 kent/src/lib/twoBit.c:482-513,725-888
 *                          + reverseComplement    kent/src/lib/dnautil.c:404-462
 *                          (genomes stay resident 2-bit packed; '-' query strand is
 *                           index arithmetic, not a reverse-complemented copy)
 *   gac_chains_upload     <- chainRead            kent/src/lib/chain.c:256-346
 *                          (the caller hands over parsed chains as SoA arrays)
 *   gac_axt_split         <- chainToAxt           kent/src/lib/chainToAxt.c:93-124
 *   gac_axt_measure       <- axtScoreSym          kent/src/lib/axt.c:196-229
 *                          + axtIdRatio           kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c:69-89
 *   gac_axt_render        <- loadSeqStrand        kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c:48-67
 *                          + axtFromBlocks        kent/src/lib/chainToAxt.c:14-91
 *   gac_axt_cut           <- chainSubsetOnT       kent/src/lib/chain.c:471-558
 *                          + chainToAxt           kent/src/lib/chainToAxt.c:93-124
 *   gac_axt_*_clip        <- chainFastSubsetOnT's clipped first and last block
 *                                                 kent/src/lib/chain.c:513-522
 *                          (writeChainPart, kent/src/hg/mouseStuff/netToAxt/netToAxt.c:76-105)
 *   gac_prenet_keep       <- chainUsed + setWithPad
 *                                                 kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c:88-137
 *   gac_axt_filter        <- getSeqIdent + getEntropy + checkAxt + processHit's counts
 *                                                 src/filterAxtIdentityEntropy.py:32-69,88-110,144-162
 *   gac_axt_psl           <- trimAlignment + accumCounts + pslFromAlign's column loop
 *                                                 kent/src/lib/psl.c:1626-1806
 *   gac_axt_score         <- axtScoreSym over axtScoreSchemeDefault (axtScoreDnaDefault)
 *                                                 kent/src/lib/axt.c:196-229,291-298,423-458
 */
#ifndef GACHAIN_H
#define GACHAIN_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAC_ABI_VERSION 1
/* Bumped when entry points are added and nothing existing changes (a caller
 * built against minor m runs with any library of minor >= m):
 * 1 = the alignment text entry points (gac_axt_*).
 * 2 = gac_axt_cut and the clip-aware gac_axt_*_clip entry points (netToAxt).
 * 3 = gac_chain_psl_counts[_device] (chainToPsl).
 * 4 = gac_net_write_ex and gac_net_release (chainNet frees a net under its writers).
 * 5 = gac_depth_count and gac_depth_count_host (netSyntenic).
 * 6 = gac_prenet_keep and gac_prenet_keep_host (chainPreNet).
 * 7 = gac_axt_filter and gac_axt_filter_host (filterAxtIdentityEntropy.py).
 * 8 = gac_axt_psl, gac_axt_psl_host and gac_axtpsl_free (axtToPsl).
 * 9 = gac_axt_score and gac_axt_score_host (axtToMaf -score / -scoreZero).
 * 10 = gac_axt_pair_counts[_device] and gac_axt_pair_counts_host (lavToAxt -dropSelf). */
#define GAC_ABI_MINOR 10

/* return codes */
#define GAC_OK 0
#define GAC_E_ARG (-1)     /* bad argument / shape */
#define GAC_E_HIP (-2)     /* HIP runtime error (device fault, OOM, no device) */
#define GAC_E_IO (-3)      /* file open/read error */
#define GAC_E_FORMAT (-4)  /* malformed input file */
#define GAC_E_STATE (-5)   /* call out of order (e.g. scoring before set_scoring) */

/* genome sides */
#define GAC_T 0 /* target / reference genome */
#define GAC_Q 1 /* query genome */

/* gac_score_ranges flags */
#define GAC_WANT_LOCAL 1u /* also compute the scoreChain/chainCleaner local score */

typedef struct gac_ctx gac_ctx;
typedef struct gac_chainset gac_chainset;

/* Piecewise-linear gap cost tables exactly as kent's struct gapCalc
 * (kent/src/lib/gapCalc.c:12-37).  small tables have small_size entries,
 * entry 0 unused (0).  Build one with gac_gapcalc_build(). */
typedef struct gac_gapcalc {
    int32_t small_size;
    int32_t long_count;
    int32_t *q_small, *t_small, *b_small; /* [small_size] */
    int32_t *long_pos;                    /* [long_count] */
    double *q_long, *t_long, *b_long;     /* [long_count] */
    int32_t q_last_pos, t_last_pos, b_last_pos;
    double q_last_val, t_last_val, b_last_val;
    double q_last_slope, t_last_slope, b_last_slope;
} gac_gapcalc;

/* One sub-chain query: chain index in the chainset and a half-open target
 * range.  [t_start, t_end) covering the whole chain scores the full chain. */
typedef struct gac_range {
    int32_t chain;
    int32_t t_start;
    int32_t t_end;
} gac_range;

/* A sub-chain whose block window the caller already knows: chain, half-open
 * target range, and the blocks chainSubsetOnT(chain, t_start, t_end) selects
 * (kent/src/lib/chain.c:481-500: from the first block with tEnd > t_start,
 * while tStart < t_end) as a chain-local first block and count.  chainNet's
 * netting walks a fill's blocks when it creates the fill (innerBounds,
 * src/chainNet/chainNet.c:356-391), so its fills come with their windows
 * (gac_net_get_fill_windows) and scoring them needs no block search
 * (subchainInfo's three rescans, chainNet.c:795-843).  A window covering the
 * chain's span scores the whole chain, as a gac_range does. */
typedef struct gac_window {
    int32_t chain;
    int32_t t_start;
    int32_t t_end;
    int32_t first_block; /* chain-local index of the window's first block */
    int32_t n_blocks;    /* blocks in the window (0: scores 0) */
} gac_window;

/* Parsed chains, struct-of-arrays.  Blocks of chain c are
 * blk_*[blk_off[c] .. blk_off[c+1]), in chain order (ascending t and q;
 * q in the chain's strand coordinates, as in the .chain file). */
typedef struct gac_chainset_desc {
    int64_t n_chains;
    const int32_t *t_seq;    /* [n_chains] index into the T genome (gac_genome_seq_index) */
    const int32_t *q_seq;    /* [n_chains] index into the Q genome */
    const uint8_t *q_strand; /* [n_chains] 0 = '+', 1 = '-' */
    const int64_t *blk_off;  /* [n_chains + 1] */
    int64_t n_blocks;
    const int32_t *blk_t;    /* [n_blocks] tStart */
    const int32_t *blk_q;    /* [n_blocks] qStart */
    const int32_t *blk_size; /* [n_blocks] size (tEnd - tStart == qEnd - qStart) */
} gac_chainset_desc;

/* ---- library / context ------------------------------------------------ */
int gac_abi_version(void);
int gac_abi_minor(void);
/* Human-readable message of the last error on this thread. */
const char *gac_last_error(void);
/* Open a context on HIP device `device`.  Fails (GAC_E_HIP) if there is no
 * usable gfx950 device: the library never falls back to the CPU. */
int gac_open(int device, gac_ctx **out);
/* Closing a context releases the device memory of every chain set still
 * open on it; such a set is left orphaned (gac_chains_context() is NULL, every
 * call on it fails with GAC_E_ARG) and gac_chains_free() only deletes it. */
void gac_close(gac_ctx *ctx);
/* Name of the device architecture the context runs on (e.g. "gfx950"). */
const char *gac_device_arch(gac_ctx *ctx);

/* ---- scoring scheme (host-side parsing, no device needed) -------------- */
/* Build gap tables from "loose", "medium" or a linearGap file
 * (gapCalcFromFile, kent/src/lib/gapCalc.c:233-255).  Free with gac_gapcalc_free. */
int gac_gapcalc_build(const char *name_or_file, gac_gapcalc **out);
void gac_gapcalc_free(gac_gapcalc *g);
/* gapCalcCost (kent/src/lib/gapCalc.c:298-331) on the host: negative
 * distances clamp to 0, q / t / both tables, interpolation in double with
 * the reference's operation order, truncated to int. */
int gac_gap_cost(const gac_gapcalc *g, int dq, int dt);
/* Read a blastz/lastz matrix file (axtScoreSchemeReadLf, axt.c:692-819), or the
 * blastz default when path is NULL (axtScoreSchemeDefault, axt.c:423-458).
 * mat[i*4+j] = matrix[query base i][target base j], i,j in A,C,G,T order.
 * gap_open/gap_extend/extra may be NULL; extra (malloc'd, caller frees) is the
 * "##blastzParms" text. */
int gac_scheme_read(const char *path, int32_t mat[16], int32_t *gap_open,
                    int32_t *gap_extend, char **extra);
/* Install matrix + gap tables on the device. */
int gac_set_scoring(gac_ctx *ctx, const int32_t mat[16], const gac_gapcalc *g);

/* ---- genomes ------------------------------------------------------------ */
/* Load every sequence of a .2bit file onto the device for side T or Q. */
int gac_genome_load_2bit(gac_ctx *ctx, int side, const char *path);
/* Or add sequences one by one from a raw .2bit payload (2 bits/base, MSB
 * first, T=0 C=1 A=2 G=3) plus N runs, then gac_genome_finalize(). */
int gac_genome_add_seq(gac_ctx *ctx, int side, const char *name, int32_t size,
                       const uint8_t *packed, int32_t n_nblocks,
                       const int32_t *n_starts, const int32_t *n_sizes);
int gac_genome_finalize(gac_ctx *ctx, int side);
int32_t gac_genome_seq_count(gac_ctx *ctx, int side);
/* Sequence index by name, or -1. */
int32_t gac_genome_seq_index(gac_ctx *ctx, int side, const char *name);
int32_t gac_genome_seq_size(gac_ctx *ctx, int side, int32_t index);
const char *gac_genome_seq_name(gac_ctx *ctx, int side, int32_t index);
/* Decode [start, end) of a resident sequence back to 'acgtn' text (test aid:
 * proves the resident layout round-trips; out must hold end-start bytes). */
int gac_genome_decode(gac_ctx *ctx, int side, int32_t index, int32_t start,
                      int32_t end, char *out);
/* The resident arrays of a finalized side (read-only; test aid): device
 * pointers of planes (uint2 {bit-0 plane, bit-1 plane} per 32-base word),
 * nmask and lmask (NULL without the soft-mask plane), and the word count.
 * Each array holds n_words + 4 words: the four past the sequences are
 * planes 0, nmask 0xffffffff, lmask 0 (scoring windows read word w + 1).
 * GAC_E_ARG: bad side or NULL pointer; GAC_E_STATE: side not finalized. */
int gac_genome_planes(gac_ctx *ctx, int side, const void **planes, const uint32_t **nmask,
                      const uint32_t **lmask, int64_t *n_words);
/* gac_genome_load_2bit with the loader's two filters.  keep (may be NULL):
 * one byte per sequence of the file, 0 = not loaded.  run_off (may be NULL):
 * the sparse upload -- sequence i of the file (kept or not) is uploaded only
 * in its word runs [run_lo[r], run_hi[r]) (32-base words, clipped to the
 * sequence), r in [run_off[i], run_off[i + 1]); N runs are applied to every
 * word, plane words outside the runs are unspecified.  The sparse upload does
 * not carry the soft-mask plane (GAC_E_ARG). */
int gac_genome_load_2bit_runs(gac_ctx *ctx, int side, const char *path, const uint8_t *keep,
                              const int64_t *run_off, const int32_t *run_lo,
                              const int32_t *run_hi);

/* ---- soft-mask plane (opt-in; chainAntiRepeat) ---------------------------
 * The reference reads sequence with twoBitReadSeqFragExt(doMask=TRUE)
 * (kent/src/lib/twoBit.c:835-874): everything upper case, then the .2bit
 * mask runs lower-cased, an N inside a run included.  A side asked for the
 * plane keeps a third bit plane beside planes/nmask: lmask[w], bit i set when
 * base 32w+i lies in a mask run (padding and tail bits 0).  Call before
 * gac_genome_load_2bit / gac_genome_add_seq of that side; without it a side
 * allocates and uploads exactly what it did before.  The sparse word-run
 * upload (chainNet -rescore's) does not carry the plane: GAC_E_ARG. */
int gac_genome_want_softmask(gac_ctx *ctx, int side);
/* gac_genome_add_seq with the sequence's mask runs (twoBit.c:854-872; ignored
 * unless the side wants the plane). */
int gac_genome_add_seq_masked(gac_ctx *ctx, int side, const char *name, int32_t size,
                              const uint8_t *packed, int32_t n_nblocks,
                              const int32_t *n_starts, const int32_t *n_sizes,
                              int32_t n_mask, const int32_t *mask_starts,
                              const int32_t *mask_sizes);
/* [start, end) of a resident sequence as twoBitReadSeqFragExt(doMask=TRUE)
 * returns it (twoBit.c:835-874): 'ACGTN', 'acgtn' inside mask runs (test
 * aid).  GAC_E_STATE without the plane. */
int gac_genome_decode_case(gac_ctx *ctx, int side, int32_t index, int32_t start,
                           int32_t end, char *out);
/* The mask runs of sequence `name` of a .2bit file as the host reader keeps
 * them (file order): *count = their number, the first min(cap, *count) written
 * to starts/sizes.  No device needed. */
int gac_twobit_mask_runs(const char *path, const char *name, int32_t cap, int32_t *starts,
                         int32_t *sizes, int32_t *count);

/* ---- chains ------------------------------------------------------------- */
/* At most 2^31 - 17 blocks per chain set (GAC_E_ARG beyond: upload in parts). */
int gac_chains_upload(gac_ctx *ctx, const gac_chainset_desc *d, gac_chainset **out);
/* Replace the contents of an uploaded set with d, reusing its device memory
 * when it is large enough (for callers that score a changing handful of
 * chains many times, e.g. chainCleaner's modified chains: no allocation or
 * free per call). Waits for calls still using the set. */
int gac_chains_reupload(gac_ctx *ctx, const gac_chainset_desc *d, gac_chainset *cs);
void gac_chains_free(gac_chainset *cs);
/* The context a set belongs to; NULL once that context was closed. */
gac_ctx *gac_chains_context(const gac_chainset *cs);
/* gac_score_ranges for chains held in host memory (no upload): each range is
 * planned on the host (its window of blocks found by binary search) and the
 * windows are scored by one kernel launch per 256 ranges reading them from
 * pinned mapped memory, gap costs and N masks on the device.  For callers
 * that score a few sub-chains of chains they keep changing (chainCleaner's
 * modified chains).  Results as gac_score_ranges. */
int gac_score_ranges_host(gac_ctx *ctx, const gac_chainset_desc *d, const gac_range *ranges,
                          int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                          int32_t *ali);
int64_t gac_chains_block_count(const gac_chainset *cs);

/* ---- scoring ------------------------------------------------------------ */
/* Score n sub-chains.  Host buffers; synchronous.  For range r of chain c the
 * sub-chain is chainSubsetOnT(c, r.t_start, r.t_end) and
 *   global[r] = chainCalcScore(sub)            (exact; reference's double is integral)
 *   local[r]  = chainCalcScoreLocal(sub)       (only with GAC_WANT_LOCAL; may be NULL otherwise)
 *   ali[r]    = sum of clipped block sizes     (chainBaseCountSubT)
 * A range selecting no block yields 0, 0, 0. */
int gac_score_ranges(gac_ctx *ctx, const gac_chainset *cs, const gac_range *ranges,
                     int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                     int32_t *ali);
/* Same on device-resident buffers, enqueued on `stream` (a hipStream_t, or
 * NULL for the context's own stream).  Returns as soon as the batch is known
 * to fit the scoring workspace (the first kernels write a status word to
 * pinned host memory; on the rare call that outgrows the workspace it is
 * grown and the batch rerun before returning); the scoring itself completes
 * asynchronously -- synchronise the stream (or gac_synchronize /
 * gac_memcpy_d2h, which are ordered after it) before reading results.
 * d_local may be NULL unless GAC_WANT_LOCAL. */
int gac_score_ranges_device(gac_ctx *ctx, const gac_chainset *cs,
                            const gac_range *d_ranges, int64_t n, uint32_t flags,
                            int64_t *d_global, int64_t *d_local, int32_t *d_ali,
                            void *stream);

/* gac_score_ranges for sub-chains given with their windows (gac_window): the
 * same results as gac_score_ranges on (chain, t_start, t_end) when each window
 * is chainSubsetOnT's; the device reads one chain record per window instead of
 * searching the chain's blocks.  A window outside its chain (first_block < 0,
 * n_blocks < 0, or past the chain's last block; chain out of range) is
 * GAC_E_ARG.  Host buffers, synchronous. */
int gac_score_windows(gac_ctx *ctx, const gac_chainset *cs, const gac_window *windows,
                      int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                      int32_t *ali);
/* The same on device-resident buffers, enqueued on `stream` (NULL: the
 * context's); returns as gac_score_ranges_device does (a bad window is
 * reported by this call, once the planning kernel has run). */
int gac_score_windows_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_windows,
                             int64_t n, uint32_t flags, int64_t *d_global, int64_t *d_local,
                             int32_t *d_ali, void *stream);

/* Every chain of the set, in order -- scoreChain's batch (the per-chain
 * chainCalcScore + chainCalcScoreLocal of src/scoreChain/scoreChain.c:207-220,
 * 301-331): global[c], local[c] (GAC_WANT_LOCAL), ali[c] for c in
 * 0..n_chains-1, equal to gac_score_ranges over ranges covering each whole
 * chain.  The chain set's own scoring plan is built at the first call and
 * kept with the set, so a call is just the scoring kernels. */
int gac_score_chains(gac_ctx *ctx, const gac_chainset *cs, uint32_t flags, int64_t *global,
                     int64_t *local, int32_t *ali);
/* The same into device buffers on `stream` (NULL: the context's); returns once
 * enqueued. */
int gac_score_chains_device(gac_ctx *ctx, const gac_chainset *cs, uint32_t flags,
                            int64_t *d_global, int64_t *d_local, int32_t *d_ali, void *stream);

/* ---- match composition (chainAntiRepeat) ---------------------------------
 * For every chain c of the set, over all aligned positions of its blocks
 * (query on the chain's strand, case travelling with the base;
 * kent/src/hg/mouseStuff/chainAntiRepeat/chainAntiRepeat.c:143-155):
 *   match[c*4 + b] = positions where query and target hold the same
 *                    nucleotide b, by .2bit code T=0 C=1 A=2 G=3 (ntVal;
 *                    degeneracyFilter's counts[], :53-66; N matches nothing)
 *   rep[c]         = positions lower-case (in a mask run) on either side
 *                    (repeatFilter's repCount, :102-112)
 *   total[c]       = sum of the block sizes (:113)
 * Exact integers.  Both sides need the soft-mask plane (GAC_E_STATE); a NULL
 * or orphaned set is GAC_E_ARG; an empty set writes nothing.  No scoring
 * setup is needed.  Host buffers, synchronous. */
int gac_chain_composition(gac_ctx *ctx, const gac_chainset *cs, int64_t *match, int64_t *rep,
                          int64_t *total);
/* The same into device buffers on `stream` (NULL: the context's); returns
 * once enqueued. */
int gac_chain_composition_device(gac_ctx *ctx, const gac_chainset *cs, int64_t *d_match,
                                 int64_t *d_rep, int64_t *d_total, void *stream);
/* chainAntiRepeat's decision for one chain from its composition:
 * degeneracyFilter (chainAntiRepeat.c:40-92) then repeatFilter (:94-117), in
 * the reference's operation order in double -- a chain without a match
 * (0/0 = NaN) is dropped as there.  1 = keep, 0 = drop.  Host only. */
int gac_antirepeat_pass(double score, const int64_t match[4], int64_t rep, int64_t total,
                        int min_score);

/* ---- PSL match counts (chainToPsl) ----------------------------------------
 * For every chain c of the set, over all aligned positions of its blocks, the
 * four exclusive classes aliStringToPsl counts
 * (kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c:106-131), tested in its
 * order on text as twoBitReadSeqFragExt(doMask=TRUE) gives it:
 *   counts[c*4 + 3] nCount    either base is N (in any case)
 *   counts[c*4 + 0] match     else equal bases, the TARGET base upper case
 *   counts[c*4 + 2] repMatch  else equal bases, the target base lower case
 *   counts[c*4 + 1] misMatch  else (whatever the case)
 * -- the order of the PSL columns.  The query's case is never read.  A '-'
 * query is the reverse complement of the whole resident sequence, as there
 * (:55-56, with the sequence's own size, not the chain header's qSize): block
 * query coordinates are the chain's, unshifted.  Exact integers.  The target
 * side needs the soft-mask plane (GAC_E_STATE), the query side does not; a
 * NULL or orphaned set is GAC_E_ARG; an empty set writes nothing.  No scoring
 * setup is needed.  Host buffer [n_chains][4], synchronous. */
int gac_chain_psl_counts(gac_ctx *ctx, const gac_chainset *cs, int64_t *counts);
/* The same counts (chainToPsl.c:106-131) into a device buffer on `stream`
 * (NULL: the context's); returns once enqueued. */
int gac_chain_psl_counts_device(gac_ctx *ctx, const gac_chainset *cs, int64_t *d_counts,
                                void *stream);

/* ---- coverage depth of ranges (netSyntenic) --------------------------------
 * count[i] = the number of positions p in [start[i], end[i]) of sequence
 * seq[i] at which the summed depth, sum over j of delta[j] where seq[j] ==
 * seq[i] and start[j] <= p < end[j], is >= threshold.  With delta +1 for a
 * fill's query range, -1 for a gap's and threshold 2 this is netSyntenic's qDup
 * (dupeTreeAddSub / dupeTreeCountOver,
 * kent/src/hg/mouseStuff/netSyntenic/netSyntenic.c:63-138) for every range at
 * once; ranges of length 0 count 0.  Sequence ids are any non-negative
 * numbers (sparse is fine).  Exact integers, within one bound that is not
 * checked: the running depth is an int32_t, here and in the host twin, so the
 * sum of |delta[j]| over the ranges covering or touching any one position of
 * a sequence must stay below 2^31 (it does for any n this call takes when
 * delta is +-1).  GAC_E_ARG: end < start, a
 * negative seq or start, threshold < 1, or more than INT32_MAX / 2 ranges.
 * n == 0 returns GAC_OK without a launch.  Host buffers, synchronous; needs
 * neither genomes nor a scoring setup. */
int gac_depth_count(gac_ctx *ctx, int64_t n, const int32_t *seq, const int32_t *start,
                    const int32_t *end, const int8_t *delta, int32_t threshold, int32_t *count);
/* The same result without a device: a threaded sort of the range ends and
 * one sweep (netSyntenic -host). */
int gac_depth_count_host(int64_t n, const int32_t *seq, const int32_t *start, const int32_t *end,
                         const int8_t *delta, int32_t threshold, int32_t *count);

/* ---- chains worth netting (chainPreNet) -------------------------------------
 * keep[i] = 1 when chain i would be written by chainPreNet
 * (kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c:104-137): in the order
 * given (the file's, best score first) a chain is kept when some base of one
 * of its blocks, on the target or on the query side, lies outside the blocks
 * of every chain kept before it, those blocks widened by `pad` bases at both
 * ends and cut to [0, size of the sequence).  A dropped chain covers nothing.
 * Chain i has the blocks [blk_off[i], blk_off[i + 1]) (blk_off[0] = 0,
 * blk_off[n] = n_blocks): block b covers [blk_t[b], blk_t[b] + blk_size[b])
 * of target sequence t_seq[i] and [blk_q[b], blk_q[b] + blk_size[b]) of query
 * sequence q_seq[i]; the query coordinates are taken as they stand in the
 * chain file, for '-' chains too, as the reference takes them.  Target and
 * query sequences are numbered apart (t_sizes[n_tseq], q_sizes[n_qseq]).  A
 * chain with t_seq or q_seq -1 is skipped (a haplotype query without
 * -inclHap): it gets 0 and covers nothing.  A block of size 0 has no base of
 * its own but covers its pad, as there.
 *
 * The device works in rounds of two passes: every pass
 * writes, per base, the lowest rank among the chains that cover it, and asks
 * every undecided chain for a base that nothing before it covers.  The per-base
 * words take 4 bytes a base of the largest sequence group: the sequences that
 * some counted chain names, of one side at a time, grouped to fit
 * GAC_PRENET_FC_BYTES (default: three quarters of the device memory free at
 * the call, after the call's other buffers).  A sequence larger than that, or
 * max_rounds rounds (<= 0: GAC_PRENET_MAX_ROUNDS) without a decision for every
 * chain, hands the whole call to gac_prenet_keep_host; stats says so.
 *
 * GAC_E_ARG: a negative start or size, a block past the end of its sequence,
 * a sequence number outside its table, pad < 0, offsets that do not ascend, or
 * more than GAC_PRENET_MAX_ITEMS chains or blocks (what the reference does
 * with such input is undefined: it writes outside its bitmap).  n == 0 returns
 * GAC_OK without a launch.  Exact integers.  Host buffers, synchronous; needs
 * neither genomes nor a scoring setup.  stats may be NULL. */
#define GAC_PRENET_MAX_ROUNDS 32
#define GAC_PRENET_MAX_ITEMS 2147483645
#define GAC_PRENET_ON_DEVICE 0   /* gac_prenet_stats.fell_back */
#define GAC_PRENET_FELL_ROUNDS 1 /* max_rounds reached: finished on the host */
#define GAC_PRENET_FELL_MEMORY 2 /* a sequence larger than the budget: host */
typedef struct gac_prenet_stats {
    int32_t rounds;    /* rounds run on the device */
    int32_t passes;    /* mark + check passes over all groups (two a round) */
    int32_t groups[2]; /* sequence groups of the target / query side */
    int32_t fell_back; /* GAC_PRENET_ON_DEVICE or why the host finished */
    int32_t pad_;
    int64_t kept;      /* chains with keep 1 */
} gac_prenet_stats;
int gac_prenet_keep(gac_ctx *ctx, int64_t n, const int64_t *blk_off, const int32_t *t_seq,
                    const int32_t *q_seq, int64_t n_blocks, const int32_t *blk_t,
                    const int32_t *blk_q, const int32_t *blk_size, int32_t n_tseq,
                    const int32_t *t_sizes, int32_t n_qseq, const int32_t *q_sizes, int32_t pad,
                    int32_t max_rounds, uint8_t *keep, gac_prenet_stats *stats);
/* The reference's own pass, chain by chain over one bitmap per named sequence
 * and side; no device (chainPreNet -host, the fallbacks). */
int gac_prenet_keep_host(int64_t n, const int64_t *blk_off, const int32_t *t_seq,
                         const int32_t *q_seq, int64_t n_blocks, const int32_t *blk_t,
                         const int32_t *blk_q, const int32_t *blk_size, int32_t n_tseq,
                         const int32_t *t_sizes, int32_t n_qseq, const int32_t *q_sizes,
                         int32_t pad, uint8_t *keep, gac_prenet_stats *stats);

/* ---- alignments worth chaining (filterAxtIdentityEntropy.py) --------------
 * keep[i] = 1 iff alignment i has a window of `window` columns that passes
 * the script's identity and entropy test (src/filterAxtIdentityEntropy.py:
 * checkAxt :88-110 over processHit's counts :144-162, getSeqIdent :41-42,
 * getEntropy :45-69).  Entry i is two rows of len[i] columns of alignment
 * text at text + t_off[i] (target) and text + q_off[i] (query); rows may lie
 * anywhere in `text` and may overlap.  With both characters ASCII-lowercased a
 * column is a match when they are equal ('n'/'n' and '-'/'-' match), and the
 * target adds to one of four counts when it is a, c, g or t.  The entry is
 * kept iff some start s with target[s] != '-' and s + window <= len has, over
 * [s, s + window), 100.0 * matches / window >= min_ident and H >= min_entropy;
 * H = 0.0 without a counted base, else with p = k / n over the counts k in the
 * order a, c, g, t, zero counts skipped: e = 0.0; e -= p * log(p); H = e /
 * log(2), all in doubles.  The order of the terms is part of the result.
 *
 * Exact by construction: the host makes, with libm, the smallest match count
 * that reaches min_ident and the table of the terms p * log(p); the device
 * (and the host twin) compare integers, subtract table entries in that order
 * and divide once.  The device takes windows up to
 * GAC_AXTF_MAX_WINDOW; a larger one runs the host twin for every entry
 * (fell_back 1).  The entries go in batches whose text stays under
 * GAC_AXTF_BATCH_BYTES (an environment knob; default: a quarter of the free
 * device memory, at most 256 MiB); an entry alone over that is decided by the
 * host twin (fell_back 2).
 *
 * GAC_E_ARG: window < 1, n < 0, a negative length or offset, a row reaching
 * past text_bytes, a NULL array with n > 0.  n == 0 returns GAC_OK without a
 * launch.  Host buffers, synchronous; needs neither genomes nor a scoring
 * setup.  st may be NULL. */
#define GAC_AXTF_MAX_WINDOW 1024
typedef struct gac_axtfilter_stats {
    int64_t kept, windows;      /* entries kept; window starts examined */
    int64_t host_entries;       /* entries decided by the host twin */
    int32_t batches, fell_back; /* 0 device; 1 window over the device cap (all entries on the host);
                                   2 some entry over the byte budget (those entries on the host) */
} gac_axtfilter_stats;
int gac_axt_filter(gac_ctx *ctx, int64_t n, const char *text, int64_t text_bytes,
                   const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                   double min_ident, double min_entropy, int32_t window,
                   uint8_t *keep, gac_axtfilter_stats *st);
/* The same decision with running window counts on nthreads host threads (<= 0:
 * GAC_THREADS, else all CPUs); no device (filterAxtIdentityEntropy.py -host,
 * the fallbacks). */
int gac_axt_filter_host(int64_t n, const char *text, int64_t text_bytes,
                        const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                        double min_ident, double min_entropy, int32_t window, int nthreads,
                        uint8_t *keep, gac_axtfilter_stats *st);

/* ---- alignments to PSL blocks (axtToPsl) -----------------------------------
 * What pslFromAlign (kent/src/lib/psl.c:1716-1806, with trimAlignment :1634 and
 * accumCounts :1680, PSL_IS_SOFTMASK set) makes of the two rows of an
 * alignment, without names, sizes, strands or coordinates.  The entries are
 * given as for gac_axt_filter: two rows of len[i] columns at text + t_off[i]
 * (target) and text + q_off[i] (query).  A gap is one of '-' '.' '=' '_'.
 *
 * The trim drops the columns before the first and after the last column
 * without a gap.  q_head / t_head count the dropped leading columns that hold a
 * query / target character (the other row has a gap there), q_tail / t_tail
 * the trailing ones; cols is what is left.  Over those columns, columns with a
 * gap in both rows are skipped and are never a "previous" column; a column
 * without a gap adds to n_count if either character is 'N', else, if the
 * characters are equal after toupper, to rep_match if either is lower case
 * and to match if not, else to mis_match; a column with a gap in the query
 * adds to t_base_insert, and to t_num_insert if the previous column's query
 * character was no gap (q_* likewise with the rows swapped).  A block is a run
 * of columns without a gap that no one-sided column interrupts; block b of
 * entry i is block[entry[i].block0 + b] = the query and target characters
 * between the first kept column and the block's first column, and the
 * block's columns.  An entry with no column left has one block (0, 0, 0), the
 * one pslFromAlign's closing addBlock makes.  The caller adds its own
 * coordinates: with qs / ts the strand coordinates of the first kept column,
 * qStarts[b] = qs + q_adv, tStarts[b] = ts + t_adv, blockSizes[b] = size.
 *
 * The blocks are variable-length output, so the result is library-owned: the
 * call allocates one gac_axtpsl_result holding entry[n] and block[n_blocks]
 * (blocks in entry order) and hands it back in *out; gac_axtpsl_free releases
 * it (NULL is allowed).  On an error *out is NULL.
 *
 * The device walks an entry in tiles of GAC_AXTPSL_TILE columns (DESIGN.md
 * 7.15).  The entries go in batches whose text stays under
 * GAC_AXTPSL_BATCH_BYTES (an environment knob; default as
 * GAC_AXTF_BATCH_BYTES); an entry alone over that is converted by the host
 * twin (fell_back 2).
 *
 * GAC_E_ARG: n < 0, a negative length or offset, a row reaching past
 * text_bytes, a NULL array with n > 0, out NULL.  n == 0 returns GAC_OK and an
 * empty result without a launch.  Host buffers, synchronous; needs neither
 * genomes nor a scoring setup.  st may be NULL. */
#define GAC_AXTPSL_TILE 512
typedef struct gac_axtpsl_entry {
    uint32_t match, mis_match, rep_match, n_count;
    uint32_t q_num_insert, q_base_insert, t_num_insert, t_base_insert;
    int32_t q_head, t_head, q_tail, t_tail; /* characters the trim dropped */
    int32_t cols;                           /* columns left after the trim */
    int32_t n_blocks;                       /* >= 1 */
    int64_t block0;                         /* index of the entry's first block */
} gac_axtpsl_entry;
typedef struct gac_axtpsl_block {
    int32_t q_adv, t_adv, size;
} gac_axtpsl_block;
typedef struct gac_axtpsl_result {
    int64_t n, n_blocks;
    gac_axtpsl_entry *entry; /* [n] */
    gac_axtpsl_block *block; /* [n_blocks] */
} gac_axtpsl_result;
typedef struct gac_axtpsl_stats {
    int64_t blocks, columns;    /* blocks returned; columns given */
    int64_t host_entries;       /* entries converted by the host twin */
    int32_t batches, fell_back; /* 0 device; 2 some entry over the byte budget (those entries on the host) */
} gac_axtpsl_stats;
int gac_axt_psl(gac_ctx *ctx, int64_t n, const char *text, int64_t text_bytes,
                const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                gac_axtpsl_result **out, gac_axtpsl_stats *st);
/* The same result by one sequential pass an entry on nthreads host threads
 * (<= 0: GAC_THREADS, else all CPUs); no device (axtToPsl -host, the fallback). */
int gac_axt_psl_host(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                     const int64_t *q_off, const int32_t *len, int nthreads,
                     gac_axtpsl_result **out, gac_axtpsl_stats *st);
void gac_axtpsl_free(gac_axtpsl_result *r);

/* ---- alignment text to blastz scores (axtToMaf -score / -scoreZero) --------
 * score[i] is what axtScoreDnaDefault returns for entry i: axtScoreSym
 * (kent/src/lib/axt.c:196-229) under axtScoreSchemeDefault (:423-458), over the
 * entry's two rows of len[i] characters at text + t_off[i] and text + q_off[i]
 * (given exactly as for gac_axt_filter and gac_axt_psl).
 *
 * A column is a gap column iff either character is '-' ('.', '=' and '_' are
 * NOT gaps here, unlike in gac_axt_psl).  A gap column costs 30; one whose
 * previous column is no gap column (column 0 included) costs 400 more.  A run
 * of gap columns is one run whichever row holds the dash, columns with a dash
 * in both rows included.  Any other column adds the blastz default matrix on
 * its two letters, case-blind:
 *            A     C     G     T
 *      A    91  -114   -31  -123
 *      C  -114   100  -125   -31
 *      G   -31  -125   100  -114
 *      T  -123   -31  -114    91
 * and 0 if either character is outside acgtACGT ('N', 'n', '.', digits, bytes
 * >= 0x80).  On bytes >= 0x80 the reference indexes its matrix with a negative
 * char, which is undefined behaviour there; here such a byte scores 0.  The sum
 * wraps as the reference's int does (two's complement, modulo 2^32).  len 0
 * scores 0.  gac_set_scoring is neither needed nor read.
 *
 * A column's contribution depends on that column and the one before it only,
 * so the device sums chunks of GAC_AXTSCORE_CHUNK columns independently
 *  and the result is exact whatever the order.  The entries go
 * in batches whose text stays under GAC_AXTSCORE_BATCH_BYTES (an environment
 * knob; default as GAC_AXTF_BATCH_BYTES); an entry alone over that is scored
 * by the host twin (fell_back 2).
 *
 * GAC_E_ARG: n < 0, a negative length or offset, a row reaching past
 * text_bytes, a NULL array with n > 0.  n == 0 returns GAC_OK without a
 * launch.  Host buffers, synchronous; needs no genomes.  st may be NULL. */
#define GAC_AXTSCORE_CHUNK 1024
typedef struct gac_axtscore_stats {
    int64_t columns;            /* columns given */
    int64_t host_entries;       /* entries scored by the host twin */
    int32_t batches, fell_back; /* 0 device; 2 some entry over the byte budget (those entries on the host) */
} gac_axtscore_stats;
int gac_axt_score(gac_ctx *ctx, int64_t n, const char *text, int64_t text_bytes,
                  const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                  int32_t *score, gac_axtscore_stats *st);
/* The same scores by one pass an entry on nthreads host threads (<= 0:
 * GAC_THREADS, else all CPUs); no device (axtToMaf -host, the fallback). */
int gac_axt_score_host(int64_t n, const char *text, int64_t text_bytes, const int64_t *t_off,
                       const int64_t *q_off, const int32_t *len, int nthreads,
                       int32_t *score, gac_axtscore_stats *st);

/* ---- alignment text (chainToAxt) ------------------------------------------
 * A piece is a window of consecutive blocks of one chain (gac_window: chain,
 * first_block, n_blocks; t_start / t_end are informative and not read) that
 * becomes one axt record.  The entry points take any block windows; the
 * sub-chains of net fills, whose first and last block are clipped, go through
 * gac_axt_cut and the _clip forms further down.  A window holding a negative
 * or double-sided gap is GAC_E_ARG.
 *
 * gac_axt_split cuts every chain of a parsed set where chainToAxt() does
 * (kent/src/lib/chainToAxt.c:105-121, called with maxChain = BIGNUM as
 * kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c:108 does): before block b
 * with previous block a, dq = b.qStart - a.qEnd, dt = b.tStart - a.tEnd, when
 * (dq > 0 && dt > 0) || dt > max_gap || dq > max_gap.  Pieces come in file
 * order; t_start / t_end are the piece's target span.  A negative dq or dt
 * (undefined in the reference) is GAC_E_FORMAT and gac_last_error names the
 * chain.  Host only; release *pieces with gac_axt_free. */
int gac_axt_split(const gac_chainset_desc *d, int32_t max_gap, gac_window **pieces, int64_t *n);
void gac_axt_free(gac_window *pieces);
/* Per piece, what axtFromBlocks + axtScoreDnaDefault and axtIdRatio compute
 * from the rendered rows (chainToAxt.c:28-40,89; kent/src/lib/axt.c:196-229,
 * 423-458; chainToAxt/chainToAxt.c:69-89), without rendering them:
 *   sym[p]   = columns: block sizes + inner gap lengths (symCount)
 *   score[p] = sum over blocks of the blastz default matrix on the letters
 *              (case-blind, a column with an N scores 0) - sum over inner
 *              gaps of length L > 0 of (400 + 30 L); summed in int64 and
 *              narrowed to int32 as the reference's int wraps.  The default
 *              matrix always: gac_set_scoring is neither needed nor read.
 *   ali[p]   = columns without a dash = sum of the block sizes
 *   match[p] = of those, letters equal case-blind, N against N included
 * (idRatio = match ? (double)match / ali : 0.0).  Both sides need the
 * soft-mask plane (GAC_E_STATE); a NULL or orphaned set, or a window outside
 * its chain, is GAC_E_ARG; n == 0 writes nothing.  Host buffers, synchronous. */
int gac_axt_measure(gac_ctx *ctx, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                    int32_t *score, int64_t *match, int64_t *ali, int64_t *sym);
/* The same with pieces and results in device memory, on `stream` (NULL: the
 * context's).  The call waits on the stream for its checks; the results stay
 * on the device. */
int gac_axt_measure_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_pieces,
                           int64_t n, int32_t *d_score, int64_t *d_match, int64_t *d_ali,
                           int64_t *d_sym, void *stream);
/* Per piece, what axtScoreSym (axt.c:196-229) needs of the letters to score
 * the piece under ANY matrix (lavToAxt -dropSelf rescores with -scoreScheme):
 *   pairs[p * 16 + q * 4 + t] = columns without a dash whose query letter is q
 *              and target letter t, A,C,G,T order as gac_scheme_read,
 *              case-blind, '-' pieces on the reverse complement
 *   n_cols[p] = columns without a dash with an N on either side (they score 0)
 * so that sum(pairs[p]) + n_cols[p] is gac_axt_measure's ali[p], and the
 * default matrix over pairs[p] minus the gap terms its score[p].  The gap terms
 * need no sequence and are the caller's.  t_start / t_end are not read.
 * Arguments, state and errors as gac_axt_measure; n == 0 writes nothing. */
int gac_axt_pair_counts(gac_ctx *ctx, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                        int64_t *pairs, int64_t *n_cols);
int gac_axt_pair_counts_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_pieces,
                               int64_t n, int64_t *d_pairs, int64_t *d_n_cols, void *stream);
/* The same on the host, no device: the sequences read from two .2bit files,
 * d->t_seq / d->q_seq numbering the files' sequences in file order.  A block
 * outside its sequence, a window outside its chain and a negative or
 * double-sided gap inside a piece are GAC_E_ARG. */
int gac_axt_pair_counts_host(const char *t_2bit, const char *q_2bit, const gac_chainset_desc *d,
                             const gac_window *pieces, int64_t n, int64_t *pairs, int64_t *n_cols);
/* The rows of every piece as axtFromBlocks fills them (chainToAxt.c:58-86)
 * from twoBitReadSeqFragExt(doMask=TRUE) text (chainToAxt/chainToAxt.c:48-67:
 * 'ACGTN', lower case in mask runs, '-' chains reverse-complemented with case
 * and N travelling with the base), laid out for axtWrite (axt.c:110-114):
 *   out[offsets[p] ..] = tSym '\n' qSym '\n' '\n'     (2 * sym[p] + 3 bytes)
 * offsets NULL: the pieces packed in order from byte 0.  No other byte of out
 * is changed.  A piece whose rows would pass out_bytes is GAC_E_ARG and
 * nothing is written.  Host buffers, synchronous (the buffer travels to the
 * device and back: batches go through gac_axt_job). */
int gac_axt_render(gac_ctx *ctx, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                   const int64_t *offsets, char *out, int64_t out_bytes);
/* The same with pieces, offsets and text in device memory, on `stream`; waits
 * on the stream for its checks and returns with the rendering enqueued. */
int gac_axt_render_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_pieces,
                          int64_t n, const int64_t *d_offsets, char *d_out, int64_t out_bytes,
                          void *stream);
/* One render in flight: a stream, device text and pinned host text of its
 * own.  submit checks the pieces, then enqueues gac_axt_render of `bytes` of
 * text and its copy to the job's pinned buffer and returns; wait gives the
 * text once it has arrived (valid until the job's next submit; bytes of it
 * that no piece's rows cover are unspecified).  Two jobs
 * used in turn overlap the host's work on one batch with the next batch's
 * rendering and copy.  text_bytes: initial capacity (grown by a larger
 * submit).  Close jobs before gac_close. */
typedef struct gac_axt_job gac_axt_job;
int gac_axt_job_open(gac_ctx *ctx, int64_t text_bytes, gac_axt_job **out);
int gac_axt_job_submit(gac_axt_job *job, const gac_chainset *cs, const gac_window *pieces,
                       int64_t n, const int64_t *offsets, int64_t bytes);
int gac_axt_job_wait(gac_axt_job *job, const char **text, int64_t *bytes);
void gac_axt_job_close(gac_axt_job *job);

/* ---- sub-chains of net fills (netToAxt) -----------------------------------
 * For range r, the pieces chainToAxt(chainSubsetOnT(chain, t_start, t_end),
 * max_gap, BIGNUM) makes (kent/src/lib/chain.c:471-558, kent/src/lib/
 * chainToAxt.c:93-124; writeChainPart, kent/src/hg/mouseStuff/netToAxt/
 * netToAxt.c:76-105), in order: (*pieces)[(*first)[r] .. (*first)[r + 1]).  A
 * piece's first_block / n_blocks are chain-local; its t_start / t_end are the
 * clipped target span (max(first block's tStart, r.t_start), min(last block's
 * tEnd, r.t_end)), so only a range's first piece can have a cut head and only
 * its last a cut tail.  A range that selects no block (t_start >= t_end
 * included) gives no piece: first[r] == first[r + 1] (the reference's "null
 * subchain").  first has n + 1 entries, first[n] == *n_pieces.
 * Everything runs on the device, cut over the selected blocks: a range costs
 * two binary searches plus what its blocks cost.  Host buffers, synchronous.
 * *pieces and *first are ONE allocation: release both with gac_axt_free(*pieces)
 * and never free *first.  A chain index out of range, or a NULL or orphaned
 * set, is GAC_E_ARG; a negative dq or dt between two blocks of a selected
 * window is GAC_E_FORMAT and gac_last_error names a chain (by its index in the
 * set) it happened in, as gac_axt_split does.  On error *pieces and *first are
 * NULL. */
int gac_axt_cut(gac_ctx *ctx, const gac_chainset *cs, const gac_range *ranges, int64_t n,
                int32_t max_gap, gac_window **pieces, int64_t **first, int64_t *n_pieces);
/* gac_axt_measure / gac_axt_render / their _device forms / gac_axt_job_submit
 * with the same arguments and results, but t_start / t_end are read
 * (chainFastSubsetOnT, chain.c:513-522): a piece's first block starts at
 * max(tStart, t_start), its last block ends at min(tEnd, t_end), the query
 * following (qStart += cut head, qEnd -= cut tail); for a one-block piece both
 * cuts apply to that block.  Inner gaps are never touched.  A piece whose first
 * or last block is left empty by its clip is GAC_E_ARG, found before anything
 * is written.  A piece whose t_start / t_end equal its blocks' span (every
 * piece of gac_axt_split) gives exactly what the unclipped entry points give;
 * those go on ignoring the two fields. */
int gac_axt_measure_clip(gac_ctx *ctx, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                         int32_t *score, int64_t *match, int64_t *ali, int64_t *sym);
int gac_axt_measure_clip_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_pieces,
                                int64_t n, int32_t *d_score, int64_t *d_match, int64_t *d_ali,
                                int64_t *d_sym, void *stream);
int gac_axt_render_clip(gac_ctx *ctx, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                        const int64_t *offsets, char *out, int64_t out_bytes);
int gac_axt_render_clip_device(gac_ctx *ctx, const gac_chainset *cs, const gac_window *d_pieces,
                               int64_t n, const int64_t *d_offsets, char *d_out, int64_t out_bytes,
                               void *stream);
int gac_axt_job_submit_clip(gac_axt_job *job, const gac_chainset *cs, const gac_window *pieces,
                            int64_t n, const int64_t *offsets, int64_t bytes);

/* ---- caller text (the kent in-process API's char* entry points) ---------
 * chainScoreBlock / axtScoreUngapped (kent/src/lib/chainConnect.c:14-22,
 * axt.c:186-194) of n blocks of caller-owned text: score[i] = sum over k <
 * size[i] of mat[q][t] (A,C,G,T order as gac_scheme_read; any other
 * character scores 0, either case).  On the device; synchronous. */
int gac_score_text_blocks(gac_ctx *ctx, int64_t n, const char *const *q, const char *const *t,
                          const int32_t *size, const int32_t mat[16], int64_t *score);
/* cBlockFindCrossover (chainConnect.c:61-105) of n overlaps on caller text:
 * lq/lt point at the left block's last overlap[i] bases (qEnd - overlap),
 * rq/rt at the right block's first.  Out: pos (offset of the crossover from
 * the right block's start) and adj (rScore + lScore - bestScore). */
int gac_text_crossovers(gac_ctx *ctx, int64_t n, const char *const *lq, const char *const *lt,
                        const char *const *rq, const char *const *rt, const int32_t *overlap,
                        const int32_t mat[16], int32_t *pos, int32_t *adj);

/* ---- axtChain ------------------------------------------------------------
 * Per-block scores: axtScoreUngapped (kent/src/lib/axt.c:186-194) of every
 * block, the scores chainPair gives the kd-tree (axtChain.c:276-282).  Pairs
 * share a target / query sequence and strand ('-': query coordinates on the
 * reverse strand, as in PSL/axt).  Blocks must lie inside their sequences. */
int gac_score_blocks(gac_ctx *ctx, int64_t n_pairs, const int32_t *t_seq, const int32_t *q_seq,
                     const uint8_t *q_strand, const int64_t *blk_off, const int32_t *blk_t,
                     const int32_t *blk_q, const int32_t *blk_size, int32_t *score);

/* The kd-tree DP of chainBlocks on the device: findBestPredecessors
 * (kent/src/lib/chainBlock.c:281-300) -- bestPredecessor (:207-263) with
 * chainConnectCost / cBlockFindCrossover (chainConnect.c:61-149) as its
 * connect cost, updateScoresOnWay (:265-279) -- for n_pairs seqPairs in one
 * launch, one wave per pair.  The caller builds each pair's tree (kdBuild,
 * :124-164) in pre-order with the hi child first:
 *   node_a[4v..] = {maxQ, maxT, cut, lo child}         internal node
 *                  {qEnd, tEnd, qStart, tStart}        leaf node
 *   node_b[2v..] = {end of v's subtree, dim (0 q, 1 t)} internal node
 *                  {end = v + 1, ~(leaf position)}     leaf node
 * node indices are relative to the pair (nodes [node_off[p], node_off[p+1])).
 * Leaves are in findBestPredecessors' target order, [leaf_off[p],
 * leaf_off[p+1]): leaf[4i..] = {qStart, qEnd, tStart, tEnd}, leaf_score[i]
 * (axtScoreUngapped), leaf_node[i] (its node), and path[path_off[i] ..
 * path_off[i+1]) = the nodes updateScoresOnWay's descent reaches for it
 * (global leaf index i; path_off has total leaves + 1 entries).  Out, per
 * leaf: total[i] = totalScore, pred[i] = best predecessor node or -1.
 * Uses the context's scoring setup (gac_set_scoring) and genomes. */
int gac_chain_dp(gac_ctx *ctx, int64_t n_pairs, const int32_t *t_seq, const int32_t *q_seq,
                 const uint8_t *q_strand, const int64_t *node_off, const int32_t *node_a,
                 const int32_t *node_b, const int64_t *leaf_off, const int32_t *leaf,
                 const int32_t *leaf_score, const int32_t *leaf_node, const int64_t *path_off,
                 const int32_t *path, int64_t *total, int32_t *pred);

/* chainBlocks' kd-tree DP for n_pairs seqPairs straight from their blocks,
 * every input of the DP built on the device:
 *   the leaf list (kent/src/lib/chainBlock.c:400-420: blocks with tStart !=
 *     tEnd, slSort by tStart over the slAddHead-built list) and its query
 *     order (kdTreeMake :166-205),
 *   the kd-trees (kdBuild :124-164, splitList/medianVal :92-122),
 *   the update paths (updateScoresOnWay :265-279) and, for the exact fast
 *     DP, each leaf's overlapping candidates,
 * then findBestPredecessors (:281-300) as in gac_chain_dp.  Blocks of pair p
 * are [blk_off[p], blk_off[p+1]) in the caller's list order (axtChain's order
 * after removeExactOverlaps), box[4g..] = {qStart, qEnd, tStart, tEnd} in
 * the pair's strand coordinates, score[g] = axtScoreUngapped.
 * fast != 0: the exact fast search (k_dp_fast) with the linear gap-cost
 * minorant lin_k / 1024 and the smallest matrix entry min_entry; ov_cap
 * (<= 1024): more overlapping candidates than this send a leaf to the
 * reference search order.  fast == 0: the reference search (k_dp).
 * Out: leaf_off[n_pairs + 1] (the leaves of pair p are [leaf_off[p],
 * leaf_off[p+1])), tord[leaf] = the pair-local block of each leaf in target
 * order, and per block total[g] = totalScore (score for a non-leaf) and
 * pred[g] = the best predecessor as a pair-local block, or -1.  A block
 * outside its sequences is GAC_E_ARG.  Uses the context's scoring setup and
 * genomes. */
/* kdTreeMake (kent/src/lib/chainBlock.c:166-205: the leaf lists and
 * kdBuild :124-164) for n_pairs seqPairs on the device -- the build of
 * gac_chain_dp_blocks -- for a caller that runs the DP itself.  Blocks as in
 * gac_chain_dp_blocks.  Out: leaf_off[n_pairs + 1], and per pair p into the
 * caller's buffers: tord[p][leaf] / qord[p][leaf] = the pair-local blocks of
 * its leaves in target / query order (at most blk_off[p+1] - blk_off[p]
 * each), lnode[p][block] = the leaf node of each block (-1: tStart ==
 * tEnd, not a leaf), nodes[p][6 v ..] = node v of the pair's 2 n - 1 (n =
 * its leaves) in pre-order with the hi child first: {lo, hi, -1, cut, maxQ,
 * maxT} for an internal node, {qStart, tStart, block, 0, qEnd, tEnd} for a
 * leaf node. */
int gac_kd_trees(gac_ctx *ctx, int64_t n_pairs, const int32_t *t_seq, const int32_t *q_seq,
                 const uint8_t *q_strand, const int64_t *blk_off, const int32_t *box,
                 int64_t *leaf_off, int32_t *const *tord, int32_t *const *qord,
                 int32_t *const *lnode, int32_t *const *nodes);

int gac_chain_dp_blocks(gac_ctx *ctx, int64_t n_pairs, const int32_t *t_seq,
                        const int32_t *q_seq, const uint8_t *q_strand, const int64_t *blk_off,
                        const int32_t *box, const int32_t *score, int fast, int64_t lin_k,
                        int32_t min_entry, int32_t ov_cap, int64_t *leaf_off, int32_t *tord,
                        int64_t *total, int32_t *pred);

/* cBlockFindCrossover (kent/src/lib/chainConnect.c:61-105) of n overlapping
 * block pairs on the device (one wave per pair, a prefix-sum / first-maximum
 * scan): left block ending at (lqe, lte), right block starting at (rqs, rts),
 * `overlap` bases, on seqPair (t_seq, q_seq, q_strand) -- strand coordinates.
 * Out: pos (crossover offset from the right block's start) and adj (the
 * score adjustment).  Uses the context's score matrix. */
int gac_crossovers(gac_ctx *ctx, int64_t n, const int32_t *t_seq, const int32_t *q_seq,
                   const uint8_t *q_strand, const int32_t *lqe, const int32_t *lte,
                   const int32_t *rqs, const int32_t *rts, const int32_t *overlap, int32_t *pos,
                   int32_t *adj);

/* axtChain's chaining of every seqPair (axtChain.c:250-309 chainPair and
 * :452-470 the final sort), replacing
 *   removeExactOverlaps          axtChain.c:173-197
 *   axtScoreUngapped per block   axt.c:186-194              (GPU, gac_score_blocks)
 *   chainBlocks                  kent/src/lib/chainBlock.c:400-452: the kd-tree
 *                                (kdBuild :124-164), bestPredecessor (:207-263),
 *                                updateScoresOnWay (:265-279), peelChains
 *                                (:311-373), scoreBlocks (:296-309)
 *   chainConnectCost             kent/src/lib/chainConnect.c:114-149 (+ cBlockFindCrossover :61-105)
 *   chainRemovePartialOverlaps   chainConnect.c:255-344, chainMergeAbutting :346-368
 *   chainCalcScore               chainConnect.c:24-40       (GPU, gac_score_ranges)
 *   minScore filter + slSort(chainCmpScore)
 * Blocks of pair p are [blk_off[p], blk_off[p+1]) in the order axtChain holds
 * them before removeExactOverlaps (input order: the PSL/axt records and their
 * blocks as read).  Pairs are processed in the given order (spList order);
 * the kd-tree DP runs on host threads (n_threads, 0 = all cores), one pair at
 * a time per thread -- or, with GAC_AXT_DP=gpu in the environment, on the
 * device (gac_chain_dp, then the crossovers of scoreBlocks and
 * chainRemovePartialOverlaps through gac_crossovers); the output is the same.
 * Output chains are in chainWrite order; ids are 1..n.
 * details_path (may be NULL): axtChain -details text.  Installs mat/g on
 * the context (gac_set_scoring). */
typedef struct gac_axt_input {
    int64_t n_pairs;
    const int32_t *t_seq;    /* [n_pairs] gac_genome_seq_index(GAC_T) */
    const int32_t *q_seq;    /* [n_pairs] gac_genome_seq_index(GAC_Q) */
    const uint8_t *q_strand; /* [n_pairs] 0 '+', 1 '-' */
    const int64_t *blk_off;  /* [n_pairs + 1] */
    const int32_t *blk_t, *blk_q, *blk_size;
} gac_axt_input;

typedef struct gac_axt_chains {
    int64_t n_chains;
    double *score;           /* chainCalcScore (integral) */
    int32_t *pair;           /* seqPair index of each chain */
    int32_t *t_start, *t_end, *q_start, *q_end;
    int64_t *blk_off;        /* [n_chains + 1] */
    int64_t n_blocks;
    int32_t *blk_t, *blk_q, *blk_size;
} gac_axt_chains;

int gac_axt_chain(gac_ctx *ctx, const int32_t mat[16], const gac_gapcalc *g,
                  const gac_axt_input *in, double min_score, int n_threads,
                  const char *details_path, gac_axt_chains **out);
void gac_axt_chains_free(gac_axt_chains *c);

/* kent's chainBlocks (kent/src/lib/chainBlock.c:392-452) with the caller's
 * cost functions -- the kd-tree DP behind axtChain, for callers that bring
 * their own ConnectCost / GapCost (chainBlock.h:13-19): the DP runs on the
 * calling thread (host: it is a sequential branch-and-bound search by the
 * reference's definition), calling connect(a, b, user) /
 * gap(dq, dt, user) with block indices.  Blocks i: q [qs, qe), t [ts, te),
 * score[i]; zero-length blocks are skipped, as kent does.  Out: chains in
 * chainCmpScore order (stable), chain c = blocks blk[off[c] .. off[c+1])
 * ascending, score[c] = scoreBlocks (block scores minus connect costs).
 * details (may be NULL): peelChains' -details text. */
typedef int (*gac_connect_fn)(int32_t a, int32_t b, void *user);
typedef int (*gac_gapcost_fn)(int dq, int dt, void *user);
typedef struct gac_block_chains {
    int32_t n_chains;
    double *score;
    int32_t *off; /* [n_chains + 1] */
    int32_t *blk;
} gac_block_chains;
int gac_chain_blocks(int32_t n, const int32_t *qs, const int32_t *qe, const int32_t *ts,
                     const int32_t *te, const int32_t *score, gac_connect_fn connect,
                     gac_gapcost_fn gap, void *user, const char *qname, int32_t qsize, char qstrand,
                     const char *tname, int32_t tsize, FILE *details, gac_block_chains **out);
void gac_block_chains_free(gac_block_chains *c);

/* ---- chainNet netting engine (host, no device needed) -------------------
 * Replaces chainNet's netting and output (src/chainNet/chainNet.c:328-896):
 * makeChroms/addChainT/addChainQ/fillSpace/finishNet/rOutputFill/...
 * Same fills, gaps and .net text; no per-fill O(blocks) list rescans.  For
 * -rescore the caller scores the partial T fills with gac_score_ranges and
 * hands the scores to gac_net_write (subchainInfo's rescoring branch,
 * chainNet.c:826-836).  Input arrays are borrowed and must outlive the net. */
typedef struct gac_net gac_net;

typedef struct gac_net_input {
    int64_t n_chains;        /* in file order (chainNet requires descending score) */
    const double *score;     /* header score */
    const int32_t *id;       /* chain id */
    const int32_t *t_seq;    /* index into t_names/t_sizes */
    const int32_t *q_seq;    /* index into q_names/q_sizes */
    const uint8_t *q_strand; /* 0 '+', 1 '-' */
    const int32_t *t_start, *t_end, *q_start, *q_end;
    const int64_t *blk_off;  /* [n_chains + 1] */
    const int32_t *blk_t, *blk_q, *blk_size;
    int32_t n_tseq;          /* target chrom.sizes, file order */
    const char *const *t_names;
    const int32_t *t_sizes;
    int32_t n_qseq;          /* query chrom.sizes, file order */
    const char *const *q_names;
    const int32_t *q_sizes;
} gac_net_input;

typedef struct gac_net_opts {
    int32_t min_space; /* -minSpace, default 25 */
    int32_t min_fill;  /* -minFill, default min_space / 2 */
    double min_score;  /* -minScore, default 2000; 0 with -rescore */
    int32_t incl_hap;  /* -inclHap */
} gac_net_opts;

/* Net chains in order until the first one with score < min_score (error if
 * scores increase).  Chains on *_hap* / *_alt* queries are skipped unless
 * incl_hap. */
int gac_net_build(const gac_net_input *in, const gac_net_opts *opts, gac_net **out);
/* The same for the sides in `sides` only (bit 1 << GAC_T, bit 1 << GAC_Q):
 * the two sides' trees are independent, so a caller that writes only the
 * target net (chainCleaner's `chainNet ... stdout /dev/null`,
 * src/chainCleaner/chainCleaner.c:1660) skips the query side.  Fill queries
 * and writes of a side not built fail with GAC_E_STATE. */
int gac_net_build_sides(const gac_net_input *in, const gac_net_opts *opts, int sides,
                        gac_net **out);
/* The same for a subset of chromosome sides: t_keep[k] / q_keep[k] != 0 =
 * net target / query sequence k (a sequence's side depends only on the
 * chains on it, so ranks of a multi-GPU run each net their own sequences;
 * the unselected ones are written as if they held no chains). */
int gac_net_build_subset(const gac_net_input *in, const gac_net_opts *opts, const uint8_t *t_keep,
                         const uint8_t *q_keep, gac_net **out);
/* Diagnostic: the per-sequence chain lists of one side as gac_net_build
 * makes them on `nthreads` threads -- every chain of the input (no score
 * cut), haplotype queries left out unless incl_hap; off[n_seq + 1] = each
 * sequence's place in chains[], whose entries keep input order inside a
 * sequence.  chains[] holds up to n_chains entries. */
int gac_net_chain_lists(const gac_net_input *in, const gac_net_opts *opts, int side, int nthreads,
                        int64_t *off, int32_t *chains);
void gac_net_free(gac_net *net);
/* number of input chains consumed (netted or skipped) before stopping */
int64_t gac_net_netted(const gac_net *net);
/* fills of one side, in .net output (pre-order) order */
int64_t gac_net_fill_count(const gac_net *net, int side);
/* Per fill: chain index, start, end (own side, + strand), aligned bases
 * (subchainInfo's subSize) and flags: bit0 = partial (rescored on T with
 * -rescore), bit1 = printed by rOutputFill under -rescore (the fill and all
 * its ancestors have ali >= min_fill).  Any pointer may be NULL. */
int gac_net_get_fills(const gac_net *net, int side, int32_t *chain, int32_t *start,
                      int32_t *end, int32_t *ali, uint8_t *flags);
/* Per target fill, in gac_net_get_fills order: the window of the fill's chain
 * that chainSubsetOnT(chain, start, end) selects (gac_window's first_block /
 * n_blocks), recorded while netting.  side must be GAC_T. */
int gac_net_get_fill_windows(const gac_net *net, int side, int32_t *first_block,
                             int32_t *n_blocks);
/* The -rescore list in one pass: the target fills that are partial and
 * printed (gac_net_get_fills flags == 3), in pre-order, as gac_window
 * records (chain, start, end and their window) with each one's pre-order
 * position in `pos` (for gac_net_write's t_scores).  *windows and *pos are
 * malloc'ed (free them); *n = their count.  side must be GAC_T. */
int gac_net_rescore_windows(const gac_net *net, int side, gac_window **windows, int64_t **pos,
                            int64_t *n);
/* Write one side's .net (outputNetSide) to path ("stdout" allowed) after the
 * n_meta '#' metadata lines.  t_scores (T side only, may be NULL): per fill
 * in gac_net_get_fills order, the rescored global score of partial fills
 * (<= 0 prints as 1); NULL = reference's proportional approximation. */
int gac_net_write(const gac_net *net, int side, const int64_t *t_scores, const char *path,
                  const char *const *meta, int32_t n_meta);
/* The same, with a "formatted" signal: on_formatted(harg) (may be NULL) is
 * called once, from a worker thread, when the last piece of the side's text
 * is formatted (or from the caller when the side has no fill).  From then on
 * the call reads neither net, t_scores nor meta -- it only copies the text it
 * holds to the file and closes it -- so the caller may release them while the
 * write completes (gac_net_release).  The hook does not run when the call
 * fails before formatting starts (bad argument, the file does not open). */
int gac_net_write_ex(const gac_net *net, int side, const int64_t *t_scores, const char *path,
                     const char *const *meta, int32_t n_meta, void (*on_formatted)(void *),
                     void *harg);
/* Release the bulk of a net (the fill/gap records, the pre-order arrays)
 * ahead of gac_net_free, on several threads (GAC_FREE_THREADS; default 16,
 * with pages_only half the host threads).
 * pages_only != 0: only the pages go (madvise, which does not hold up other
 * threads' malloc/free the way unmapping does); gac_net_free unmaps the then
 * empty ranges.  Only gac_net_free (or another gac_net_release) may follow;
 * any other call on the net fails with GAC_E_STATE.  No gac_net_* call on
 * this net may be reading it: with gac_net_write_ex, call it once every
 * write in flight has signalled. */
void gac_net_release(gac_net *net, int pages_only);
/* The same text written to an open stream (e.g. an open_memstream buffer:
 * chainNet -nranks formats a rank's part in memory, then writes it in place). */
int gac_net_write_file(const gac_net *net, int side, const int64_t *t_scores, FILE *f,
                       const char *const *meta, int32_t n_meta);
/* The same text formatted on all threads and returned as buffers (chainNet
 * -nranks writes a rank's part in place from them, with no staging copy):
 * *bufs[0 .. *nbufs) in order, malloc'ed (free each and the arrays), *lens
 * their lengths; the n_meta '#' lines are the first buffer. */
int gac_net_format(const gac_net *net, int side, const int64_t *t_scores,
                   const char *const *meta, int32_t n_meta, char ***bufs, size_t **lens,
                   int64_t *nbufs);
/* The target net in two phases, for -rescore: _begin formats everything but
 * the rescored partial fills' scores (which fills print does not depend on
 * them when minScore <= 1: a rescored score is >= 1, chainNet.c:244-245),
 * e.g. while the GPU computes them; _end inserts the scores and writes the
 * same text as gac_net_write(..., t_scores, ...).  _free drops a prepared
 * net that is not written. */
typedef struct gac_net_wpre gac_net_wpre;
int gac_net_write_begin(const gac_net *net, int side, const char *const *meta, int32_t n_meta,
                        gac_net_wpre **out);
int gac_net_write_end(gac_net_wpre *w, const int64_t *t_scores, FILE *f);
void gac_net_write_free(gac_net_wpre *w);

/* ---- the -nranks collective (gac_allgather) ---------------
 * One process per GPU of one node.  A communicator joins `nranks` processes
 * through a rendezvous prefix: a path the ranks share and that is unique to
 * the run (the tools use their output path plus the run's GAC_RANK_TOKEN);
 * the host backend keeps its part and barrier files next to it.
 *   GAC_COMM_RCCL  ncclAllGather over xGMI (librccl loaded at run time; the
 *                  unique id passes through the rendezvous files), `device`
 *                  = this rank's GPU; RCCL refuses two ranks on one device.
 *   GAC_COMM_HOST  part files in the node's page cache, no device.
 *   GAC_COMM_AUTO  GAC_COMM=rccl|host if set, else RCCL when device >= 0.
 * A wait gives up after timeout_s seconds (<= 0: 600) or when alive(peer,
 * user) returns 0 (NULL: no check), with GAC_E_STATE.  Every rank must make
 * the same calls in the same order. */
typedef struct gac_comm gac_comm;
#define GAC_COMM_AUTO 0
#define GAC_COMM_HOST 1
#define GAC_COMM_RCCL 2
int gac_comm_open(const char *rendezvous, int nranks, int rank, int device, int backend,
                  double timeout_s, int (*alive)(int rank, void *user), void *user,
                  gac_comm **out);
int gac_comm_backend(const gac_comm *comm); /* GAC_COMM_HOST / GAC_COMM_RCCL */
double gac_comm_init_seconds(const gac_comm *comm); /* RCCL set-up time (0: host) */
/* ncclAllGather: `bytes` from every rank; recv holds nranks * bytes, rank r's
 * part at r * bytes.  Host buffers, synchronous. */
int gac_allgather(gac_comm *comm, const void *send, size_t bytes, void *recv);
/* parts of any size: *recv = malloc'd concatenation in rank order (free()),
 * counts[0 .. nranks) = each rank's bytes */
int gac_allgatherv(gac_comm *comm, const void *send, size_t bytes, void **recv, size_t *counts);
int gac_comm_barrier(gac_comm *comm);
void gac_comm_close(gac_comm *comm);

/* ---- device memory helpers (for callers without their own allocator) ---- */
int gac_dev_alloc(gac_ctx *ctx, size_t bytes, void **dptr);
int gac_dev_free(gac_ctx *ctx, void *dptr);
/* Synchronous copies, ordered after all work enqueued on the context's stream. */
int gac_memcpy_h2d(gac_ctx *ctx, void *dst, const void *src, size_t bytes);
int gac_memcpy_d2h(gac_ctx *ctx, void *dst, const void *src, size_t bytes);
int gac_synchronize(gac_ctx *ctx);

/* ---- kernel timing (HIP events on the launch stream) -------------------- */
#define GAC_K_PLAN 0     /* block-window search + scans + tile map (k_plan, k_tilemap_fused or k_scan_agg + k_tilemap) */
#define GAC_K_TILE 1     /* tile scoring: bases, gaps, per-tile scan (dominant) */
#define GAC_K_COMBINE 2  /* multi-tile range combine */
#define GAC_K_DEPTH 3    /* gac_depth_count: events, sort, scans, counts (one lap per call) */
#define GAC_K_PRENET 4   /* gac_prenet_keep: every pass's fill, scans, mark and check (one lap per call) */
#define GAC_K_AXTFILTER 5 /* gac_axt_filter: the window kernel (one lap per batch) */
#define GAC_K_AXTPSL 6    /* gac_axt_psl: count, scan and emit (one lap per batch) */
#define GAC_K_AXTSCORE 7  /* gac_axt_score: chunk counts, scan and the score kernel (one lap per batch) */
#define GAC_K_COUNT 8
#define GAC_PROF_ALL ((1 << GAC_K_COUNT) - 1)
/* Event timing of each launch of the kernels in `mask` (bits 1 << GAC_K_*;
 * 0 = off, GAC_PROF_ALL = all).  Each timed kernel adds two event markers
 * to the stream. */
int gac_prof_enable(gac_ctx *ctx, int mask);
/* Synchronise, fold recorded events, and return total ms + launch count of
 * kernel `k` since the last reset. */
int gac_prof_read(gac_ctx *ctx, int k, double *total_ms, int64_t *launches);
int gac_prof_reset(gac_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* GACHAIN_H */
