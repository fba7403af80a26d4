// gac_kernels.h -- device data layout shared by the HIP kernels and the
// C-ABI implementation (gac_device.hip and the gac_abi_*.hip units), and the one declaration of
// every launcher of gac_kernels.hip, gac_compose.hip, gac_axtout.hip, gac_depth.hip,
// gac_prenet.hip, gac_axtfilter.hip, gac_axtpsl.hip and gac_axtscore.hip (each includes this header, so its definitions are checked against it).
// gfx950 only.
//
// HBM layout (see DESIGN.md "Data layout in HBM"):
//   genome side (T or Q): 32 bases per "word"
//     planes[w] : uint2 {x = bit0 plane, y = bit1 plane} of 2-bit codes
//                 T=0 C=1 A=2 G=3 (the .2bit code; kent dnautil.h:23-28),
//                 base 32w+i at bit i of each plane
//     nmask[w]  : uint32, bit i set = base 32w+i is N (or padding)
//     every sequence starts on a word boundary; word_off[s] = first word
//   chains: DChain[c] + blocks blk[b] = int4 {tStart, qStart, size | flags, gap}
//     flags (bits 29/30 of .z): the block's target/query bases contain an N
//     (precomputed at upload; blocks without N skip the N-mask loads)
//     gap: gapCalcCost to the chain's next block (k_block_gaps_flat, per scoring
//     setup; 0 after the last block)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gachain.h"

namespace gac {

constexpr int kWave = 64;        // CDNA wavefront
constexpr int kTileBlocks = 64;  // blocks per tile (one per lane)
constexpr int kWavesPerWG = 4;   // 256-thread workgroups
constexpr int kMaxLong = 32;     // long gap positions
constexpr long long kNeg = -(1LL << 61);  // -inf of the local-score monoid
constexpr int kSizeMask = (1 << 29) - 1;  // block size field of blk[].z
constexpr int kTHasN = 1 << 29;           // blk[].z: target bases contain an N
constexpr int kQHasN = 1 << 30;           // blk[].z: query bases contain an N

// Compact copy of the block records for k_tile (12 B instead of 16: fewer
// 128-B lines per scored window), written with the gaps per scoring setup:
// {tStart, qStart, w}, w = size (bits 0-11) | gap (bits 12-29) | tN << 30 |
// qN << 31.  A block of kB12Wide or more bases, or a gap costing 2^18 - 1 or
// more, has size field kB12Wide: k_tile reads its 16-B record instead.
struct Blk12 {
    int32_t t, q;
    uint32_t w;
};
static_assert(sizeof(Blk12) == 12, "Blk12 layout");
constexpr int kB12Wide = 0xFFF;
constexpr int kB12GapMax = (1 << 18) - 1;

struct DChain {
    int64_t blk_off;
    int32_t nblk;
    int32_t t_seq;
    int32_t q_seq;
    int32_t qinfo;     // q_seq size (reverse-complement index base) | strand << 31
    int32_t tstart;    // target span of the blocks
    int32_t tend;
    int64_t idx_off;   // this chain's bucket index in ScoreArgs::bucket
    int32_t shift;     // bucket width = 2^shift target bases
    int32_t pad;
    int64_t tbase;     // global base index of the target sequence start (word_off * 32)
    int64_t qbase;     // '+': global base index of the query sequence start;
                       // '-': ~(word_off * 32 + qSize)  (as RangeDesc::qbase)
};
static_assert(sizeof(DChain) == 64, "DChain layout: one 64-byte record");

// Bucket index of a chain (built at upload): the target span [tstart, tend)
// is cut into nb = ((tend - tstart - 1) >> shift) + 1 buckets of 2^shift
// bases (shift chosen so that nb <= 2 * blocks), and
//   bucket[idx_off + k] = first block with tEnd > tstart + (k << shift),
//   bucket[idx_off + nb] = blocks.
// The first block with tEnd > s then lies in [bucket[k], bucket[k + 1]],
// k = (s - tstart) >> shift: one 8-byte load plus a search of that bracket
// (usually one or two blocks) replaces a log2(blocks) binary search.

struct GapDev {
    int32_t small_size;
    int32_t long_count;
    int32_t last_pos[3];  // q, t, both
    int32_t pad;
    double last_val[3];
    double last_slope[3];
    int32_t long_pos[kMaxLong];
    double long_val[3][kMaxLong];
};

// A scoring setup's gap costs for the upload kernels (k_block_gaps_flat, and
// k_build_flat when the setup precedes the chains): blk12 null = none.
struct UploadGaps {
    Blk12 *blk12;
    GapDev g;
    const int32_t *small, *tab;
    int len;
};

// Per-range descriptor written by k_plan (two 16-B loads in k_tile).
struct RangeDesc {
    int64_t tbase;   // global base index of the target sequence start (word_off * 32)
    int64_t qbase;   // '+': global base index of the query sequence start
                     // '-': ~(word_off * 32 + qSize)  (negative)
    int32_t b0;      // first block of the window (global block index)
    int32_t nblk;    // blocks in the window
    int32_t s, e;    // target clip range
};
static_assert(sizeof(RangeDesc) == 32, "RangeDesc layout");

// Partial result of a range segment inside one tile: additive parts + the
// local-score max-plus element  s_out = max(s_in + A, B); m_out = max(m_in, s_in + C, D)
struct SegSum {
    long long g;    // sum(block) - sum(gap)
    long long ali;  // aligned bases
    long long A, B, C, D;
};

struct Range {
    int32_t chain, t_start, t_end;
};

// A range with its window of blocks known to the caller (gac_window):
// chain-local first block and count (chainSubsetOnT's window of
// [t_start, t_end)).
struct Window {
    int32_t chain, t_start, t_end, first, nblk;
};
static_assert(sizeof(Window) == 20, "Window layout (gac_window)");

// Result of one range of a small batch (k_small writes it straight to pinned
// host memory).
struct SmallOut {
    long long g, l;
    int32_t ali, pad;
};

struct ScoreArgs {
    const uint2 *t_planes;
    const uint32_t *t_nmask;
    const int64_t *t_woff;
    const uint2 *q_planes;
    const uint32_t *q_nmask;
    const int64_t *q_woff;
    const DChain *chains;
    int64_t n_chains;
    const int4 *blk;     // [n_blocks + 8] {tStart, qStart, size | N flags, gap to next}
    const Blk12 *blk12;  // [n_blocks] the same, compact (k_tile)
    const int2 *tspan;   // [n_blocks + 8] {tStart, tEnd} (window searches; padded)
    const uint32_t *bucket;  // chain bucket indexes (see DChain)
    const Range *ranges;
    const Window *wins;  // non-null: the ranges come with their windows (k_plan<true>)
    int64_t n;
    // workspace
    RangeDesc *rdesc;    // [n]
    int32_t *nblk;       // [n]   window blocks per range
    int32_t *goff;       // [n]   exclusive scan of nblk inside the plan workgroup
    int32_t *pb0;        // [n]   first window block (compact copy of rdesc.b0)
    int32_t *gflat;      // [n]   flat offset of each range's first window block
    int32_t *tile_r0;    // [T]   range owning each tile's first flat block
    SegSum *sum_head;    // [T]   partial segment containing the tile's first block
    SegSum *sum_tail;    // [T]   partial segment containing the tile's last block
    // cross-tile fold (k_fold_tiles / k_fold_super), per super-tile of 64 tiles
    SegSum *sup_head;    // [U]   fold of the heads, in super-tile u, of a range begun before it
    SegSum *sup_tail;    // [U]   prefix of the range that continues past super-tile u
    int32_t *sup_tail_r; // [U]   that range, or -1
    int32_t *agg;        // [G]   window blocks of each plan workgroup (k_plan; saturated)
    int32_t *plan_off;   // [G+1] flat offset of plan workgroup w
    unsigned long long *lbflag;  // [G] k_plan_lb's look-back words {value, call tag, state}
    int32_t *status;     // [32]  W (flat blocks, saturated), T (tiles), 1 = workspace too
                         //       small; status[5]: a window lay outside its chain (k_plan<true>,
                         //       published to host_status[3] and cleared); status[8]:
                         //       k_plan_lb's workgroup tickets (re-armed by the last one)
    int32_t *host_status;  // pinned host words: status[0..4) + call_tag (k_scan_agg)
    int32_t call_tag;
    int32_t cap_tiles;   // tile_r0 / sum_head / sum_tail capacity
    // outputs
    long long *out_g;
    long long *out_l;
    int32_t *out_ali;
    int32_t want_local;
    int32_t gap_len;           // gap_tab entries per kind
    const int32_t *gap_tab;    // [3][gap_len] gapCalcCost by kind (q, t, both) and length
    const int32_t *small_tab;  // [3][small_size] q, t, both
    int32_t coef[16];          // score matrix in the multilinear basis of the bits
                               // (t1, t0, d1, d0), d = q ^ t: coef[S], S = t1<<3 |
                               // t0<<2 | d1<<1 | d0 (set bits = factors)
    int32_t sym;               // matrix is strand-symmetric: coef[8..15] == 0
    int32_t scan64;            // A/B probe (GAC_TILE_SCAN64=1): k_tile's 64-bit scans only
    int32_t xcd_chunk;         // A/B probe (GAC_TILE_XCD=1): each XCD takes one contiguous
                               // eighth of the tiles (default: per-round XCD blocks)
    GapDev gap;
    const int32_t *out_perm;  // non-null: the results of range (position) p go to
                              // chain out_perm[p] (the whole-chain plan in target order)
    const int32_t *tile_perm; // non-null: k_tile's schedule, tile_perm[k] = the k-th tile
                              // scored (whole chains: target order of the tiles' first blocks)
};

constexpr int kSmallMax = 256;  // ranges per small-batch call

// k_small_server's mailbox, in pinned coherent host memory: the host writes
// kind, n and the inputs, then req; the server writes done, and state = 2
// when it exits (idle or stop)
// k_small_server's mailbox, in pinned coherent host memory: the host writes
// kind, n and the inputs, then req; the server writes done, and state = 2
// when it exits (idle or stop)
struct SmallMail {
    uint32_t req;    // host: the request word (written last, srv_word)
    uint32_t kind;   // (unused)
    uint32_t n;      // (unused)
    uint32_t stop;   // host: 1 = exit now
    uint32_t done;   // server: the last completed request
    uint32_t state;  // server: 2 = exited
    uint32_t pad[26];
};
// its device-side copy for the other workgroups (the request number, kind
// and range count, read from the mailbox by workgroup 0 only) and the
// completion count: uncached device memory, zeroed per launch
struct SmallSync {
    uint32_t seq, kind, n, cnt;
    uint32_t pad[28];  // (GAC_SRV_TRACE's phase words)
};
constexpr int kSrvWaves = 256;  // resident server waves at most (64 workgroups)
// the request word: bits 0-19 the request number (never 0), 20-28 the range
// count (<= kSmallMax), 29 the kind (0: Range batch of the uploaded set; 1:
// host-planned RangeDesc + pool); 0xffffffff (never a request) = exit
__host__ __device__ constexpr uint32_t srv_word(uint32_t seq, uint32_t kind, uint32_t n) {
    return (seq & 0xfffffu) | ((n & 0x1ffu) << 20) | ((kind & 1u) << 29);
}

// Genome upload (k_relayout): one sequence's place in the staged raw .2bit
// payloads and in the planes.
struct SeqDev {
    int64_t byte_off;  // into staging
    int64_t word_off;  // into planes
    int32_t size;
    int32_t pad;
};

// An N run (or soft-mask run) for k_nruns, pre-split on the host into pieces
// of <= 1024 bases.
struct NPiece {
    int64_t bit0;  // global base index (word_off*32 + start)
    int32_t len;
    int32_t pad;
};

// One run of a sparse genome upload (bytes): its place in the staging layout
// (8-byte aligned), its offset in the packed upload (8-byte aligned), length.
struct SparseRun {
    int64_t dst, src, len;
};

// One ungapped block for k_blocks (axtScoreUngapped): global plane positions
// of its first target base and, for the query, of its first base ('+') or
// one past its last base on the forward strand ('-').
struct BlockJob {
    int64_t tp, qp;
    int32_t n;
    int32_t minus;
};

// Text jobs of the kent-API shims (k_text_blocks / k_text_xover): offsets
// into one uploaded byte buffer of caller text.
struct TextJob {
    int64_t q, t;  // offsets of the query / target text
    int32_t n;     // bases
    int32_t pad;
};

struct TextXJob {
    int64_t lq, lt, rq, rt;  // left block's last `ov` bases, right block's first
    int32_t ov;
    int32_t pad;
};

struct M25 {  // score by text code, [q * 5 + t]; code 4 (not acgt) scores 0
    int32_t m[25];
};

// The per-chain base counts of an uploaded set (gac_compose.hip): what the
// walk over the aligned bases reads.  lmask[w]: the opt-in soft-mask plane of
// a genome side, indexed like nmask -- bit i set = base 32w+i lies in a .2bit
// mask run (lower case with twoBitReadSeqFragExt's doMask); padding words and
// tail bits are 0.
struct ChainWalkArgs {
    const uint2 *t_planes, *q_planes;
    const uint32_t *t_nmask, *q_nmask, *t_lmask, *q_lmask;
    const DChain *chains;
    const int4 *blk;
    const int32_t *coff, *tile_c0;  // the chain set's compact offsets / tile chains
    int64_t n_chains, n_blocks, ntiles;
};

// k_compose: chainAntiRepeat's match composition
struct ComposeArgs : ChainWalkArgs {
    unsigned long long *match;  // [n_chains][4] by code T, C, A, G (zeroed by the caller)
    unsigned long long *rep;    // [n_chains]
    unsigned long long *total;  // [n_chains]
};

// k_psl_counts: chainToPsl's counts; q_lmask is not read (may be NULL)
struct PslArgs : ChainWalkArgs {
    unsigned long long *counts;  // [n_chains][4] match, misMatch, repMatch, nCount (zeroed by the caller)
};

// k_axt_stat / k_axt_render (gac_axtout.hip): pieces (block windows of chains,
// gac_window; t_start / t_end are read in clip mode only) measured and written out as
// alignment rows.  The pieces' blocks laid end to end are the call's virtual
// blocks: pboff[p] = first virtual block of piece p, V = pboff[n].
constexpr int kAxtBadWindow = 1;  // status[0] bits: a window outside its chain
constexpr int kAxtBadGap = 2;     // a negative or double-sided gap inside a piece
constexpr int kAxtBadOut = 4;     // a piece's rows outside the text buffer
constexpr int kAxtBadClip = 8;    // clip mode: a piece's first or last block left empty
struct AxtArgs {
    const uint2 *t_planes, *q_planes;
    const uint32_t *t_nmask, *q_nmask, *t_lmask, *q_lmask;
    const DChain *chains;
    const int4 *blk;
    int64_t n_chains;
    const Window *pieces;  // [n]
    int64_t n, V;
    int32_t clip;          // host only: the launchers pick the kernels that read t_start / t_end
                           // (netToAxt's clipped first and last block, chain.c:513-522)
    int64_t *pboff;        // [n + 1]
    int64_t *part;         // [max(n, V) / 2048 + 2] the scans' workgroup totals
    int32_t *status;       // [1] kAxtBad* bits (zeroed by the caller)
    // measure
    unsigned long long *acc;  // [n][4] score, match, ali, sym (zeroed by the caller)
    int32_t *score;           // [n]
    int64_t *match, *ali, *sym;
    // render
    int64_t *S;              // [V + 1] exclusive scan of the virtual blocks' columns
    const int64_t *offsets;  // [n] byte offset of each piece's rows (null: packed in order)
    int64_t *off;            // [n] the offsets used
    char *out;
    int64_t out_bytes;
};

// k_axt_pairs (gac_axtout.hip): the plan fields of AxtArgs and the two result
// arrays, which the workgroups add into directly
struct AxtPairArgs : AxtArgs {
    unsigned long long *pairs;  // [n][16] q * 4 + t, A,C,G,T order (zeroed by the caller)
    unsigned long long *ncols;  // [n] columns with an N on either side (zeroed by the caller)
};

// k_cut_* (gac_axtout.hip): ranges (chain, tStart, tEnd) to the clipped pieces
// chainToAxt(chainSubsetOnT(...)) makes.  The ranges' selected blocks laid end
// to end are the call's virtual blocks: rboff[r] = first of range r.
struct AxtCutArgs {
    const DChain *chains;
    const int4 *blk;
    int64_t n_chains;
    const Range *ranges;  // [n]
    int64_t n, V, P;      // ranges, virtual blocks, pieces
    int32_t max_gap;
    int32_t *rfirst;      // [n] chain-local first block of each range
    int64_t *rboff;       // [n + 1]
    int64_t *pidx;        // [V + 2] break flags, then their exclusive scan (pidx[V] = P)
    int64_t *part;        // [max(n, V) / 2048 + 2]
    int32_t *status;      // [0] kAxtBad* bits, [1] the lowest range with a negative gap
    Window *pieces;       // [P]
    int64_t *first;       // [n + 1]
};

// ---- launchers and launch helpers of gac_kernels.hip
int plan_grid(int64_t n);
int persistent_blocks_per_cu(int which, int sym);
hipError_t launch_plan(const ScoreArgs &a, hipStream_t s);
hipError_t launch_tilemap(const ScoreArgs &a, hipStream_t s);
hipError_t launch_plan_lb(const ScoreArgs &a, hipStream_t s);
bool plan_lb();
hipError_t launch_tile(const ScoreArgs &a, int grid, hipStream_t s);
hipError_t launch_combine(const ScoreArgs &a, int grid, hipStream_t s);
hipError_t launch_small(const ScoreArgs &a, const Range *rin, SmallOut *out, hipStream_t s);
hipError_t launch_small_host(const ScoreArgs &a, const RangeDesc *hin, const int4 *pool,
                             SmallOut *out, hipStream_t s);
hipError_t launch_small_server(const ScoreArgs &a0, const ScoreArgs &a1, const Range *rin,
                               const RangeDesc *hin, const int4 *pool, SmallOut *out,
                               SmallMail *mail, SmallSync *sy, uint32_t last_done, uint64_t idle,
                               uint32_t trace, int wgs, hipStream_t s);
hipError_t launch_relayout(const uint8_t *raw, const SeqDev *seqs, int nseq, int64_t nwords,
                           uint2 *planes, uint32_t *nmask, hipStream_t s);
hipError_t launch_gap_table(const GapDev &g, const int32_t *small, int len, int32_t *tab,
                            hipStream_t s);
hipError_t launch_nruns(const NPiece *p, int64_t n, uint32_t *nmask, hipStream_t s);
hipError_t launch_build_index(const int32_t *bt, const int32_t *bq, const int32_t *bs, int64_t nb,
                              const DChain *chains, int64_t n_chains, const int32_t *coff,
                              const int32_t *tile_c0, int2 *tspan, uint32_t *bucket,
                              hipStream_t s);
hipError_t launch_build_flat(const int32_t *bt, const int32_t *bq, const int32_t *bs, int64_t nb,
                             const DChain *chains, int64_t n_chains, int32_t *coff,
                             int32_t *tile_c0, int4 *crun, const longlong2 *t_runs,
                             int64_t n_trun, const longlong2 *q_runs, int64_t n_qrun,
                             const int64_t *q_woff, int4 *blk, int2 *tspan, uint32_t *bucket,
                             const UploadGaps &G, bool index, hipStream_t s);
hipError_t launch_block_gaps_flat(const int32_t *coff, const int32_t *tile_c0, int64_t nb,
                                  int4 *blk, Blk12 *blk12, const UploadGaps &G, hipStream_t s);
hipError_t launch_scatter(const SparseRun *runs, int64_t n, const uint64_t *compact,
                          uint64_t *raw, hipStream_t s);
hipError_t launch_blocks(const ScoreArgs &a, const BlockJob *jobs, int64_t n, int32_t *out,
                         hipStream_t s);
hipError_t launch_whole_plan(const DChain *chains, int64_t n, RangeDesc *rdesc, int32_t *nblk,
                             int32_t *gflat, int32_t *tile_r0, hipStream_t s);
hipError_t launch_zero_list(const int32_t *list, int64_t n, long long *g, long long *l,
                            int32_t *ali, hipStream_t s);
hipError_t launch_tile_order(const DChain *chains, const int4 *blk, const int32_t *tile_r0,
                             int64_t T, unsigned long long *keys, int32_t *vals, int32_t *perm,
                             void *tmp, size_t &tmp_bytes, hipStream_t s);
hipError_t launch_whole_plan_sorted(const DChain *chains, int64_t n, int32_t *perm,
                                    unsigned long long *keys, int32_t *vals, RangeDesc *rdesc,
                                    int32_t *nblk, int32_t *gflat, int32_t *pb0,
                                    int32_t *tile_r0, int32_t *inv, void *tmp,
                                    size_t &tmp_bytes, hipStream_t s);
hipError_t launch_text_blocks(const uint8_t *text, const TextJob *jobs, int64_t n, const M25 &m,
                              long long *out, hipStream_t s);
hipError_t launch_text_xover(const uint8_t *text, const TextXJob *jobs, int64_t n, const M25 &m,
                             int32_t *pos, int32_t *adj, hipStream_t s);
// ---- gac_compose.hip
hipError_t launch_compose(const ComposeArgs &a, hipStream_t s);
hipError_t launch_psl_counts(const PslArgs &a, hipStream_t s);
// ---- gac_axtout.hip
hipError_t launch_axt_plan(const AxtArgs &a, hipStream_t s);
hipError_t launch_axt_stat(const AxtArgs &a, hipStream_t s);
hipError_t launch_axt_pairs(const AxtPairArgs &a, hipStream_t s);
hipError_t launch_axt_place(const AxtArgs &a, hipStream_t s);
hipError_t launch_axt_render(const AxtArgs &a, hipStream_t s);
hipError_t launch_axt_cut_find(const AxtCutArgs &a, hipStream_t s);
hipError_t launch_axt_cut_flag(const AxtCutArgs &a, hipStream_t s);
hipError_t launch_axt_cut_emit(const AxtCutArgs &a, hipStream_t s);

// ---- gac_depth.hip: coverage depth of n ranges (gac_depth_count).  Event e
// < n is the start of range e, event n + i the end of range i; arrays of 2n
// unless noted.
struct DepthArgs {
    int64_t n;
    int32_t threshold;
    const int32_t *seq, *start, *end;  // [n]
    const int8_t *delta;               // [n]
    unsigned long long *key;           // (seq << 32) | position, by event
    int32_t *val;                      // the event id, by event
    const unsigned long long *skey;    // the keys sorted
    const int32_t *sval;               // the events in that order
    int32_t *sdelta;                   // their signed deltas
    int32_t *where;                    // by event: its sorted position
    const int32_t *excl;               // exclusive scan of sdelta
    long long *len;                    // covered length from k to k + 1
    const long long *before;           // exclusive scan of len
    int32_t *count;                    // [n]
};
hipError_t launch_depth_events(const DepthArgs &a, hipStream_t s);
hipError_t launch_depth_gather(const DepthArgs &a, hipStream_t s);
hipError_t launch_depth_cover(const DepthArgs &a, hipStream_t s);
hipError_t launch_depth_out(const DepthArgs &a, hipStream_t s);

// ---- gac_prenet.hip: chainPreNet's keep decision (gac_prenet_keep).  A pass
// works on one side (0 target, 1 query) and one group of its sequences: the
// words fc[sbase[seq] + position] of the group's sequences hold the lowest
// rank (chain index) that covers the base, kPrenetNone = nothing.
constexpr uint32_t kPrenetNone = 0xffffffffu;
constexpr uint8_t kPrenetUndecided = 0, kPrenetKept = 1, kPrenetDropped = 2, kPrenetSkipped = 3;
struct PrenetArgs {
    int64_t n, nb;                // chains, blocks
    int32_t pad;
    int32_t side, group;          // this pass
    int32_t with_undecided;       // the covering set: 1 = kept and undecided chains, 0 = kept only
    const int64_t *boff;          // [n + 1]
    const int32_t *seq[2];        // [n] per side, -1 = skipped
    const int32_t *bstart[2];     // [nb] per side
    const int32_t *bsize;         // [nb]
    int32_t *bchain;              // [nb] the chain of every block
    const int32_t *ssize[2];      // per side [sequences]
    const int32_t *sgroup[2];     // the group of every sequence (-1: no counted chain names it)
    const int64_t *sbase[2];      // its first word in its group's fc
    uint8_t *state;               // [n] kPrenet*
    uint8_t *open;                // [n] 1 = an open base found in this pass
    long long *len;               // [nb + 1] flat bases of every block in this step (0: not in it)
    const long long *off;         // [nb + 1] their exclusive scan; off[nb] = the total
    long long *badr;              // [nb] the fc word of a block's first flat base in this step
    uint32_t *fc;
    unsigned long long *counts;   // [2] chains left undecided, chains kept (k_prenet_decide adds)
};
hipError_t launch_prenet_setup(const PrenetArgs &a, hipStream_t s);
// the flat lengths of the covering chains' padded blocks / the undecided chains' blocks
hipError_t launch_prenet_len(const PrenetArgs &a, bool mark, hipStream_t s);
hipError_t launch_prenet_mark(const PrenetArgs &a, hipStream_t s);
hipError_t launch_prenet_check(const PrenetArgs &a, hipStream_t s);
// after a round's first pass: open undecided chains are kept; after its second:
// undecided chains that are not open are dropped, and the counts are added up
hipError_t launch_prenet_decide(const PrenetArgs &a, int pass, hipStream_t s);
hipError_t launch_prenet_flags(const PrenetArgs &a, uint8_t *keep, hipStream_t s);

// ---- gac_axtfilter.hip: filterAxtIdentityEntropy's window test (gac_axt_filter).
// The unit of work is a chunk: up to kAxtfTile - window consecutive window
// starts of one entry, whose kAxtfTile - 1 columns at most are one workgroup's
// tile.  ent[i].chunk0 = the first chunk of entry i (ent[n].chunk0 = all
// chunks; an entry shorter than the window has none).
constexpr int kAxtfTile = 2048;       // columns of a tile, one less used: the packed prefix
                                      // counts are 11-bit fields (<= 2047)
constexpr int kAxtfMaxWindow = 1024;  // GAC_AXTF_MAX_WINDOW: a chunk keeps >= 1024 starts
struct AxtfEntry {
    int64_t t, q;    // byte offsets of the rows in text
    int32_t len;     // columns
    int32_t pad;
    int64_t chunk0;
};
static_assert(sizeof(AxtfEntry) == 32, "AxtfEntry layout");
struct AxtfArgs {
    const uint8_t *text;
    int64_t text_bytes;
    const AxtfEntry *ent;  // [n + 1]
    int64_t n;
    int32_t window, m_min;  // a window passes the identity test with >= m_min matches
    const double *term;     // [window (window + 1) / 2] p log p at n (n - 1) / 2 + k - 1
    double ln2, min_entropy;
    uint32_t *keep;  // [n] one word an entry (zeroed by the caller): passing chunks store 1
};
// enforces 1 <= window <= kAxtfMaxWindow (the tile bound) and the grid limit
hipError_t launch_axt_filter(const AxtfArgs &a, int64_t chunks, hipStream_t s);

// ---- gac_axtpsl.hip: axtToPsl's counts and blocks (gac_axt_psl).  A wave
// walks an entry in tiles of kAxtpTile columns; the count pass writes the
// entries' records and block counts, the emit pass (after the 64-bit scan of
// the counts) the blocks at boff[i] on.
constexpr int kAxtpTile = GAC_AXTPSL_TILE;
struct AxtpEntry {
    int64_t t, q;  // byte offsets of the rows in text
    int32_t len;   // columns
    int32_t pad;
};
static_assert(sizeof(AxtpEntry) == 24, "AxtpEntry layout");
struct AxtpArgs {
    const uint8_t *text;
    int64_t text_bytes;
    const AxtpEntry *ent;   // [n]
    int64_t n;
    gac_axtpsl_entry *out;  // [n] block0 is written by the emit pass (relative to the batch)
    long long *nblk;        // [n + 1] blocks of every entry (the caller zeroes nblk[n])
    const long long *boff;  // [n + 1] their exclusive scan
    gac_axtpsl_block *blk;  // [nb]
    int64_t nb;             // boff[n]: no block is written at or past it
};
hipError_t launch_axt_psl_count(const AxtpArgs &a, hipStream_t s);
hipError_t launch_axt_psl_emit(const AxtpArgs &a, hipStream_t s);

// ---- gac_axtscore.hip: axtScoreSym under the default scheme (gac_axt_score).
// The unit of work is a chunk: up to kAxtsChunk consecutive columns of one
// entry, summed by one wave.  launch_axt_score_chunks writes every entry's
// number of chunks, the shared 64-bit scan (dt_scan64) turns them into first
// chunks, and launch_axt_score adds each chunk's sum into its entry's score.
constexpr int kAxtsChunk = GAC_AXTSCORE_CHUNK;
struct AxtsEntry {
    int64_t t, q;  // row offsets into the batch's text
    int32_t len, pad;
};
static_assert(sizeof(AxtsEntry) == 24, "AxtsEntry layout");
struct AxtsArgs {
    const uint8_t *text;
    int64_t text_bytes, n;
    const AxtsEntry *ent;      // [n]
    long long *nchunk;         // [n + 1] written by the chunks pass; [n] zeroed by the caller
    const long long *chunk0;   // [n + 1] exclusive scan of nchunk
    uint32_t *score;           // [n] zeroed by the caller; sums modulo 2^32
};
hipError_t launch_axt_score_chunks(const AxtsArgs &a, hipStream_t s);
hipError_t launch_axt_score(const AxtsArgs &a, int64_t chunks, hipStream_t s);

}  // namespace gac
