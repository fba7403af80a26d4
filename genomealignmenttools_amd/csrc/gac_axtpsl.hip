// gac_axtpsl.hip -- axtToPsl's column loop (gac_axt_psl; kent/src/lib/psl.c:
// 1634-1665 trimAlignment, :1680-1714 accumCounts, :1716-1806 pslFromAlign):
// the counts, the trim and the blocks of an alignment's two rows.  gfx950 only.
//
// pslFromAlign is a state machine over the columns.  Here every column gets a
// kind -- 0 a gap in both rows (skipped), 1 no gap, 2 a gap in the query
// (target insert), 3 a gap in the target (query insert) -- and the machine
// becomes sums and "last value" scans over the kinds:
//   prev(j)   the kind of the last column before j that is not 0 (0: none)
//   F, E      the first and the last column of kind 1: the trim keeps [F, E]
//   start     a column of kind 1 with prev != 1 opens a block; its index is
//             the number of starts before it, and it lies q_adv = the columns
//             of kind 1 and 3 in [F, j) and t_adv = those of kind 1 and 2
//             after the first kept column
//   end       a column of kind 2 or 3 with prev == 1 closes the open block:
//             size = the columns of kind 1 before j - those before its start
//             (the last value scan of the starts); a block still open at the
//             entry's end is closed there
//   inserts   a column of kind 2 with prev != 2 after F adds to tNumInsert,
//             one of kind 3 with prev != 3 to qNumInsert; those after E are
//             the tail's and are taken off with a snapshot at E
// Nothing of this needs to know the trim in advance: F is where the count of
// kind 1 is still zero, and whatever is counted inclusively at the last kind-1
// column seen so far is the value at E when the entry ends.
//
// A workgroup of one wave takes an entry and walks it in tiles of kAxtpTile
// columns; what crosses a tile edge -- the counts so far, prev, the open
// block's start, the snapshots at F and E -- is wave-uniform and stays in
// registers.  In a tile:
//   load    lane-consecutive bytes of both rows, classified on the way into
//           one code byte per column in LDS (kind, and for kind 1 which count
//           it adds to); a lane then takes its 8 consecutive codes as one word
//   scan 1  the kinds' counts (three 10-bit fields, a tile has 512 columns)
//           and the last kind, across the lanes by shuffles
//   walk    a lane walks its 8 columns from prev and its exclusive counts:
//           starts, insert openings and the counts of kind 1 (six 10-bit
//           fields of one 64-bit word), its last start
//   scan 2  those, the same way
//   emit    (second pass only) the lane walks its columns again and stores
//           q_adv / t_adv at every start and the size at every end
// The count pass stores the entry's record and its number of blocks; the
// blocks of all entries are placed by a 64-bit exclusive scan of those
// (dt_scan64), and the emit pass repeats the walk and writes every block at
// its place.  No workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kAxtpPer = kAxtpTile / kWave;  // columns a lane walks
constexpr int64_t kAxtpMaxGrid = 1 << 20;    // workgroups; the rest by grid stride
constexpr int kAxtpBits = 10;                // a packed field
constexpr unsigned kAxtpField = (1u << kAxtpBits) - 1;
static_assert(kAxtpPer == 8, "a lane's columns are one 64-bit LDS word of codes");
static_assert(kAxtpTile <= (int)kAxtpField, "a tile's counts fit a packed field");

// code byte of a column: bits 0-1 the kind, bits 2-3 for kind 1 the count
enum { kSkip = 0, kAli = 1, kTIns = 2, kQIns = 3 };
enum { kMatch = 0, kMis = 1, kRep = 2, kN = 3 };
// fields of the second scan's word
enum { fStart = 0, fQNum = 1, fTNum = 2, fMatch = 3, fRep = 4, fN = 5 };

__device__ __forceinline__ bool axtp_del(unsigned c) { return c == '-' || c == '.' || c == '=' || c == '_'; }
__device__ __forceinline__ unsigned axtp_upper(unsigned c) {
    return c - 'a' <= (unsigned)('z' - 'a') ? c - 32 : c;
}

__device__ __forceinline__ unsigned axtp_code(unsigned tc, unsigned qc) {
    const bool td = axtp_del(tc), qd = axtp_del(qc);
    if (td || qd) return td && qd ? kSkip : qd ? kTIns : kQIns;
    const unsigned tu = axtp_upper(tc), qu = axtp_upper(qc);
    const unsigned cls = (tc == 'N' || qc == 'N') ? kN : tu != qu ? kMis : (tu != tc || qu != qc) ? kRep : kMatch;
    return kAli | cls << 2;
}

__device__ __forceinline__ unsigned field(unsigned long long v, int f) {
    return (unsigned)(v >> (kAxtpBits * f)) & kAxtpField;
}

template <bool EMIT>
__global__ void __launch_bounds__(kWave) k_axt_psl(AxtpArgs a) {
    __shared__ unsigned long long code8[kAxtpTile / 8];
    uint8_t *code = reinterpret_cast<uint8_t *>(code8);
    const int lane = threadIdx.x;

    for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {
        const AxtpEntry e = a.ent[i];
        int64_t L = e.len;
        // (the host checked the rows against the text; a record that fails here is not read)
        if (L < 0 || e.t < 0 || e.q < 0 || e.t > a.text_bytes - L || e.q > a.text_bytes - L) L = 0;
        const uint8_t *trow = a.text + e.t, *qrow = a.text + e.q;
        const int64_t b0 = EMIT ? a.boff[i] : 0;

        // so far, over the tiles walked (wave-uniform)
        unsigned nA = 0, nT = 0, nQ = 0;                             // columns of kind 1, 2, 3
        unsigned nS = 0, nQn = 0, nTn = 0, nM = 0, nR = 0, nN = 0;  // starts, openings, counts
        unsigned prev = kSkip;
        unsigned open_a = 0;         // columns of kind 1 before the last start
        unsigned fT = 0, fQ = 0;     // at F: the head's columns of kind 2, 3
        unsigned eT = 0, eQ = 0, eQn = 0, eTn = 0;  // at E, inclusive
        int64_t F = -1, E = -1;

        for (int64_t c0 = 0; c0 < L; c0 += kAxtpTile) {
            const int64_t left = L - c0;
            const int ncols = (int)(left < kAxtpTile ? left : kAxtpTile);
            for (int j = lane; j < kAxtpTile; j += kWave)
                code[j] = (uint8_t)(j < ncols ? axtp_code(trow[c0 + j], qrow[c0 + j]) : kSkip);
            __syncthreads();
            const unsigned long long codes = code8[lane];
            __syncthreads();  // the next tile's stores come after every lane's load

            // scan 1: the kinds' counts and the last kind
            unsigned s1 = 0, lk = kSkip;
#pragma unroll
            for (int k = 0; k < kAxtpPer; ++k) {
                const unsigned kind = (unsigned)(codes >> (8 * k)) & 3u;
                if (kind != kSkip) {
                    s1 += 1u << (kAxtpBits * (kind - 1));
                    lk = kind;
                }
            }
            unsigned in1 = s1;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned o = __shfl_up(in1, d, kWave), ol = __shfl_up(lk, d, kWave);
                if (lane >= d) {
                    in1 += o;
                    if (lk == kSkip) lk = ol;
                }
            }
            const unsigned ex1 = in1 - s1;
            unsigned pin = __shfl_up(lk, 1, kWave);
            if (lane == 0) pin = kSkip;
            if (pin == kSkip) pin = prev;  // nothing but skipped columns before the lane's
            const unsigned a0 = nA + (ex1 & kAxtpField), t0 = nT + ((ex1 >> kAxtpBits) & kAxtpField),
                           q0 = nQ + ((ex1 >> (2 * kAxtpBits)) & kAxtpField);
            const unsigned long long has_ali = __ballot((s1 & kAxtpField) != 0);

            // walk: the events of the lane's columns, and what is counted up to
            // and with its last column of kind 1
            unsigned long long s2 = 0, s2_ali = 0;
            int ls = -1;  // columns of kind 1 before the lane's last start
            unsigned lt = 0, lq = 0, lt_ali = 0, lq_ali = 0, lt_first = 0, lq_first = 0;
            int k_first = -1, k_last = -1;
            {
                unsigned p = pin, al = a0;
#pragma unroll
                for (int k = 0; k < kAxtpPer; ++k) {
                    const unsigned c = (unsigned)(codes >> (8 * k)) & 0xfu, kind = c & 3u;
                    if (kind == kSkip) continue;
                    if (kind == kAli) {
                        if (p != kAli) {
                            s2 += 1ull << (kAxtpBits * fStart);
                            ls = (int)al;
                        }
                        const unsigned cls = c >> 2;
                        if (cls == kMatch) s2 += 1ull << (kAxtpBits * fMatch);
                        if (cls == kRep) s2 += 1ull << (kAxtpBits * fRep);
                        if (cls == kN) s2 += 1ull << (kAxtpBits * fN);
                        if (k_first < 0) k_first = k, lt_first = lt, lq_first = lq;
                        ++al;
                        k_last = k, s2_ali = s2, lt_ali = lt, lq_ali = lq;
                    } else if (kind == kTIns) {
                        if (al > 0 && p != kTIns) s2 += 1ull << (kAxtpBits * fTNum);
                        ++lt;
                    } else {
                        if (al > 0 && p != kQIns) s2 += 1ull << (kAxtpBits * fQNum);
                        ++lq;
                    }
                    p = kind;
                }
            }

            // scan 2: the events' counts and the last start
            unsigned long long in2 = s2;
            int lsc = ls;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned long long o = __shfl_up(in2, d, kWave);
                const int ol = __shfl_up(lsc, d, kWave);
                if (lane >= d) {
                    in2 += o;
                    if (lsc < 0) lsc = ol;
                }
            }
            const unsigned long long ex2 = in2 - s2;

            // F and E: the first lane with a column of kind 1 in the first tile
            // that has one, the last such lane of every tile that has one
            if (has_ali != 0) {
                if (F < 0) {
                    const int src = __ffsll((long long)has_ali) - 1;
                    F = c0 + src * kAxtpPer + __shfl(k_first, src, kWave);
                    fT = __shfl(t0 + lt_first, src, kWave);
                    fQ = __shfl(q0 + lq_first, src, kWave);
                }
                const int src = 63 - __clzll((long long)has_ali);
                E = c0 + src * kAxtpPer + __shfl(k_last, src, kWave);
                eT = __shfl(t0 + lt_ali, src, kWave);
                eQ = __shfl(q0 + lq_ali, src, kWave);
                const unsigned long long at = __shfl(ex2 + s2_ali, src, kWave);
                eQn = nQn + field(at, fQNum);
                eTn = nTn + field(at, fTNum);
            }

            if (EMIT) {
                int cur = __shfl_up(lsc, 1, kWave);
                if (lane == 0) cur = -1;
                if (cur < 0) cur = (int)open_a;
                unsigned p = pin, al = a0, tt = t0, qq = q0;
                int64_t at = b0 + nS + field(ex2, fStart);  // the next block to open
#pragma unroll
                for (int k = 0; k < kAxtpPer; ++k) {
                    const unsigned kind = (unsigned)(codes >> (8 * k)) & 3u;
                    if (kind == kSkip) continue;
                    if (kind == kAli) {
                        if (p != kAli) {
                            if (at >= 0 && at < a.nb) {
                                a.blk[at].q_adv = (int32_t)(al + qq - fQ);
                                a.blk[at].t_adv = (int32_t)(al + tt - fT);
                            }
                            cur = (int)al;
                            ++at;
                        }
                        ++al;
                    } else {
                        if (p == kAli && at - 1 >= 0 && at - 1 < a.nb) a.blk[at - 1].size = (int32_t)al - cur;
                        if (kind == kTIns)
                            ++tt;
                        else
                            ++qq;
                    }
                    p = kind;
                }
            }

            // the tile's totals into the running state
            const unsigned tot1 = __shfl(in1, kWave - 1, kWave), tlk = __shfl(lk, kWave - 1, kWave);
            const unsigned long long tot2 = __shfl(in2, kWave - 1, kWave);
            const int tls = __shfl(lsc, kWave - 1, kWave);
            nA += tot1 & kAxtpField, nT += (tot1 >> kAxtpBits) & kAxtpField;
            nQ += (tot1 >> (2 * kAxtpBits)) & kAxtpField;
            nS += field(tot2, fStart), nQn += field(tot2, fQNum), nTn += field(tot2, fTNum);
            nM += field(tot2, fMatch), nR += field(tot2, fRep), nN += field(tot2, fN);
            if (tlk != kSkip) prev = tlk;
            if (tls >= 0) open_a = (unsigned)tls;
        }

        if (lane == 0) {
            if (!EMIT) {
                gac_axtpsl_entry r;
                r.match = nM, r.rep_match = nR, r.n_count = nN, r.mis_match = nA - nM - nR - nN;
                r.q_num_insert = eQn, r.t_num_insert = eTn;
                r.q_base_insert = eQ - fQ, r.t_base_insert = eT - fT;
                r.q_head = (int32_t)fQ, r.t_head = (int32_t)fT;
                r.q_tail = (int32_t)(nQ - eQ), r.t_tail = (int32_t)(nT - eT);
                if (F < 0) {  // no column without a gap: everything is head, as trimAlignment has it
                    r.q_base_insert = r.t_base_insert = 0;
                    r.q_head = (int32_t)nQ, r.t_head = (int32_t)nT;
                    r.q_tail = r.t_tail = 0;
                }
                r.cols = F < 0 ? 0 : (int32_t)(E - F + 1);
                r.n_blocks = nS ? (int32_t)nS : 1;
                r.block0 = 0;
                a.out[i] = r;
                a.nblk[i] = nS ? nS : 1;
            } else {
                a.out[i].block0 = b0;
                if (nS == 0) {
                    if (b0 >= 0 && b0 < a.nb) a.blk[b0] = gac_axtpsl_block{0, 0, 0};
                } else if (prev == kAli) {  // the last block is open at the entry's end
                    const int64_t at = b0 + nS - 1;
                    if (at >= 0 && at < a.nb) a.blk[at].size = (int32_t)(nA - open_a);
                }
            }
        }
    }
}

}  // namespace

static unsigned axtp_grid(int64_t n) { return (unsigned)(n < kAxtpMaxGrid ? n : kAxtpMaxGrid); }

hipError_t launch_axt_psl_count(const AxtpArgs &a, hipStream_t s) {
    if (a.n < 0) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_axt_psl<false>, dim3(axtp_grid(a.n)), dim3(kWave), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_axt_psl_emit(const AxtpArgs &a, hipStream_t s) {
    if (a.n < 0 || a.nb < 0) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_axt_psl<true>, dim3(axtp_grid(a.n)), dim3(kWave), 0, s, a);
    return hipGetLastError();
}

}  // namespace gac
