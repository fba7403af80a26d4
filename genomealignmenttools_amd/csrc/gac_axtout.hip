// gac_axtout.hip -- chain pieces back to alignment text (gac_axt_measure,
// gac_axt_render; chainToAxt's axtFromBlocks + axtScoreSym + axtIdRatio,
// kent/src/lib/chainToAxt.c:14-91, kent/src/lib/axt.c:196-229,
// kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c:69-89).  gfx950 only.
//
// A piece is a window of consecutive blocks of one chain (gac_window: chain,
// first block, count) without a double-sided gap inside.  The pieces of a
// call are laid end to end as one "virtual" block array (pboff = exclusive
// scan of their block counts), and that array is cut as k_compose cuts the
// flat block array: a wave takes a tile of 64 consecutive virtual blocks, one
// per lane, whatever pieces they belong to, and spreads the tile's work items
// over its lanes.
//
//   k_axt_stat    items are 32-base chunks of the blocks.  Block scores come
//                 from AND/popcount over the planes with the blastz default
//                 matrix; the gap terms and the column counts need no
//                 sequence and are added once per block.  Per-piece sums go
//                 registers -> wave shuffles or LDS slots -> one global
//                 atomicAdd per workgroup, piece and counter.
//   k_axt_pairs   k_axt_stat's walk for any score scheme (lavToAxt -dropSelf):
//                 per piece the 16 letter-pair counts and the N columns.
//   k_axt_render  a block's run on a row is its inner gap's columns followed
//                 by its bases; the run's first column is S[v] - S[first v of
//                 the piece], S = exclusive scan of gap + size over the
//                 virtual blocks.  Items are the 16-byte aligned windows of
//                 the output that a run touches: a lane decodes the <= 16
//                 columns of one window from the plane words (funnel shift,
//                 bit reversal for '-') and stores them with one 16-byte
//                 store; only a run's first and last window fall back to
//                 4-byte and single-byte stores.
//   k_cut_*       netToAxt's ranges (chain, tStart, tEnd) to clipped pieces
//                 (gac_axt_cut): see the section near the end.  The kernels
//                 above are templates on kClip, which makes a piece's first
//                 and last block honour its t_start / t_end (gac_axt_*_clip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kAxtSlots = kWavesPerWG * kTileBlocks;  // virtual blocks (so pieces at most) per workgroup
constexpr int kScanPer = 8;                           // elements per thread of the scan kernels
constexpr int kScanChunk = 256 * kScanPer;

typedef uint32_t au32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t au32x2a4 __attribute__((ext_vector_type(2), aligned(4)));

__device__ __forceinline__ uint32_t afunnel(uint32_t hi, uint32_t lo, int sh) {
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
}

// 32 mask bits from global base index (w * 32 + sh): words w, w + 1
__device__ __forceinline__ uint32_t amask_window(const uint32_t *m, int64_t w, int sh) {
    const au32x2a4 v = *reinterpret_cast<const au32x2a4 *>(m + w);
    return afunnel(v.y, v.x, sh);
}

__device__ __forceinline__ void axt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------ scan
// Exclusive scan of the workgroup's 256 values (total: their sum).
__device__ __forceinline__ long long axt_wg_scan(long long x, long long *s_w, long long &total) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    long long incl = x;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += o;
    }
    __syncthreads();  // (s_w may still be read from the previous call)
    if (lane == kWave - 1) s_w[wv] = incl;
    __syncthreads();
    long long base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerWG; ++w) {
        if (w < wv) base += s_w[w];
        total += s_w[w];
    }
    return base + incl - x;
}

// part[g] = sum of chunk g of arr[0, m)
__global__ void __launch_bounds__(256) k_axt_scan_part(const long long *arr, int64_t m, long long *part) {
    __shared__ long long s_w[kWavesPerWG];
    const int64_t i0 = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPer;
    long long x = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k)
        if (i0 + k < m) x += arr[i0 + k];
    long long total;
    axt_wg_scan(x, s_w, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one workgroup: part[0, G) to its exclusive scan, part[G] = the total
__global__ void __launch_bounds__(256) k_axt_scan_top(long long *part, int64_t G) {
    __shared__ long long s_w[kWavesPerWG];
    long long carry = 0;
    for (int64_t g0 = 0; g0 < G; g0 += 256) {
        const int64_t g = g0 + threadIdx.x;
        const long long x = g < G ? part[g] : 0;
        long long total;
        const long long ex = axt_wg_scan(x, s_w, total);
        if (g < G) part[g] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) part[G] = carry;
}

// arr[0, m) to its exclusive scan in place, arr[m] = the total
__global__ void __launch_bounds__(256) k_axt_scan_apply(long long *arr, int64_t m, const long long *part,
                                                       int64_t G) {
    __shared__ long long s_w[kWavesPerWG];
    const int64_t i0 = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPer;
    long long e[kScanPer], x = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        e[k] = i0 + k < m ? arr[i0 + k] : 0;
        x += e[k];
    }
    long long total;
    long long run = part[blockIdx.x] + axt_wg_scan(x, s_w, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (i0 + k < m) arr[i0 + k] = run;
        run += e[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) arr[m] = part[G];
}

// ------------------------------------------------------------------ plan
// One lane per piece: its window checked against its chain; pboff[i] = its
// blocks (0 for a bad one, so no later kernel touches it).  kClip: t_start /
// t_end must leave a base of the first and of the last block.
template <bool kClip>
__global__ void __launch_bounds__(256) k_axt_plan(AxtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const Window w = a.pieces[i];
    long long nb = 0;
    bool bad = w.chain < 0 || w.chain >= a.n_chains || w.first < 0 || w.nblk < 0;
    if (!bad) {
        const int32_t have = a.chains[w.chain].nblk;
        bad = (int64_t)w.first + w.nblk > have;
    }
    if (bad) {
        atomicOr(a.status, kAxtBadWindow);
    } else if (kClip && w.nblk > 0) {
        const int4 *b = a.blk + a.chains[w.chain].blk_off + w.first;
        const int4 f = b[0], l = b[w.nblk - 1];
        const long long fe = (long long)f.x + (f.z & kSizeMask), le = (long long)l.x + (l.z & kSizeMask);
        const long long s = w.t_start > f.x ? w.t_start : f.x;  // the first block's start
        const long long e = w.t_end < le ? w.t_end : le;        // the last block's end
        // (one block: both cuts are its own; more: the first keeps its end, the last its start)
        bad = w.nblk == 1 ? s >= e : (s >= fe || e <= l.x);
        if (bad) atomicOr(a.status, kAxtBadClip);
    }
    if (!bad) nb = w.nblk;
    a.pboff[i] = nb;
}

// A virtual block: its piece, its block record and the inner gap before it.
struct AxtLoc {
    int64_t p, v0;  // piece, the piece's first virtual block
    int4 bk;
    int size, gap;  // gap: columns of the one-sided gap to the previous block of the piece
    bool tgap;      // the gap is target bases (dashes on the query row)
    bool bad;       // negative or double-sided gap (treated as none)
    DChain ch;
};

// kClip: the piece's first block starts at max(tStart, t_start), its last ends
// at min(tEnd, t_end), the query following (chainFastSubsetOnT, chain.c:513-522);
// k_axt_plan has checked that both keep a base.  Inner gaps lie between
// unclipped block ends.
template <bool kClip>
__device__ __forceinline__ AxtLoc axt_locate(const AxtArgs &a, int64_t v) {
    AxtLoc L;
    int64_t lo = 0, hi = a.n - 1;  // last p with pboff[p] <= v (empty pieces share an offset)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.pboff[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    L.p = lo;
    L.v0 = a.pboff[lo];
    const Window w = a.pieces[lo];
    L.ch = a.chains[w.chain];
    const int64_t b = L.ch.blk_off + w.first + (v - L.v0);
    L.bk = a.blk[b];
    L.size = L.bk.z & kSizeMask;
    L.gap = 0;
    L.tgap = false;
    L.bad = false;
    if (v > L.v0) {
        const int4 pk = a.blk[b - 1];
        const int psz = pk.z & kSizeMask;
        const long long dt = (long long)L.bk.x - ((long long)pk.x + psz);
        const long long dq = (long long)L.bk.y - ((long long)pk.y + psz);
        if (dt < 0 || dq < 0 || (dt > 0 && dq > 0) || dt + dq >= (1 << 30)) {
            L.bad = true;
        } else {
            L.gap = (int)(dt + dq);
            L.tgap = dt > 0;
        }
    }
    if (kClip) {
        const int end = L.bk.x + L.size;
        if (v == L.v0 && w.t_start > L.bk.x) {
            const int head = w.t_start - L.bk.x;
            L.bk.x += head;
            L.bk.y += head;
            L.size -= head;
        }
        if (v - L.v0 == w.nblk - 1 && w.t_end < end) L.size -= end - w.t_end;
    }
    return L;
}

// ------------------------------------------------------------------ stat
constexpr int kStatVals = 2;  // in the chunk loop: score, match (ali / sym: once per block)

struct StatWave {
    int coff[kTileBlocks];        // exclusive chunk prefix per lane-block
    long long tpos[kTileBlocks];  // global base index of the block's target start
    long long qpos[kTileBlocks];  // '+': of its query start; '-': of (qSize - qStart)
    int lenq[kTileBlocks];        // size | tN (bit 29) | qN (bit 30) | minus (bit 31)
    int slot[kTileBlocks];        // the block's piece slot in the workgroup
};

// As k_compose's comp_flush: the lanes' register sums to the piece slots.
__device__ __forceinline__ void stat_flush(unsigned long long (*acc)[4], int lane, int &cur,
                                           unsigned long long (&v)[kStatVals], bool want) {
    const bool have = cur >= 0;
    if (!__ballot(want && have)) return;
    const unsigned long long hm = __ballot(have);
    const int u = __shfl(cur, (int)__builtin_ctzll(hm), kWave);
    if (!__ballot(have && cur != u)) {
#pragma unroll
        for (int k = 0; k < kStatVals; ++k) {
            unsigned long long s = have ? v[k] : 0ull;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
            if (lane == 0 && s) atomicAdd(&acc[u][k], s);
            v[k] = 0;
        }
        cur = -1;
    } else if (want && have) {
#pragma unroll
        for (int k = 0; k < kStatVals; ++k) {
            if (v[k]) atomicAdd(&acc[cur][k], v[k]);
            v[k] = 0;
        }
        cur = -1;
    }
}

template <bool kClip>
__global__ void __launch_bounds__(256) k_axt_stat(AxtArgs a) {
    __shared__ StatWave s_w[kWavesPerWG];
    __shared__ unsigned long long s_acc[kAxtSlots][4];  // score, match, ali, sym
    __shared__ long long s_piece[kAxtSlots];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_acc[threadIdx.x][k] = 0ull;
    s_piece[threadIdx.x] = -1;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const int64_t V0 = (int64_t)blockIdx.x * kAxtSlots;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerWG + wv;
    if (tile * kTileBlocks < a.V) {  // (wave-uniform; no workgroup barrier inside)
        StatWave &W = s_w[wv];
        const int64_t v = tile * kTileBlocks + lane;
        int len = 0, lenq = 0, slot = 0;
        long long tpos = 0, qpos = 0;
        if (v < a.V) {
            const AxtLoc L = axt_locate<kClip>(a, v);
            if (L.bad) atomicOr(a.status, kAxtBadGap);
            len = L.size;
            const bool minus = L.ch.qbase < 0;
            tpos = L.ch.tbase + L.bk.x;
            qpos = minus ? ~L.ch.qbase - L.bk.y : L.ch.qbase + L.bk.y;
            lenq = len | (minus ? (int)0x80000000 : 0) | (L.bk.z & (kTHasN | kQHasN));
            slot = (int)((L.v0 > V0 ? L.v0 : V0) - V0);
            s_piece[slot] = L.p;  // (every block of the piece writes the same value)
            // the terms that need no sequence: a gap run of g columns costs
            // 400 + 30 g (axt.c:211-220); ali and sym count columns
            if (L.gap > 0)
                atomicAdd(&s_acc[slot][0], (unsigned long long)(-(400ll + 30ll * L.gap)));
            if (len > 0) atomicAdd(&s_acc[slot][2], (unsigned long long)len);
            if (len + L.gap > 0) atomicAdd(&s_acc[slot][3], (unsigned long long)(len + L.gap));
        }
        const int nch = (len + 31) >> 5;
        int incl = nch;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        const int C = __shfl(incl, kWave - 1, kWave);
        W.coff[lane] = incl - nch;  // (lanes past the last block hold C)
        W.tpos[lane] = tpos;
        W.qpos[lane] = qpos;
        W.lenq[lane] = lenq;
        W.slot[lane] = slot;
        axt_wave_sync();

        int cur = -1;
        unsigned long long acc[kStatVals] = {0, 0};
        for (int c0 = 0; c0 < C; c0 += kWave) {
            const int j = c0 + lane;
            const bool on = j < C;
            int k = 0;
            if (on) {  // block owning chunk j: the largest k with coff[k] <= j
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (W.coff[k + step] <= j) k += step;
            }
            const int sl = on ? W.slot[k] : -1;
            stat_flush(s_acc, lane, cur, acc, on && sl != cur);
            if (on) {
                const int lq = W.lenq[k];
                const int off = (j - W.coff[k]) << 5;
                const int n = min(32, (lq & kSizeMask) - off);  // >= 1: chunk j exists
                const bool minus = lq < 0;
                const int sh = 32 - n;
                const int64_t tp = W.tpos[k] + off;
                // '-': the forward window that ends where the chunk starts
                const int64_t qp = minus ? W.qpos[k] - off - n : W.qpos[k] + off;
                const int64_t tw = tp >> 5, qw = qp >> 5;
                const int sht = (int)(tp & 31), shq = (int)(qp & 31);
                const au32x4a8 tv = *reinterpret_cast<const au32x4a8 *>(a.t_planes + tw);
                const au32x4a8 qv = *reinterpret_cast<const au32x4a8 *>(a.q_planes + qw);
                uint32_t nm = 0, qn = 0;
                if (lq & kTHasN) nm = amask_window(a.t_nmask, tw, sht);
                if (lq & kQHasN) qn = amask_window(a.q_nmask, qw, shq);
                const uint32_t t0 = afunnel(tv.z, tv.x, sht), t1 = afunnel(tv.w, tv.y, sht);
                uint32_t q0 = afunnel(qv.z, qv.x, shq), q1 = afunnel(qv.w, qv.y, shq);
                if (minus) {
                    q0 = __builtin_bitreverse32(q0) >> sh;
                    q1 = ~(__builtin_bitreverse32(q1) >> sh);
                    qn = __builtin_bitreverse32(qn) >> sh;
                }
                const uint32_t in = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
                const uint32_t ok = in & ~(nm | qn);  // a column with an N scores 0
                const uint32_t d0 = t0 ^ q0, d1 = t1 ^ q1;
                // codes T=0 C=1 A=2 G=3; the default matrix (axt.c:434-452) by
                // d = q ^ t: 0: 91 (A, T) / 100 (C, G); 1: -31; 3: -114;
                // 2: -123 (A/T) / -125 (C/G)
                const uint32_t eq = ~d0 & ~d1 & ok, tv2 = ~d0 & d1 & ok;
                const int sc = 91 * __builtin_popcount(eq) + 9 * __builtin_popcount(eq & t0) -
                               31 * __builtin_popcount(d0 & ~d1 & ok) -
                               114 * __builtin_popcount(d0 & d1 & ok) -
                               123 * __builtin_popcount(tv2) - 2 * __builtin_popcount(tv2 & t0);
                acc[0] += (unsigned long long)(long long)sc;
                // axtIdRatio: letters equal, N against N included
                acc[1] += (unsigned long long)(__builtin_popcount(eq) +
                                               __builtin_popcount(nm & qn & in));
                cur = sl;
            }
        }
        stat_flush(s_acc, lane, cur, acc, true);
    }
    __syncthreads();
    const long long p = s_piece[threadIdx.x];
    if (p >= 0) {  // one add per (workgroup, piece, counter)
        const unsigned long long *s = s_acc[threadIdx.x];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s[k]) atomicAdd(&a.acc[p * 4 + k], s[k]);
    }
}

// acc to the caller's arrays; the score narrows to int as the reference's
// int arithmetic wraps
__global__ void __launch_bounds__(256) k_axt_fin(AxtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const unsigned long long *s = a.acc + i * 4;
    a.score[i] = (int32_t)(uint32_t)s[0];
    a.match[i] = (int64_t)s[1];
    a.ali[i] = (int64_t)s[2];
    a.sym[i] = (int64_t)s[3];
}

// ------------------------------------------------------------------ pairs
// k_axt_pairs (gac_axt_pair_counts): k_axt_stat's walk with the letters kept
// apart.  Per 32-column chunk, four masks of the target code and four of the
// query code give the 16 (query, target) letter masks; their popcounts under
// `ok` and the popcount of the columns with an N are the lane's 17 counters.
// A lane adds at most 32 to a counter per chunk and walks fewer than 2^24
// chunks of a tile (64 blocks below 2^29 bases over 64 lanes), so 32-bit lane
// registers hold; a wave's and a workgroup's sums do not (256 blocks of 2^29
// bases), so the LDS slots and the global counters are 64 bits wide.
constexpr int kPairVals = 17;  // [0, 16): q * 4 + t in A, C, G, T order; [16]: N columns

// .2bit code (T=0 C=1 A=2 G=3) to the A, C, G, T index of gac_scheme_read
__device__ __forceinline__ constexpr int pair_acgt(int code) {
    return code == 0 ? 3 : code == 1 ? 1 : code == 2 ? 0 : 2;
}

// As stat_flush: the lanes' register sums to the piece slots.
__device__ __forceinline__ void pair_flush(unsigned long long (*acc)[kPairVals], int lane, int &cur,
                                           uint32_t (&v)[kPairVals], bool want) {
    const bool have = cur >= 0;
    if (!__ballot(want && have)) return;
    const unsigned long long hm = __ballot(have);
    const int u = __shfl(cur, (int)__builtin_ctzll(hm), kWave);
    if (!__ballot(have && cur != u)) {
#pragma unroll
        for (int k = 0; k < kPairVals; ++k) {
            unsigned long long s = have ? (unsigned long long)v[k] : 0ull;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
            if (lane == 0 && s) atomicAdd(&acc[u][k], s);
            v[k] = 0;
        }
        cur = -1;
    } else if (want && have) {
#pragma unroll
        for (int k = 0; k < kPairVals; ++k) {
            if (v[k]) atomicAdd(&acc[cur][k], (unsigned long long)v[k]);
            v[k] = 0;
        }
        cur = -1;
    }
}

__global__ void __launch_bounds__(256) k_axt_pairs(AxtPairArgs a) {
    __shared__ StatWave s_w[kWavesPerWG];
    __shared__ unsigned long long s_acc[kAxtSlots][kPairVals];
    __shared__ long long s_piece[kAxtSlots];
#pragma unroll
    for (int k = 0; k < kPairVals; ++k) s_acc[threadIdx.x][k] = 0ull;
    s_piece[threadIdx.x] = -1;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const int64_t V0 = (int64_t)blockIdx.x * kAxtSlots;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerWG + wv;
    if (tile * kTileBlocks < a.V) {  // (wave-uniform; no workgroup barrier inside)
        StatWave &W = s_w[wv];
        const int64_t v = tile * kTileBlocks + lane;
        int len = 0, lenq = 0, slot = 0;
        long long tpos = 0, qpos = 0;
        if (v < a.V) {
            const AxtLoc L = axt_locate<false>(a, v);
            if (L.bad) atomicOr(a.status, kAxtBadGap);
            len = L.size;
            const bool minus = L.ch.qbase < 0;
            tpos = L.ch.tbase + L.bk.x;
            qpos = minus ? ~L.ch.qbase - L.bk.y : L.ch.qbase + L.bk.y;
            lenq = len | (minus ? (int)0x80000000 : 0) | (L.bk.z & (kTHasN | kQHasN));
            slot = (int)((L.v0 > V0 ? L.v0 : V0) - V0);
            s_piece[slot] = L.p;  // (every block of the piece writes the same value)
        }
        const int nch = (len + 31) >> 5;
        int incl = nch;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        const int C = __shfl(incl, kWave - 1, kWave);
        W.coff[lane] = incl - nch;  // (lanes past the last block hold C)
        W.tpos[lane] = tpos;
        W.qpos[lane] = qpos;
        W.lenq[lane] = lenq;
        W.slot[lane] = slot;
        axt_wave_sync();

        int cur = -1;
        uint32_t acc[kPairVals];
#pragma unroll
        for (int k = 0; k < kPairVals; ++k) acc[k] = 0;
        for (int c0 = 0; c0 < C; c0 += kWave) {
            const int j = c0 + lane;
            const bool on = j < C;
            int k = 0;
            if (on) {  // block owning chunk j: the largest k with coff[k] <= j
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (W.coff[k + step] <= j) k += step;
            }
            const int sl = on ? W.slot[k] : -1;
            pair_flush(s_acc, lane, cur, acc, on && sl != cur);
            if (on) {
                const int lq = W.lenq[k];
                const int off = (j - W.coff[k]) << 5;
                const int n = min(32, (lq & kSizeMask) - off);  // >= 1: chunk j exists
                const bool minus = lq < 0;
                const int sh = 32 - n;
                const int64_t tp = W.tpos[k] + off;
                // '-': the forward window that ends where the chunk starts
                const int64_t qp = minus ? W.qpos[k] - off - n : W.qpos[k] + off;
                const int64_t tw = tp >> 5, qw = qp >> 5;
                const int sht = (int)(tp & 31), shq = (int)(qp & 31);
                const au32x4a8 tv = *reinterpret_cast<const au32x4a8 *>(a.t_planes + tw);
                const au32x4a8 qv = *reinterpret_cast<const au32x4a8 *>(a.q_planes + qw);
                uint32_t nm = 0, qn = 0;
                if (lq & kTHasN) nm = amask_window(a.t_nmask, tw, sht);
                if (lq & kQHasN) qn = amask_window(a.q_nmask, qw, shq);
                const uint32_t t0 = afunnel(tv.z, tv.x, sht), t1 = afunnel(tv.w, tv.y, sht);
                uint32_t q0 = afunnel(qv.z, qv.x, shq), q1 = afunnel(qv.w, qv.y, shq);
                if (minus) {
                    q0 = __builtin_bitreverse32(q0) >> sh;
                    q1 = ~(__builtin_bitreverse32(q1) >> sh);
                    qn = __builtin_bitreverse32(qn) >> sh;
                }
                const uint32_t in = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
                const uint32_t ok = in & ~(nm | qn);
                // by code T=0 C=1 A=2 G=3 (bit 0: plane 0, bit 1: plane 1)
                const uint32_t tm[4] = {~t0 & ~t1 & ok, t0 & ~t1 & ok, ~t0 & t1 & ok, t0 & t1 & ok};
                const uint32_t qm[4] = {~q0 & ~q1, q0 & ~q1, ~q0 & q1, q0 & q1};
#pragma unroll
                for (int qc = 0; qc < 4; ++qc)
#pragma unroll
                    for (int tc = 0; tc < 4; ++tc)
                        acc[pair_acgt(qc) * 4 + pair_acgt(tc)] +=
                            (uint32_t)__builtin_popcount(qm[qc] & tm[tc]);
                acc[16] += (uint32_t)__builtin_popcount((nm | qn) & in);
                cur = sl;
            }
        }
        pair_flush(s_acc, lane, cur, acc, true);
    }
    __syncthreads();
    const long long p = s_piece[threadIdx.x];
    if (p >= 0) {  // one add per (workgroup, piece, counter)
        const unsigned long long *s = s_acc[threadIdx.x];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (s[k]) atomicAdd(&a.pairs[p * 16 + k], s[k]);
        if (s[16]) atomicAdd(&a.ncols[p], s[16]);
    }
}

// ---------------------------------------------------------------- columns
// S[v] = columns of virtual block v (inner gap + size), scanned afterwards.
template <bool kClip>
__global__ void __launch_bounds__(256) k_axt_cols(AxtArgs a) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.V) return;
    const AxtLoc L = axt_locate<kClip>(a, v);
    if (L.bad) atomicOr(a.status, kAxtBadGap);
    a.S[v] = (long long)L.size + L.gap;
}

// One lane per piece: where its rows go, checked against the buffer.
__global__ void __launch_bounds__(256) k_axt_place(AxtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const long long s0 = a.S[a.pboff[i]], sym = a.S[a.pboff[i + 1]] - s0;
    const long long off = a.offsets ? a.offsets[i] : 2 * s0 + 3 * i;
    a.off[i] = off;
    if (off < 0 || off > a.out_bytes || 2 * sym + 3 > a.out_bytes - off)
        atomicOr(a.status, kAxtBadOut);
}

// the three line ends of every piece: tSym '\n' qSym '\n' '\n'
__global__ void __launch_bounds__(256) k_axt_seps(AxtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const long long sym = a.S[a.pboff[i + 1]] - a.S[a.pboff[i]];
    char *o = a.out + a.off[i];
    o[sym] = '\n';
    o[2 * sym + 1] = '\n';
    o[2 * sym + 2] = '\n';
}

// ----------------------------------------------------------------- render
struct RenderWave {
    long long coff[kTileBlocks];  // exclusive window prefix per lane-block (both rows)
    long long addr[2][kTileBlocks];  // address of the run's first column on the t / q row
    long long src[2][kTileBlocks];   // global base index of the row's first base (q '-':
                                     // one past it on the forward strand)
    int nwt[kTileBlocks];            // windows of the t row
    int w[kTileBlocks];              // columns of the run (gap + size)
    int dash[2][kTileBlocks];        // leading '-' columns of each row; bit 31 of [1]: minus
};

// 4 bits to the low bit of 4 bytes
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (x * 0x00204081u) & 0x01010101u; }

template <bool kClip>
__global__ void __launch_bounds__(256) k_axt_render(AxtArgs a) {
    __shared__ RenderWave s_w[kWavesPerWG];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerWG + wv;
    if (tile * kTileBlocks >= a.V) return;  // (wave-uniform; no workgroup barrier below)
    RenderWave &W = s_w[wv];
    const int64_t v = tile * kTileBlocks + lane;
    long long nw = 0;
    int nwt = 0, w = 0, dt = 0, dq = 0;
    long long at = 0, aq = 0, st = 0, sq = 0;
    if (v < a.V) {
        const AxtLoc L = axt_locate<kClip>(a, v);
        const long long s0 = a.S[L.v0], sym = a.S[a.pboff[L.p + 1]] - s0;
        const long long col = a.S[v] - s0;
        w = L.size + L.gap;
        at = (long long)(uintptr_t)a.out + a.off[L.p] + col;
        aq = at + sym + 1;
        const bool minus = L.ch.qbase < 0;
        // the row that holds the gap's bases runs on from them into the block
        const int tback = L.tgap ? L.gap : 0, qback = L.tgap ? 0 : L.gap;
        dt = L.tgap ? 0 : L.gap;
        dq = L.tgap ? L.gap : 0;
        st = L.ch.tbase + L.bk.x - tback;
        const long long qs = (long long)L.bk.y - qback;
        sq = minus ? ~L.ch.qbase - qs : L.ch.qbase + qs;
        if (minus) dq |= (int)0x80000000;
        if (w > 0) {
            nwt = (int)(((at + w + 15) >> 4) - (at >> 4));
            nw = nwt + (((aq + w + 15) >> 4) - (aq >> 4));
        }
    }
    long long incl = nw;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += o;
    }
    const long long C = __shfl(incl, kWave - 1, kWave);
    W.coff[lane] = incl - nw;  // (lanes past the last block hold C)
    W.addr[0][lane] = at;
    W.addr[1][lane] = aq;
    W.src[0][lane] = st;
    W.src[1][lane] = sq;
    W.nwt[lane] = nwt;
    W.w[lane] = w;
    W.dash[0][lane] = dt;
    W.dash[1][lane] = dq;
    axt_wave_sync();

    for (long long c0 = 0; c0 < C; c0 += kWave) {
        const long long j = c0 + lane;
        if (j >= C) continue;
        int k = 0;  // block owning window j: the largest k with coff[k] <= j
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            if (W.coff[k + step] <= j) k += step;
        long long r = j - W.coff[k];
        const int row = r >= W.nwt[k] ? 1 : 0;
        if (row) r -= W.nwt[k];
        const long long A = W.addr[row][k];
        const int dword = W.dash[row][k];
        const int nd = dword & 0x7fffffff;
        const bool minus = dword < 0;
        const int wk = W.w[k];
        const long long wa = (A & ~15ll) + 16 * r;  // the window's address
        // the window holds run columns [i0, i0 + 16); [lo, hi) of them exist
        const long long i0 = wa - A;
        const long long lo = i0 > 0 ? i0 : 0, hi = i0 + 16 < wk ? i0 + 16 : wk;
        const long long bl = lo > nd ? lo : nd;  // the first of them that is a base
        const int nb = (int)(hi - bl);
        uint32_t b0 = 0, b1 = 0, bn = 0, bm = 0;
        if (nb > 0) {
            const long long s = bl - nd;  // bases before it on the row
            const uint2 *pl = row ? a.q_planes : a.t_planes;
            const uint32_t *nmk = row ? a.q_nmask : a.t_nmask;
            const uint32_t *lmk = row ? a.q_lmask : a.t_lmask;
            // '-': the forward window that ends where these bases start
            const long long bp = minus ? W.src[row][k] - s - nb : W.src[row][k] + s;
            const int64_t bw = bp >> 5;
            const int shb = (int)(bp & 31);
            const au32x4a8 pv = *reinterpret_cast<const au32x4a8 *>(pl + bw);
            b0 = afunnel(pv.z, pv.x, shb);
            b1 = afunnel(pv.w, pv.y, shb);
            bn = amask_window(nmk, bw, shb);
            bm = amask_window(lmk, bw, shb);
            if (minus) {
                // rc base i = comp(fwd[bp + nb - 1 - i]): bit-reversed words,
                // complement = code ^ 2; N and case travel with the base
                const int sh = 32 - nb;
                b0 = __builtin_bitreverse32(b0) >> sh;
                b1 = ~(__builtin_bitreverse32(b1) >> sh);
                bn = __builtin_bitreverse32(bn) >> sh;
                bm = __builtin_bitreverse32(bm) >> sh;
            }
            const uint32_t in = (1u << nb) - 1u;  // (nb <= 16)
            const int up = (int)(bl - i0);
            b0 = (b0 & in) << up;
            b1 = (b1 & in) << up;
            bn = (bn & in) << up;
            bm = (bm & in) << up;
        }
        const long long ndw = nd - i0;  // window columns that are dashes
        const uint32_t bd = ndw <= 0 ? 0u : ndw >= 16 ? 0xffffu : ((1u << (int)ndw) - 1u);
        const uint32_t vm = ((1u << (int)(hi - i0)) - 1u) & ~((1u << (int)(lo - i0)) - 1u);
        uint32_t d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t s0 = spread4((b0 >> (4 * q)) & 15u), s1 = spread4((b1 >> (4 * q)) & 15u);
            const uint32_t sn = spread4((bn >> (4 * q)) & 15u) * 0xffu;
            const uint32_t sm = spread4((bm >> (4 * q)) & 15u);
            const uint32_t sd = spread4((bd >> (4 * q)) & 15u) * 0xffu;
            // 'T' 'C' 'A' 'G' = 0x54 - 0x11 b0 - 0x13 b1 + 0x17 b0 b1 (no borrow between bytes)
            uint32_t ch = 0x54545454u - s0 * 0x11u - s1 * 0x13u + (s0 & s1) * 0x17u;
            ch = (ch & ~sn) | (0x4e4e4e4eu & sn);  // 'N'
            ch |= sm << 5;                         // lower case inside a mask run
            d[q] = (ch & ~sd) | (0x2d2d2d2du & sd);  // '-'
        }
        char *o = reinterpret_cast<char *>((uintptr_t)wa);
        if (vm == 0xffffu) {
            *reinterpret_cast<uint4 *>(o) = make_uint4(d[0], d[1], d[2], d[3]);
        } else {  // the run's first or last window
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t m4 = (vm >> (4 * q)) & 15u;
                if (m4 == 15u) {
                    *reinterpret_cast<uint32_t *>(o + 4 * q) = d[q];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((m4 >> e) & 1u) o[4 * q + e] = (char)(d[q] >> (8 * e));
                }
            }
        }
    }
}

// -------------------------------------------------------------------- cut
// Ranges to clipped pieces (gac_axt_cut; netToAxt's chainSubsetOnT +
// chainToAxt, kent/src/lib/chain.c:471-558, kent/src/lib/chainToAxt.c:93-124).
// Only k_cut_find has a lane per range (two binary searches); the rest is cut
// over the selected blocks, so a range costs what its blocks cost.

// One lane per range: the blocks chainSubsetOnT selects -- from the first with
// tEnd > t_start (chain.c:482-486) up to the first with tStart >= t_end (:510).
__global__ void __launch_bounds__(256) k_cut_find(AxtCutArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const Range r = a.ranges[i];
    int first = 0;
    long long cnt = 0;
    if (r.chain < 0 || r.chain >= a.n_chains) {
        atomicOr(a.status, kAxtBadWindow);
    } else if (r.t_start < r.t_end) {
        const DChain ch = a.chains[r.chain];
        const int4 *b = a.blk + ch.blk_off;
        int lo = 0, hi = ch.nblk;  // first block with tEnd > t_start
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int4 k = b[mid];
            if ((long long)k.x + (k.z & kSizeMask) > r.t_start) hi = mid;
            else lo = mid + 1;
        }
        first = lo;
        hi = ch.nblk;  // first block (from there on) with tStart >= t_end
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (b[mid].x >= r.t_end) hi = mid;
            else lo = mid + 1;
        }
        cnt = lo - first;
    }
    a.rfirst[i] = first;
    a.rboff[i] = cnt;
}

// virtual block v: its range and its index inside the range's window
__device__ __forceinline__ int64_t cut_locate(const AxtCutArgs &a, int64_t v, int64_t &j) {
    int64_t lo = 0, hi = a.n - 1;  // last r with rboff[r] <= v (empty ranges share an offset)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.rboff[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    j = v - a.rboff[lo];
    return lo;
}

// One lane per virtual block: 1 where a piece starts (chainToAxt.c:109-111 with
// maxChain = BIGNUM; the reference compares ints).
__global__ void __launch_bounds__(256) k_cut_flag(AxtCutArgs a) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.V) return;
    int64_t j;
    const int64_t r = cut_locate(a, v, j);
    long long f = 1;
    if (j > 0) {
        const int4 *b = a.blk + a.chains[a.ranges[r].chain].blk_off + a.rfirst[r] + j;
        const int4 k = b[0], pk = b[-1];
        const int psz = pk.z & kSizeMask;
        const int dt = k.x - (pk.x + psz), dq = k.y - (pk.y + psz);
        if (dt < 0 || dq < 0) {
            atomicOr(a.status, kAxtBadGap);
            atomicMin(a.status + 1, (int)r);
        }
        f = (dq > 0 && dt > 0) || dt > a.max_gap || dq > a.max_gap;
    }
    a.pidx[v] = f;
}

// One lane per virtual block, after the scan of the flags (block v lies in
// piece pidx[v + 1] - 1 and starts it when pidx[v + 1] > pidx[v]): a piece's
// head writes chain, first block and the clipped start, its tail the clipped
// end and its own chain-local index + 1 (k_cut_close turns that into a count).
__global__ void __launch_bounds__(256) k_cut_emit(AxtCutArgs a) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= a.V) return;
    int64_t j;
    const int64_t r = cut_locate(a, v, j);
    const Range rg = a.ranges[r];
    const int cb = a.rfirst[r] + (int)j;
    const int4 k = a.blk[a.chains[rg.chain].blk_off + cb];
    const int64_t here = a.pidx[v], next = a.pidx[v + 1];
    Window *w = a.pieces + (next - 1);
    if (next > here) {
        w->chain = rg.chain;
        w->first = cb;
        w->t_start = k.x > rg.t_start ? k.x : rg.t_start;
    }
    // (pidx[V + 1] is never read: v + 1 == V is the last range's last block)
    if (v + 1 == a.rboff[r + 1] || a.pidx[v + 2] > next) {
        const int end = k.x + (k.z & kSizeMask);
        w->t_end = end < rg.t_end ? end : rg.t_end;
        w->nblk = cb + 1;
    }
}

// lanes [0, P): the piece's block count; lanes [0, n]: first[r]
__global__ void __launch_bounds__(256) k_cut_close(AxtCutArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.P) a.pieces[i].nblk -= a.pieces[i].first;
    if (i <= a.n) a.first[i] = i < a.n ? a.pidx[a.rboff[i]] : a.P;
}

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// arr[0, m) -> exclusive scan in place, arr[m] = total; part: m / 2048 + 2 entries
static hipError_t axt_scan(long long *arr, int64_t m, long long *part, hipStream_t s) {
    if (m <= 0) return hipMemsetAsync(arr, 0, sizeof(long long), s);
    const int64_t G = (m + kScanChunk - 1) / kScanChunk;
    hipLaunchKernelGGL(k_axt_scan_part, dim3((unsigned)G), dim3(256), 0, s, arr, m, part);
    hipLaunchKernelGGL(k_axt_scan_top, dim3(1), dim3(256), 0, s, part, G);
    hipLaunchKernelGGL(k_axt_scan_apply, dim3((unsigned)G), dim3(256), 0, s, arr, m, part, G);
    return hipGetLastError();
}

// gac_axt_cut in three steps, the host reading one count between them:
// the ranges' windows and rboff (rboff[n] = V) ...
hipError_t launch_axt_cut_find(const AxtCutArgs &a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(k_cut_find, dim3(grid256(a.n)), dim3(256), 0, s, a);
    return axt_scan((long long *)a.rboff, a.n, (long long *)a.part, s);
}

// ... the break flags and their scan (pidx[V] = P, the pieces) ...
hipError_t launch_axt_cut_flag(const AxtCutArgs &a, hipStream_t s) {
    if (a.V > 0) hipLaunchKernelGGL(k_cut_flag, dim3(grid256(a.V)), dim3(256), 0, s, a);
    return axt_scan((long long *)a.pidx, a.V, (long long *)a.part, s);
}

// ... and the pieces and first[0 .. n]
hipError_t launch_axt_cut_emit(const AxtCutArgs &a, hipStream_t s) {
    if (a.V > 0) hipLaunchKernelGGL(k_cut_emit, dim3(grid256(a.V)), dim3(256), 0, s, a);
    const int64_t m = a.P > a.n + 1 ? a.P : a.n + 1;
    hipLaunchKernelGGL(k_cut_close, dim3(grid256(m)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// pieces checked, pboff scanned (pboff[n] = V, the virtual blocks)
hipError_t launch_axt_plan(const AxtArgs &a, hipStream_t s) {
    if (a.n > 0)
        hipLaunchKernelGGL(a.clip ? k_axt_plan<true> : k_axt_plan<false>, dim3(grid256(a.n)), dim3(256),
                           0, s, a);
    return axt_scan((long long *)a.pboff, a.n, (long long *)a.part, s);
}

// acc (zeroed by the caller) and the caller's four arrays
hipError_t launch_axt_stat(const AxtArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.V > 0)
        hipLaunchKernelGGL(a.clip ? k_axt_stat<true> : k_axt_stat<false>,
                           dim3((unsigned)((a.V + kAxtSlots - 1) / kAxtSlots)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_axt_fin, dim3(grid256(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// pairs and ncols (zeroed by the caller) take the workgroups' sums as they are
hipError_t launch_axt_pairs(const AxtPairArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.V <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_axt_pairs, dim3((unsigned)((a.V + kAxtSlots - 1) / kAxtSlots)), dim3(256), 0, s,
                       a);
    return hipGetLastError();
}

// S, the pieces' offsets and the buffer check (status)
hipError_t launch_axt_place(const AxtArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.V > 0)
        hipLaunchKernelGGL(a.clip ? k_axt_cols<true> : k_axt_cols<false>, dim3(grid256(a.V)), dim3(256),
                           0, s, a);
    const hipError_t e = axt_scan((long long *)a.S, a.V, (long long *)a.part, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_axt_place, dim3(grid256(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_axt_render(const AxtArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_axt_seps, dim3(grid256(a.n)), dim3(256), 0, s, a);
    if (a.V > 0)
        hipLaunchKernelGGL(a.clip ? k_axt_render<true> : k_axt_render<false>,
                           dim3((unsigned)((a.V + kAxtSlots - 1) / kAxtSlots)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gac
