// gac_compose.hip -- per-chain base counts of an uploaded chain set: one walk
// over the aligned bases (chain_walk), instantiated with a counting policy as
//   k_compose     gac_chain_composition: chainAntiRepeat's degeneracyFilter /
//                 repeatFilter counts (kent/src/hg/mouseStuff/chainAntiRepeat/
//                 chainAntiRepeat.c:53-66, 102-114)
//   k_psl_counts  gac_chain_psl_counts: chainToPsl's match / misMatch /
//                 repMatch / nCount (kent/src/hg/mouseStuff/chainToPsl/
//                 chainToPsl.c:106-131)
// gfx950 only.
//
// Work is cut as k_tile cuts it: a wave takes a tile of 64 consecutive blocks
// of the flat block array (whatever chains they belong to), one block per
// lane, and spreads the tile's 32-base chunks over its lanes, so a chain of
// one huge block and 64 one-base blocks of 64 chains cost what their bases
// cost.  Sums stay on chip until the end: a lane adds chunk counts in
// registers while its chunks stay in one chain; when the chain changes the
// wave folds its registers with shuffles (all lanes in one chain) or the lanes
// add to the workgroup's per-chain slots in LDS (chain boundaries inside 64
// chunks); each workgroup then issues one global atomicAdd per counter for
// every chain it met.  Integer sums: any order gives the same result.
//
// A policy P names its kernel arguments (Args, a ChainWalkArgs), the number of
// sums it keeps per chain (kVals), whether it reads the query's soft-mask
// plane (kQLower), what a chunk of up to 32 aligned bases adds to the sums
// (count) and where a workgroup's sums of one chain go (emit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kCompSlots = kWavesPerWG * kTileBlocks;  // blocks (so chains at most) per workgroup

typedef uint32_t cu32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef uint32_t cu32x2a4 __attribute__((ext_vector_type(2), aligned(4)));

__device__ __forceinline__ uint32_t cfunnel(uint32_t hi, uint32_t lo, int sh) {
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
}

// 32 mask bits from global base index (w * 32 + sh): words w, w + 1
__device__ __forceinline__ uint32_t mask_window(const uint32_t *m, int64_t w, int sh) {
    const cu32x2a4 v = *reinterpret_cast<const cu32x2a4 *>(m + w);
    return cfunnel(v.y, v.x, sh);
}

// LDS handed between the lanes of one wave (as gac_kernels.hip's wave_sync_lds)
__device__ __forceinline__ void comp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct CompWave {
    int coff[kTileBlocks];         // exclusive chunk prefix per lane-block
    long long tpos[kTileBlocks];   // global base index of the block's target start
    long long qpos[kTileBlocks];   // '+': of its query start; '-': of (qSize - qStart)
    int lenq[kTileBlocks];         // size | tN (bit 29) | qN (bit 30) | minus (bit 31)
    int slot[kTileBlocks];         // the block's chain slot in the workgroup
};

// Flush the lanes' register sums to the chain slots.  Called by the whole
// wave; `want`: this lane's chain changes now.  When every lane holding sums
// holds them for one chain the wave folds them first (one LDS add per
// counter); otherwise the lanes that change chain add their own.
template <int kVals>
__device__ __forceinline__ void comp_flush(unsigned long long (*acc)[kVals], int lane, int &cur,
                                           uint32_t (&v)[kVals], bool want) {
    const bool have = cur >= 0;
    if (!__ballot(want && have)) return;
    const unsigned long long hm = __ballot(have);
    const int u = __shfl(cur, (int)__builtin_ctzll(hm), kWave);
    if (!__ballot(have && cur != u)) {
#pragma unroll
        for (int k = 0; k < kVals; ++k) {
            unsigned long long s = have ? v[k] : 0u;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
            if (lane == 0 && s) atomicAdd(&acc[u][k], s);
            v[k] = 0;
        }
        cur = -1;
    } else if (want && have) {
#pragma unroll
        for (int k = 0; k < kVals; ++k) {
            if (v[k]) atomicAdd(&acc[cur][k], (unsigned long long)v[k]);
            v[k] = 0;
        }
        cur = -1;
    }
}

// chainAntiRepeat: matches by nucleotide, positions lower-case on either
// side, aligned bases
struct ComposePolicy {
    typedef ComposeArgs Args;
    static constexpr int kVals = 6;  // match[4], rep, total
    static constexpr bool kQLower = true;
    // t0 / t1: the target's code planes; eq: equal bases (N on neither side);
    // nn: N on either side; tl / ql: lower case; in: the chunk's n valid bits
    static __device__ __forceinline__ void count(uint32_t (&v)[kVals], uint32_t t0, uint32_t t1,
                                                 uint32_t eq, uint32_t nn, uint32_t tl, uint32_t ql,
                                                 uint32_t in, int n) {
        v[0] += (uint32_t)__builtin_popcount(eq & ~t0 & ~t1);  // T
        v[1] += (uint32_t)__builtin_popcount(eq & t0 & ~t1);   // C
        v[2] += (uint32_t)__builtin_popcount(eq & ~t0 & t1);   // A
        v[3] += (uint32_t)__builtin_popcount(eq & t0 & t1);    // G
        v[4] += (uint32_t)__builtin_popcount((tl | ql) & in);
        v[5] += (uint32_t)n;
    }
    static __device__ __forceinline__ void emit(const Args &a, int c, const unsigned long long *s) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s[k]) atomicAdd(&a.match[(int64_t)c * 4 + k], s[k]);
        if (s[4]) atomicAdd(&a.rep[c], s[4]);
        if (s[5]) atomicAdd(&a.total[c], s[5]);
    }
};

// chainToPsl (chainToPsl.c:106-124): N on either side first, then equal bases
// by the target's case, the rest mismatches; the query's case is not read
struct PslPolicy {
    typedef PslArgs Args;
    static constexpr int kVals = 4;  // match, repMatch, nCount, aligned bases
    static constexpr bool kQLower = false;
    static __device__ __forceinline__ void count(uint32_t (&v)[kVals], uint32_t, uint32_t,
                                                 uint32_t eq, uint32_t nn, uint32_t tl, uint32_t,
                                                 uint32_t, int n) {
        v[0] += (uint32_t)__builtin_popcount(eq & ~tl);
        v[1] += (uint32_t)__builtin_popcount(eq & tl);
        v[2] += (uint32_t)__builtin_popcount(nn);
        v[3] += (uint32_t)n;
    }
    static __device__ __forceinline__ void emit(const Args &a, int c, const unsigned long long *s) {
        unsigned long long *o = a.counts + (int64_t)c * 4;  // match, misMatch, repMatch, nCount
        const unsigned long long mis = s[3] - s[0] - s[1] - s[2];
        if (s[0]) atomicAdd(&o[0], s[0]);
        if (mis) atomicAdd(&o[1], mis);
        if (s[1]) atomicAdd(&o[2], s[1]);
        if (s[2]) atomicAdd(&o[3], s[2]);
    }
};

template <class P>
__device__ __forceinline__ void chain_walk(const typename P::Args &a) {
    constexpr int kVals = P::kVals;
    __shared__ CompWave s_w[kWavesPerWG];
    __shared__ unsigned long long s_acc[kCompSlots][kVals];
    __shared__ int s_chain[kCompSlots];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kVals; ++k) s_acc[threadIdx.x][k] = 0ull;
    s_chain[threadIdx.x] = -1;
    __syncthreads();
    const int64_t B0 = (int64_t)blockIdx.x * kCompSlots;
    const int64_t tile = (int64_t)blockIdx.x * kWavesPerWG + wv;
    if (tile < a.ntiles) {  // (wave-uniform; no workgroup barrier inside)
        CompWave &W = s_w[wv];
        const int64_t b = tile * kTileBlocks + lane;
        int len = 0, lenq = 0, slot = 0;
        long long tpos = 0, qpos = 0;
        if (b < a.n_blocks) {
            // the block's chain: last c in [tile_c0[tile], tile_c0[tile + 1]]
            // with coff[c] <= b (an empty chain shares its offset with the next)
            int64_t lo = a.tile_c0[tile], hi = a.tile_c0[tile + 1 < a.ntiles ? tile + 1 : a.ntiles];
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (a.coff[mid] <= b) lo = mid;
                else hi = mid - 1;
            }
            const DChain ch = a.chains[lo];
            const int4 bk = a.blk[b];
            len = bk.z & kSizeMask;
            const bool minus = ch.qbase < 0;
            tpos = ch.tbase + bk.x;
            qpos = minus ? ~ch.qbase - bk.y : ch.qbase + bk.y;
            lenq = len | (minus ? (int)0x80000000 : 0) | (bk.z & (kTHasN | kQHasN));
            // slot: the chain's first block inside this workgroup
            const int64_t first = a.coff[lo];
            slot = (int)((first > B0 ? first : B0) - B0);
            s_chain[slot] = (int)lo;  // (every block of the chain writes the same value)
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
        comp_wave_sync();

        int cur = -1;
        uint32_t v[kVals] = {};
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
            comp_flush(s_acc, lane, cur, v, on && sl != cur);
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
                const cu32x4a8 tv = *reinterpret_cast<const cu32x4a8 *>(a.t_planes + tw);
                const cu32x4a8 qv = *reinterpret_cast<const cu32x4a8 *>(a.q_planes + qw);
                const uint32_t tl = mask_window(a.t_lmask, tw, sht);
                uint32_t ql = 0;
                if (P::kQLower) ql = mask_window(a.q_lmask, qw, shq);
                uint32_t nm = 0, qn = 0;
                if (lq & kTHasN) nm = mask_window(a.t_nmask, tw, sht);
                if (lq & kQHasN) qn = mask_window(a.q_nmask, qw, shq);
                const uint32_t t0 = cfunnel(tv.z, tv.x, sht), t1 = cfunnel(tv.w, tv.y, sht);
                uint32_t q0 = cfunnel(qv.z, qv.x, shq), q1 = cfunnel(qv.w, qv.y, shq);
                if (minus) {
                    // rc base i = comp(fwd[qp + n - 1 - i]): bit-reversed words,
                    // complement = code ^ 2 (the bit-1 plane); masks only reversed
                    q0 = __builtin_bitreverse32(q0) >> sh;
                    q1 = ~(__builtin_bitreverse32(q1) >> sh);
                    ql = __builtin_bitreverse32(ql) >> sh;
                    qn = __builtin_bitreverse32(qn) >> sh;
                }
                const uint32_t in = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
                const uint32_t eq = ~((t0 ^ q0) | (t1 ^ q1)) & ~(nm | qn) & in;
                P::count(v, t0, t1, eq, (nm | qn) & in, tl, ql, in, n);
                cur = sl;
            }
        }
        comp_flush(s_acc, lane, cur, v, true);
    }
    __syncthreads();
    const int c = s_chain[threadIdx.x];
    if (c >= 0) P::emit(a, c, s_acc[threadIdx.x]);  // one add per (workgroup, chain, counter)
}

__global__ void __launch_bounds__(256) k_compose(ComposeArgs a) { chain_walk<ComposePolicy>(a); }

__global__ void __launch_bounds__(256) k_psl_counts(PslArgs a) { chain_walk<PslPolicy>(a); }

}  // namespace

hipError_t launch_compose(const ComposeArgs &a, hipStream_t s) {
    const int64_t g = (a.ntiles + kWavesPerWG - 1) / kWavesPerWG;
    if (g <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_compose, dim3((unsigned)g), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_psl_counts(const PslArgs &a, hipStream_t s) {
    const int64_t g = (a.ntiles + kWavesPerWG - 1) / kWavesPerWG;
    if (g <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_psl_counts, dim3((unsigned)g), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gac
