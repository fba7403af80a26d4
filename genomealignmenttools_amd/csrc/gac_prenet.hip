// gac_prenet.hip -- chainPreNet's keep decision (gac_prenet_keep;
// kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c:104-137): which chains, in
// file order, still have a base that the padded blocks of the chains kept
// before them leave clear.  gfx950 only.
//
// The reference sets a bitmap chain by chain.  Here the question is asked per
// base for all chains at once: fc[base] = the lowest rank (chain index) among
// the chains of a covering set A whose padded blocks hold the base, and chain
// i is open under A when one of its own bases has fc >= i (nothing, itself or
// a later chain got there first).  A dropped chain covers nothing, so the
// covering set is the kept set K itself, the one set with K = open-under(K).
// Open-under is antitone in A: with L <= K <= U, open-under(U) <= K <=
// open-under(L).  A round therefore takes two passes (gac_abi_prenet.hip):
// with U = kept + undecided, the undecided chains that are open are kept; with
// L = kept only, those that are not open are dropped.  The lowest undecided
// chain is settled in every round (everything below it is decided, so U and L
// agree there).
//
// A pass, per side and per group of that side's sequences:
//   fill   fc = kPrenetNone (a memset of the group's words)
//   len    per block: its padded, clipped length if its chain is in the
//          covering set and its sequence in the group, else 0 -- then the
//          shared 64-bit scan.  The scan is the compaction: blocks of other
//          chains and groups take no room in the flat layout.
//   mark   flat over those bases: a workgroup takes kPrenetTile consecutive flat
//          bases, finds the blocks of its first and last one, drops the
//          number of every block between them at its first flat base in an
//          LDS table and takes the running maximum: the block of every flat
//          base, without a search per base; consecutive lanes touch
//          consecutive words.  A lane loads the word and sends atomicMin only
//          when the word is above its rank (a stale word is never below the
//          true one, so a skipped atomic was not needed); deep coverage comes
//          mostly from later, lower chains, which skip.
//   len, scan, check   the same layout over the unpadded blocks of the undecided
//          chains: a lane whose base has fc >= its rank stores 1 into
//          open[chain], once per run of lanes of one chain (every writer
//          writes the same value); chains already open are not looked at again.
//
// Memory: 4 bytes per base of the largest group, 40 bytes per block (three
// inputs, the chain, length, offset and first word), 19 per chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kPrenetThreads = 256;
constexpr int64_t kPrenetMaxGrid = 2048;  // workgroups; the rest by grid stride
constexpr int kPrenetTile = 4096;         // flat bases per workgroup step

__device__ __forceinline__ int64_t prenet_id() {
    return (int64_t)blockIdx.x * kPrenetThreads + threadIdx.x;
}

__device__ __forceinline__ int64_t prenet_stride() {
    return (int64_t)gridDim.x * kPrenetThreads;
}

// the last k in [lo, hi] with off[k] <= f (off ascends, off[lo] <= f)
__device__ __forceinline__ int64_t prenet_find(const long long *off, int64_t lo, int64_t hi,
                                               long long f) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= f)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_chains(PrenetArgs a) {
    for (int64_t i = prenet_id(); i < a.n; i += prenet_stride()) {
        a.state[i] = a.seq[0][i] < 0 || a.seq[1][i] < 0 ? kPrenetSkipped : kPrenetUndecided;
        a.open[i] = 0;
    }
}

__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_bchain(PrenetArgs a) {
    for (int64_t b = prenet_id(); b < a.nb; b += prenet_stride())
        a.bchain[b] = (int32_t)prenet_find((const long long *)a.boff, 0, a.n - 1, b);
}

template <bool MARK>
__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_len(PrenetArgs a) {
    const int sd = a.side;
    for (int64_t b = prenet_id(); b <= a.nb; b += prenet_stride()) {
        long long len = 0;
        if (b < a.nb) {
            const int32_t c = a.bchain[b];
            const uint8_t st = a.state[c];
            const bool live = MARK ? st == kPrenetKept || (a.with_undecided && st == kPrenetUndecided)
                                   : st == kPrenetUndecided && !a.open[c];
            if (live) {
                const int32_t seq = a.seq[sd][c];
                if (a.sgroup[sd][seq] == a.group) {
                    const long long start = a.bstart[sd][b], z = a.bsize[b];
                    long long s = start;
                    if (MARK) {
                        s = start - a.pad < 0 ? 0 : start - a.pad;
                        const long long size = a.ssize[sd][seq];
                        const long long e = start + z + a.pad > size ? size : start + z + a.pad;
                        len = e - s;
                    } else {
                        len = z;
                    }
                    a.badr[b] = a.sbase[sd][seq] + s;
                }
            }
        }
        a.len[b] = len;
    }
}

// where flat position p of a step lives in the step's LDS table: one word of
// padding per 16, so that a thread's 16 consecutive entries and a wave's 64
// consecutive ones both spread over the banks
__device__ __forceinline__ int prenet_slot(int p) { return p + (p >> 4); }

template <bool MARK>
__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_flat(PrenetArgs a) {
    constexpr int kPer = kPrenetTile / kPrenetThreads;
    __shared__ int64_t ends[2];
    __shared__ int32_t idx[kPrenetTile + kPrenetTile / 16];  // per flat base: its block - lo
    __shared__ int32_t wmax[kPrenetThreads / kWave];
    const long long total = a.off[a.nb];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (long long f0 = (long long)blockIdx.x * kPrenetTile; f0 < total;
         f0 += (long long)gridDim.x * kPrenetTile) {
        const long long f1 = f0 + kPrenetTile < total ? f0 + kPrenetTile : total;
        if (tid == 0) ends[0] = prenet_find(a.off, 0, a.nb, f0);
        if (tid == kWave) ends[1] = prenet_find(a.off, 0, a.nb, f1 - 1);
        for (int k = 0; k < kPer; ++k) idx[prenet_slot(k * kPrenetThreads + tid)] = 0;
        __syncthreads();
        // the step's blocks are [lo, hi]; those after lo that have bases start
        // inside it, each at a place of its own
        const int64_t lo = ends[0], hi = ends[1];
        for (int64_t b = lo + 1 + tid; b <= hi; b += kPrenetThreads) {
            const long long o = a.off[b];
            if (a.off[b + 1] > o) idx[prenet_slot((int)(o - f0))] = (int32_t)(b - lo);
        }
        __syncthreads();
        // running maximum over the step = the block each flat base lies in
        int32_t v[kPer], m = 0;
        for (int j = 0; j < kPer; ++j) {
            const int32_t x = idx[prenet_slot(tid * kPer + j)];
            m = x > m ? x : m;
            v[j] = m;
        }
        int32_t inc = m;
        for (int d = 1; d < kWave; d <<= 1) {
            const int32_t t = __shfl_up(inc, d);
            if (lane >= d && t > inc) inc = t;
        }
        if (lane == kWave - 1) wmax[wave] = inc;
        int32_t pre = __shfl_up(inc, 1);
        if (lane == 0) pre = 0;
        __syncthreads();
        for (int w = 0; w < wave; ++w) pre = wmax[w] > pre ? wmax[w] : pre;
        for (int j = 0; j < kPer; ++j) idx[prenet_slot(tid * kPer + j)] = v[j] > pre ? v[j] : pre;
        __syncthreads();
        for (int k = 0; k < kPer; ++k) {
            const int p = k * kPrenetThreads + tid;
            const long long f = f0 + p;
            int32_t c = -1;
            bool hit = false;
            if (f < f1) {
                const int64_t b = lo + idx[prenet_slot(p)];
                c = a.bchain[b];
                uint32_t *w = a.fc + (a.badr[b] + (f - a.off[b]));
                if (MARK) {
                    if (*w > (uint32_t)c) atomicMin(w, (uint32_t)c);
                } else if (!a.open[c]) {
                    hit = *w >= (uint32_t)c;
                }
            }
            if (!MARK) {
                // one store per run of lanes of one chain
                const int32_t pc = __shfl_up(c, 1);
                const int ph = __shfl_up((int)hit, 1);
                if (hit && (lane == 0 || pc != c || !ph)) a.open[c] = 1;
            }
        }
        __syncthreads();  // the tables are rewritten by the next step
    }
}

// pass 1: the undecided chains open under kept + undecided are kept; pass 2:
// those not open under the kept chains are dropped, and what is left is counted
__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_decide(PrenetArgs a, int pass) {
    const int64_t n_up = (a.n + kPrenetThreads - 1) / kPrenetThreads * kPrenetThreads;
    for (int64_t i = prenet_id(); i < n_up; i += prenet_stride()) {
        uint8_t st = kPrenetSkipped;
        if (i < a.n) {
            st = a.state[i];
            if (st == kPrenetUndecided) {
                const bool open = a.open[i] != 0;
                if (pass == 1 && open) st = kPrenetKept;
                if (pass == 2 && !open) st = kPrenetDropped;
                a.state[i] = st;
            }
            a.open[i] = 0;
        }
        if (pass == 2) {
            const unsigned long long und = __ballot(st == kPrenetUndecided);
            const unsigned long long kept = __ballot(st == kPrenetKept);
            if ((threadIdx.x & (kWave - 1)) == 0) {
                if (und) atomicAdd(&a.counts[0], (unsigned long long)__popcll(und));
                if (kept) atomicAdd(&a.counts[1], (unsigned long long)__popcll(kept));
            }
        }
    }
}

__global__ void __launch_bounds__(kPrenetThreads)
    k_prenet_flags(PrenetArgs a, uint8_t *keep) {
    for (int64_t i = prenet_id(); i < a.n; i += prenet_stride())
        keep[i] = a.state[i] == kPrenetKept;
}

unsigned prenet_grid(int64_t items) {
    const int64_t g = (items + kPrenetThreads - 1) / kPrenetThreads;
    return (unsigned)(g < 1 ? 1 : g > kPrenetMaxGrid ? kPrenetMaxGrid : g);
}

}  // namespace

hipError_t launch_prenet_setup(const PrenetArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_prenet_chains, dim3(prenet_grid(a.n)), dim3(kPrenetThreads), 0, s, a);
    if (a.nb > 0)
        hipLaunchKernelGGL(k_prenet_bchain, dim3(prenet_grid(a.nb)), dim3(kPrenetThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_prenet_len(const PrenetArgs &a, bool mark, hipStream_t s) {
    if (mark)
        hipLaunchKernelGGL(k_prenet_len<true>, dim3(prenet_grid(a.nb + 1)), dim3(kPrenetThreads), 0, s,
                           a);
    else
        hipLaunchKernelGGL(k_prenet_len<false>, dim3(prenet_grid(a.nb + 1)), dim3(kPrenetThreads), 0,
                           s, a);
    return hipGetLastError();
}

// the flat total is on the device only: a full grid, idle workgroups leave at once
hipError_t launch_prenet_mark(const PrenetArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_prenet_flat<true>, dim3((unsigned)kPrenetMaxGrid), dim3(kPrenetThreads), 0, s,
                       a);
    return hipGetLastError();
}

hipError_t launch_prenet_check(const PrenetArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_prenet_flat<false>, dim3((unsigned)kPrenetMaxGrid), dim3(kPrenetThreads), 0,
                       s, a);
    return hipGetLastError();
}

hipError_t launch_prenet_decide(const PrenetArgs &a, int pass, hipStream_t s) {
    hipLaunchKernelGGL(k_prenet_decide, dim3(prenet_grid(a.n)), dim3(kPrenetThreads), 0, s, a, pass);
    return hipGetLastError();
}

hipError_t launch_prenet_flags(const PrenetArgs &a, uint8_t *keep, hipStream_t s) {
    hipLaunchKernelGGL(k_prenet_flags, dim3(prenet_grid(a.n)), dim3(kPrenetThreads), 0, s, a, keep);
    return hipGetLastError();
}

}  // namespace gac
