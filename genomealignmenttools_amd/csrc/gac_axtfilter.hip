// gac_axtfilter.hip -- filterAxtIdentityEntropy's window test (gac_axt_filter;
// src/filterAxtIdentityEntropy.py:88-110 checkAxt over :144-162 processHit's
// counts, :41-42 getSeqIdent, :45-69 getEntropy): which alignments have a
// window of W columns, starting on a target base, with enough matching columns
// and enough entropy of the target's a/c/g/t counts.  gfx950 only.
//
// The script keeps five running counts per column and takes differences.  Here
// a workgroup takes a chunk -- CH = kAxtfTile - W consecutive window starts of
// one entry -- and with it the chunk's CH + W - 1 columns of both rows:
//   load   lane-consecutive bytes of both rows, classified on the way into one
//          code byte per column in LDS: the target's count (a c g t or none),
//          the column matches, the target is a gap
//   scan   a thread sums the packed increments of its 8 consecutive columns,
//          the workgroup scans the threads' totals (shuffles, then the four
//          waves' totals), and P[j + 1] = the counts of columns [0, j] goes to
//          LDS.  The five counts share one 64-bit word, 11 bits each (a c g t
//          match from bit 0): a tile holds at most kAxtfTile - 1 = 2047
//          columns, so no field of a prefix overflows into its neighbour, and
//          since the fields of a prefix never decrease, P[s + W] - P[s] is
//          borrow-free field by field.  launch_axt_filter refuses a window
//          that would break the bound.
//   test   a lane per window start s: the difference, target[s] != '-',
//          matches >= m_min (the host turned minSeqIdent into that integer),
//          and the entropy from the host's table of p log p: e = 0.0, then
//          e -= term in a, c, g, t order, zero counts skipped, and e / ln2 >=
//          minEntropy.  IEEE double subtractions and one division; nothing
//          here calls a transcendental, and the unit is built with
//          -ffp-contract=off like the rest.
//   mark   the workgroup ORs its lanes' results at a barrier and one lane
//          stores 1 into the entry's own 32-bit word: every writer of a word
//          writes the same value, no read-modify-write.
// A workgroup finds its entry by binary search over the entries' first chunks
// (the host's 64-bit prefix); all offsets into the text are 64-bit, and rows
// start at any byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kAxtfThreads = 256;
constexpr int kAxtfPer = kAxtfTile / kAxtfThreads;  // columns a thread scans
constexpr int64_t kAxtfMaxGrid = 1 << 20;           // workgroups; the rest by grid stride
constexpr int kAxtfBits = 11;                       // a packed field
constexpr unsigned long long kAxtfField = (1ull << kAxtfBits) - 1;
static_assert(kAxtfPer == 8, "a thread's columns are one 64-bit LDS word of codes");
static_assert(kAxtfTile - 1 <= (int)kAxtfField, "a tile's counts fit a packed field");
static_assert(kAxtfMaxWindow < kAxtfTile, "a chunk holds at least one window start");

// code byte of a column: bits 0-2 the target's count (0-3 = a c g t, 4 = none),
// bit 3 the column matches, bit 4 the target is '-'
constexpr unsigned kCodeNone = 4, kCodeMatch = 8, kCodeGap = 16;

__device__ __forceinline__ unsigned axtf_lower(unsigned c) {
    return c - 'A' <= (unsigned)('Z' - 'A') ? c + 32 : c;
}

__device__ __forceinline__ unsigned axtf_code(unsigned tc, unsigned qc) {
    const unsigned t = axtf_lower(tc);
    unsigned code = t == 'a' ? 0u : t == 'c' ? 1u : t == 'g' ? 2u : t == 't' ? 3u : kCodeNone;
    if (t == axtf_lower(qc)) code |= kCodeMatch;
    if (tc == '-') code |= kCodeGap;
    return code;
}

__device__ __forceinline__ unsigned long long axtf_inc(unsigned code) {
    const unsigned cls = code & 7u;
    unsigned long long v = cls < 4u ? 1ull << (kAxtfBits * cls) : 0ull;
    if (code & kCodeMatch) v += 1ull << (kAxtfBits * 4);
    return v;
}

__global__ void __launch_bounds__(kAxtfThreads) k_axt_filter(AxtfArgs a, int64_t chunks) {
    __shared__ unsigned long long P[kAxtfTile + 1];
    __shared__ unsigned long long code8[kAxtfTile / 8];
    __shared__ unsigned long long wave_total[kAxtfThreads / kWave];
    uint8_t *code = reinterpret_cast<uint8_t *>(code8);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int W = a.window, CH = kAxtfTile - W;

    for (int64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        // the last entry whose first chunk is <= chunk (entries without a chunk
        // share the first chunk of the next one that has some, and precede it)
        int64_t lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (a.ent[mid].chunk0 <= chunk)
                lo = mid;
            else
                hi = mid - 1;
        }
        const AxtfEntry e = a.ent[lo];
        const int64_t L = e.len;
        const int64_t s0 = (chunk - e.chunk0) * CH;  // the chunk's first start = its first column
        const int64_t left = L - W + 1 - s0;         // starts from s0 on
        int nstarts = (int)(left < CH ? left : CH);
        // (the host checked the rows against the text; a record that fails here is not read)
        if (e.chunk0 > chunk || e.t < 0 || e.q < 0 || e.t > a.text_bytes - L || e.q > a.text_bytes - L)
            nstarts = 0;
        const int ncols = nstarts > 0 ? nstarts + W - 1 : 0;  // <= kAxtfTile - 1

        const uint8_t *trow = a.text + e.t + s0, *qrow = a.text + e.q + s0;
        for (int j = tid; j < kAxtfTile; j += kAxtfThreads)
            code[j] = (uint8_t)(j < ncols ? axtf_code(trow[j], qrow[j]) : kCodeNone);
        __syncthreads();

        // inclusive counts of the thread's columns, then of everything before them
        const unsigned long long codes = code8[tid];
        unsigned long long run[kAxtfPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kAxtfPer; ++k) {
            sum += axtf_inc((unsigned)(codes >> (8 * k)) & 0xffu);
            run[k] = sum;
        }
        unsigned long long incl = sum;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) wave_total[wave] = incl;
        __syncthreads();
        unsigned long long before = incl - sum;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        if (tid == 0) P[0] = 0;
#pragma unroll
        for (int k = 0; k < kAxtfPer; ++k) P[tid * kAxtfPer + k + 1] = before + run[k];
        __syncthreads();

        int pass = 0;
        for (int s = tid; s < nstarts; s += kAxtfThreads) {
            const unsigned long long d = P[s + W] - P[s];
            const int m = (int)((d >> (kAxtfBits * 4)) & kAxtfField);
            if ((code[s] & kCodeGap) || m < a.m_min) continue;
            int cnt[4], n = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                cnt[b] = (int)((d >> (kAxtfBits * b)) & kAxtfField);
                n += cnt[b];
            }
            double H = 0.0;
            if (n != 0) {
                const int row = n * (n - 1) / 2 - 1;  // term[row + k]: p = k / n
                double ent = 0.0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (cnt[b] != 0) ent -= a.term[row + cnt[b]];
                H = ent / a.ln2;
            }
            if (H >= a.min_entropy) pass = 1;
        }
        // (also the barrier between this chunk's LDS reads and the next one's writes)
        if (__syncthreads_or(pass) && tid == 0) a.keep[lo] = 1u;
    }
}

}  // namespace

hipError_t launch_axt_filter(const AxtfArgs &a, int64_t chunks, hipStream_t s) {
    // the packed counters' bound: CH + W - 1 = kAxtfTile - 1 columns, CH >= 1
    if (a.window < 1 || a.window > kAxtfMaxWindow || a.n < 0 || chunks < 0) return hipErrorInvalidValue;
    if (a.n == 0 || chunks == 0) return hipSuccess;
    const int64_t grid = chunks < kAxtfMaxGrid ? chunks : kAxtfMaxGrid;
    hipLaunchKernelGGL(k_axt_filter, dim3((unsigned)grid), dim3(kAxtfThreads), 0, s, a, chunks);
    return hipGetLastError();
}

}  // namespace gac
