// gac_axtscore.hip -- axtToMaf -score's column sum (gac_axt_score;
// kent/src/lib/axt.c:196-229 axtScoreSym over :423-458 axtScoreSchemeDefault):
// the blastz score of an alignment's two rows.  gfx950 only.
//
// axtScoreSym walks the columns with one flag, lastGap.  That flag is nothing
// but "column i - 1 is a gap column", so column i adds
//   gap(i)  ? -30 - (i > 0 && gap(i - 1) ? 0 : 400)
//           : matrix[t[i]][q[i]]
// where gap(i) = either character is '-'.  The score is a plain integer sum of
// terms that each depend on two neighbouring columns: no scan, any order, and
// exact modulo 2^32, which is how the reference's int wraps.
//
// The work is flat over chunks of kAxtsChunk consecutive columns of one entry
// (pieces of chains average under a hundred columns, net pieces and lastz hits
// run to hundreds of kilobases: a wave per entry would leave one wave with all
// the work).  k_axt_score_chunks writes every entry's number of chunks, the
// shared 64-bit scan makes them first chunks, and in k_axt_score a wave takes
// a chunk, finds its entry by binary search over the first chunks, sums the
// chunk's columns four a lane and a step, reduces across its lanes and adds the
// sum to the entry's 32-bit word with one atomic.  An entry without columns has
// no chunk and keeps the zero the caller stored.
//
// The two rows of an entry start at unrelated bytes.  A lane's four columns
// of a row are taken from the two aligned 32-bit words that hold them, shifted
// by the row's own misalignment; the words before a row's first and after its
// last byte that this touches lie inside the batch's buffer (launch_axt_score's
// contract: 4-byte aligned, 8 readable bytes past text_bytes) and their bytes
// never reach a sum.  The column before a lane's first one comes from the lane
// below, from the step before, or, for a chunk's first column, from the two
// bytes before it in the rows -- never for column 0 of an entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gac_kernels.h"

namespace gac {

namespace {

constexpr int kAxtsThreads = 256;
constexpr int kAxtsWaves = kAxtsThreads / kWave;  // chunks a workgroup takes at a time
constexpr int kAxtsPer = 4;                       // columns a lane sums in a step: one word a row
constexpr int kAxtsStep = kWave * kAxtsPer;       // columns a wave sums in a step
constexpr int64_t kAxtsMaxGrid = 1 << 20;         // workgroups; the rest by grid stride
static_assert(kAxtsChunk % kAxtsStep == 0, "a chunk is whole steps");

constexpr int kGapOpen = 400, kGapExtend = 30;
// the matrix, a c g t by a c g t, one signed byte a cell (row-major from bit 0)
constexpr unsigned long long cell(int v) { return (unsigned long long)(uint8_t)(int8_t)v; }
constexpr unsigned long long row(int a, int c, int g, int t) {
    return cell(a) | cell(c) << 8 | cell(g) << 16 | cell(t) << 24;
}
constexpr unsigned long long kMatAC = row(91, -114, -31, -123) | row(-114, 100, -125, -31) << 32;
constexpr unsigned long long kMatGT = row(-31, -125, 100, -114) | row(-123, -31, -114, 91) << 32;

// a c g t in either case -> 0 1 2 3, anything else -> 4
__device__ __forceinline__ unsigned axts_class(unsigned c) {
    const unsigned l = c | 0x20u;
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

__device__ __forceinline__ int axts_matrix(unsigned tc, unsigned qc) {
    const unsigned t = axts_class(tc), q = axts_class(qc);
    if ((t | q) & 4u) return 0;
    const unsigned long long m = t < 2u ? kMatAC : kMatGT;
    return (int)(int8_t)(m >> (8u * (((t & 1u) << 2) | q)));
}

// the four bytes at p (any alignment) from the two aligned words around them
__device__ __forceinline__ uint32_t axts_load4(const uint8_t *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const unsigned long long two = (unsigned long long)w[1] << 32 | w[0];
    return (uint32_t)(two >> (8u * (unsigned)(a & 3u)));
}

__global__ void __launch_bounds__(kAxtsThreads) k_axt_score_chunks(AxtsArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kAxtsThreads + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * kAxtsThreads) {
        const AxtsEntry e = a.ent[i];
        int64_t L = e.len;
        // (the host checked the rows against the text; a record that fails here is not read)
        if (L < 0 || e.t < 0 || e.q < 0 || e.t > a.text_bytes - L || e.q > a.text_bytes - L) L = 0;
        a.nchunk[i] = (L + kAxtsChunk - 1) / kAxtsChunk;
    }
}

__global__ void __launch_bounds__(kAxtsThreads) k_axt_score(AxtsArgs a, int64_t chunks) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;

    for (int64_t chunk = (int64_t)blockIdx.x * kAxtsWaves + wave; chunk < chunks; chunk += (int64_t)gridDim.x * kAxtsWaves) {
        // the last entry whose first chunk is <= chunk (entries without a chunk
        // share the first chunk of the next one that has some, and precede it)
        int64_t lo = 0, hi = a.n - 1;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (a.chunk0[mid] <= chunk)
                lo = mid;
            else
                hi = mid - 1;
        }
        const AxtsEntry e = a.ent[lo];
        const int64_t L = e.len;
        const int64_t c0 = (chunk - a.chunk0[lo]) * kAxtsChunk;  // the chunk's first column
        // (as in the chunks pass: nothing of a record that fails is read; a
        // chunk past its entry's columns means the scan and the records disagree)
        if (c0 < 0 || c0 >= L || e.t < 0 || e.q < 0 || e.t > a.text_bytes - L || e.q > a.text_bytes - L) continue;
        const int64_t left = L - c0;
        const int ncols = (int)(left < kAxtsChunk ? left : kAxtsChunk);
        const uint8_t *trow = a.text + e.t + c0, *qrow = a.text + e.q + c0;

        // is the column before the chunk a gap column (wave-uniform)
        unsigned carry = 0;
        if (c0 > 0) carry = trow[-1] == '-' || qrow[-1] == '-';

        int sum = 0;
        for (int s0 = 0; s0 < ncols; s0 += kAxtsStep) {
            const int j = s0 + lane * kAxtsPer;  // the lane's first column in the chunk
            const int nv = ncols - j;            // its columns, if positive (more than 4: all 4)
            uint32_t tw = 0, qw = 0;
            if (nv > 0) tw = axts_load4(trow + j), qw = axts_load4(qrow + j);
            unsigned gaps = 0;  // bit k: the lane's column k is a gap column
            int part = 0;
#pragma unroll
            for (int k = 0; k < kAxtsPer; ++k) {
                const unsigned tc = (tw >> (8 * k)) & 0xffu, qc = (qw >> (8 * k)) & 0xffu;
                if (k >= nv) continue;
                if (tc == '-' || qc == '-') {
                    gaps |= 1u << k;
                    part -= kGapExtend;
                } else {
                    part += axts_matrix(tc, qc);
                }
            }
            // the openings: gap columns whose previous column is none
            unsigned below = __shfl_up(gaps >> (kAxtsPer - 1), 1, kWave);
            if (lane == 0) below = carry;
            const unsigned opens = gaps & ~(gaps << 1 | (below & 1u));
            part -= kGapOpen * __popc(opens);
            sum += part;
            carry = __shfl(gaps >> (kAxtsPer - 1), kWave - 1, kWave) & 1u;  // (read only after a full step)
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, kWave);
        if (lane == 0) atomicAdd(a.score + lo, (uint32_t)sum);
    }
}

}  // namespace

hipError_t launch_axt_score_chunks(const AxtsArgs &a, hipStream_t s) {
    if (a.n < 0) return hipErrorInvalidValue;
    if (a.n == 0) return hipSuccess;
    const int64_t want = (a.n + kAxtsThreads - 1) / kAxtsThreads;
    const int64_t grid = want < kAxtsMaxGrid ? want : kAxtsMaxGrid;
    hipLaunchKernelGGL(k_axt_score_chunks, dim3((unsigned)grid), dim3(kAxtsThreads), 0, s, a);
    return hipGetLastError();
}

// a.text: 4-byte aligned, and 8 bytes past a.text_bytes readable
hipError_t launch_axt_score(const AxtsArgs &a, int64_t chunks, hipStream_t s) {
    if (a.n < 0 || chunks < 0 || (reinterpret_cast<uintptr_t>(a.text) & 3u)) return hipErrorInvalidValue;
    if (a.n == 0 || chunks == 0) return hipSuccess;
    const int64_t want = (chunks + kAxtsWaves - 1) / kAxtsWaves;
    const int64_t grid = want < kAxtsMaxGrid ? want : kAxtsMaxGrid;
    hipLaunchKernelGGL(k_axt_score, dim3((unsigned)grid), dim3(kAxtsThreads), 0, s, a, chunks);
    return hipGetLastError();
}

}  // namespace gac
