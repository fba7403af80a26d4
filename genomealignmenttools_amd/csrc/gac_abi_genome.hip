// gac_abi_genome.hip -- libgachain's C ABI, the resident genomes: sequence
// registration, the staged upload through the context's pinned buffers and the
// relayout to bit planes (gac_genome_*).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "gac_ctx.h"

using namespace gac;

// ----------------------------------------------------------------- genomes
static Genome *side_of(gac_ctx *c, int side) {
    if (!c || (side != GAC_T && side != GAC_Q)) return nullptr;
    return &c->g[side];
}

void gac::free_genome(Genome &g) {
    if (g.tb_open) gac_twobit_close(&g.tb);
    if (g.planes) hipFree(g.planes);
    if (g.nmask) hipFree(g.nmask);
    if (g.lmask) hipFree(g.lmask);
    if (g.d_woff) hipFree(g.d_woff);
    if (g.d_nrun) hipFree(g.d_nrun);
    g = Genome();
}

// copy = false: the payload stays where it is (a mapped .2bit file kept open
// by the genome) and is read straight into pinned staging at finalize.
static int add_seq(gac_ctx *c, int side, const char *name, int32_t size, const uint8_t *packed,
                   bool copy, int32_t n_nblocks, const int32_t *n_starts,
                   const int32_t *n_sizes, int32_t n_mask = 0, const int32_t *m_starts = nullptr,
                   const int32_t *m_sizes = nullptr) {
    Genome *g = side_of(c, side);
    if (!g || !name || size < 0 || (size > 0 && !packed) || n_nblocks < 0 || n_mask < 0 ||
        (n_nblocks > 0 && (!n_starts || !n_sizes)) ||
        (n_mask > 0 && (!m_starts || !m_sizes)))
        return gac_fail(GAC_E_ARG, "gac_genome_add_seq: bad argument");
    if (g->final) return gac_fail(GAC_E_STATE, "genome side %d already finalized", side);
    if (g->index.count(name)) return gac_fail(GAC_E_ARG, "duplicate sequence %s", name);
    // (before anything is stored: a refused call leaves the side as it was)
    for (int32_t i = 0; i < n_nblocks; ++i) {
        const int64_t s = n_starts[i], len = n_sizes[i];
        if (s < 0 || len < 0 || s + len > size)
            return gac_fail(GAC_E_FORMAT, "N block %d of %s out of range", i, name);
    }
    int32_t idx = (int32_t)g->names.size();
    g->index[name] = idx;
    g->names.push_back(name);
    g->sizes.push_back(size);
    size_t nbytes = ((size_t)size + 3) / 4;
    if (copy) {
        size_t off = (g->raw.size() + 7) & ~(size_t)7;
        g->raw.resize(off + nbytes);
        if (nbytes) memcpy(g->raw.data() + off, packed, nbytes);
        g->raw_off.push_back((int64_t)off);
        g->ext.push_back(nullptr);
    } else {
        g->raw_off.push_back(-1);
        g->ext.push_back(packed);
    }
    {
        std::vector<std::pair<int32_t, int32_t>> runs;
        for (int32_t i = 0; i < n_nblocks; ++i)
            if (n_sizes[i] > 0) runs.emplace_back(n_starts[i], n_starts[i] + n_sizes[i]);
        std::sort(runs.begin(), runs.end());
        size_t k0 = g->nrun_start.size();
        for (const auto &r : runs) {
            const size_t k = g->nrun_start.size();
            if (k > k0 && r.first <= g->nrun_start[k - 1] + g->nrun_size[k - 1]) {
                const int32_t e = std::max(g->nrun_start[k - 1] + g->nrun_size[k - 1], r.second);
                g->nrun_size[k - 1] = e - g->nrun_start[k - 1];
            } else {
                g->nrun_start.push_back(r.first);
                g->nrun_size.push_back(r.second - r.first);
            }
        }
        g->nrun_off.push_back((int64_t)g->nrun_start.size());
    }
    for (int32_t i = 0; i < n_nblocks; ++i) {
        int64_t s = n_starts[i], len = n_sizes[i];
        while (len > 0) {
            int32_t piece = (int32_t)(len < 1024 ? len : 1024);
            g->npieces.push_back(NPiece{s, piece, 0});
            g->npiece_seq.push_back(idx);
            s += piece;
            len -= piece;
        }
    }
    // mask runs (only for a side that wants the plane): pieces as above; a
    // run reaching past the sequence is clipped (twoBit.c:858-872 clips the
    // runs to the fragment it lower-cases)
    for (int32_t i = 0; g->want_mask && i < n_mask; ++i) {
        int64_t s = m_starts[i], e = s + (int64_t)m_sizes[i];
        if (s < 0) s = 0;
        if (e > size) e = size;
        while (s < e) {
            const int32_t piece = (int32_t)(e - s < 1024 ? e - s : 1024);
            g->mpieces.push_back(NPiece{s, piece, 0});
            g->mpiece_seq.push_back(idx);
            s += piece;
        }
    }
    return GAC_OK;
}

extern "C" int gac_genome_add_seq(gac_ctx *c, int side, const char *name, int32_t size,
                                  const uint8_t *packed, int32_t n_nblocks,
                                  const int32_t *n_starts, const int32_t *n_sizes) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    return add_seq(c, side, name, size, packed, true, n_nblocks, n_starts, n_sizes);
}

extern "C" int gac_genome_add_seq_masked(gac_ctx *c, int side, const char *name, int32_t size,
                                         const uint8_t *packed, int32_t n_nblocks,
                                         const int32_t *n_starts, const int32_t *n_sizes,
                                         int32_t n_mask, const int32_t *mask_starts,
                                         const int32_t *mask_sizes) {
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    return add_seq(c, side, name, size, packed, true, n_nblocks, n_starts, n_sizes, n_mask,
                   mask_starts, mask_sizes);
}

extern "C" int gac_genome_want_softmask(gac_ctx *c, int side) {
    gac_clear_error();
    Genome *g = side_of(c, side);
    if (!g) return gac_fail(GAC_E_ARG, "gac_genome_want_softmask: bad argument");
    CTX_LOCK(c);
    if (g->final || !g->names.empty())
        return gac_fail(GAC_E_STATE, "gac_genome_want_softmask: side %d already has sequences",
                        side);
    g->want_mask = true;
    return GAC_OK;
}

// Staged upload of the packed payloads to d_raw (layout: seqs[i].byte_off,
// 8-byte aligned): host threads copy 32 MB windows into two alternating
// pinned buffers while the previous window's DMA runs.
// (GAC_PIN_MB overrides the window size: measurement knob)
static size_t pin_bytes() {
    static const size_t b = getenv("GAC_PIN_MB") ? (size_t)std::max(1, atoi(getenv("GAC_PIN_MB"))) << 20
                                                  : (size_t)32 << 20;
    return b;
}

struct StageJob {
    const Genome *g;
    const SeqDev *seqs;
    int nseq;
    size_t lo, hi;   // window of the staging layout
    uint8_t *dst;    // pinned buffer (window start)
    int nt;
};

static void *stage_thread_body(StageJob *J, int t) {
    const size_t len = J->hi - J->lo, per = (len + J->nt - 1) / J->nt;
    const size_t a = J->lo + std::min(len, per * t), b = J->lo + std::min(len, per * (t + 1));
    if (a >= b) return nullptr;
    // sequences overlapping [a, b): binary search the first
    int lo = 0, hi = J->nseq;
    while (lo < hi) {
        const int m = (lo + hi) / 2;
        const size_t end = (size_t)J->seqs[m].byte_off + ((size_t)J->seqs[m].size + 3) / 4;
        if (end <= a) lo = m + 1;
        else hi = m;
    }
    size_t pos = a;
    for (int i = lo; i < J->nseq && pos < b; ++i) {
        const size_t s0 = (size_t)J->seqs[i].byte_off;
        const size_t s1 = s0 + ((size_t)J->seqs[i].size + 3) / 4;
        if (s0 > pos) {  // alignment padding
            const size_t z = std::min(s0, b) - pos;
            memset(J->dst + (pos - J->lo), 0, z);
            pos += z;
            if (pos >= b) break;
        }
        const size_t e = std::min(s1, b);
        if (e > pos) {
            memcpy(J->dst + (pos - J->lo), J->g->packed(i) + (pos - s0), e - pos);
            pos = e;
        }
    }
    if (pos < b) memset(J->dst + (pos - J->lo), 0, b - pos);
    return nullptr;
}

struct StageArg {
    StageJob *J;
    std::atomic<int> next;
};

static void *stage_thread(void *p) {
    StageArg *A = (StageArg *)p;
    for (int t; (t = A->next.fetch_add(1)) < A->J->nt;) stage_thread_body(A->J, t);
    return nullptr;
}

static int ensure_pinned(gac_ctx *c) {
    for (int k = 0; k < 2; ++k) {
        if (!c->pin[k]) HIPCHK(hipHostMalloc((void **)&c->pin[k], pin_bytes(), hipHostMallocDefault));
        if (!c->pin_ev[k]) HIPCHK(hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming));
    }
    return GAC_OK;
}

// Sparse: the runs' bytes packed (compact layout, SparseRun::src), staged the
// same way through the pinned windows.
struct StageRunsJob {
    const Genome *g;
    const SparseRun *runs;
    const int32_t *seq;  // registered sequence of each run
    const SeqDev *seqs;
    int64_t nruns;
    size_t lo, hi;
    uint8_t *dst;
    int nt;
};

static void stage_runs_body(StageRunsJob *J, int t) {
    const size_t len = J->hi - J->lo, per = (len + J->nt - 1) / J->nt;
    const size_t a = J->lo + std::min(len, per * t), b = J->lo + std::min(len, per * (t + 1));
    if (a >= b) return;
    int64_t lo = 0, hi = J->nruns;  // first run ending after a
    while (lo < hi) {
        const int64_t m = (lo + hi) / 2;
        if ((size_t)(J->runs[m].src + ((J->runs[m].len + 7) & ~7LL)) <= a) lo = m + 1;
        else hi = m;
    }
    size_t pos = a;
    for (int64_t r = lo; r < J->nruns && pos < b; ++r) {
        const SparseRun &R = J->runs[r];
        const size_t s0 = (size_t)R.src, s1 = s0 + (size_t)R.len;
        const size_t e0 = s0 + (((size_t)R.len + 7) & ~(size_t)7);  // padded end
        const int k = J->seq[r];
        const uint8_t *from = J->g->packed(k) + (R.dst - J->seqs[k].byte_off);
        if (s1 > pos) {
            const size_t e = std::min(s1, b);
            memcpy(J->dst + (pos - J->lo), from + (pos - s0), e - pos);
            pos = e;
        }
        if (pos < b && e0 > pos) {
            const size_t e = std::min(e0, b);
            memset(J->dst + (pos - J->lo), 0, e - pos);
            pos = e;
        }
    }
    if (pos < b) memset(J->dst + (pos - J->lo), 0, b - pos);
}

struct StageRunsArg {
    StageRunsJob *J;
    std::atomic<int> next;
};

static void *stage_runs_thread(void *p) {
    StageRunsArg *A = (StageRunsArg *)p;
    for (int t; (t = A->next.fetch_add(1)) < A->J->nt;) stage_runs_body(A->J, t);
    return nullptr;
}

static int upload_runs(gac_ctx *c, const Genome *g, const SeqDev *seqs, const SparseRun *runs,
                       const int32_t *seq, int64_t nruns, uint8_t *d_compact, size_t bytes) {
    int rc = ensure_pinned(c);
    if (rc != GAC_OK) return rc;
    const int nt = std::max(1, std::min(16, gac_host_threads()));
    int k = 0;
    for (size_t lo = 0; lo < bytes; lo += pin_bytes(), k ^= 1) {
        const size_t hi = std::min(bytes, lo + pin_bytes());
        HIPCHK(hipEventSynchronize(c->pin_ev[k]));
        StageRunsJob J = {g, runs, seq, seqs, nruns, lo, hi, c->pin[k], nt};
        StageRunsArg A;
        A.J = &J;
        A.next = 0;
        gac_run_threads(nt, stage_runs_thread, &A);
        HIPCHK(hipMemcpyAsync(d_compact + lo, c->pin[k], hi - lo, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->pin_ev[k], c->stream));
    }
    return GAC_OK;
}

static int upload_payloads(gac_ctx *c, const Genome *g, const SeqDev *seqs, int nseq,
                           uint8_t *d_raw, size_t raw_bytes) {
    int rc = ensure_pinned(c);
    if (rc != GAC_OK) return rc;
    const int nt = std::max(1, std::min(16, gac_host_threads()));
    int k = 0;
    for (size_t lo = 0; lo < raw_bytes; lo += pin_bytes(), k ^= 1) {
        const size_t hi = std::min(raw_bytes, lo + pin_bytes());
        HIPCHK(hipEventSynchronize(c->pin_ev[k]));  // its previous DMA is done
        StageJob J = {g, seqs, nseq, lo, hi, c->pin[k], nt};
        StageArg A;
        A.J = &J;
        A.next = 0;
        gac_run_threads(nt, stage_thread, &A);
        HIPCHK(hipMemcpyAsync(d_raw + lo, c->pin[k], hi - lo, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->pin_ev[k], c->stream));
    }
    return GAC_OK;
}

// Pageable host array -> device through the context's pinned staging buffers
// (threaded copies into one buffer while the other one's DMA runs).
struct CopyJob {
    const uint8_t *src;
    uint8_t *dst;
    size_t len;
    int nt;
    std::atomic<int> next;
};

static void *copy_thread(void *p) {
    CopyJob *J = (CopyJob *)p;
    const size_t per = (J->len + J->nt - 1) / J->nt;
    for (int t; (t = J->next.fetch_add(1)) < J->nt;) {
        const size_t a = std::min(J->len, per * t), b = std::min(J->len, per * (t + 1));
        if (b > a) memcpy(J->dst + a, J->src + a, b - a);
    }
    return nullptr;
}

int gac::upload_staged(gac_ctx *c, void *d_dst, const void *h_src, size_t bytes) {
    int rc = ensure_pinned(c);
    if (rc != GAC_OK) return rc;
    const int nt = std::max(1, std::min(16, gac_host_threads()));
    int k = 0;
    for (size_t lo = 0; lo < bytes; lo += pin_bytes(), k ^= 1) {
        const size_t hi = std::min(bytes, lo + pin_bytes());
        HIPCHK(hipEventSynchronize(c->pin_ev[k]));
        CopyJob J;
        J.src = (const uint8_t *)h_src + lo;
        J.dst = c->pin[k];
        J.len = hi - lo;
        J.nt = (hi - lo) >= (4u << 20) ? nt : 1;
        J.next = 0;
        gac_run_threads(J.nt, copy_thread, &J);
        HIPCHK(hipMemcpyAsync((uint8_t *)d_dst + lo, c->pin[k], hi - lo, hipMemcpyHostToDevice,
                              c->stream));
        HIPCHK(hipEventRecord(c->pin_ev[k], c->stream));
    }
    return GAC_OK;
}

// GAC_TIMING laps of a genome upload
struct FinLaps {
    bool on = getenv("GAC_TIMING") != nullptr;
    int side;
    double t = wall_s();
    void operator()(const char *what) {
        if (!on) return;
        const double n = wall_s();
        fprintf(stderr, "[gac_genome_finalize %c] %-22s %.3f s\n", side ? 'Q' : 'T', what, n - t);
        t = n;
    }
};

extern "C" int gac_genome_finalize(gac_ctx *c, int side) {
    gac_clear_error();
    Genome *g = side_of(c, side);
    if (!g) return gac_fail(GAC_E_ARG, "gac_genome_finalize: bad side");
    CTX_LOCK(c);
    if (g->final) return gac_fail(GAC_E_STATE, "genome side %d already finalized", side);
    if (g->want_mask && g->sparse)
        return gac_fail(GAC_E_ARG, "the sparse genome upload does not carry the soft-mask plane");
    FinLaps lap;
    lap.side = side;
    HIPCHK(hipSetDevice(c->device));
    const int nseq = (int)g->names.size();
    std::vector<SeqDev> seqs(nseq);
    g->woff.resize(nseq);
    int64_t w = 0;
    size_t raw_bytes = 0;  // staging layout: payloads 8-byte aligned, in sequence order
    for (int i = 0; i < nseq; ++i) {
        raw_bytes = (raw_bytes + 7) & ~(size_t)7;
        seqs[i].byte_off = (int64_t)raw_bytes;
        raw_bytes += ((size_t)g->sizes[i] + 3) / 4;
        seqs[i].word_off = w;
        seqs[i].size = g->sizes[i];
        g->woff[i] = w;
        w += ((int64_t)g->sizes[i] + 31) / 32;
    }
    g->n_words = w;
    // the scoring kernels index plane words in 32 bits (2^37 bases per side)
    if (w + 4 > (int64_t)UINT32_MAX)
        return gac_fail(GAC_E_ARG, "genome of %lld words: over the 2^32-word plane limit", (long long)w);
    const int64_t alloc_words = w + 4;  // padding: windows read word w+1
    HIPCHK(hipMalloc(&g->planes, alloc_words * sizeof(uint2)));
    HIPCHK(hipMalloc(&g->nmask, alloc_words * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&g->d_woff, (nseq ? nseq : 1) * sizeof(int64_t)));
    // (k_relayout writes every word of the sequences: only the padding words
    // past them are set here)
    HIPCHK(hipMemsetAsync(g->planes + w, 0, (alloc_words - w) * sizeof(uint2), c->stream));
    HIPCHK(hipMemsetAsync(g->nmask + w, 0xff, (alloc_words - w) * sizeof(uint32_t), c->stream));
    if (g->want_mask) {  // all zero, then the mask runs are OR-ed in (k_nruns)
        HIPCHK(hipMalloc(&g->lmask, alloc_words * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(g->lmask, 0, alloc_words * sizeof(uint32_t), c->stream));
    }
    if (nseq) {
        HIPCHK(hipMemcpyAsync(g->d_woff, g->woff.data(), nseq * sizeof(int64_t),
                              hipMemcpyHostToDevice, c->stream));
        uint8_t *d_raw = nullptr;
        SeqDev *d_seqs = nullptr;
        NPiece *d_np = nullptr, *d_mp = nullptr;
        HIPCHK(hipMalloc(&d_raw, raw_bytes + 16));
        HIPCHK(hipMalloc(&d_seqs, nseq * sizeof(SeqDev)));
        lap("allocations");
        uint8_t *d_compact = nullptr;
        SparseRun *d_runs = nullptr;
        if (g->sparse) {  // only the listed word runs
            std::vector<SparseRun> runs;
            std::vector<int32_t> rseq;
            int64_t compact = 0;
            for (size_t r = 0; r < g->run_seq.size(); ++r) {
                const int k = g->run_seq[r];
                const int64_t pay = ((int64_t)g->sizes[k] + 3) / 4;
                const int64_t b0 = (int64_t)g->run_lo[r] * 8, b1 = std::min<int64_t>((int64_t)g->run_hi[r] * 8, pay);
                if (b1 <= b0) continue;
                runs.push_back(SparseRun{seqs[k].byte_off + b0, compact, b1 - b0});
                rseq.push_back(k);
                compact += ((b1 - b0) + 7) & ~7LL;
            }
            HIPCHK(hipMalloc(&d_compact, (size_t)compact + 16));
            HIPCHK(hipMalloc(&d_runs, std::max<size_t>(runs.size(), 1) * sizeof(SparseRun)));
            int rc = upload_runs(c, g, seqs.data(), runs.data(), rseq.data(), (int64_t)runs.size(),
                                 d_compact, (size_t)compact);
            if (rc != GAC_OK) return rc;
            HIPCHK(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(SparseRun),
                                  hipMemcpyHostToDevice, c->stream));
            HIPCHK(launch_scatter(d_runs, (int64_t)runs.size(), (const uint64_t *)d_compact,
                                  (uint64_t *)d_raw, c->stream));
            lap("sparse runs queued");
        } else {
            int rc = upload_payloads(c, g, seqs.data(), nseq, d_raw, raw_bytes);
            if (rc != GAC_OK) return rc;
            lap("payload copies queued");
        }
        HIPCHK(hipMemcpyAsync(d_seqs, seqs.data(), nseq * sizeof(SeqDev), hipMemcpyHostToDevice,
                              c->stream));
        HIPCHK(launch_relayout(d_raw, d_seqs, nseq, w, g->planes, g->nmask, c->stream));
        const int64_t np = (int64_t)g->npieces.size();
        if (np) {
            for (int64_t i = 0; i < np; ++i)
                g->npieces[i].bit0 += g->woff[g->npiece_seq[i]] * 32;
            HIPCHK(hipMalloc(&d_np, np * sizeof(NPiece)));
            HIPCHK(hipMemcpyAsync(d_np, g->npieces.data(), np * sizeof(NPiece),
                                  hipMemcpyHostToDevice, c->stream));
            HIPCHK(launch_nruns(d_np, np, g->nmask, c->stream));
        }
        const int64_t nmp = (int64_t)g->mpieces.size();
        if (nmp) {
            for (int64_t i = 0; i < nmp; ++i)
                g->mpieces[i].bit0 += g->woff[g->mpiece_seq[i]] * 32;
            HIPCHK(hipMalloc(&d_mp, nmp * sizeof(NPiece)));
            HIPCHK(hipMemcpyAsync(d_mp, g->mpieces.data(), nmp * sizeof(NPiece),
                                  hipMemcpyHostToDevice, c->stream));
            HIPCHK(launch_nruns(d_mp, nmp, g->lmask, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));
        lap("relayout + N runs done");
        if (d_compact) hipFree(d_compact);
        if (d_runs) hipFree(d_runs);
        hipFree(d_raw);
        hipFree(d_seqs);
        if (d_np) hipFree(d_np);
        if (d_mp) hipFree(d_mp);
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    std::vector<NPiece>().swap(g->npieces);
    std::vector<int32_t>().swap(g->npiece_seq);
    std::vector<NPiece>().swap(g->mpieces);
    std::vector<int32_t>().swap(g->mpiece_seq);
    {  // global N runs (chain-level N test at chain upload)
        std::vector<longlong2> gr(g->nrun_start.size());
        for (int i = 0; i < nseq; ++i)
            for (int64_t k = g->nrun_off[i]; k < g->nrun_off[i + 1]; ++k) {
                gr[k].x = g->woff[i] * 32 + g->nrun_start[k];
                gr[k].y = gr[k].x + g->nrun_size[k];
            }
        g->n_nrun = (int64_t)gr.size();
        HIPCHK(hipMalloc(&g->d_nrun, std::max<size_t>(gr.size(), 1) * sizeof(longlong2)));
        if (!gr.empty())
            HIPCHK(hipMemcpy(g->d_nrun, gr.data(), gr.size() * sizeof(longlong2),
                             hipMemcpyHostToDevice));
    }
    g->final = true;
    return GAC_OK;
}

extern "C" int gac_genome_load_2bit(gac_ctx *c, int side, const char *path) {
    gac_clear_error();
    if (!side_of(c, side) || !path) return gac_fail(GAC_E_ARG, "gac_genome_load_2bit: bad argument");
    gac_twobit tb;
    int rc = gac_twobit_open(path, &tb);
    if (rc != GAC_OK) return rc;
    return gac_genome_load_twobit(c, side, &tb);
}

extern "C" int gac_genome_load_2bit_runs(gac_ctx *c, int side, const char *path,
                                         const uint8_t *keep, const int64_t *run_off,
                                         const int32_t *run_lo, const int32_t *run_hi) {
    gac_clear_error();
    if (!side_of(c, side) || !path || (run_off && (!run_lo || !run_hi)))
        return gac_fail(GAC_E_ARG, "gac_genome_load_2bit_runs: bad argument");
    gac_twobit tb;
    int rc = gac_twobit_open(path, &tb);
    if (rc != GAC_OK) return rc;
    return gac_genome_load_twobit_runs(c, side, &tb, keep, run_off, run_lo, run_hi);
}

extern "C" int gac_genome_load_twobit(gac_ctx *c, int side, gac_twobit *tbp) {
    return gac_genome_load_twobit_runs(c, side, tbp, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int gac_genome_load_twobit_keep(gac_ctx *c, int side, gac_twobit *tbp,
                                           const uint8_t *keep) {
    return gac_genome_load_twobit_runs(c, side, tbp, keep, nullptr, nullptr, nullptr);
}

extern "C" int gac_genome_load_twobit_runs(gac_ctx *c, int side, gac_twobit *tbp,
                                           const uint8_t *keep, const int64_t *run_off,
                                           const int32_t *run_lo, const int32_t *run_hi) {
    gac_clear_error();
    if (!side_of(c, side) || !tbp) {
        if (tbp) gac_twobit_close(tbp);
        return gac_fail(GAC_E_ARG, "gac_genome_load_twobit: bad argument");
    }
    CTX_LOCK(c);
    gac_twobit tb = *tbp;
    int rc = GAC_OK;
    std::vector<int32_t> ns, nz, ms, mz;
    const bool want_mask = side_of(c, side)->want_mask;
    if (want_mask && run_off) {
        gac_twobit_close(&tb);
        return gac_fail(GAC_E_ARG, "the sparse genome upload does not carry the soft-mask plane");
    }
    for (uint32_t i = 0; i < tb.seq_count && rc == GAC_OK; ++i) {
        if (keep && !keep[i]) continue;  // a sequence this process never scores
        const gac_twobit_seq &s = tb.seqs[i];
        ns.resize(s.n_count);
        nz.resize(s.n_count);
        for (uint32_t k = 0; k < s.n_count; ++k) {
            ns[k] = (int32_t)gac_twobit_u32(&tb, s.n_starts_raw + 4 * k);
            nz[k] = (int32_t)gac_twobit_u32(&tb, s.n_sizes_raw + 4 * k);
        }
        const uint32_t mc = want_mask ? s.m_count : 0;
        ms.resize(mc);
        mz.resize(mc);
        for (uint32_t k = 0; k < mc; ++k) {
            ms[k] = (int32_t)gac_twobit_u32(&tb, s.m_starts_raw + 4 * k);
            mz[k] = (int32_t)gac_twobit_u32(&tb, s.m_sizes_raw + 4 * k);
        }
        rc = add_seq(c, side, s.name, (int32_t)s.size, s.packed, false, (int32_t)s.n_count,
                     ns.data(), nz.data(), (int32_t)mc, ms.data(), mz.data());
        if (rc == GAC_OK && run_off) {  // this sequence's word runs
            Genome *g = side_of(c, side);
            g->sparse = true;
            const int32_t k = (int32_t)g->names.size() - 1;
            const int64_t nw = ((int64_t)s.size + 31) / 32;
            for (int64_t r = run_off[i]; r < run_off[i + 1]; ++r) {
                const int32_t lo = std::max<int32_t>(0, run_lo[r]);
                const int32_t hi = (int32_t)std::min<int64_t>(nw, run_hi[r]);
                if (hi <= lo) continue;
                g->run_seq.push_back(k);
                g->run_lo.push_back(lo);
                g->run_hi.push_back(hi);
            }
        }
    }
    if (rc != GAC_OK) {  // the side holds pointers into tb: drop it whole
        free_genome(*side_of(c, side));
        gac_twobit_close(&tb);
        return rc;
    }
    // the payloads are read from the mapping at finalize and by gac_genome_view
    Genome *g = side_of(c, side);
    g->tb = tb;
    g->tb_open = true;
    return gac_genome_finalize(c, side);
}

extern "C" int32_t gac_genome_seq_count(gac_ctx *c, int side) {
    Genome *g = side_of(c, side);
    return g ? (int32_t)g->names.size() : -1;
}

extern "C" int32_t gac_genome_seq_index(gac_ctx *c, int side, const char *name) {
    Genome *g = side_of(c, side);
    if (!g || !name) return -1;
    auto it = g->index.find(name);
    return it == g->index.end() ? -1 : it->second;
}

extern "C" int32_t gac_genome_seq_size(gac_ctx *c, int side, int32_t i) {
    Genome *g = side_of(c, side);
    if (!g || i < 0 || i >= (int32_t)g->sizes.size()) return -1;
    return g->sizes[i];
}

extern "C" const char *gac_genome_seq_name(gac_ctx *c, int side, int32_t i) {
    Genome *g = side_of(c, side);
    if (!g || i < 0 || i >= (int32_t)g->names.size()) return nullptr;
    return g->names[i].c_str();
}

extern "C" int gac_genome_decode(gac_ctx *c, int side, int32_t i, int32_t start, int32_t end,
                                 char *out) {
    gac_clear_error();
    Genome *g = side_of(c, side);
    if (!g || !g->final || i < 0 || i >= (int32_t)g->sizes.size() || start < 0 ||
        end > g->sizes[i] || start > end || !out)
        return gac_fail(GAC_E_ARG, "gac_genome_decode: bad argument");
    if (start == end) return GAC_OK;
    HIPCHK(hipSetDevice(c->device));
    const int64_t w0 = g->woff[i] + start / 32, w1 = g->woff[i] + (end - 1) / 32 + 1;
    std::vector<uint2> pl(w1 - w0);
    std::vector<uint32_t> nm(w1 - w0);
    HIPCHK(hipMemcpy(pl.data(), g->planes + w0, pl.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(nm.data(), g->nmask + w0, nm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    static const char nt[4] = {'t', 'c', 'a', 'g'};
    for (int32_t p = start; p < end; ++p) {
        const int64_t w = g->woff[i] + p / 32 - w0;
        const int b = p & 31;
        if ((nm[w] >> b) & 1u) {
            out[p - start] = 'n';
        } else {
            const int code = (int)(((pl[w].y >> b) & 1u) << 1 | ((pl[w].x >> b) & 1u));
            out[p - start] = nt[code];
        }
    }
    return GAC_OK;
}

extern "C" int gac_genome_planes(gac_ctx *c, int side, const void **planes,
                                 const uint32_t **nmask, const uint32_t **lmask,
                                 int64_t *n_words) {
    gac_clear_error();
    Genome *g = side_of(c, side);
    if (!g || !planes || !nmask || !lmask || !n_words)
        return gac_fail(GAC_E_ARG, "gac_genome_planes: bad argument");
    CTX_LOCK(c);
    if (!g->final) return gac_fail(GAC_E_STATE, "genome side %d is not finalized", side);
    *planes = g->planes;
    *nmask = g->nmask;
    *lmask = g->lmask;
    *n_words = g->n_words;
    return GAC_OK;
}

extern "C" int gac_genome_view(gac_ctx *c, int side, int32_t i, gac_seq_view *v) {
    Genome *g = side_of(c, side);
    if (!g || !g->final || i < 0 || i >= (int32_t)g->sizes.size() || !v)
        return gac_fail(GAC_E_ARG, "gac_genome_view: bad argument");
    v->packed = g->packed(i);
    v->size = g->sizes[i];
    v->n_start = g->nrun_start.data() + g->nrun_off[i];
    v->n_size = g->nrun_size.data() + g->nrun_off[i];
    v->n_count = (int32_t)(g->nrun_off[i + 1] - g->nrun_off[i]);
    return GAC_OK;
}

extern "C" int gac_genome_decode_case(gac_ctx *c, int side, int32_t i, int32_t start, int32_t end,
                                      char *out) {
    gac_clear_error();
    Genome *g = side_of(c, side);
    if (!g || !g->final || i < 0 || i >= (int32_t)g->sizes.size() || start < 0 ||
        end > g->sizes[i] || start > end || !out)
        return gac_fail(GAC_E_ARG, "gac_genome_decode_case: bad argument");
    if (!g->lmask) return gac_fail(GAC_E_STATE, "genome side %d has no soft-mask plane", side);
    if (start == end) return GAC_OK;
    int rc = gac_genome_decode(c, side, i, start, end, out);
    if (rc != GAC_OK) return rc;
    const int64_t w0 = g->woff[i] + start / 32, w1 = g->woff[i] + (end - 1) / 32 + 1;
    std::vector<uint32_t> lm(w1 - w0);
    HIPCHK(hipMemcpy(lm.data(), g->lmask + w0, lm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int32_t p = start; p < end; ++p) {
        const int64_t w = g->woff[i] + p / 32 - w0;
        if (!((lm[w] >> (p & 31)) & 1u)) out[p - start] = (char)(out[p - start] - 'a' + 'A');
    }
    return GAC_OK;
}
