// gac_abi_chains.hip -- libgachain's C ABI, the chain sets: the host-side
// build of a set, its upload and its release (gac_chains_*).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "gac_ctx.h"

using namespace gac;

// ----------------------------------------------------------------- chains
// Host-side build of the device chain set, in parallel over chain ranges
// balanced by blocks: validation + DChain records (pass 1), bucket-index
// offsets (serial prefix), then blocks / spans / bucket indexes (pass 2).
struct UploadJob {
    gac_ctx *c;
    const gac_chainset_desc *d;
    DChain *ch;
    const int64_t *cut;  // chain ranges per task
    std::atomic<int> next;
    int ntask;
    std::atomic<long long> err_chain;  // first failing chain (pass 1), -1 if none
};

static void upload_pass1(UploadJob *J, int64_t i0, int64_t i1) {
    const gac_chainset_desc *d = J->d;
    gac_ctx *c = J->c;
    for (int64_t i = i0; i < i1; ++i) {
        const int32_t ts = d->t_seq[i], qs = d->q_seq[i];
        DChain &x = J->ch[i];
        bool bad = ts < 0 || ts >= (int32_t)c->g[0].sizes.size() || qs < 0 ||
                   qs >= (int32_t)c->g[1].sizes.size();
        const int64_t b0 = d->blk_off[i], b1 = d->blk_off[i + 1];
        bad = bad || b0 < 0 || b1 < b0 || b1 > d->n_blocks || b1 - b0 > INT32_MAX;
        if (!bad) {
            const int32_t tsize = c->g[0].sizes[ts], qsize = c->g[1].sizes[qs];
            int64_t pt = 0, pq = 0;
            for (int64_t b = b0; b < b1 && !bad; ++b) {
                const int64_t t = d->blk_t[b], q = d->blk_q[b], z = d->blk_size[b];
                bad = z < 0 || z >= (1 << 29) || t < 0 || q < 0 || t + z > tsize || q + z > qsize ||
                      (b > b0 && (t < pt || q < pq));
                pt = t + z;
                pq = q + z;
            }
            x.qinfo = qsize | (d->q_strand[i] ? (int32_t)0x80000000 : 0);
        }
        if (bad) {  // reported (with the serial check's message) by the caller
            long long cur = J->err_chain.load();
            while ((cur < 0 || i < cur) && !J->err_chain.compare_exchange_weak(cur, i)) {
            }
            return;
        }
        x.blk_off = b0;
        x.nblk = (int32_t)(b1 - b0);
        x.t_seq = ts;
        x.q_seq = qs;
        x.tstart = b1 > b0 ? d->blk_t[b0] : 0;
        x.tend = b1 > b0 ? d->blk_t[b1 - 1] + d->blk_size[b1 - 1] : 0;
        const int64_t span = (int64_t)x.tend - x.tstart;
        int shift = 0;
        while (span > 0 && (((span - 1) >> shift) + 1) > std::max<int64_t>(2 * x.nblk, 1)) ++shift;
        x.shift = shift;
        x.pad = 0;
        x.idx_off = (span > 0 ? ((span - 1) >> shift) + 1 : 0) + 1;  // count until the prefix
        x.tbase = c->g[0].woff[ts] * 32;
        const int64_t qw = c->g[1].woff[qs] * 32;
        x.qbase = x.qinfo < 0 ? ~(qw + (x.qinfo & 0x7fffffff)) : qw;
    }
}

static void *upload_thread(void *p) {
    UploadJob *J = (UploadJob *)p;
    for (int t; (t = J->next.fetch_add(1)) < J->ntask;) {
        upload_pass1(J, J->cut[t], J->cut[t + 1]);
    }
    return nullptr;
}

static void free_whole_plan(gac_chainset *cs) {
    void *w[] = {cs->w_rdesc, cs->w_nblk, cs->w_gflat, cs->w_tile_r0, cs->w_status,
                 cs->w_empty, cs->w_pb0,  cs->w_perm,  cs->w_tile_perm};
    for (void *p : w)
        if (p) hipFree(p);
    cs->w_rdesc = nullptr;
    cs->w_nblk = cs->w_gflat = cs->w_tile_r0 = cs->w_status = cs->w_empty = nullptr;
    cs->w_pb0 = cs->w_perm = cs->w_tile_perm = nullptr;
    cs->w_sorted = false;
    cs->w_nempty = 0;
    cs->w_ready = false;
}

// device buffer *p of capacity *cap holds at least want elements of sz bytes
// (grown with headroom; the contents are not kept)
hipError_t gac::ensure_buf(void **p, size_t *cap, size_t want, size_t sz) {
    if (*p && *cap >= want) return hipSuccess;
    if (*p) hipFree(*p);
    *p = nullptr;
    const size_t n = want + want / 4 + 64;
    const hipError_t e = hipMalloc(p, n * sz);
    *cap = e == hipSuccess ? n : 0;
    return e;
}

// the context's scoring setup, as the upload kernels take it
UploadGaps gac::upload_gaps(const gac_ctx *c, Blk12 *blk12) {
    UploadGaps G;
    G.blk12 = blk12;
    G.g = c->gap;
    G.small = c->d_small;
    G.tab = c->d_gap_tab;
    G.len = c->gap_len;
    return G;
}

// the chain set's contents := d (its device buffers reused where they fit)
static int chains_fill(gac_ctx *c, const gac_chainset_desc *d, gac_chainset *cs) {
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before uploading chains");
    if (d->n_chains < 0 || d->n_blocks < 0 || (d->n_chains && (!d->t_seq || !d->q_seq ||
                                                                !d->q_strand || !d->blk_off)))
        return gac_fail(GAC_E_ARG, "gac_chains_upload: bad descriptor");
    if (d->n_chains && d->blk_off[d->n_chains] != d->n_blocks)
        return gac_fail(GAC_E_ARG, "blk_off[n_chains] != n_blocks");
    // every block belongs to a chain: the flat upload kernels find a block's
    // chain by its offset, so blocks before chain 0 (or with no chain) would
    // be written to negative positions
    if (d->n_chains && d->blk_off[0] != 0)
        return gac_fail(GAC_E_ARG, "blk_off[0] != 0");
    if (!d->n_chains && d->n_blocks)
        return gac_fail(GAC_E_ARG, "blocks without chains (n_chains == 0, n_blocks > 0)");
    // the kernels index blocks of one chain set with int32 (RangeDesc::b0,
    // flat windows): a larger set must be uploaded in parts
    if (d->n_blocks > (int64_t)INT32_MAX - 16)
        return gac_fail(GAC_E_ARG, "chain set of %lld blocks: at most %d per gac_chains_upload "
                        "(upload it in parts)", (long long)d->n_blocks, INT32_MAX - 16);
    const int64_t n = d->n_chains;
    const bool timing = getenv("GAC_TIMING") != nullptr;
    double t_lap = wall_s();
    const double t_fill0 = t_lap;
    auto lap = [&](const char *what) {
        if (!timing) return;
        const double t = wall_s();
        fprintf(stderr, "[gac_chains_upload] %-22s %.3f s\n", what, t - t_lap);
        t_lap = t;
    };
    // (not value-initialised: upload_pass1 writes every field of every good
    // chain on its own thread, so the 64 B/chain are first touched in
    // parallel instead of zeroed on this thread -- 320 MB at C5)
    // (freed on a detached thread when the fill returns: freeing it here
    // waited ~0.11 s at axtChain's C4 chain scoring -- glibc trimming the
    // heap top behind other threads' unmapping, r05c4t4; a private mapping
    // instead was slower still, r05c4t5)
    const size_t n_rec = (size_t)(n ? n : 1);
    struct LateArr {
        DChain *p;
        size_t bytes;
        explicit LateArr(size_t k) : p((DChain *)malloc(k * sizeof(DChain))), bytes(k * sizeof(DChain)) {}
        ~LateArr() {
            DChain *q = p;
            if (!q) return;
            // only the tens-of-MB staging of C4/C5-sized sets goes to a
            // thread: a small set (tests, re-uploads, loops) frees inline
            if (bytes < ((size_t)16 << 20)) {
                free(q);
                return;
            }
            try {
                std::thread([q] { free(q); }).detach();
            } catch (...) {
                free(q);
            }
        }
        DChain *get() const { return p; }
        DChain &operator[](size_t i) const { return p[i]; }
    } ch(n_rec);
    if (!ch.get()) return gac_fail(GAC_E_HIP, "gac_chains_upload: out of host memory");
    if (!n) memset(ch.get(), 0, sizeof(DChain));
    // tasks: contiguous chain ranges of about equal blocks + chains
    const int nt = std::max(1, std::min(64, gac_host_threads()));
    const int ntask = (int)std::min<int64_t>(std::max<int64_t>(n, 1), 8 * nt);
    std::vector<int64_t> cut(ntask + 1, n);
    {
        const int64_t work = d->n_blocks + n;
        int64_t i = 0;
        cut[0] = 0;
        for (int t = 1; t < ntask; ++t) {
            const int64_t target = work * t / ntask;
            while (i < n && d->blk_off[i] + i < target) ++i;
            cut[t] = i;
        }
        cut[ntask] = n;
    }
    UploadJob J;
    J.c = c;
    J.d = d;
    J.ch = ch.get();
    J.cut = cut.data();
    J.ntask = ntask;
    J.next = 0;
    J.err_chain = -1;
    gac_run_threads(std::min(nt, ntask), upload_thread, &J);
    if (J.err_chain.load() >= 0) {  // the first bad chain: the serial checks, for the message
        const int64_t i = J.err_chain.load();
        const int32_t ts = d->t_seq[i], qs = d->q_seq[i];
        if (ts < 0 || ts >= (int32_t)c->g[0].sizes.size() || qs < 0 ||
            qs >= (int32_t)c->g[1].sizes.size())
            return gac_fail(GAC_E_ARG, "chain %lld: sequence index out of range", (long long)i);
        const int64_t b0 = d->blk_off[i], b1 = d->blk_off[i + 1];
        if (b0 < 0 || b1 < b0 || b1 > d->n_blocks || b1 - b0 > INT32_MAX)
            return gac_fail(GAC_E_ARG, "chain %lld: bad block offsets", (long long)i);
        const int32_t tsize = c->g[0].sizes[ts], qsize = c->g[1].sizes[qs];
        int64_t pt = 0, pq = 0;
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t t = d->blk_t[b], q = d->blk_q[b], z = d->blk_size[b];
            if (z < 0 || z >= (1 << 29) || t < 0 || q < 0 || t + z > tsize || q + z > qsize)
                return gac_fail(GAC_E_FORMAT,
                                "chain %lld block %lld [t %lld q %lld size %lld] outside its "
                                "sequences (tSize %d qSize %d)",
                                (long long)i, (long long)(b - b0), (long long)t, (long long)q,
                                (long long)z, tsize, qsize);
            if (b > b0 && (t < pt || q < pq))
                return gac_fail(GAC_E_FORMAT, "chain %lld: blocks not ascending (negative gap)",
                                (long long)i);
            pt = t + z;
            pq = q + z;
        }
        return gac_fail(GAC_E_FORMAT, "chain %lld: invalid", (long long)i);
    }
    lap("chain records + checks");
    int64_t idx_n = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t k = ch[i].idx_off;
        ch[i].idx_off = idx_n;
        idx_n += k;
    }
    HIPCHK(hipSetDevice(c->device));
    cs->ctx = c;
    cs->n_chains = d->n_chains;
    cs->n_blocks = d->n_blocks;
    cs->gap_version = 0;  // block gaps are computed at the next scoring call
    free_whole_plan(cs);
    const size_t nb = (size_t)d->n_blocks;
    // the caller's block arrays, staged; blocks / spans / buckets are built
    // from them on the device (k_build_*)
    hipError_t e = ensure_buf((void **)&cs->chains, &cs->cap_chains, n_rec, sizeof(DChain));
    if (e == hipSuccess) e = ensure_buf((void **)&cs->blk, &cs->cap_blocks, nb + 8, sizeof(int4));
    if (e == hipSuccess) e = ensure_buf((void **)&cs->blk12, &cs->cap_blk12, nb + 8, sizeof(Blk12));
    // (the window-search index -- spans, bucket entries -- is allocated
    // with the index itself: ensure_index, or here when it is built eagerly)
    static const bool eager = [] {
        const char *v = getenv("GAC_UP_INDEX");
        return v && !strcmp(v, "eager");
    }();
    cs->idx_n = idx_n;
    if (e == hipSuccess && eager)
        e = ensure_buf((void **)&cs->tspan, &cs->cap_tspan, nb + 8, sizeof(int2));
    if (e == hipSuccess && eager)
        e = ensure_buf((void **)&cs->bucket, &cs->cap_idx, (size_t)std::max<int64_t>(idx_n, 1), 4);
    if (e == hipSuccess)
        e = ensure_buf((void **)&cs->d_stage, &cs->cap_stage, std::max<size_t>(3 * nb, 1), 4);
    int32_t *d_bt = cs->d_stage;
    int rc = GAC_OK;
    lap("allocations");
    if (e == hipSuccess) rc = upload_staged(c, cs->chains, ch.get(), n_rec * sizeof(DChain));
    if (e == hipSuccess && rc == GAC_OK && nb) rc = upload_staged(c, d_bt, d->blk_t, nb * 4);
    if (e == hipSuccess && rc == GAC_OK && nb) rc = upload_staged(c, d_bt + nb, d->blk_q, nb * 4);
    if (e == hipSuccess && rc == GAC_OK && nb) rc = upload_staged(c, d_bt + 2 * nb, d->blk_size, nb * 4);
    lap("staged copies");
    // blocks, spans, bucket indexes and per-block N flags (scoring skips the
    // N-mask loads of N-free blocks), one lane per block
    const int64_t ntiles = ((int64_t)nb + 63) >> 6;
    if (e == hipSuccess)
        e = ensure_buf((void **)&cs->d_coff, &cs->cap_coff, (size_t)(n + 1), sizeof(int32_t));
    if (e == hipSuccess)
        e = ensure_buf((void **)&cs->d_tile_c0, &cs->cap_tile_c0, (size_t)(ntiles + 1), sizeof(int32_t));
    if (e == hipSuccess)
        e = ensure_buf((void **)&cs->d_crun, &cs->cap_crun, (size_t)(n ? n : 1), sizeof(int4));
    // with the scoring already set, the block gaps and 12-byte records come
    // out of the same pass (GAC_UP_FUSE=0: at the first scoring call, as
    // when the scoring follows the chains)
    static const bool fuse = [] {
        const char *v = getenv("GAC_UP_FUSE");
        return !(v && v[0] == '0');
    }();
    const bool gaps = fuse && c->scoring;
    const UploadGaps G = gaps ? upload_gaps(c, cs->blk12) : UploadGaps{};
    // the window-search index only on demand: chainNet -rescore hands its
    // windows over and whole chains need none (GAC_UP_INDEX=eager: now)
    if (e == hipSuccess && rc == GAC_OK)
        e = launch_build_flat(d_bt, d_bt + nb, d_bt + 2 * nb, (int64_t)nb, cs->chains, n, cs->d_coff,
                              cs->d_tile_c0, cs->d_crun, c->g[0].d_nrun, c->g[0].n_nrun,
                              c->g[1].d_nrun, c->g[1].n_nrun, c->g[1].d_woff, cs->blk, cs->tspan,
                              cs->bucket, G, eager, c->stream);
    cs->idx_ready = eager;
    if (e == hipSuccess && rc == GAC_OK && gaps) cs->gap_version = c->gap_version;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    lap("device build + sync");
    if (timing)
        fprintf(stderr, "[gac_chains_upload] laps from the fill's start: %.3f s\n", wall_s() - t_fill0);
    if (rc != GAC_OK) return rc;
    if (e != hipSuccess) return gac_fail(GAC_E_HIP, "chain upload failed: %s", hipGetErrorString(e));
    return GAC_OK;
}

extern "C" int gac_chains_upload(gac_ctx *c, const gac_chainset_desc *d, gac_chainset **out) {
    gac_clear_error();
    if (!c || !d || !out) return gac_fail(GAC_E_ARG, "gac_chains_upload: NULL argument");
    const double t_in = wall_s();
    CTX_LOCK(c);
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[gac_chains_upload] context lock          %.3f s\n", wall_s() - t_in);
    *out = nullptr;
    gac_chainset *cs = new gac_chainset();
    cs->ctx = c;
    c->sets.push_back(cs);
    const double t_f = wall_s();
    const int rc = chains_fill(c, d, cs);
    const double t_r = wall_s();
    if (rc != GAC_OK) {
        gac_chains_free(cs);
        return rc;
    }
    *out = cs;
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[gac_chains_upload] total                 %.3f s (before the fill %.3f, "
                        "fill %.3f)\n", wall_s() - t_in, t_f - t_in, t_r - t_f);
    return GAC_OK;
}

extern "C" int gac_chains_reupload(gac_ctx *c, const gac_chainset_desc *d, gac_chainset *cs) {
    gac_clear_error();
    if (!c || !d || !cs) return gac_fail(GAC_E_ARG, "gac_chains_reupload: NULL argument");
    if (cs->ctx != c) return gac_fail(GAC_E_ARG, "gac_chains_reupload: a set of another context");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));  // (calls in flight may still read the set)
    return chains_fill(c, d, cs);
}

void gac::free_set_memory(gac_chainset *cs) {
    hipSetDevice(cs->ctx->device);  // (hipFree waits for work still using them)
    void *bufs[] = {cs->chains, cs->blk,     cs->blk12,     cs->tspan,  cs->bucket,
                    cs->d_stage, cs->d_coff, cs->d_tile_c0, cs->d_crun};
    for (void *p : bufs)
        if (p) hipFree(p);
    cs->chains = nullptr;
    cs->blk = nullptr;
    cs->blk12 = nullptr;
    cs->tspan = nullptr;
    cs->bucket = nullptr;
    cs->d_stage = nullptr;
    cs->d_coff = cs->d_tile_c0 = nullptr;
    cs->d_crun = nullptr;
    free_whole_plan(cs);
}

extern "C" void gac_chains_free(gac_chainset *cs) {
    if (!cs) return;
    if (gac_ctx *c = cs->ctx) {  // (NULL: its context was closed, the memory went with it)
        CTX_LOCK(c);
        free_set_memory(cs);
        c->sets.erase(std::remove(c->sets.begin(), c->sets.end(), cs), c->sets.end());
        if (c->srv.cs == cs) c->srv.cs = nullptr;
    }
    delete cs;
}

extern "C" gac_ctx *gac_chains_context(const gac_chainset *cs) { return cs ? cs->ctx : nullptr; }

extern "C" int64_t gac_chains_block_count(const gac_chainset *cs) { return cs ? cs->n_blocks : -1; }
