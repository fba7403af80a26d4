// gac_device.hip -- libgachain's C ABI (include/gachain.h), the device scoring
// paths: gac_score_blocks, the workspace and the launch pipeline, the resident
// small-batch server, whole chains, ranges and windows (gac_score_*), and the
// kent-API text entry points.  The other subjects of the ABI are the
// gac_abi_*.hip units; all of them share gac_ctx.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <vector>

#include "gac_ctx.h"

using namespace gac;

constexpr size_t kStatusBytes = 128;  // status[0..9) (see ScoreArgs::status)

// The block jobs of gac_score_blocks, 1 M-block chunks on all threads (one
// pair can hold a quarter of a whole-genome run); the first bad block in
// order is kept for the serial message.
struct BlockFill {
    const int64_t *blk_off;
    int64_t np, n;
    const int32_t *bt, *bq, *bs;
    const int64_t *tw, *qw;  // per pair: global base of the target / query sequence
    const int32_t *tsz, *qsz;
    const uint8_t *minus;
    BlockJob *jobs;
    std::atomic<int64_t> next, err_b;
};

static void *block_fill_thread(void *arg) {
    BlockFill *F = (BlockFill *)arg;
    const int64_t chunk = 1 << 20;
    for (int64_t a; (a = F->next.fetch_add(chunk)) < F->n;) {
        const int64_t e = std::min(F->n, a + chunk);
        int64_t p = std::upper_bound(F->blk_off, F->blk_off + F->np + 1, a) - F->blk_off - 1;
        for (int64_t b = a; b < e; ++b) {
            if (b < F->blk_off[0]) {  // (before the first pair: an empty job, as before)
                F->jobs[b] = BlockJob{0, 0, 0, 0};
                continue;
            }
            if (p < 0) p = 0;
            while (b >= F->blk_off[p + 1]) ++p;  // (past empty pairs too)
            const int32_t bt = F->bt[b], bq = F->bq[b], sz = F->bs[b];
            if (bt < 0 || bq < 0 || sz < 0 || (int64_t)bt + sz > F->tsz[p] ||
                (int64_t)bq + sz > F->qsz[p]) {
                int64_t cur = F->err_b.load();
                while ((cur < 0 || b < cur) && !F->err_b.compare_exchange_weak(cur, b)) {
                }
                break;
            }
            BlockJob &j = F->jobs[b];
            j.tp = F->tw[p] + bt;
            j.minus = F->minus[p];
            j.qp = j.minus ? F->qw[p] + (F->qsz[p] - bq) : F->qw[p] + bq;
            j.n = sz;
        }
    }
    return nullptr;
}

extern "C" int gac_score_blocks(gac_ctx *c, int64_t n_pairs, const int32_t *t_seq,
                                const int32_t *q_seq, const uint8_t *q_strand,
                                const int64_t *blk_off, const int32_t *blk_t,
                                const int32_t *blk_q, const int32_t *blk_size, int32_t *score) {
    gac_clear_error();
    if (!c || n_pairs < 0 || (n_pairs && (!t_seq || !q_seq || !q_strand || !blk_off)))
        return gac_fail(GAC_E_ARG, "gac_score_blocks: bad argument");
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_score_blocks before gac_set_scoring");
    CTX_LOCK(c);
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before scoring blocks");
    const int64_t n = n_pairs ? blk_off[n_pairs] : 0;
    if (n == 0) return GAC_OK;
    if (!blk_t || !blk_q || !blk_size || !score)
        return gac_fail(GAC_E_ARG, "gac_score_blocks: NULL block array");
    const Genome &T = c->g[0], &Q = c->g[1];
    std::vector<int64_t> tw(n_pairs), qw(n_pairs);
    std::vector<int32_t> tsz(n_pairs), qsz(n_pairs);
    std::vector<uint8_t> minus(n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int32_t ts = t_seq[p], qs = q_seq[p];
        if (ts < 0 || ts >= (int32_t)T.sizes.size() || qs < 0 || qs >= (int32_t)Q.sizes.size())
            return gac_fail(GAC_E_ARG, "gac_score_blocks: pair %lld: bad sequence index",
                            (long long)p);
        if (blk_off[p + 1] < blk_off[p])
            return gac_fail(GAC_E_ARG, "gac_score_blocks: pair %lld: block offsets descend",
                            (long long)p);
        tw[p] = T.woff[ts] * 32, qw[p] = Q.woff[qs] * 32;
        tsz[p] = T.sizes[ts], qsz[p] = Q.sizes[qs];
        minus[p] = q_strand[p] ? 1 : 0;
    }
    // (not value-initialised: every job is written by a fill thread)
    std::unique_ptr<BlockJob[]> jobs(new BlockJob[n]);
    BlockFill F;
    F.blk_off = blk_off, F.np = n_pairs, F.n = n;
    F.bt = blk_t, F.bq = blk_q, F.bs = blk_size;
    F.tw = tw.data(), F.qw = qw.data(), F.tsz = tsz.data(), F.qsz = qsz.data();
    F.minus = minus.data();
    F.jobs = jobs.get();
    F.next = 0;
    F.err_b = -1;
    const int nt = std::max(1, std::min(16, gac_host_threads()));
    gac_run_threads((int)std::min<int64_t>(nt, (n + (1 << 20) - 1) >> 20), block_fill_thread, &F);
    if (F.err_b.load() >= 0) {  // the first bad block in order, as the serial check reports it
        const int64_t b = F.err_b.load();
        const int64_t p = std::upper_bound(blk_off, blk_off + n_pairs + 1, b) - blk_off - 1;
        return gac_fail(GAC_E_ARG, "block %lld (%d %d %d) outside %s/%s", (long long)b, blk_t[b],
                        blk_q[b], blk_size[b], T.names[t_seq[p]].c_str(), Q.names[q_seq[p]].c_str());
    }
    HIPCHK(hipSetDevice(c->device));
    BlockJob *d_jobs = nullptr;
    int32_t *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_jobs, n * sizeof(BlockJob)));
    HIPCHK(hipMalloc((void **)&d_out, n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(d_jobs, jobs.get(), n * sizeof(BlockJob), hipMemcpyHostToDevice,
                          c->stream));
    ScoreArgs a;
    memset(&a, 0, sizeof(a));
    a.t_planes = T.planes;
    a.t_nmask = T.nmask;
    a.q_planes = Q.planes;
    a.q_nmask = Q.nmask;
    memcpy(a.coef, c->coef, sizeof(a.coef));
    a.sym = c->sym;
    HIPCHK(launch_blocks(a, d_jobs, n, d_out, c->stream));
    HIPCHK(hipMemcpyAsync(score, d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hipFree(d_jobs);
    hipFree(d_out);
    return GAC_OK;
}

// ----------------------------------------------------------------- launch
static int ensure_ws(gac_ctx *c, int64_t n, int64_t max_tiles, hipStream_t s) {
    // buffers may still be in use by calls in flight (on this stream or, for
    // the device-pointer API, on the stream of the previous call)
    if (n > c->ws_n || max_tiles > c->ws_tiles || !c->status) {
        HIPCHK(hipStreamSynchronize(s));
        if (c->ws_last && c->ws_last != s) HIPCHK(hipEventSynchronize(c->ws_ev));
    }
    if (n > c->ws_n) {
        int64_t cap = n + n / 2 + 1024;
        void *bufs[] = {c->rdesc, c->nblk, c->goff, c->pb0, c->agg, c->plan_off, c->lbflag, c->gflat, c->lbflag};
        for (void *p : bufs)
            if (p) hipFree(p);
        c->rdesc = nullptr;
        c->lbflag = nullptr;
        c->nblk = c->goff = c->pb0 = c->plan_off = c->gflat = nullptr;
        c->agg = nullptr;
        const int64_t G = plan_grid(cap) + 2;
        HIPCHK(hipMalloc(&c->rdesc, cap * sizeof(RangeDesc)));
        HIPCHK(hipMalloc(&c->nblk, cap * 4));
        HIPCHK(hipMalloc(&c->goff, cap * 4));
        HIPCHK(hipMalloc(&c->pb0, cap * 4));
        HIPCHK(hipMalloc(&c->gflat, cap * 4));
        HIPCHK(hipMalloc(&c->agg, G * 4));
        HIPCHK(hipMalloc(&c->plan_off, G * 4));
        HIPCHK(hipMalloc(&c->lbflag, G * 8));
        HIPCHK(hipMemsetAsync(c->lbflag, 0, G * 8, s));  // (no tag: "not yet")
        // (this memset returns success but leaves hipErrorInvalidValue as the
        // thread's last error on this runtime, which the next launch check
        // would report as its own: consumed here; r06lbdbg)
        (void)hipGetLastError();
        c->ws_n = cap;
    }
    if (!c->status) {
        HIPCHK(hipMalloc(&c->status, kStatusBytes));
        HIPCHK(hipMemsetAsync(c->status, 0, kStatusBytes, s));
    }
    if (max_tiles > c->ws_tiles) {
        int64_t cap = max_tiles + max_tiles / 4 + 1024;
        void *old[] = {c->sum_head, c->sum_tail, c->tile_r0, c->sup_head, c->sup_tail,
                       c->sup_tail_r};
        for (void *p : old)
            if (p) hipFree(p);
        c->sum_head = c->sum_tail = c->sup_head = c->sup_tail = nullptr;
        c->tile_r0 = c->sup_tail_r = nullptr;
        const int64_t ucap = cap / kWave + 2;
        HIPCHK(hipMalloc(&c->sum_head, cap * sizeof(SegSum)));
        HIPCHK(hipMalloc(&c->sum_tail, cap * sizeof(SegSum)));
        HIPCHK(hipMalloc(&c->tile_r0, cap * 4));
        HIPCHK(hipMalloc(&c->sup_head, ucap * sizeof(SegSum)));
        HIPCHK(hipMalloc(&c->sup_tail, ucap * sizeof(SegSum)));
        HIPCHK(hipMalloc(&c->sup_tail_r, ucap * 4));
        c->ws_tiles = cap;
    }
    return GAC_OK;
}

// Spin on the pinned status words until k_scan_agg of call `tag` has written
// them (checking now and then that the stream is still busy).
static int wait_status(gac_ctx *c, hipStream_t s, int32_t tag, int32_t st[4]) {
    volatile int32_t *h = c->h_stat;
    for (uint64_t spin = 0;; ++spin) {
        if (h[4] == tag) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            for (int k = 0; k < 4; ++k) st[k] = h[k];
            return GAC_OK;
        }
        if ((spin & 1023) == 1023) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess && h[4] != tag)
                return gac_fail(GAC_E_HIP, "scoring status never arrived (call %d)", tag);
            if (q != hipSuccess && q != hipErrorNotReady)
                return gac_fail(GAC_E_HIP, "scoring failed: %s", hipGetErrorString(q));
        }
        __builtin_ia32_pause();
    }
}

// the set's window-search index (spans + bucket entries), built at the first
// call that searches windows (stream-ordered before it)
static int ensure_index(gac_ctx *c, const gac_chainset *cs_in, hipStream_t s) {
    gac_chainset *cs = const_cast<gac_chainset *>(cs_in);
    if (cs->idx_ready || (cs->n_blocks == 0 && cs->n_chains == 0)) return GAC_OK;
    const int64_t nb = cs->n_blocks;
    HIPCHK(ensure_buf((void **)&cs->tspan, &cs->cap_tspan, (size_t)nb + 8, sizeof(int2)));
    HIPCHK(ensure_buf((void **)&cs->bucket, &cs->cap_idx, (size_t)std::max<int64_t>(cs->idx_n, 1), 4));
    const int32_t *d_bt = cs->d_stage;
    HIPCHK(launch_build_index(d_bt, d_bt + nb, d_bt + 2 * nb, nb, cs->chains, cs->n_chains,
                              cs->d_coff, cs->d_tile_c0, cs->tspan, cs->bucket, s));
    cs->idx_ready = true;
    return GAC_OK;
}

// The part of ScoreArgs that does not depend on the chain set, the batch or
// the workspace: the genomes, the local flag and the context's scoring setup.
static void base_args(const gac_ctx *c, uint32_t flags, ScoreArgs &a) {
    memset(&a, 0, sizeof(a));
    const Genome &T = c->g[0], &Q = c->g[1];
    a.t_planes = T.planes;
    a.t_nmask = T.nmask;
    a.t_woff = T.d_woff;
    a.q_planes = Q.planes;
    a.q_nmask = Q.nmask;
    a.q_woff = Q.d_woff;
    a.want_local = (flags & GAC_WANT_LOCAL) ? 1 : 0;
    a.gap_len = c->gap_len;
    a.gap_tab = c->d_gap_tab;
    a.small_tab = c->d_small;
    memcpy(a.coef, c->coef, sizeof(a.coef));
    a.sym = c->sym;
    a.gap = c->gap;
}

// One call = k_plan, the tile map (k_tilemap_fused, or k_scan_agg + k_tilemap
// above 1 M ranges), k_tile and the cross-tile fold (k_fold_tiles +
// k_fold_super); the host waits only for the status words (pinned memory),
// not for the scoring itself.  The flat block count W is only known on the
// device (ranges may overlap), so the kernels check the workspace capacity
// themselves; on overflow k_tile and the folds do nothing and the call grows the
// workspace to the reported {W, T} and runs once more (first call or a larger
// batch only).
// Checks shared by both scoring paths, the per-setup block gaps, and the
// kernel arguments that do not depend on the workspace.
static int prepare_args(gac_ctx *c, const gac_chainset *cs, int64_t n, uint32_t flags,
                        const void *d_l, hipStream_t s, ScoreArgs &a) {
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_set_scoring() not called");
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "chainset does not belong to this context");
    if (n < 0 || n > INT32_MAX / 2) return gac_fail(GAC_E_ARG, "bad range count %lld", (long long)n);
    if ((flags & GAC_WANT_LOCAL) && !d_l) return gac_fail(GAC_E_ARG, "GAC_WANT_LOCAL needs local output");
    if (n == 0) return GAC_OK;
    if (cs->gap_version != c->gap_version) {  // blk[].w for this scoring setup
        HIPCHK(launch_block_gaps_flat(cs->d_coff, cs->d_tile_c0, cs->n_blocks, cs->blk, cs->blk12,
                                      upload_gaps(c, cs->blk12), s));
        const_cast<gac_chainset *>(cs)->gap_version = c->gap_version;
    }
    base_args(c, flags, a);
    a.chains = cs->chains;
    a.n_chains = cs->n_chains;
    a.blk = cs->blk;
    static const bool blk16 = [] {
        const char *e = getenv("GAC_TILE_BLK16");
        return e && e[0] == '1';
    }();
    a.blk12 = blk16 ? nullptr : cs->blk12;
    a.tspan = cs->tspan;
    a.bucket = cs->bucket;
    a.n = n;
    static const int scan64 = [] {
        const char *e = getenv("GAC_TILE_SCAN64");
        return e && e[0] == '1' ? 1 : 0;
    }();
    a.scan64 = scan64;
    static const int xcd_chunk = [] {
        const char *e = getenv("GAC_TILE_XCD");
        return e && e[0] == '1' ? 1 : 0;
    }();
    a.xcd_chunk = xcd_chunk;
    return GAC_OK;
}

static int score_device_split(gac_ctx *c, const ScoreArgs &a_base, const Range *d_ranges,
                              const Window *d_wins, int64_t n, long long *d_g, long long *d_l,
                              int32_t *d_ali, hipStream_t s);

// ------------------------------------------------ the small-batch server ----
// k_small_server (gac_kernels.hip) keeps a grid resident between the calls of
// a run of small batches (chainCleaner's replay loop), so a call costs a
// mailbox round trip instead of a launch and a stream synchronisation.  Only
// the small-batch entry points keep it running; every other entry point parks
// it first (CTX_LOCK), and the grid exits by itself after `idle` without a
// request.  On by default (GAC_SMALL_SERVER=0: a k_small launch per batch):
// 16.5 vs 23.6 us per 20-range call of an uploaded set, 23.4 vs 30.6 for
// host-held chains, chainCleaner's C3 loop 0.19 vs 0.27 s in its 10 k calls
// (r05lat6).
// (bounded: a grid that has not drained kParkSecs after its stop -- wedged,
// or never scheduled -- is left behind, the server marked unusable, and the
// caller gets an error instead of an unbounded hipStreamSynchronize)
constexpr double kParkSecs = 10.0;

void gac::srv_park(gac_ctx *c) {
    SmallServer &v = c->srv;
    if (!v.running) return;
    __atomic_store_n(&v.mail->stop, 1u, __ATOMIC_RELEASE);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t it = 1;; ++it) {
        const hipError_t q = hipStreamQuery(v.st);
        if (q != hipErrorNotReady) break;  // drained (or failed: reported by the next call)
        if ((it & 1023) == 0) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > kParkSecs) {
                v.wedged = true;
                v.on = false;
                v.running = false;
                return;  // (stop stays set: the grid exits whenever it runs)
            }
        }
        __builtin_ia32_pause();
    }
    __atomic_store_n(&v.mail->stop, 0u, __ATOMIC_RELEASE);
    v.running = false;
}

void gac::srv_free(gac_ctx *c) {
    SmallServer &v = c->srv;
    if (v.wedged) return;  // (a grid may still read these: left allocated)
    void *h[] = {v.mail, v.h_in, v.h_hq, v.h_pool, v.h_out};
    for (void *p : h)
        if (p) hipHostFree(p);
    if (v.d_sync) hipFree(v.d_sync);
    if (v.st) hipStreamDestroy(v.st);
    const bool on = v.on;
    const uint64_t idle = v.idle;
    const int wgs = v.wgs;
    v = SmallServer();
    v.on = on;
    v.idle = idle;
    v.wgs = wgs;
}

static int srv_alloc(gac_ctx *c) {
    SmallServer &v = c->srv;
    if (v.mail) return GAC_OK;
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent;
    // the inputs: coherent (uncached on the device) or, GAC_SRV_INPUT=nc,
    // cached and invalidated by each workgroup's acquire fence per request
    const char *iv = getenv("GAC_SRV_INPUT");
    const unsigned fin = iv && strcmp(iv, "nc") == 0 ? (unsigned)hipHostMallocMapped : fl;
    v.in_fl = fin;
    HIPCHK(hipStreamCreateWithFlags(&v.st, hipStreamNonBlocking));
    HIPCHK(hipHostMalloc((void **)&v.mail, sizeof(SmallMail), fl));
    memset(v.mail, 0, sizeof(SmallMail));
    HIPCHK(hipHostGetDevicePointer((void **)&v.d_mail, v.mail, 0));
    HIPCHK(hipHostMalloc((void **)&v.h_in, kSmallMax * sizeof(Range), fin));
    HIPCHK(hipHostGetDevicePointer((void **)&v.d_in, v.h_in, 0));
    HIPCHK(hipHostMalloc((void **)&v.h_hq, kSmallMax * sizeof(RangeDesc), fin));
    HIPCHK(hipHostGetDevicePointer((void **)&v.d_hq, v.h_hq, 0));
    HIPCHK(hipHostMalloc((void **)&v.h_out, kSmallMax * sizeof(SmallOut), fl));
    HIPCHK(hipHostGetDevicePointer((void **)&v.d_out, v.h_out, 0));
    // uncached device memory: the broadcast word and the count are polled
    // by workgroups on every XCD, whose L2s are not coherent with each other
    HIPCHK(hipExtMallocWithFlags((void **)&v.d_sync, sizeof(SmallSync), hipDeviceMallocUncached));
    v.seq = 0;
    return GAC_OK;
}

// the pool of host-planned window records: grown (while parked) to `need`
static int srv_pool(gac_ctx *c, int64_t need) {
    SmallServer &v = c->srv;
    if (need <= v.pool_cap) return GAC_OK;
    srv_park(c);
    if (v.h_pool) hipHostFree(v.h_pool);
    v.h_pool = nullptr;
    v.pool_cap = 0;
    const int64_t cap = std::max<int64_t>(need + need / 2, 1 << 16);
    HIPCHK(hipHostMalloc((void **)&v.h_pool, cap * sizeof(int4), v.in_fl));
    HIPCHK(hipHostGetDevicePointer((void **)&v.d_pool, v.h_pool, 0));
    v.pool_cap = cap;
    return GAC_OK;
}

static int srv_launch(gac_ctx *c) {
    SmallServer &v = c->srv;
    HIPCHK(hipMemsetAsync(v.d_sync, 0, sizeof(SmallSync), v.st));
    __atomic_store_n(&v.mail->state, 1u, __ATOMIC_RELEASE);
    __atomic_store_n(&v.mail->done, v.seq, __ATOMIC_RELEASE);
    static const uint32_t trace = getenv("GAC_SRV_TRACE") ? 1u : 0u;
    HIPCHK(launch_small_server(v.a0, v.a1, v.d_in, v.d_hq, v.d_pool, v.d_out, v.d_mail, v.d_sync,
                               v.seq, v.idle, trace, v.wgs, v.st));
    v.running = true;
    ++v.launches;
    return GAC_OK;
}

// a resident grid for requests of this kind: kind 0 scores ranges of `cs`
// (prepared like the k_small path: gaps, window index), kind 1 host-planned
// descriptors (any grid with the same local flag takes them)
static int srv_ensure(gac_ctx *c, const gac_chainset *cs, uint32_t flags) {
    SmallServer &v = c->srv;
    if (v.wedged) return gac_fail(GAC_E_HIP, "small-batch server disabled: an earlier grid did not exit");
    const int local = (flags & GAC_WANT_LOCAL) ? 1 : 0;
    if (v.running && v.local == local && v.gap_version == c->gap_version && (!cs || v.cs == cs))
        return GAC_OK;
    srv_park(c);
    int rc = srv_alloc(c);
    if (rc != GAC_OK) return rc;
    if (!cs) cs = v.cs;  // (a freed set is cleared from v.cs by gac_chains_free)
    ScoreArgs a1;
    base_args(c, flags, a1);
    ScoreArgs a0 = a1;
    if (cs) {
        long long dummy = 0;
        if ((rc = prepare_args(c, cs, 1, flags, &dummy, c->stream, a0)) != GAC_OK) return rc;
        if ((rc = ensure_index(c, cs, c->stream)) != GAC_OK) return rc;
        a0.tspan = cs->tspan;  // (allocated with the index)
        a0.bucket = cs->bucket;
        HIPCHK(hipStreamSynchronize(c->stream));  // (the gaps and the index, before the grid)
    }
    if ((rc = srv_pool(c, 1)) != GAC_OK) return rc;
    v.a0 = a0;
    v.a1 = a1;
    v.cs = cs;
    v.local = local;
    v.gap_version = c->gap_version;
    return srv_launch(c);
}

// one request: inputs already in the mailbox buffers; waits for the results
static int srv_call(gac_ctx *c, uint32_t kind, int64_t n) {
    SmallServer &v = c->srv;
    const uint32_t prev = v.seq;  // (the last request word; 20-bit numbers, never 0)
    uint32_t num = ((prev & 0xfffffu) + 1) & 0xfffffu;
    if (num == 0) num = 1;
    const uint32_t seq = srv_word(num, kind, (uint32_t)n);
    v.seq = seq;
    __atomic_store_n(&v.mail->req, seq, __ATOMIC_RELEASE);
    ++v.requests;
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t it = 1;; ++it) {
        if (__atomic_load_n(&v.mail->done, __ATOMIC_ACQUIRE) == seq) return GAC_OK;
        if (__atomic_load_n(&v.mail->state, __ATOMIC_ACQUIRE) == 2u) {
            // the grid left (idle) before it saw this request: once it has
            // drained, a new one takes the request from the mailbox
            HIPCHK(hipStreamSynchronize(v.st));
            v.running = false;
            if (__atomic_load_n(&v.mail->done, __ATOMIC_ACQUIRE) == seq) return GAC_OK;
            v.seq = prev;
            const int rc = srv_launch(c);
            v.seq = seq;
            if (rc != GAC_OK) return rc;
            continue;
        }
        if ((it & 4095) == 0) {
            struct timespec t1;
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 10.0) {
                srv_park(c);  // (bounded)
                return gac_fail(GAC_E_HIP, "small-batch server: no answer to request %u in 10 s%s",
                                seq, v.wedged ? " (grid did not exit; server disabled)" : "");
            }
            const hipError_t q = hipStreamQuery(v.st);
            if (q != hipSuccess && q != hipErrorNotReady)
                return gac_fail(GAC_E_HIP, "small-batch server failed: %s", hipGetErrorString(q));
        }
        __builtin_ia32_pause();
    }
}

// the results of a small batch, from the pinned records the kernel wrote
// (the server's h_out, or h_small_out of a k_small launch)
static void unpack_small(const SmallOut *out, int64_t n, uint32_t flags, int64_t *global,
                         int64_t *local, int32_t *ali) {
    for (int64_t i = 0; i < n; ++i) {
        const SmallOut o = out[i];
        global[i] = o.g;
        ali[i] = o.ali;
        if (flags & GAC_WANT_LOCAL) local[i] = o.l;
    }
}

// d_wins non-null: the ranges come with their windows (gac_score_windows*),
// d_ranges is ignored
static int score_device(gac_ctx *c, const gac_chainset *cs, const Range *d_ranges,
                        const Window *d_wins, int64_t n, uint32_t flags, long long *d_g,
                        long long *d_l, int32_t *d_ali, hipStream_t s) {
    ScoreArgs a_base;
    if (c->ws_last && c->ws_last != s) HIPCHK(hipStreamWaitEvent(s, c->ws_ev, 0));
    int rc = prepare_args(c, cs, n, flags, d_l, s, a_base);
    if (rc != GAC_OK || n == 0) return rc;
    if (!d_wins && (rc = ensure_index(c, cs, s)) != GAC_OK) return rc;
    a_base.tspan = cs->tspan;  // (allocated with the index)
    a_base.bucket = cs->bucket;
    rc = score_device_split(c, a_base, d_ranges, d_wins, n, d_g, d_l, d_ali, s);
    if (hipEventRecord(c->ws_ev, s) == hipSuccess) c->ws_last = s;
    return rc;
}

// One batch through the pipeline; a batch whose window blocks overflow int32
// (kernels index flat blocks with 32 bits) is split in halves, recursively.
static int score_device_split(gac_ctx *c, const ScoreArgs &a_base, const Range *d_ranges,
                              const Window *d_wins, int64_t n, long long *d_g, long long *d_l,
                              int32_t *d_ali, hipStream_t s) {
    int rc;
    // first guess for an empty workspace: 8 window blocks per range
    const int64_t guess = c->ws_tiles ? 0 : 8 * n;
    rc = ensure_ws(c, n, guess / kTileBlocks + 1, s);
    if (rc != GAC_OK) return rc;
    ScoreArgs a = a_base;
    a.ranges = d_wins ? nullptr : d_ranges;
    a.wins = d_wins;
    a.out_g = d_g;
    a.out_l = d_l;
    a.out_ali = d_ali;
    for (int pass = 0; pass < 2; ++pass) {
        a.rdesc = c->rdesc;
        a.nblk = c->nblk;
        a.goff = c->goff;
        a.pb0 = c->pb0;
        a.agg = c->agg;
        a.plan_off = c->plan_off;
        a.lbflag = c->lbflag;
        a.gflat = c->gflat;
        a.status = c->status;
        a.tile_r0 = c->tile_r0;
        a.sum_head = c->sum_head;
        a.sum_tail = c->sum_tail;
        a.sup_head = c->sup_head;
        a.sup_tail = c->sup_tail;
        a.sup_tail_r = c->sup_tail_r;
        a.host_status = c->d_h_stat;
        a.call_tag = ++c->call_seq;
        if (a.call_tag <= 0) a.call_tag = c->call_seq = 1;
        a.cap_tiles = (int32_t)(c->ws_tiles < INT32_MAX ? c->ws_tiles : INT32_MAX);
        {
            PROF_BEGIN(GAC_K_PLAN);
            if (plan_lb()) {
                HIPCHK(launch_plan_lb(a, s));
            } else {
                HIPCHK(launch_plan(a, s));
                HIPCHK(launch_tilemap(a, s));
            }
            PROF_END(GAC_K_PLAN);
        }
        {
            PROF_BEGIN(GAC_K_TILE);
            HIPCHK(launch_tile(a, c->tile_grid_sym[a.sym ? 1 : 0][a.want_local ? 1 : 0], s));
            PROF_END(GAC_K_TILE);
        }
        {
            PROF_BEGIN(GAC_K_COMBINE);
            HIPCHK(launch_combine(a, c->combine_grid, s));
            PROF_END(GAC_K_COMBINE);
        }
        // wait for k_scan_agg's status words only; the rest runs on
        int32_t st[4];
        rc = wait_status(c, s, a.call_tag, st);
        if (rc != GAC_OK) return rc;
        if (st[3]) {  // k_plan<true>: a window outside its chain (it selected nothing)
            HIPCHK(hipStreamSynchronize(s));
            return gac_fail(GAC_E_ARG, "a window's blocks lie outside its chain (or its chain "
                            "index is out of range)");
        }
        if (st[0] == INT32_MAX) {  // W >= 2^31: two halves
            HIPCHK(hipStreamSynchronize(s));
            if (n < 2) return gac_fail(GAC_E_ARG, "one range's window exceeds 2^31 blocks");
            const int64_t h = n / 2;
            ScoreArgs b = a_base;
            b.n = h;
            rc = score_device_split(c, b, d_ranges, d_wins, h, d_g, d_l, d_ali, s);
            if (rc != GAC_OK) return rc;
            b.n = n - h;
            return score_device_split(c, b, d_wins ? nullptr : d_ranges + h,
                                      d_wins ? d_wins + h : nullptr, n - h, d_g + h,
                                      d_l ? d_l + h : nullptr, d_ali + h, s);
        }
        if (!st[2]) return GAC_OK;
        rc = ensure_ws(c, n, st[1], s);  // (synchronises before growing)
        if (rc != GAC_OK) return rc;
    }
    return gac_fail(GAC_E_STATE, "scoring workspace still too small after growing it");
}

// ----------------------------------------------------------------- whole chains
// scoreChain's batch: every chain of the set, in order (kent chainCalcScore +
// chainCalcScoreLocal per chain).  The plan is the chain set's own, built
// once; a call is the empty-chain zeroing (if any), k_tile and the fold.
static int ensure_whole(gac_ctx *c, gac_chainset *cs, hipStream_t s) {
    if (cs->w_ready) return GAC_OK;
    const int64_t n = cs->n_chains, nb = cs->n_blocks;
    const int64_t T = (nb + kTileBlocks - 1) / kTileBlocks;
    HIPCHK(hipMalloc(&cs->w_rdesc, std::max<int64_t>(n, 1) * sizeof(RangeDesc)));
    HIPCHK(hipMalloc(&cs->w_nblk, std::max<int64_t>(n, 1) * 4));
    HIPCHK(hipMalloc(&cs->w_gflat, std::max<int64_t>(n, 1) * 4));
    HIPCHK(hipMalloc(&cs->w_tile_r0, std::max<int64_t>(T, 1) * 4));
    HIPCHK(hipMalloc(&cs->w_status, kStatusBytes));
    const int32_t st[8] = {(int32_t)nb, (int32_t)T, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(cs->w_status, st, sizeof(st), hipMemcpyHostToDevice, s));
    // set order by default; GAC_WHOLE_ORDER=target plans the chains in
    // target order (r03k/r03m, C5: k_tile 2.29 vs 2.34 ms, but the scatter
    // back to chain order cost 0.13 ms; r03zb, results stored straight to
    // the chain: k_tile 2.34 vs 2.19 ms in set order, so set order stays)
    const char *ord = getenv("GAC_WHOLE_ORDER");
    const bool sorted = ord && !strcmp(ord, "target");
    if (sorted) {
        HIPCHK(hipMalloc(&cs->w_pb0, n * 4));
        HIPCHK(hipMalloc(&cs->w_perm, n * 4));
        unsigned long long *keys = nullptr;
        int32_t *vals = nullptr, *perm = nullptr, *inv = nullptr;
        void *tmp = nullptr;
        size_t tmp_bytes = 0;
        int rc = GAC_OK;
        hipError_t e = launch_whole_plan_sorted(cs->chains, n, nullptr, nullptr, nullptr, nullptr,
                                                cs->w_nblk, cs->w_gflat, nullptr, nullptr, nullptr,
                                                nullptr, tmp_bytes, s);
        if (e == hipSuccess) e = hipMalloc(&keys, 2 * n * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc(&vals, 3 * n * 4);
        perm = vals ? vals + n : nullptr;
        inv = vals ? vals + 2 * n : nullptr;
        if (e == hipSuccess) e = hipMalloc(&tmp, std::max<size_t>(tmp_bytes, 16));
        if (e == hipSuccess)
            e = launch_whole_plan_sorted(cs->chains, n, perm, keys, vals, cs->w_rdesc, cs->w_nblk,
                                         cs->w_gflat, cs->w_pb0, cs->w_tile_r0, inv, tmp,
                                         tmp_bytes, s);
        if (e == hipSuccess) e = hipMemcpyAsync(cs->w_perm, perm, n * 4, hipMemcpyDeviceToDevice, s);
        std::vector<int32_t> hinv(n);
        if (e == hipSuccess) e = hipMemcpyAsync(hinv.data(), inv, n * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        std::vector<int32_t> empty;  // chains without blocks (inv -1): zeroed by every call
        for (int64_t i = 0; e == hipSuccess && i < n; ++i)
            if (hinv[i] < 0) empty.push_back((int32_t)i);
        cs->w_nempty = (int64_t)empty.size();
        if (e == hipSuccess && !empty.empty()) {
            e = hipMalloc(&cs->w_empty, empty.size() * 4);
            if (e == hipSuccess)
                e = hipMemcpy(cs->w_empty, empty.data(), empty.size() * 4, hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) rc = gac_fail(GAC_E_HIP, "whole-chain plan: %s", hipGetErrorString(e));
        if (keys) hipFree(keys);
        if (vals) hipFree(vals);
        if (tmp) hipFree(tmp);
        if (rc != GAC_OK) return rc;
        cs->w_sorted = true;
        cs->w_ready = true;
        return GAC_OK;
    }
    HIPCHK(launch_whole_plan(cs->chains, n, cs->w_rdesc, cs->w_nblk, cs->w_gflat, cs->w_tile_r0, s));
    // k_tile's schedule: the tiles in the target order of their first
    // blocks (GAC_WHOLE_TILES=set: tile order), so that the tiles an XCD
    // scores at once share target plane lines in its L2 (chains are in score
    // order, so neighbouring tiles of the set are far apart on the target)
    static const bool tiles_set = [] {
        const char *e = getenv("GAC_WHOLE_TILES");
        return e && !strcmp(e, "set");
    }();
    if (!tiles_set && T > 1) {
        unsigned long long *keys = nullptr;
        int32_t *vals = nullptr;
        void *tmp = nullptr;
        size_t tmp_bytes = 0;
        hipError_t e = launch_tile_order(cs->chains, cs->blk, cs->w_tile_r0, T, nullptr, nullptr,
                                         nullptr, nullptr, tmp_bytes, s);
        if (e == hipSuccess) e = hipMalloc(&keys, 2 * T * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc(&vals, T * 4);
        if (e == hipSuccess) e = hipMalloc(&cs->w_tile_perm, T * 4);
        if (e == hipSuccess) e = hipMalloc(&tmp, std::max<size_t>(tmp_bytes, 16));
        if (e == hipSuccess)
            e = launch_tile_order(cs->chains, cs->blk, cs->w_tile_r0, T, keys, vals,
                                  cs->w_tile_perm, tmp, tmp_bytes, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (keys) hipFree(keys);
        if (vals) hipFree(vals);
        if (tmp) hipFree(tmp);
        if (e != hipSuccess) return gac_fail(GAC_E_HIP, "whole-chain tile order: %s", hipGetErrorString(e));
    }
    // chains without blocks: their results are zeroed by every call
    std::vector<int32_t> nblk(n);
    HIPCHK(hipMemcpyAsync(nblk.data(), cs->w_nblk, n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<int32_t> empty;
    for (int64_t i = 0; i < n; ++i)
        if (nblk[i] == 0) empty.push_back((int32_t)i);
    cs->w_nempty = (int64_t)empty.size();
    if (!empty.empty()) {
        HIPCHK(hipMalloc(&cs->w_empty, empty.size() * 4));
        HIPCHK(hipMemcpy(cs->w_empty, empty.data(), empty.size() * 4, hipMemcpyHostToDevice));
    }
    cs->w_ready = true;
    return GAC_OK;
}

static int score_whole(gac_ctx *c, const gac_chainset *cs_in, uint32_t flags, long long *d_g,
                       long long *d_l, int32_t *d_ali, hipStream_t s) {
    gac_chainset *cs = const_cast<gac_chainset *>(cs_in);
    ScoreArgs a;
    if (c->ws_last && c->ws_last != s) HIPCHK(hipStreamWaitEvent(s, c->ws_ev, 0));
    int rc = prepare_args(c, cs, cs ? cs->n_chains : 0, flags, d_l, s, a);
    if (rc != GAC_OK || cs->n_chains == 0) return rc;
    if (cs->n_chains > INT32_MAX / 2) return gac_fail(GAC_E_ARG, "too many chains");
    rc = ensure_whole(c, cs, s);
    if (rc != GAC_OK) return rc;
    const int64_t T = (cs->n_blocks + kTileBlocks - 1) / kTileBlocks;
    rc = ensure_ws(c, 0, T, s);
    if (rc != GAC_OK) return rc;
    a.ranges = nullptr;
    a.out_g = d_g;
    a.out_l = d_l;
    a.out_ali = d_ali;
    a.rdesc = cs->w_rdesc;
    a.nblk = cs->w_nblk;
    a.gflat = cs->w_gflat;
    a.pb0 = cs->w_sorted ? cs->w_pb0 : cs->w_gflat;
    a.out_perm = cs->w_sorted ? cs->w_perm : nullptr;
    a.tile_perm = cs->w_sorted ? nullptr : cs->w_tile_perm;
    a.tile_r0 = cs->w_tile_r0;
    a.status = cs->w_status;
    a.sum_head = c->sum_head;
    a.sum_tail = c->sum_tail;
    a.sup_head = c->sup_head;
    a.sup_tail = c->sup_tail;
    a.sup_tail_r = c->sup_tail_r;
    a.cap_tiles = (int32_t)(c->ws_tiles < INT32_MAX ? c->ws_tiles : INT32_MAX);
    HIPCHK(launch_zero_list(cs->w_empty, cs->w_nempty, d_g, a.want_local ? d_l : nullptr, d_ali, s));
    {
        PROF_BEGIN(GAC_K_TILE);
        HIPCHK(launch_tile(a, c->tile_grid_sym[a.sym ? 1 : 0][a.want_local ? 1 : 0], s));
        PROF_END(GAC_K_TILE);
    }
    {
        PROF_BEGIN(GAC_K_COMBINE);
        HIPCHK(launch_combine(a, c->combine_grid, s));
        PROF_END(GAC_K_COMBINE);
    }
    if (hipEventRecord(c->ws_ev, s) == hipSuccess) c->ws_last = s;
    return GAC_OK;
}

// ------------------------------------------------- host-API staging ----
// The staging buffers of the host entry points hold `need` records of
// sizeof(Range) in (ranges, or windows counted in Range units) and as many
// results out; grown with headroom, the contents are not kept.  A failed
// allocation leaves none of them -- io_n == 0 and all four pointers null --
// so that a later, smaller call allocates again instead of passing the test.
static int ensure_io(gac_ctx *c, int64_t need) {
    if (need <= c->io_n) return GAC_OK;
    const int64_t cap = need + need / 2 + 1024;
    auto release = [c] {
        void *bufs[] = {c->d_ranges, c->d_g, c->d_l, c->d_ali};
        for (void *p : bufs)
            if (p) hipFree(p);
        c->d_ranges = nullptr;
        c->d_g = c->d_l = nullptr;
        c->d_ali = nullptr;
        c->io_n = 0;
    };
    auto alloc = [c, cap]() -> int {
        HIPCHK(hipMalloc(&c->d_ranges, cap * sizeof(Range)));
        HIPCHK(hipMalloc(&c->d_g, cap * 8));
        HIPCHK(hipMalloc(&c->d_l, cap * 8));
        HIPCHK(hipMalloc(&c->d_ali, cap * 4));
        c->io_n = cap;
        return GAC_OK;
    };
    release();
    const int rc = alloc();
    if (rc != GAC_OK) release();
    return rc;
}

// the staged results of n records back to the caller, and the wait for them
static int read_io(gac_ctx *c, int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                   int32_t *ali, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(global, c->d_g, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ali, c->d_ali, n * 4, hipMemcpyDeviceToHost, s));
    if (flags & GAC_WANT_LOCAL)
        HIPCHK(hipMemcpyAsync(local, c->d_l, n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return GAC_OK;
}

extern "C" int gac_score_chains_device(gac_ctx *c, const gac_chainset *cs, uint32_t flags,
                                       int64_t *d_g, int64_t *d_l, int32_t *d_ali, void *stream) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    if (!cs) return gac_fail(GAC_E_ARG, "NULL chainset");
    if (cs->n_chains > 0 && (!d_g || !d_ali)) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return score_whole(c, cs, flags, (long long *)d_g, (long long *)d_l, d_ali, s);
}

extern "C" int gac_score_chains(gac_ctx *c, const gac_chainset *cs, uint32_t flags, int64_t *global,
                                int64_t *local, int32_t *ali) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    if (!cs) return gac_fail(GAC_E_ARG, "NULL chainset");
    const int64_t n = cs->n_chains;
    if (n == 0) return GAC_OK;
    if (!global || !ali || ((flags & GAC_WANT_LOCAL) && !local)) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_io(c, n);
    if (rc != GAC_OK) return rc;
    hipStream_t s = c->stream;
    rc = score_whole(c, cs, flags, c->d_g, c->d_l, c->d_ali, s);
    if (rc != GAC_OK) return rc;
    return read_io(c, n, flags, global, local, ali, s);
}

extern "C" int gac_score_ranges_device(gac_ctx *c, const gac_chainset *cs, const gac_range *d_ranges,
                                       int64_t n, uint32_t flags, int64_t *d_g, int64_t *d_l,
                                       int32_t *d_ali, void *stream) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    if (n > 0 && (!d_ranges || !d_g || !d_ali)) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return score_device(c, cs, (const Range *)d_ranges, nullptr, n, flags, (long long *)d_g,
                        (long long *)d_l, d_ali, s);
}

extern "C" int gac_score_windows_device(gac_ctx *c, const gac_chainset *cs,
                                        const gac_window *d_wins, int64_t n, uint32_t flags,
                                        int64_t *d_g, int64_t *d_l, int32_t *d_ali, void *stream) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    if (n > 0 && (!d_wins || !d_g || !d_ali)) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    return score_device(c, cs, nullptr, (const Window *)d_wins, n, flags, (long long *)d_g,
                        (long long *)d_l, d_ali, s);
}

// ranges of chains given in host memory: planned here (window by binary
// search over the chain's block starts/ends), scored by k_small<HOST> reading
// the window records from pinned mapped memory, 256 ranges per launch
extern "C" int gac_score_ranges_host(gac_ctx *c, const gac_chainset_desc *d, const gac_range *r,
                                     int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                                     int32_t *ali) {
    gac_clear_error();
    if (!c || !d) return gac_fail(GAC_E_ARG, "gac_score_ranges_host: NULL argument");
    CTX_LOCK_SMALL(c);
    if (!c->srv.on) srv_park(c);
    if (n < 0) return gac_fail(GAC_E_ARG, "negative range count");
    if (n == 0) return GAC_OK;
    if (!r || !global || !ali || ((flags & GAC_WANT_LOCAL) && !local))
        return gac_fail(GAC_E_ARG, "NULL buffer");
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_set_scoring() not called");
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before scoring");
    if (d->n_chains < 0 || d->n_blocks < 0 || !d->blk_off || !d->t_seq || !d->q_seq ||
        !d->q_strand || (d->n_blocks && (!d->blk_t || !d->blk_q || !d->blk_size)))
        return gac_fail(GAC_E_ARG, "gac_score_ranges_host: incomplete chain set descriptor");
    if (d->blk_off[0] != 0 || d->blk_off[d->n_chains] != d->n_blocks)
        return gac_fail(GAC_E_ARG, "gac_score_ranges_host: blk_off must run from 0 to n_blocks");
    HIPCHK(hipSetDevice(c->device));
    const bool srv = c->srv.on;  // the resident grid takes the batches
    if (srv) {
        const int rc = srv_ensure(c, nullptr, flags);
        if (rc != GAC_OK) return rc;
    } else if (!c->h_hq) {
        HIPCHK(hipHostMalloc((void **)&c->h_hq, kSmallMax * sizeof(RangeDesc), hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer((void **)&c->d_hq, c->h_hq, 0));
    }
    const Genome &T = c->g[0], &Q = c->g[1];
    ScoreArgs a;
    base_args(c, flags, a);
    hipStream_t s = c->stream;
    for (int64_t i0 = 0; i0 < n; i0 += kSmallMax) {
        const int64_t m = std::min<int64_t>(kSmallMax, n - i0);
        // windows (and their checks) first, to size the pool
        int64_t lo[kSmallMax], hi[kSmallMax], tot = 0;
        for (int64_t k = 0; k < m; ++k) {
            const gac_range &q = r[i0 + k];
            if (q.chain < 0 || q.chain >= d->n_chains)
                return gac_fail(GAC_E_ARG, "range %lld: chain %d out of range",
                                (long long)(i0 + k), q.chain);
            const int64_t b0 = d->blk_off[q.chain], b1 = d->blk_off[q.chain + 1];
            if (b0 < 0 || b0 > b1 || b1 > d->n_blocks)
                return gac_fail(GAC_E_ARG, "range %lld: chain %d has blocks [%lld, %lld) outside "
                                "[0, %lld)", (long long)(i0 + k), q.chain, (long long)b0,
                                (long long)b1, (long long)d->n_blocks);
            int64_t a0 = b0, a1 = b1;  // first block ending past s
            while (a0 < a1) {
                const int64_t mid = (a0 + a1) >> 1;
                if ((int64_t)d->blk_t[mid] + d->blk_size[mid] > q.t_start) a1 = mid;
                else a0 = mid + 1;
            }
            int64_t e0 = a0, e1 = b1;  // first block starting at or past e
            while (e0 < e1) {
                const int64_t mid = (e0 + e1) >> 1;
                if (d->blk_t[mid] >= q.t_end) e1 = mid;
                else e0 = mid + 1;
            }
            lo[k] = a0;
            hi[k] = std::max(a0, e0);
            tot += hi[k] - lo[k];
        }
        if (srv) {
            if (tot > c->srv.pool_cap) {  // (parks the grid to grow the pool)
                int rc = srv_pool(c, tot);
                if (rc != GAC_OK || (rc = srv_ensure(c, nullptr, flags)) != GAC_OK) return rc;
            }
        } else if (tot > c->pool_cap) {
            if (c->h_pool) hipHostFree(c->h_pool);
            c->h_pool = nullptr;
            c->pool_cap = 0;
            const int64_t cap = tot + tot / 2 + 1024;
            HIPCHK(hipHostMalloc((void **)&c->h_pool, cap * sizeof(int4), hipHostMallocMapped));
            HIPCHK(hipHostGetDevicePointer((void **)&c->d_pool, c->h_pool, 0));
            c->pool_cap = cap;
        }
        RangeDesc *hq = srv ? c->srv.h_hq : c->h_hq;
        int4 *pool = srv ? c->srv.h_pool : c->h_pool;
        int64_t j = 0;
        for (int64_t k = 0; k < m; ++k) {
            const gac_range &q = r[i0 + k];
            const int32_t ts = d->t_seq[q.chain], qs = d->q_seq[q.chain];
            if (ts < 0 || ts >= (int32_t)T.sizes.size() || qs < 0 || qs >= (int32_t)Q.sizes.size())
                return gac_fail(GAC_E_ARG, "chain %d: sequence index out of range", q.chain);
            const int64_t tsize = T.sizes[ts], qsize = Q.sizes[qs];
            RangeDesc &h = hq[k];
            h.tbase = T.woff[ts] * 32;
            const int64_t qw = Q.woff[qs] * 32;
            h.qbase = d->q_strand[q.chain] ? ~(qw + qsize) : qw;
            h.b0 = (int32_t)j;
            h.nblk = (int32_t)(hi[k] - lo[k]);
            h.s = q.t_start;
            h.e = q.t_end;
            int64_t pt = 0, pq = 0;
            for (int64_t b = lo[k]; b < hi[k]; ++b, ++j) {
                const int64_t t = d->blk_t[b], qq = d->blk_q[b], z = d->blk_size[b];
                if (z < 0 || z >= (1 << 29) || t < 0 || qq < 0 || t + z > tsize || qq + z > qsize ||
                    (b > lo[k] && (t < pt || qq < pq)))
                    return gac_fail(GAC_E_FORMAT, "chain %d: block [t %lld q %lld size %lld] "
                                    "outside its sequences or not ascending", q.chain,
                                    (long long)t, (long long)qq, (long long)z);
                pt = t + z;
                pq = qq + z;
                pool[j] = make_int4((int)t, (int)qq, (int)z, 0);
            }
        }
        if (srv) {
            const int rc = srv_call(c, 1, m);
            if (rc != GAC_OK) return rc;
            unpack_small(c->srv.h_out, m, flags, global + i0, local ? local + i0 : nullptr, ali + i0);
            continue;
        }
        a.n = m;
        HIPCHK(launch_small_host(a, c->d_hq, c->d_pool, c->d_small_out, s));
        HIPCHK(hipStreamSynchronize(s));
        unpack_small(c->h_small_out, m, flags, global + i0, local ? local + i0 : nullptr, ali + i0);
    }
    return GAC_OK;
}

extern "C" int gac_score_ranges(gac_ctx *c, const gac_chainset *cs, const gac_range *ranges,
                                int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                                int32_t *ali) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK_SMALL(c);
    if (n < 0) return gac_fail(GAC_E_ARG, "negative range count");
    if (n == 0) return GAC_OK;
    if (!ranges || !global || !ali || ((flags & GAC_WANT_LOCAL) && !local))
        return gac_fail(GAC_E_ARG, "NULL buffer");
    if (!cs) return gac_fail(GAC_E_ARG, "NULL chainset");
    if (n > c->small_max || !c->srv.on) srv_park(c);
    for (int64_t i = 0; i < n; ++i)
        if (ranges[i].chain < 0 || ranges[i].chain >= cs->n_chains)
            return gac_fail(GAC_E_ARG, "range %lld: chain %d out of range", (long long)i,
                            ranges[i].chain);
    HIPCHK(hipSetDevice(c->device));
    if (n <= c->small_max && c->srv.on) {  // a request to the resident grid
        if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_set_scoring() not called");
        if (cs->ctx != c) return gac_fail(GAC_E_ARG, "chainset does not belong to this context");
        int rc = srv_ensure(c, cs, flags);
        if (rc != GAC_OK) return rc;
        memcpy(c->srv.h_in, ranges, (size_t)n * sizeof(Range));
        if ((rc = srv_call(c, 0, n)) != GAC_OK) return rc;
        unpack_small(c->srv.h_out, n, flags, global, local, ali);
        return GAC_OK;
    }
    if (n <= c->small_max) {
        // one launch; ranges in and results out through pinned host memory
        hipStream_t s = c->stream;
        ScoreArgs a;
        int rc = prepare_args(c, cs, n, flags, local, s, a);
        if (rc != GAC_OK) return rc;
        if ((rc = ensure_index(c, cs, s)) != GAC_OK) return rc;
        a.tspan = cs->tspan;  // (allocated with the index)
        a.bucket = cs->bucket;
        memcpy(c->h_small_in, ranges, (size_t)n * sizeof(Range));
        HIPCHK(launch_small(a, c->d_small_in, c->d_small_out, s));
        HIPCHK(hipStreamSynchronize(s));
        unpack_small(c->h_small_out, n, flags, global, local, ali);
        return GAC_OK;
    }
    int rc = ensure_io(c, n);
    if (rc != GAC_OK) return rc;
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->d_ranges, ranges, n * sizeof(Range), hipMemcpyHostToDevice, s));
    rc = score_device(c, cs, c->d_ranges, nullptr, n, flags, c->d_g, c->d_l, c->d_ali, s);
    if (rc != GAC_OK) return rc;
    return read_io(c, n, flags, global, local, ali, s);
}

extern "C" int gac_score_windows(gac_ctx *c, const gac_chainset *cs, const gac_window *wins,
                                 int64_t n, uint32_t flags, int64_t *global, int64_t *local,
                                 int32_t *ali) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    CTX_LOCK(c);
    if (n < 0) return gac_fail(GAC_E_ARG, "negative window count");
    if (n == 0) return GAC_OK;
    if (!wins || !global || !ali || ((flags & GAC_WANT_LOCAL) && !local))
        return gac_fail(GAC_E_ARG, "NULL buffer");
    if (!cs) return gac_fail(GAC_E_ARG, "NULL chainset");
    HIPCHK(hipSetDevice(c->device));
    // the window records in the range staging buffer (20 B each: sized by
    // the 12-B ranges' capacity + one half)
    const int64_t need = (n * (int64_t)sizeof(Window) + sizeof(Range) - 1) / sizeof(Range);
    int rc = ensure_io(c, need);
    if (rc != GAC_OK) return rc;
    hipStream_t s = c->stream;
    Window *d_w = reinterpret_cast<Window *>(c->d_ranges);
    HIPCHK(hipMemcpyAsync(d_w, wins, n * sizeof(Window), hipMemcpyHostToDevice, s));
    rc = score_device(c, cs, nullptr, d_w, n, flags, c->d_g, c->d_l, c->d_ali, s);
    if (rc != GAC_OK) return rc;
    return read_io(c, n, flags, global, local, ali, s);
}

// ----------------------------------------------------------------- text (kent API)
// Caller-owned char text scored on the device (the kent in-process API's
// chainScoreBlock / axtScoreUngapped / cBlockFindCrossover take raw text):
// the batch's text is packed into one buffer, uploaded, scored, read back.
static M25 text_matrix(const int32_t mat[16]) {
    M25 m;
    memset(&m, 0, sizeof(m));
    for (int q = 0; q < 4; ++q)
        for (int t = 0; t < 4; ++t) m.m[q * 5 + t] = mat[q * 4 + t];
    return m;
}

template <class J>
static int text_run(gac_ctx *c, const std::vector<uint8_t> &text, const std::vector<J> &jobs,
                    size_t out_bytes, void **d_text, J **d_jobs, void **d_out) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(d_text, std::max<size_t>(text.size(), 1)));
    HIPCHK(hipMalloc((void **)d_jobs, jobs.size() * sizeof(J)));
    HIPCHK(hipMalloc(d_out, out_bytes));
    HIPCHK(hipMemcpyAsync(*d_text, text.data(), text.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(*d_jobs, jobs.data(), jobs.size() * sizeof(J), hipMemcpyHostToDevice,
                          c->stream));
    return GAC_OK;
}

extern "C" int gac_score_text_blocks(gac_ctx *c, int64_t n, const char *const *q,
                                     const char *const *t, const int32_t *size,
                                     const int32_t mat[16], int64_t *score) {
    gac_clear_error();
    if (!c || n < 0 || (n && (!q || !t || !size || !mat || !score)))
        return gac_fail(GAC_E_ARG, "gac_score_text_blocks: bad argument");
    if (n == 0) return GAC_OK;
    CTX_LOCK(c);
    std::vector<TextJob> jobs(n);
    size_t tot = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (size[i] < 0) return gac_fail(GAC_E_ARG, "block %lld: negative size", (long long)i);
        tot += 2 * (size_t)size[i];
    }
    std::vector<uint8_t> text(tot);
    size_t o = 0;
    for (int64_t i = 0; i < n; ++i) {
        jobs[i] = TextJob{(int64_t)o, (int64_t)(o + size[i]), size[i], 0};
        memcpy(&text[o], q[i], size[i]);
        memcpy(&text[o + size[i]], t[i], size[i]);
        o += 2 * (size_t)size[i];
    }
    void *d_text = nullptr, *d_out = nullptr;
    TextJob *d_jobs = nullptr;
    int rc = text_run(c, text, jobs, n * 8, &d_text, &d_jobs, &d_out);
    if (rc == GAC_OK) {
        hipError_t e = launch_text_blocks((const uint8_t *)d_text, d_jobs, n, text_matrix(mat),
                                          (long long *)d_out, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(score, d_out, n * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = gac_fail(GAC_E_HIP, "gac_score_text_blocks: %s", hipGetErrorString(e));
    }
    hipStreamSynchronize(c->stream);
    hipFree(d_text);
    hipFree(d_jobs);
    hipFree(d_out);
    return rc;
}

extern "C" int gac_text_crossovers(gac_ctx *c, int64_t n, const char *const *lq,
                                   const char *const *lt, const char *const *rq,
                                   const char *const *rt, const int32_t *overlap,
                                   const int32_t mat[16], int32_t *pos, int32_t *adj) {
    gac_clear_error();
    if (!c || n < 0 || (n && (!lq || !lt || !rq || !rt || !overlap || !mat || !pos || !adj)))
        return gac_fail(GAC_E_ARG, "gac_text_crossovers: bad argument");
    if (n == 0) return GAC_OK;
    CTX_LOCK(c);
    std::vector<TextXJob> jobs(n);
    size_t tot = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (overlap[i] < 0) return gac_fail(GAC_E_ARG, "overlap %lld: negative", (long long)i);
        tot += 4 * (size_t)overlap[i];
    }
    std::vector<uint8_t> text(tot);
    size_t o = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t v = overlap[i];
        jobs[i] = TextXJob{(int64_t)o, (int64_t)(o + v), (int64_t)(o + 2 * (size_t)v),
                           (int64_t)(o + 3 * (size_t)v), v, 0};
        memcpy(&text[o], lq[i], v);
        memcpy(&text[o + v], lt[i], v);
        memcpy(&text[o + 2 * (size_t)v], rq[i], v);
        memcpy(&text[o + 3 * (size_t)v], rt[i], v);
        o += 4 * (size_t)v;
    }
    void *d_text = nullptr, *d_out = nullptr;
    TextXJob *d_jobs = nullptr;
    int rc = text_run(c, text, jobs, n * 8, &d_text, &d_jobs, &d_out);
    if (rc == GAC_OK) {
        int32_t *d_pos = (int32_t *)d_out, *d_adj = d_pos + n;
        hipError_t e = launch_text_xover((const uint8_t *)d_text, d_jobs, n, text_matrix(mat), d_pos,
                                         d_adj, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(pos, d_pos, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(adj, d_adj, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = gac_fail(GAC_E_HIP, "gac_text_crossovers: %s", hipGetErrorString(e));
    }
    hipStreamSynchronize(c->stream);
    hipFree(d_text);
    hipFree(d_jobs);
    hipFree(d_out);
    return rc;
}
