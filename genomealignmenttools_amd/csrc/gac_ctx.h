// gac_ctx.h -- what the units of the C-ABI implementation (gac_device.hip and
// gac_abi_*.hip, one per subject of include/gachain.h) share: the context, the chain set, and the
// few helpers that cross units.  Internal: never installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "gac_kernels.h"
#include "gachain.h"
#include "host/gac_host.h"

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return gac_fail(GAC_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                            __FILE__, __LINE__);                                            \
    } while (0)

namespace gac {

struct Genome {
    // host-side staging until finalize
    std::vector<std::string> names;
    std::vector<int32_t> sizes;
    std::unordered_map<std::string, int32_t> index;
    std::vector<uint8_t> raw;       // payloads copied by gac_genome_add_seq, 8-B aligned
    std::vector<int64_t> raw_off;   // per seq: offset into raw (-1: payload is ext[i])
    std::vector<const uint8_t *> ext;  // per seq: payload inside the mapped .2bit file
    gac_twobit tb{};                // mapping kept open for ext (gac_genome_load_2bit)
    bool tb_open = false;
    // sparse upload (gac_genome_load_twobit_runs): only these word runs of
    // registered sequence run_seq[k], [run_lo, run_hi) in 32-base words
    bool sparse = false;
    std::vector<int32_t> run_seq, run_lo, run_hi;
    std::vector<NPiece> npieces;    // bit0 relative to the seq start until finalize
    std::vector<int32_t> npiece_seq;
    // soft-mask plane (opt-in, gac_genome_want_softmask): the mask runs as
    // pieces like the N runs, and the plane itself (null: not asked for)
    bool want_mask = false;
    std::vector<NPiece> mpieces;
    std::vector<int32_t> mpiece_seq;
    uint32_t *lmask = nullptr;
    // host copy kept after finalize (raw stays): merged, sorted N runs per
    // sequence, CSR by nrun_off -- host-side base access (gac_genome_view)
    std::vector<int64_t> nrun_off{0};
    std::vector<int32_t> nrun_start, nrun_size;
    // device
    bool final = false;
    std::vector<int64_t> woff;      // host copy of word offsets
    int64_t n_words = 0;
    uint2 *planes = nullptr;
    uint32_t *nmask = nullptr;
    int64_t *d_woff = nullptr;
    longlong2 *d_nrun = nullptr;    // the N runs as global {start, end} bases, sorted
    int64_t n_nrun = 0;
    const uint8_t *packed(int i) const { return ext[i] ? ext[i] : raw.data() + raw_off[i]; }
};

struct Prof {
    int kernel;
    hipEvent_t a, b;
};

// the resident small-batch server of a context (default; GAC_SMALL_SERVER=0
// launches k_small per batch instead)
struct SmallServer {
    bool on = false;       // enabled for this context
    bool running = false;  // a grid is resident (or exiting: mail->state 2)
    hipStream_t st = nullptr;
    SmallMail *mail = nullptr, *d_mail = nullptr;  // pinned, coherent
    SmallSync *d_sync = nullptr;
    Range *h_in = nullptr, *d_in = nullptr;        // pinned, coherent [kSmallMax]
    RangeDesc *h_hq = nullptr, *d_hq = nullptr;    // pinned, coherent [kSmallMax]
    int4 *h_pool = nullptr, *d_pool = nullptr;     // pinned, coherent, grown while parked
    int64_t pool_cap = 0;
    SmallOut *h_out = nullptr, *d_out = nullptr;   // pinned, coherent [kSmallMax]
    uint32_t seq = 0;                  // the last request made (= completed: calls wait)
    const gac_chainset *cs = nullptr;  // the set of kind-0 requests (nullptr: none)
    uint32_t gap_version = 0;
    int local = -1;
    ScoreArgs a0, a1;                  // the resident grid's arguments
    uint64_t idle = 2000000;           // exit after 20 ms without a request (100 MHz ticks)
    int64_t launches = 0, requests = 0;
    unsigned in_fl = 0;  // hipHostMalloc flags of the inputs
    int wgs = 16;        // workgroups of the grid (GAC_SRV_WGS, 1..kSrvWaves/4)
    bool wedged = false; // a grid did not exit within kParkSecs of its stop:
                         // the server is not used again (no unbounded wait)
};

}  // namespace gac

struct AxtWs;  // gac_abi_seqout.hip

struct gac_ctx {
    // every entry point that touches the context's state holds this (the
    // ABI is thread-safe per context; calls are serialised)
    std::recursive_mutex mu;
    // the scoring workspace is stream-ordered: ws_ev is recorded on the
    // stream of the last call that used it (ws_last); a call on another
    // stream waits for it on the device, and growing the workspace waits
    // for it on the host
    hipEvent_t ws_ev = nullptr;
    hipStream_t ws_last = nullptr;
    int device = 0;
    char arch[64] = {0};
    hipStream_t stream = nullptr;
    gac::Genome g[2];
    bool scoring = false;
    int32_t coef[16];  // multilinear basis (ScoreArgs::coef)
    uint32_t gap_version = 0;  // bumped by every gac_set_scoring
    int sym = 0;
    gac::GapDev gap;
    int32_t *d_small = nullptr;
    int32_t *d_gap_tab = nullptr;  // [3][gap_len]
    int gap_len = 0;
    // workspace
    int64_t ws_n = 0;
    gac::RangeDesc *rdesc = nullptr;
    int32_t *nblk = nullptr, *goff = nullptr;
    int32_t *pb0 = nullptr;                  // [ws_n]
    int32_t *agg = nullptr;                  // [plan workgroups]
    int32_t *plan_off = nullptr;             // [plan workgroups]
    unsigned long long *lbflag = nullptr;    // [plan workgroups] k_plan_lb's look-back words
    int32_t *gflat = nullptr;                // [ws_n]
    int32_t *status = nullptr;               // [8]
    int64_t ws_tiles = 0;
    int32_t *tile_r0 = nullptr;              // [ws_tiles]
    gac::SegSum *sum_head = nullptr, *sum_tail = nullptr;
    gac::SegSum *sup_head = nullptr, *sup_tail = nullptr;  // [ws_tiles / 64 + 2]
    int32_t *sup_tail_r = nullptr;
    // staging for the host API
    int64_t io_n = 0;
    gac::Range *d_ranges = nullptr;
    long long *d_g = nullptr, *d_l = nullptr;
    int32_t *d_ali = nullptr;
    gac::Range *h_small_in = nullptr;     // pinned, mapped: ranges of a small batch [kSmallMax]
    gac::SmallOut *h_small_out = nullptr; // pinned, mapped, coherent: its results
    gac::Range *d_small_in = nullptr;     // their device addresses
    gac::SmallOut *d_small_out = nullptr;
    int small_max = gac::kSmallMax;  // batches up to this size take k_small (GAC_SMALL_MAX)
    // gac_score_ranges_host: planned ranges and their window records, pinned
    // and mapped (the kernel reads them over the bus), grown on demand
    gac::RangeDesc *h_hq = nullptr, *d_hq = nullptr;  // [kSmallMax]
    int4 *h_pool = nullptr, *d_pool = nullptr;
    int64_t pool_cap = 0;
    int32_t mat[16] = {0};           // the current scoring setup (gac_set_scoring)
    gac_gapcalc *gap_src = nullptr;
    int32_t *h_stat = nullptr;   // pinned, coherent host words written by k_scan_agg [8]
    int32_t *d_h_stat = nullptr; // its device address
    int32_t call_seq = 0;
    // k_tile grids (resident workgroups) by [strand-symmetric matrix][local]
    int tile_grid_sym[2][2] = {{2048, 2048}, {2048, 2048}};
    int combine_grid = 512;
    // pinned staging for genome uploads (two buffers, alternating)
    uint8_t *pin[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    // profiling
    int prof = 0;  // mask of timed kernels
    std::vector<gac::Prof> prof_pending;
    std::vector<hipEvent_t> prof_free;
    double prof_ms[GAC_K_COUNT] = {0};
    int64_t prof_n[GAC_K_COUNT] = {0};
    // chain sets still open on this context: gac_close releases their
    // device memory and orphans them (ctx = NULL), so a set freed after its
    // context (a kent-shim cache, a garbage-collected binding) is only deleted
    std::vector<gac_chainset *> sets;
    gac::SmallServer srv;
    // gac_axt_measure / gac_axt_render: the host entry points' workspace and
    // the render jobs still open (orphaned by gac_close like the sets)
    AxtWs *axt = nullptr;
    std::vector<struct gac_axt_job *> axt_jobs;
};

struct gac_chainset {
    gac_ctx *ctx;
    int64_t n_chains;
    int64_t n_blocks;
    gac::DChain *chains = nullptr;
    int4 *blk = nullptr;  // {tStart, qStart, size | N flags, gap}, padded by one entry
    gac::Blk12 *blk12 = nullptr;  // compact copy for k_tile (written with the gaps)
    uint32_t gap_version = 0;  // scoring setup the blk[].w gaps were computed for
    int2 *tspan = nullptr;  // {tStart, tEnd}
    uint32_t *bucket = nullptr;  // per-chain bucket indexes
    // whole-chain plan (gac_score_chains; built at its first call): the
    // scoring workspace of the batch "range c = chain c", fixed per set
    bool w_ready = false;
    gac::RangeDesc *w_rdesc = nullptr;  // [n_chains]
    int32_t *w_nblk = nullptr;     // [n_chains]
    int32_t *w_gflat = nullptr;    // [n_chains] first block (= flat offset)
    int32_t *w_tile_r0 = nullptr;  // [tiles] chain owning each tile's first block
    int32_t *w_status = nullptr;   // {W, T, 0, 0}
    int32_t *w_empty = nullptr;    // chains without blocks (their results are 0)
    int64_t w_nempty = 0;
    // target-ordered plan (k_whole_keys): positions p are chains in target
    // order; w_pb0[p] their first blocks, results stored to chain w_perm[p]
    bool w_sorted = false;
    int32_t *w_pb0 = nullptr;
    int32_t *w_perm = nullptr;
    // set-order plan's tile schedule (k_tile's tile_perm): tiles in the
    // target order of their first blocks
    int32_t *w_tile_perm = nullptr;
    // capacities (gac_chains_reupload refills these buffers when they fit)
    size_t cap_chains = 0, cap_blocks = 0, cap_blk12 = 0, cap_tspan = 0, cap_idx = 0;
    int32_t *d_stage = nullptr;  // the caller's block arrays, staged (3 x blocks)
    size_t cap_stage = 0;
    // flat (lane per block) kernels: compact chain offsets [n + 1], the chain
    // of every 64-block tile's first block [tiles + 1], per-chain N-run
    // ranges {t first, t end, q first, q end} (empty: no run in its span)
    int32_t *d_coff = nullptr, *d_tile_c0 = nullptr;
    int4 *d_crun = nullptr;
    size_t cap_coff = 0, cap_tile_c0 = 0, cap_crun = 0;
    // the window-search index (tspan, bucket) is built: at upload
    // (GAC_UP_INDEX=eager) or at the first call that searches windows
    bool idx_ready = false;
    int64_t idx_n = 0;  // bucket entries of the index
};

namespace gac {

// ---- helpers that cross units, by the unit that defines them
// gac_abi_context.hip
double wall_s();
hipEvent_t prof_event(gac_ctx *c);
// gac_abi_genome.hip
void free_genome(Genome &g);
// pageable host array -> device through the context's pinned staging buffers
int upload_staged(gac_ctx *c, void *d_dst, const void *h_src, size_t bytes);
// gac_abi_chains.hip
hipError_t ensure_buf(void **p, size_t *cap, size_t want, size_t sz);
UploadGaps upload_gaps(const gac_ctx *c, Blk12 *blk12);
void free_set_memory(gac_chainset *cs);
// gac_device.hip
void srv_park(gac_ctx *c);
void srv_free(gac_ctx *c);
// gac_abi_seqout.hip
void axt_release(gac_ctx *c);

// 2bit code T=0 C=1 A=2 G=3 -> A,C,G,T index
inline int acgt_of_code(int code) {
    static const int m[4] = {3, 1, 0, 2};
    return m[code];
}

// ---- the batches of the alignment-text calls (gac_axt_filter, gac_axt_psl):
// consecutive entries -- two rows of len[i] bytes at t_off[i] and q_off[i] of
// the caller's text -- while the text they need stays under a byte budget.
constexpr int64_t kAxtDefaultBudget = 256ll << 20;  // bytes of text a batch
constexpr int64_t kAxtBatchEntries = 1ll << 21;     // entries a batch (64 MB of records)
constexpr int64_t kAxtJoinGap = 64;                 // spans this close are uploaded as one

// The text a batch needs: the span of its target rows and the span of its
// query rows (one span when they overlap or nearly touch, as the rows of an
// axt file do; two when a caller keeps the sides apart).
struct AxtSpans {
    int64_t tlo = 0, thi = 0, qlo = 0, qhi = 0;
    bool any = false;
    void add(int64_t t, int64_t q, int64_t L) {
        if (!any) {
            tlo = t, thi = t + L, qlo = q, qhi = q + L, any = true;
            return;
        }
        tlo = std::min(tlo, t), thi = std::max(thi, t + L);
        qlo = std::min(qlo, q), qhi = std::max(qhi, q + L);
    }
    bool joined() const { return tlo <= qhi + kAxtJoinGap && qlo <= thi + kAxtJoinGap; }
    int64_t bytes() const {
        return joined() ? std::max(thi, qhi) - std::min(tlo, qlo) : (thi - tlo) + (qhi - qlo);
    }
    // where the spans go in the batch's buffer: the rows of an entry at t and q
    // of the text are at t_base() + (t - tlo) and q_base() + (q - qlo)
    int64_t lo() const { return std::min(tlo, qlo); }
    int64_t t_base() const { return joined() ? tlo - lo() : 0; }
    int64_t q_base() const { return joined() ? qlo - lo() : thi - tlo; }
};

struct AxtBatch {
    int64_t first, end;  // entries [first, end) of the call (the skipped ones and those left
                         // to the host among them are not uploaded)
    int64_t n;           // entries uploaded
    AxtSpans sp;
};

struct AxtPlan {
    std::vector<AxtBatch> batches;
    std::vector<int64_t> host_idx;  // entries alone over the budget, ascending
    int64_t n_dev = 0, max_n = 0, max_bytes = 0;  // entries uploaded; the largest batch
};

// skip(i): entry i takes no part (it is neither uploaded nor left to the host)
template <class Skip>
inline void axt_plan_batches(int64_t n, const int64_t *t_off, const int64_t *q_off, const int32_t *len,
                             int64_t budget, Skip skip, AxtPlan &P) {
    AxtBatch b{0, 0, 0, AxtSpans()};
    auto close = [&](int64_t end) {
        b.end = end;
        if (b.n > 0) {
            P.batches.push_back(b);
            P.n_dev += b.n;
            P.max_n = std::max(P.max_n, b.n);
            P.max_bytes = std::max(P.max_bytes, b.sp.bytes());
        }
        b = AxtBatch{end, end, 0, AxtSpans()};
    };
    for (int64_t i = 0; i < n; ++i) {
        if (skip(i)) continue;
        const int64_t L = len[i];
        AxtSpans one;
        one.add(t_off[i], q_off[i], L);
        if (one.bytes() > budget) {
            P.host_idx.push_back(i);
            continue;
        }
        AxtSpans with = b.sp;
        with.add(t_off[i], q_off[i], L);
        if (b.n > 0 && (with.bytes() > budget || b.n >= kAxtBatchEntries)) {
            close(i);
            with = one;
        }
        b.sp = with;
        ++b.n;
    }
    close(n);
}

// the byte budget: the environment knob `env`, else a quarter of the free
// device memory, at most kAxtDefaultBudget
inline hipError_t axt_batch_budget(const char *env, int64_t *budget) {
    *budget = 0;
    if (const char *v = getenv(env)) *budget = atoll(v);
    if (*budget > 0) return hipSuccess;
    size_t free_b = 0, total_b = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess) return e;
    *budget = std::max<int64_t>(1, std::min<int64_t>((int64_t)(free_b / 4), kAxtDefaultBudget));
    return hipSuccess;
}

// a batch's text into its buffer, in one span or two
inline int axt_upload_spans(gac_ctx *c, char *d_text, const char *text, const AxtSpans &sp) {
    if (sp.joined()) return upload_staged(c, d_text, text + sp.lo(), (size_t)sp.bytes());
    int rc = upload_staged(c, d_text, text + sp.tlo, (size_t)(sp.thi - sp.tlo));
    if (rc == GAC_OK)
        rc = upload_staged(c, d_text + sp.q_base(), text + sp.qlo, (size_t)(sp.qhi - sp.qlo));
    return rc;
}

struct CtxLock {
    std::lock_guard<std::recursive_mutex> g;
    CtxLock(gac_ctx *c, bool park) : g(c->mu) {
        if (park) srv_park(c);
    }
};

}  // namespace gac

// held by every entry point that uses a context (see gac_ctx::mu); it also
// parks the small-batch server (k_small_server) first, so that nothing else
// runs beside a resident grid -- only the small-batch paths keep it
#define CTX_LOCK(c) gac::CtxLock ctx_lock_((c), true)
#define CTX_LOCK_SMALL(c) gac::CtxLock ctx_lock_((c), false)

// times the launches between them as kernel k (gac_prof_*); c and s are the
// caller's context and stream
#define PROF_BEGIN(k)                                   \
    hipEvent_t _pa = nullptr, _pb = nullptr;            \
    if (c->prof & (1 << (k))) {                         \
        _pa = gac::prof_event(c);                       \
        _pb = gac::prof_event(c);                       \
        hipEventRecord(_pa, s);                         \
    }
#define PROF_END(k)                                          \
    if (_pa) {                                               \
        hipEventRecord(_pb, s);                              \
        c->prof_pending.push_back(gac::Prof{(k), _pa, _pb}); \
    }
