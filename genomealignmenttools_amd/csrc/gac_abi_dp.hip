// gac_abi_dp.hip -- libgachain's C ABI, axtChain's device side: the kd-tree
// DP set-up and launches (gac_chain_dp*), gac_kd_trees, gac_crossovers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "gac_ctx.h"
#include "gac_dp.h"

using namespace gac;

// ----------------------------------------------------------------- chaining DP
// DpArgs common part: genomes, matrix by code, gap setup
static void dp_base_args(gac_ctx *c, DpArgs &a) {
    memset(&a, 0, sizeof(a));
    a.t_planes = c->g[0].planes;
    a.t_nmask = c->g[0].nmask;
    a.q_planes = c->g[1].planes;
    a.q_nmask = c->g[1].nmask;
    a.gap = c->gap;
    a.small_tab = c->d_small;
    a.gap_tab = c->d_gap_tab;
    a.gap_len = c->gap_len;
    for (int q = 0; q < 4; ++q)
        for (int t = 0; t < 4; ++t) a.m16[q * 4 + t] = c->mat[acgt_of_code(q) * 4 + acgt_of_code(t)];
}

// global base index of a pair's target start / query start ('-': ~(start + qSize))
static int pair_bases(gac_ctx *c, int32_t ts, int32_t qs, uint8_t minus, int64_t &tb,
                      int64_t &qb) {
    const Genome &T = c->g[0], &Q = c->g[1];
    if (ts < 0 || ts >= (int32_t)T.sizes.size() || qs < 0 || qs >= (int32_t)Q.sizes.size())
        return gac_fail(GAC_E_ARG, "bad sequence index (%d, %d)", ts, qs);
    tb = T.woff[ts] * 32;
    qb = minus ? ~(Q.woff[qs] * 32 + Q.sizes[qs]) : Q.woff[qs] * 32;
    return GAC_OK;
}

template <class T>
static int dev_upload(gac_ctx *c, T **d, const void *h, size_t n) {
    *d = nullptr;
    if (n == 0) return GAC_OK;
    HIPCHK(hipMalloc((void **)d, n * sizeof(T)));
    if (h) HIPCHK(hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return GAC_OK;
}

// the fast DP's waves per pair: k_dp_spec with 16 (GAC_DP_WAVES=4/8/16; 1:
// k_dp_fast, one wave per pair -- 7.2x slower on the C4-shaped set, r06spec7)
static int dp_waves() {
    static int waves = -1;
    if (waves < 0) {
        const char *wv = getenv("GAC_DP_WAVES");
        int w = wv && *wv ? atoi(wv) : 16;
        waves = (w == 4 || w == 8 || w == 16) ? w : 1;
    }
    return waves;
}

// k_dp_fast (fast) or k_dp over a.n_pairs pairs; GAC_DP_PROF: k_dp_fast's
// per-phase cycle counters, summed over pairs, to stderr
static hipError_t dp_launch(gac_ctx *c, DpArgs &a, int grid, bool fast) {
    unsigned long long *d_prof = nullptr;
    hipError_t e = hipSuccess;
    const char *dpprof = getenv("GAC_DP_PROF");
    if (fast && dpprof && *dpprof && *dpprof != '0' &&
        (e = hipMalloc(&d_prof, kDpProf * sizeof(unsigned long long))) == hipSuccess)
        e = hipMemsetAsync(d_prof, 0, kDpProf * sizeof(unsigned long long), c->stream);
    a.prof = d_prof;
    const double tk0 = wall_s();
    const int waves = dp_waves();
    // (k_dp_spec's watchdog flag: the caller's, or one of our own)
    int32_t *d_err_own = nullptr;
    if (e == hipSuccess && fast && waves > 1 && !a.err &&
        (e = hipMalloc(&d_err_own, sizeof(int32_t))) == hipSuccess &&
        (e = hipMemsetAsync(d_err_own, 0, sizeof(int32_t), c->stream)) == hipSuccess)
        a.err = d_err_own;
    if (e == hipSuccess)
        e = !fast ? launch_dp(a, grid, c->stream)
                  : (waves > 1 ? launch_dp_spec(a, grid, waves, c->stream) : launch_dp_fast(a, grid, c->stream));
    if (d_err_own) {
        int32_t h = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&h, d_err_own, sizeof(h), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && h) e = hipErrorLaunchTimeOut;  // (the in-order commit stalled)
        hipFree(d_err_own);
        a.err = nullptr;
    }
    if (d_prof && e == hipSuccess) {
        unsigned long long pv[kDpProf];
        e = hipMemcpyAsync(pv, d_prof, sizeof(pv), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) {
            const double secs = wall_s() - tk0, L = pv[kPfLeaves] ? (double)pv[kPfLeaves] : 1.0;
            fprintf(stderr,
                    "[gac_chain_dp] %s %.3f s, %llu pairs, %llu leaves, %llu fallbacks; per leaf: "
                    "%.2f windows, %.3f fallback windows, %.3f windows with an overlapping candidate, "
                    "%.2f overlap checks; cycles per leaf: load %.0f seed %.0f walk %.0f "
                    "(node loads + bounds %.0f) anomalies %.0f fallback %.0f commit %.0f; next windows: %.2f per leaf, "
                    "%.3f contiguous\n",
                    waves > 1 ? "k_dp_spec" : "k_dp_fast", secs, (unsigned long long)a.n_pairs,
                    pv[kPfLeaves], pv[kPfFallbacks],
                    pv[kPfWindows] / L, pv[kPfFbWindows] / L, pv[kPfXoverWin] / L, pv[kPfOvChecks] / L,
                    pv[kPfCycLoad] / L, pv[kPfCycSeed] / L, pv[kPfCycWalk] / L, pv[kPfCycXover] / L,
                    pv[kPfCycAnom] / L, pv[kPfCycFb] / L, pv[kPfCycCommit] / L, pv[kPfNextWin] / L,
                    pv[kPfNextWin] ? (double)pv[kPfNextSeq] / pv[kPfNextWin] : 0.0);
            if (waves > 1)
                fprintf(stderr, "[gac_chain_dp] k_dp_spec, %d waves per pair: per leaf %.0f cycles searching, "
                        "%.0f waiting for its turn, in order: %.0f the leaves since the snapshot, %.0f "
                        "anomalies, %.0f commit; then %.0f publishing; %.3f of the leaves "
                        "searched beside earlier ones\n", waves, pv[kPfCycWalk] / L, pv[kPfCycLoad] / L,
                        pv[kPfCycSeed] / L, pv[kPfCycAnom] / L, pv[kPfCycCommit] / L, pv[kPfCycFb] / L,
                        pv[kPfXoverWin] / L);
        }
        hipFree(d_prof);
        a.prof = nullptr;
    }
    return e;
}

extern "C" int gac_chain_dp(gac_ctx *c, int64_t n_pairs, const int32_t *t_seq, const int32_t *q_seq,
                            const uint8_t *q_strand, const int64_t *node_off,
                            const int32_t *node_a, const int32_t *node_b, const int64_t *leaf_off,
                            const int32_t *leaf, const int32_t *leaf_score,
                            const int32_t *leaf_node, const int64_t *path_off,
                            const int32_t *path, int64_t *total, int32_t *pred) {
    return gac_chain_dp_ex(c, n_pairs, t_seq, q_seq, q_strand, node_off, node_a, node_b, leaf_off,
                           leaf, leaf_score, leaf_node, path_off, path, nullptr, nullptr, 0, 0,
                           total, pred);
}

// gac_chain_dp with the exact fast DP (k_dp_fast) when ov_off is given: the
// linear gap-cost minorant lin_k / 1024, the smallest matrix entry, and each
// leaf's overlapping candidates (leaf nodes; -1 = too many to list)
extern "C" int gac_chain_dp_ex(gac_ctx *c, int64_t n_pairs, const int32_t *t_seq,
                               const int32_t *q_seq, const uint8_t *q_strand,
                               const int64_t *node_off, const int32_t *node_a,
                               const int32_t *node_b, const int64_t *leaf_off,
                               const int32_t *leaf, const int32_t *leaf_score,
                               const int32_t *leaf_node, const int64_t *path_off,
                               const int32_t *path, const int64_t *ov_off, const int32_t *ov,
                               int64_t lin_k, int32_t min_entry, int64_t *total, int32_t *pred) {
    gac_clear_error();
    if (!c || n_pairs < 0 ||
        (n_pairs && (!t_seq || !q_seq || !q_strand || !node_off || !leaf_off || !path_off)))
        return gac_fail(GAC_E_ARG, "gac_chain_dp: bad argument");
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_chain_dp before gac_set_scoring");
    CTX_LOCK(c);
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before gac_chain_dp");
    if (n_pairs == 0) return GAC_OK;
    const int64_t nn = node_off[n_pairs], nl = leaf_off[n_pairs], np_ = path_off[nl];
    if (nl == 0) return GAC_OK;
    if (!node_a || !node_b || !leaf || !leaf_score || !leaf_node || !path || !total || !pred)
        return gac_fail(GAC_E_ARG, "gac_chain_dp: NULL array");
    std::vector<DpPair> pairs(n_pairs);
    std::vector<long long> tot0(nn, 0);
    for (int64_t p = 0; p < n_pairs; ++p) {
        DpPair &P = pairs[p];
        int rc = pair_bases(c, t_seq[p], q_seq[p], q_strand[p], P.tbase, P.qbase);
        if (rc != GAC_OK) return rc;
        const int64_t n_nodes = node_off[p + 1] - node_off[p], n_leaves = leaf_off[p + 1] - leaf_off[p];
        if (n_nodes < 0 || n_nodes > 0x7fffffff || n_leaves < 0 || (n_leaves > 0 && n_nodes < 1))
            return gac_fail(GAC_E_ARG, "gac_chain_dp: pair %lld: bad tree size", (long long)p);
        P.node_off = node_off[p];
        P.leaf_off = leaf_off[p];
        P.n_nodes = (int32_t)n_nodes;
        P.n_leaves = (int32_t)n_leaves;
        for (int64_t i = leaf_off[p]; i < leaf_off[p + 1]; ++i) {
            const int32_t v = leaf_node[i];
            if (v < 0 || v >= n_nodes || node_b[2 * (node_off[p] + v) + 1] != ~(int32_t)(i - leaf_off[p]))
                return gac_fail(GAC_E_ARG, "gac_chain_dp: leaf %lld: bad node", (long long)i);
            tot0[node_off[p] + v] = leaf_score[i];
        }
    }
    // a kernel reading past its pair would fault: check the structure first
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t o = node_off[p];
        const int32_t n = pairs[p].n_nodes;
        for (int32_t v = 0; v < n; ++v) {
            const int32_t end = node_b[2 * (o + v)], info = node_b[2 * (o + v) + 1];
            const int32_t lo = node_a[4 * (o + v) + 3];
            if (end <= v || end > n || (info >= 0 && (info > 1 || lo <= v + 1 || lo >= end)))
                return gac_fail(GAC_E_ARG, "gac_chain_dp: pair %lld node %d: bad links", (long long)p, v);
        }
    }
    for (int64_t p = 0; p < n_pairs; ++p)
        for (int64_t i = leaf_off[p]; i < leaf_off[p + 1]; ++i)
            for (int64_t k = path_off[i]; k < path_off[i + 1]; ++k)
                if (path[k] < 0 || path[k] >= pairs[p].n_nodes)
                    return gac_fail(GAC_E_ARG, "gac_chain_dp: leaf %lld: bad path node", (long long)i);
    const bool fast = ov_off != nullptr;
    const int64_t nov = fast ? ov_off[nl] : 0;
    if (fast) {
        if (ov_off[0] != 0 || (nov && !ov) || lin_k < 0)
            return gac_fail(GAC_E_ARG, "gac_chain_dp: bad overlap lists");
        for (int64_t p = 0; p < n_pairs; ++p)
            for (int64_t i = leaf_off[p]; i < leaf_off[p + 1]; ++i) {
                if (ov_off[i + 1] < ov_off[i])
                    return gac_fail(GAC_E_ARG, "gac_chain_dp: leaf %lld: bad overlap offsets", (long long)i);
                for (int64_t k = ov_off[i]; k < ov_off[i + 1]; ++k) {
                    const int32_t v = ov[k];
                    if (v != -1 && (v < 0 || v >= pairs[p].n_nodes ||
                                    node_b[2 * (node_off[p] + v) + 1] >= 0))
                        return gac_fail(GAC_E_ARG, "gac_chain_dp: leaf %lld: bad overlap node",
                                        (long long)i);
                }
            }
    }
    HIPCHK(hipSetDevice(c->device));
    DpArgs a;
    dp_base_args(c, a);
    a.n_pairs = n_pairs;
    DpPair *d_pairs = nullptr;
    int4 *d_na = nullptr, *d_lf = nullptr;
    int2 *d_nb = nullptr;
    long long *d_ms = nullptr, *d_tot = nullptr, *d_total = nullptr;
    int32_t *d_score = nullptr, *d_node = nullptr, *d_path = nullptr, *d_pred = nullptr;
    int64_t *d_poff = nullptr;
    long long *d_nw = nullptr;
    int64_t *d_ovoff = nullptr;
    int32_t *d_ov = nullptr;
    int rc = GAC_OK;
    if (fast) {
        std::vector<long long> nw0(nn, INT64_MIN / 4);
        if ((rc = dev_upload(c, &d_nw, nw0.data(), nn)) != GAC_OK ||
            (rc = dev_upload(c, &d_ovoff, ov_off, nl + 1)) != GAC_OK ||
            (rc = dev_upload(c, &d_ov, nov ? ov : nullptr, nov ? nov : 1)) != GAC_OK) {
            hipStreamSynchronize(c->stream);
            hipFree(d_nw);
            hipFree(d_ovoff);
            hipFree(d_ov);
            return rc;
        }
        hipStreamSynchronize(c->stream);  // (nw0 leaves scope)
    }
    if ((rc = dev_upload(c, &d_pairs, pairs.data(), n_pairs)) == GAC_OK &&
        (rc = dev_upload(c, &d_na, node_a, nn)) == GAC_OK &&
        (rc = dev_upload(c, &d_nb, node_b, nn)) == GAC_OK &&
        (rc = dev_upload(c, &d_ms, nullptr, nn)) == GAC_OK &&
        (rc = dev_upload(c, &d_tot, tot0.data(), nn)) == GAC_OK &&
        (rc = dev_upload(c, &d_lf, leaf, nl)) == GAC_OK &&
        (rc = dev_upload(c, &d_score, leaf_score, nl)) == GAC_OK &&
        (rc = dev_upload(c, &d_node, leaf_node, nl)) == GAC_OK &&
        (rc = dev_upload(c, &d_poff, path_off, nl + 1)) == GAC_OK &&
        (rc = dev_upload(c, &d_path, path, np_ ? np_ : 1)) == GAC_OK &&
        (rc = dev_upload(c, &d_total, nullptr, nl)) == GAC_OK &&
        (rc = dev_upload(c, &d_pred, nullptr, nl)) == GAC_OK) {
        hipError_t e = hipMemsetAsync(d_ms, 0, nn * sizeof(long long), c->stream);
        a.pairs = d_pairs;
        a.nd_ms = d_ms;
        a.nd_tot = d_tot;
        a.nd_a = d_na;
        a.nd_b = d_nb;
        a.lf = d_lf;
        a.lf_score = d_score;
        a.lf_node = d_node;
        a.path_off = d_poff;
        a.path = d_path;
        a.lf_total = d_total;
        a.lf_pred = d_pred;
        a.nd_nw = d_nw;
        a.ov_off = d_ovoff;
        a.ov = d_ov;
        a.lin_k = lin_k;
        a.min_entry = min_entry;
        // one wave per pair, every pair resident at once (largest first is
        // the caller's order; the grid covers them all)
        const int grid = (int)std::min<int64_t>(n_pairs, 1 << 20);
        if (e == hipSuccess) e = dp_launch(c, a, grid, fast);
        if (e == hipSuccess)
            e = hipMemcpyAsync(total, d_total, nl * sizeof(long long), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pred, d_pred, nl * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = gac_fail(GAC_E_HIP, "gac_chain_dp: %s", hipGetErrorString(e));
    }
    hipStreamSynchronize(c->stream);
    hipFree(d_pairs);
    hipFree(d_na);
    hipFree(d_nb);
    hipFree(d_ms);
    hipFree(d_tot);
    hipFree(d_lf);
    hipFree(d_score);
    hipFree(d_node);
    hipFree(d_poff);
    hipFree(d_path);
    hipFree(d_total);
    hipFree(d_pred);
    hipFree(d_nw);
    hipFree(d_ovoff);
    hipFree(d_ov);
    return rc;
}

// device allocations of one call, freed together (after a stream sync)
namespace {
struct DevBufs {
    std::vector<void *> p;
    hipError_t e = hipSuccess;
    template <class T>
    T *take(int64_t n) {
        void *q = nullptr;
        if (e == hipSuccess) e = hipMalloc(&q, (size_t)(n > 0 ? n : 1) * sizeof(T));
        if (q) p.push_back(q);
        return (T *)q;
    }
    ~DevBufs() {
        for (void *q : p) hipFree(q);
    }
};
}  // namespace

// the device build's set-up shared by gac_chain_dp_blocks and gac_kd_trees:
// uploads, leaves in target order and leaf offsets (leaf_off, host), node
// offsets, every array of the build; u.t.L == 0: no leaves (nothing else set)
namespace {
struct DtSetup {
    DtTree t;
    std::vector<DpPair> pairs;
    std::vector<int64_t> node_off;
    int levels = 0;
    int64_t *d_leaf_off = nullptr;
    int32_t *d_err = nullptr;
    long long *d_total = nullptr, *d_lf_total = nullptr;
    int32_t *d_pred = nullptr, *d_lf_pred = nullptr, *d_out_tord = nullptr;
    DpPair *d_pairs = nullptr;
    double t0 = 0, t1 = 0;
};
}  // namespace

static int dt_setup(gac_ctx *c, const char *who, int64_t P, const int32_t *t_seq,
                    const int32_t *q_seq, const uint8_t *q_strand, const int64_t *blk_off,
                    const int32_t *box, const int32_t *score, int fast, int32_t ov_cap,
                    int64_t *leaf_off, DevBufs &M, DtSetup &u) {
    const int64_t B = blk_off[P];
    u.t0 = wall_s();
    const bool timing = getenv("GAC_TIMING") != nullptr;
    (void)timing;
    std::vector<DpPair> &pairs = u.pairs;
    pairs.resize(P);
    std::vector<int2> sizes(P);
    for (int64_t p = 0; p < P; ++p) {
        int rc = pair_bases(c, t_seq[p], q_seq[p], q_strand[p], pairs[p].tbase, pairs[p].qbase);
        if (rc != GAC_OK) return rc;
        sizes[p] = make_int2(c->g[0].sizes[t_seq[p]], c->g[1].sizes[q_seq[p]]);
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DtTree &t = u.t;
    memset(&t, 0, sizeof(t));
    t.P = P;
    t.B = B;
    t.fast = fast ? 1 : 0;
    t.ov_cap = ov_cap;
    int bits = 0;
    while ((1LL << bits) <= P) ++bits;
    t.end_bit = 31 + bits;
    int64_t *d_blk_off = M.take<int64_t>(P + 1);
    int2 *d_sizes = M.take<int2>(P);
    int4 *d_box = M.take<int4>(B);
    int32_t *d_score = M.take<int32_t>(B);
    unsigned long long *d_keys = M.take<unsigned long long>(2 * B);
    int32_t *d_vals = M.take<int32_t>(2 * B);
    int64_t *d_leaf_off = u.d_leaf_off = M.take<int64_t>(P + 1);
    int32_t *d_err = u.d_err = M.take<int32_t>(1);
    t.tpos = M.take<int32_t>(B);
    t.qpos = M.take<int32_t>(B);
    t.posd = M.take<int32_t>(B);
    u.d_total = M.take<long long>(B);
    u.d_pred = M.take<int32_t>(B);
    if (M.e != hipSuccess)
        return gac_fail(GAC_E_HIP, "%s: hipMalloc: %s", who, hipGetErrorString(M.e));
    size_t b_sort = 0;
    HIPCHK(dt_sort_pairs(nullptr, b_sort, d_keys, d_keys + B, d_vals, d_vals + B, B, t.end_bit, s));
    void *d_tmp = M.take<uint8_t>((int64_t)b_sort);
    HIPCHK(M.e);
    HIPCHK(hipMemcpyAsync(d_blk_off, blk_off, (P + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_sizes, sizes.data(), P * sizeof(int2), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_box, box, B * sizeof(int4), hipMemcpyHostToDevice, s));
    if (score)
        HIPCHK(hipMemcpyAsync(d_score, score, B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    else
        HIPCHK(hipMemsetAsync(d_score, 0, B * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int32_t), s));
    // ---- leaves in target order, per-pair leaf offsets
    HIPCHK(launch_dt_keys(P, B, d_blk_off, d_sizes, d_box, d_keys, d_vals, d_err, s));
    HIPCHK(dt_sort_pairs(d_tmp, b_sort, d_keys, d_keys + B, d_vals, d_vals + B, B, t.end_bit, s));
    HIPCHK(launch_dt_leaf_off(P, B, d_keys + B, d_leaf_off, s));
    int32_t h_err = 0;
    HIPCHK(hipMemcpyAsync(leaf_off, d_leaf_off, (P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double t1 = wall_s();
    (void)t1;
    if (h_err & 1) {  // the first bad block, as a serial check reports it
        for (int64_t p = 0; p < P; ++p)
            for (int64_t g = blk_off[p]; g < blk_off[p + 1]; ++g) {
                const int32_t *b = box + 4 * g;
                if (b[0] < 0 || b[0] > b[1] || b[1] > sizes[p].y || b[2] < 0 || b[2] > b[3] ||
                    b[3] > sizes[p].x)
                    return gac_fail(GAC_E_ARG, "%s: pair %lld block %lld (%d-%d, %d-%d) "
                                    "outside its sequences", who, (long long)p, (long long)(g - blk_off[p]),
                                    b[0], b[1], b[2], b[3]);
            }
        return gac_fail(GAC_E_ARG, "%s: a block outside its sequences", who);
    }
    const int64_t L = leaf_off[P];
    u.t1 = t1;
    if (L == 0) return GAC_OK;
    std::vector<int64_t> &node_off = u.node_off;
    node_off.resize(P + 1);
    int64_t maxnl = 0;
    node_off[0] = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t nl = leaf_off[p + 1] - leaf_off[p];
        maxnl = std::max(maxnl, nl);
        node_off[p + 1] = node_off[p] + (nl ? 2 * nl - 1 : 0);
        pairs[p].node_off = node_off[p];
        pairs[p].leaf_off = leaf_off[p];
        pairs[p].n_nodes = (int32_t)(node_off[p + 1] - node_off[p]);
        pairs[p].n_leaves = (int32_t)nl;
    }
    const int64_t N = node_off[P];
    int &levels = u.levels;
    levels = 0;
    for (int64_t n = maxnl; n > 1; n -= n / 2) ++levels;
    t.L = L;
    t.N = N;
    t.blk_off = d_blk_off;
    t.box = d_box;
    t.score = d_score;
    t.keys = d_keys + B;
    t.tord = d_vals + B;
    t.leaf_off = d_leaf_off;
    int64_t *d_node_off = M.take<int64_t>(P + 1);
    t.node_off = d_node_off;
    t.pidx = M.take<int32_t>(L);
    t.key2 = M.take<unsigned long long>(2 * L);
    t.val2 = M.take<int32_t>(2 * L);
    t.ql = M.take<int32_t>(L);
    t.tl = M.take<int32_t>(L);
    t.spare = M.take<int32_t>(L);
    t.sstart = M.take<int32_t>(L);
    t.slen = M.take<int32_t>(L);
    t.snode = M.take<int32_t>(L);
    t.flag = M.take<int32_t>(L);
    t.excl = M.take<int32_t>(L);
    t.ndep = M.take<int32_t>(N);
    t.ndl = M.take<int32_t>(N);
    t.qbox = M.take<int4>(L);
    t.qtp = M.take<int32_t>(L);
    t.msz = M.take<int32_t>(P);
    t.over = M.take<uint8_t>(L);
    t.pcnt = M.take<long long>(L + 1);
    t.ocnt = M.take<long long>(L + 1);
    t.err = d_err;
    t.na = M.take<int4>(N);
    t.nb = M.take<int2>(N);
    t.tot = M.take<long long>(N);
    t.ms = M.take<long long>(N);
    t.nw = M.take<long long>(N);
    t.lf = M.take<int4>(L);
    t.lsc = M.take<int32_t>(L);
    t.lnode = M.take<int32_t>(L);
    t.poff = M.take<long long>(L + 1);
    t.ooff = M.take<long long>(L + 1);
    u.d_lf_total = M.take<long long>(L);
    u.d_lf_pred = M.take<int32_t>(L);
    u.d_out_tord = M.take<int32_t>(L);
    DpPair *d_pairs = u.d_pairs = M.take<DpPair>(P);
    if (M.e != hipSuccess)
        return gac_fail(GAC_E_HIP, "%s: hipMalloc: %s", who, hipGetErrorString(M.e));
    size_t need = b_sort, b = 0;
    HIPCHK(dt_sort_pairs(nullptr, b, t.key2, t.key2 + L, t.val2, t.val2 + L, L, t.end_bit, s));
    need = std::max(need, b);
    HIPCHK(dt_scan32(nullptr, b, t.flag, t.excl, L, s));
    need = std::max(need, b);
    HIPCHK(dt_scan64(nullptr, b, t.pcnt, t.poff, L + 1, s));
    need = std::max(need, b);
    t.tmp = need > b_sort ? M.take<uint8_t>((int64_t)need) : d_tmp;
    t.tmp_bytes = need;
    HIPCHK(M.e);
    HIPCHK(hipMemcpyAsync(d_node_off, node_off.data(), (P + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), P * sizeof(DpPair), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(t.pcnt, 0, (L + 1) * sizeof(long long), s));
    HIPCHK(hipMemsetAsync(t.ocnt, 0, (L + 1) * sizeof(long long), s));
    return GAC_OK;
}

// chainBlocks' DP for n_pairs pairs from their blocks: the leaves, kd-trees,
// update paths and overlap lists built on the device (gac_dptree.hip), then
// k_dp_fast (fast) or k_dp; see include/gachain.h
extern "C" int gac_chain_dp_blocks(gac_ctx *c, int64_t n_pairs, const int32_t *t_seq,
                                   const int32_t *q_seq, const uint8_t *q_strand,
                                   const int64_t *blk_off, const int32_t *box, const int32_t *score,
                                   int fast, int64_t lin_k, int32_t min_entry, int32_t ov_cap,
                                   int64_t *leaf_off, int32_t *tord, int64_t *total, int32_t *pred) {
    gac_clear_error();
    if (!c || n_pairs < 0 || (n_pairs && (!t_seq || !q_seq || !q_strand || !blk_off || !leaf_off)))
        return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: bad argument");
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_chain_dp_blocks before gac_set_scoring");
    CTX_LOCK(c);
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before gac_chain_dp_blocks");
    if (n_pairs == 0) return GAC_OK;
    if (n_pairs >= (1LL << 30)) return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: too many pairs");
    const int64_t P = n_pairs, B = blk_off[P];
    if (blk_off[0] != 0 || B < 0 || B > 0x7fffffffLL)
        return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: bad block offsets");
    for (int64_t p = 0; p < P; ++p)
        if (blk_off[p + 1] < blk_off[p])
            return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: pair %lld: block offsets descend",
                            (long long)p);
    if (B && (!box || !score || !tord || !total || !pred))
        return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: NULL array");
    if (fast && lin_k < 0) return gac_fail(GAC_E_ARG, "gac_chain_dp_blocks: bad lin_k");
    if (B == 0) {
        for (int64_t p = 0; p <= P; ++p) leaf_off[p] = 0;
        return GAC_OK;
    }
    const bool timing = getenv("GAC_TIMING") != nullptr;
    DevBufs M;
    DtSetup u;
    int rc0 = dt_setup(c, "gac_chain_dp_blocks", P, t_seq, q_seq, q_strand, blk_off, box, score, fast,
                       ov_cap, leaf_off, M, u);
    if (rc0 != GAC_OK) return rc0;
    const double t0 = u.t0, t1 = u.t1;
    if (u.t.L == 0) {
        for (int64_t g = 0; g < B; ++g) {
            total[g] = score[g];
            pred[g] = -1;
        }
        return GAC_OK;
    }
    DtTree &t = u.t;
    hipStream_t s = c->stream;
    const int64_t L = t.L;
    const int levels = u.levels;
    int32_t *d_err = u.d_err;
    long long *d_total = u.d_total, *d_lf_total = u.d_lf_total;
    int32_t *d_pred = u.d_pred, *d_lf_pred = u.d_lf_pred, *d_out_tord = u.d_out_tord;
    DpPair *d_pairs = u.d_pairs;
    int64_t *d_leaf_off = u.d_leaf_off;
    const int64_t N = t.N;
    int32_t h_err = 0;
    // ---- query order, the trees, path and overlap counts
    HIPCHK(launch_dt_tree(t, levels, s));
    long long n_path = 0, n_ov = 0;
    HIPCHK(hipMemcpyAsync(&n_path, t.poff + L, sizeof(long long), hipMemcpyDeviceToHost, s));
    if (fast) HIPCHK(hipMemcpyAsync(&n_ov, t.ooff + L, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_err)
        return gac_fail(GAC_E_HIP, "gac_chain_dp_blocks: device tree build failed (%d)", h_err);
    int32_t *d_path = M.take<int32_t>(n_path);
    int32_t *d_ov = M.take<int32_t>(n_ov);
    if (M.e != hipSuccess)
        return gac_fail(GAC_E_HIP, "gac_chain_dp_blocks: hipMalloc: %s", hipGetErrorString(M.e));
    HIPCHK(launch_dt_lists(t, d_path, d_ov, s));
    HIPCHK(hipMemcpyAsync(&h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_err)
        return gac_fail(GAC_E_HIP, "gac_chain_dp_blocks: device path build failed (%d)", h_err);
    const double t2 = wall_s();
    // ---- the DP
    DpArgs a;
    dp_base_args(c, a);
    a.n_pairs = P;
    a.pairs = d_pairs;
    a.nd_ms = t.ms;
    a.nd_tot = t.tot;
    a.nd_a = t.na;
    a.nd_b = t.nb;
    a.lf = t.lf;
    a.lf_score = t.lsc;
    a.lf_node = t.lnode;
    a.path_off = (const int64_t *)t.poff;
    a.path = d_path;
    a.lf_total = d_lf_total;
    a.lf_pred = d_lf_pred;
    a.nd_nw = fast ? t.nw : nullptr;
    a.ov_off = fast ? (const int64_t *)t.ooff : nullptr;
    a.ov = fast ? d_ov : nullptr;
    a.lin_k = lin_k;
    a.min_entry = min_entry;
    a.err = d_err;
    const int grid = (int)std::min<int64_t>(P, 1 << 20);
    HIPCHK(dp_launch(c, a, grid, fast != 0));
    {
        // the DP runs for seconds beside the host's own DP threads: wait
        // without spinning a core (hipStreamSynchronize may busy-wait)
        hipEvent_t done;
        HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        hipError_t e = hipEventRecord(done, s);
        while (e == hipSuccess && (e = hipEventQuery(done)) == hipErrorNotReady) {
            const struct timespec nap = {0, 500000};
            nanosleep(&nap, nullptr);
            e = hipSuccess;
        }
        hipEventDestroy(done);
        HIPCHK(e);
    }
    const double t3 = wall_s();
    if (const char *dd = getenv("GAC_DT_DUMP")) {  // (debug: the built arrays, raw)
        auto dump = [&](const char *name, const void *d, size_t bytes) {
            std::vector<char> h(bytes);
            if (hipMemcpy(h.data(), d, bytes, hipMemcpyDeviceToHost) != hipSuccess) return;
            std::string f = std::string(dd) + "/" + name;
            if (FILE *o = fopen(f.c_str(), "wb")) {
                fwrite(h.data(), 1, bytes, o);
                fclose(o);
            }
        };
        dump("leaf_off", d_leaf_off, (P + 1) * 8);
        dump("lf", t.lf, L * 16);
        dump("lnode", t.lnode, L * 4);
        dump("na", t.na, N * 16);
        dump("nb", t.nb, N * 8);
        dump("poff", t.poff, (L + 1) * 8);
        dump("path", d_path, n_path * 4);
        if (fast) dump("ooff", t.ooff, (L + 1) * 8);
        if (fast) dump("ov", d_ov, n_ov * 4);
        dump("lf_total", d_lf_total, L * 8);
        dump("lf_pred", d_lf_pred, L * 4);
    }
    HIPCHK(launch_dt_out(t, d_lf_total, d_lf_pred, d_out_tord, d_total, d_pred, s));
    HIPCHK(hipMemcpyAsync(tord, d_out_tord, L * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(total, d_total, B * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pred, d_pred, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_err)
        return gac_fail(GAC_E_HIP, "gac_chain_dp_blocks: %s (%d)",
                        (h_err & 32) ? "the DP's in-order commit stalled" : "a predecessor is not a leaf",
                        h_err);
    if (timing)
        fprintf(stderr,
                "[gac_chain_dp_blocks] %lld pairs, %lld blocks, %lld leaves, %d levels, %lld path "
                "nodes, %lld overlap entries: upload + leaves %.3f s, trees + paths + overlaps %.3f s, "
                "%s %.3f s, results %.3f s\n",
                (long long)P, (long long)B, (long long)L, levels, n_path, n_ov, t1 - t0, t2 - t1,
                !fast ? "k_dp" : (dp_waves() > 1 ? "k_dp_spec" : "k_dp_fast"), t3 - t2, wall_s() - t3);
    return GAC_OK;
}

// kdTreeMake for n_pairs pairs on the device (gac_dptree.hip's build), out
// in the host DP's layout, per pair into the caller's buffers; see
// include/gachain.h
extern "C" int gac_kd_trees(gac_ctx *c, int64_t n_pairs, const int32_t *t_seq, const int32_t *q_seq,
                            const uint8_t *q_strand, const int64_t *blk_off, const int32_t *box,
                            int64_t *leaf_off, int32_t *const *tord, int32_t *const *qord,
                            int32_t *const *lnode, int32_t *const *nodes) {
    gac_clear_error();
    if (!c || n_pairs < 0 || (n_pairs && (!t_seq || !q_seq || !q_strand || !blk_off || !leaf_off)))
        return gac_fail(GAC_E_ARG, "gac_kd_trees: bad argument");
    CTX_LOCK(c);
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before gac_kd_trees");
    if (n_pairs == 0) return GAC_OK;
    if (n_pairs >= (1LL << 30)) return gac_fail(GAC_E_ARG, "gac_kd_trees: too many pairs");
    const int64_t P = n_pairs, B = blk_off[P];
    if (blk_off[0] != 0 || B < 0 || B > 0x7fffffffLL)
        return gac_fail(GAC_E_ARG, "gac_kd_trees: bad block offsets");
    for (int64_t p = 0; p < P; ++p)
        if (blk_off[p + 1] < blk_off[p])
            return gac_fail(GAC_E_ARG, "gac_kd_trees: pair %lld: block offsets descend", (long long)p);
    if (B && (!box || !tord || !qord || !lnode || !nodes))
        return gac_fail(GAC_E_ARG, "gac_kd_trees: NULL array");
    if (B == 0) {
        for (int64_t p = 0; p <= P; ++p) leaf_off[p] = 0;
        return GAC_OK;
    }
    const double t0 = wall_s();
    DevBufs M;
    DtSetup u;
    int rc = dt_setup(c, "gac_kd_trees", P, t_seq, q_seq, q_strand, blk_off, box, nullptr, 0, 0,
                      leaf_off, M, u);
    if (rc != GAC_OK) return rc;
    hipStream_t s = c->stream;
    DtTree &t = u.t;
    if (t.L == 0) {
        for (int64_t p = 0; p < P; ++p)
            for (int64_t g = 0; g < blk_off[p + 1] - blk_off[p]; ++g) lnode[p][g] = -1;
        return GAC_OK;
    }
    int32_t *d_nodes = M.take<int32_t>(6 * t.N);
    int32_t *d_qord = M.take<int32_t>(t.L);
    int32_t *d_lnode_blk = M.take<int32_t>(B);
    if (M.e != hipSuccess)
        return gac_fail(GAC_E_HIP, "gac_kd_trees: hipMalloc: %s", hipGetErrorString(M.e));
    HIPCHK(launch_dt_build(t, u.levels, s));
    HIPCHK(launch_dt_host(t, d_nodes, u.d_out_tord, d_qord, d_lnode_blk, s));
    int32_t h_err = 0;
    HIPCHK(hipMemcpyAsync(&h_err, u.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_err) return gac_fail(GAC_E_HIP, "gac_kd_trees: device tree build failed (%d)", h_err);
    const double t1 = wall_s();
    for (int64_t p = 0; p < P; ++p) {
        const int64_t nl = leaf_off[p + 1] - leaf_off[p], nb = blk_off[p + 1] - blk_off[p];
        if (nl) {
            HIPCHK(hipMemcpyAsync(tord[p], u.d_out_tord + leaf_off[p], nl * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(qord[p], d_qord + leaf_off[p], nl * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(nodes[p], d_nodes + 6 * u.node_off[p],
                                  (2 * nl - 1) * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        if (nb)
            HIPCHK(hipMemcpyAsync(lnode[p], d_lnode_blk + blk_off[p], nb * sizeof(int32_t),
                                  hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (getenv("GAC_TIMING"))
        fprintf(stderr, "[gac_kd_trees] %lld pairs, %lld blocks, %lld leaves, %d levels: build %.3f s, "
                        "results %.3f s\n", (long long)P, (long long)B, (long long)t.L, u.levels,
                t1 - t0, wall_s() - t1);
    return GAC_OK;
}

extern "C" int gac_crossovers(gac_ctx *c, int64_t n, const int32_t *t_seq, const int32_t *q_seq,
                              const uint8_t *q_strand, const int32_t *lqe, const int32_t *lte,
                              const int32_t *rqs, const int32_t *rts, const int32_t *overlap,
                              int32_t *pos, int32_t *adj) {
    gac_clear_error();
    if (!c || n < 0 || (n && (!t_seq || !q_seq || !q_strand || !lqe || !lte || !rqs || !rts ||
                              !overlap || !pos || !adj)))
        return gac_fail(GAC_E_ARG, "gac_crossovers: bad argument");
    if (!c->scoring) return gac_fail(GAC_E_STATE, "gac_crossovers before gac_set_scoring");
    CTX_LOCK(c);
    if (!c->g[0].final || !c->g[1].final)
        return gac_fail(GAC_E_STATE, "load both genomes before gac_crossovers");
    if (n == 0) return GAC_OK;
    std::vector<XoverJob> jobs(n);
    const Genome &T = c->g[0], &Q = c->g[1];
    for (int64_t j = 0; j < n; ++j) {
        XoverJob &J = jobs[j];
        int rc = pair_bases(c, t_seq[j], q_seq[j], q_strand[j], J.tbase, J.qbase);
        if (rc != GAC_OK) return rc;
        const int32_t ov = overlap[j];
        if (ov < 0 || lqe[j] - ov < 0 || lte[j] - ov < 0 || rqs[j] < 0 || rts[j] < 0 ||
            lqe[j] > Q.sizes[q_seq[j]] || (int64_t)rqs[j] + ov > Q.sizes[q_seq[j]] ||
            lte[j] > T.sizes[t_seq[j]] || (int64_t)rts[j] + ov > T.sizes[t_seq[j]])
            return gac_fail(GAC_E_ARG, "gac_crossovers: overlap %lld outside its sequences",
                            (long long)j);
        J.lqe = lqe[j];
        J.lte = lte[j];
        J.rqs = rqs[j];
        J.rts = rts[j];
        J.ov = ov;
        J.pad = 0;
    }
    HIPCHK(hipSetDevice(c->device));
    DpArgs a;
    dp_base_args(c, a);
    XoverJob *d_jobs = nullptr;
    int32_t *d_pos = nullptr, *d_adj = nullptr;
    int rc = GAC_OK;
    if ((rc = dev_upload(c, &d_jobs, jobs.data(), n)) == GAC_OK &&
        (rc = dev_upload(c, &d_pos, nullptr, n)) == GAC_OK &&
        (rc = dev_upload(c, &d_adj, nullptr, n)) == GAC_OK) {
        hipError_t e = launch_xover(a, d_jobs, n, d_pos, d_adj, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(pos, d_pos, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(adj, d_adj, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = gac_fail(GAC_E_HIP, "gac_crossovers: %s", hipGetErrorString(e));
    }
    hipStreamSynchronize(c->stream);
    hipFree(d_jobs);
    hipFree(d_pos);
    hipFree(d_adj);
    return rc;
}
