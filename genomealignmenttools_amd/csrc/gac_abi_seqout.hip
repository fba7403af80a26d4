// gac_abi_seqout.hip -- libgachain's C ABI, the sequence tools' output: match
// composition, PSL match counts, and the alignment text entry points
// (gac_axt_*).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "gac_ctx.h"

using namespace gac;

// ------------------------------------------------------ match composition
// (chainAntiRepeat; k_compose reads the set as the upload left it: no
// scoring setup, no workspace)
static void chain_walk_args(const gac_ctx *c, const gac_chainset *cs, ChainWalkArgs &a) {
    a.t_planes = c->g[0].planes;
    a.q_planes = c->g[1].planes;
    a.t_nmask = c->g[0].nmask;
    a.q_nmask = c->g[1].nmask;
    a.t_lmask = c->g[0].lmask;
    a.q_lmask = c->g[1].lmask;
    a.chains = cs->chains;
    a.blk = cs->blk;
    a.coff = cs->d_coff;
    a.tile_c0 = cs->d_tile_c0;
    a.n_chains = cs->n_chains;
    a.n_blocks = cs->n_blocks;
    a.ntiles = (cs->n_blocks + 63) >> 6;
}

static int compose_device(gac_ctx *c, const gac_chainset *cs, int64_t *d_match, int64_t *d_rep,
                          int64_t *d_total, hipStream_t s) {
    if (!c->g[0].final || !c->g[1].final || !c->g[0].lmask || !c->g[1].lmask)
        return gac_fail(GAC_E_STATE, "gac_chain_composition: both genome sides need the "
                                     "soft-mask plane (gac_genome_want_softmask before loading)");
    const int64_t n = cs->n_chains;
    if (n == 0) return GAC_OK;
    if (!d_match || !d_rep || !d_total) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipMemsetAsync(d_match, 0, (size_t)n * 4 * 8, s));
    HIPCHK(hipMemsetAsync(d_rep, 0, (size_t)n * 8, s));
    HIPCHK(hipMemsetAsync(d_total, 0, (size_t)n * 8, s));
    ComposeArgs a;
    chain_walk_args(c, cs, a);
    a.match = (unsigned long long *)d_match;
    a.rep = (unsigned long long *)d_rep;
    a.total = (unsigned long long *)d_total;
    HIPCHK(launch_compose(a, s));
    return GAC_OK;
}

// The host forms of the per-chain counts: `k` caller arrays of words[i] int64
// per chain, laid one after the other in one device buffer that `body` (the
// _device form) fills, then copied back.  c and cs are checked by the caller.
template <class Body>
static int chain_counts_host(gac_ctx *c, const gac_chainset *cs, const char *who, int k,
                             int64_t *const *out, const int *words, Body body) {
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = cs->n_chains;
    int64_t *d = nullptr;
    size_t tot = 0;
    for (int i = 0; i < k; ++i) tot += (size_t)words[i];
    if (n) {
        for (int i = 0; i < k; ++i)
            if (!out[i]) return gac_fail(GAC_E_ARG, "NULL buffer");
        HIPCHK(hipMalloc(&d, (size_t)n * tot * 8));
    }
    hipStream_t s = c->stream;
    int rc = body(d, n, s);
    hipError_t e = hipSuccess;
    if (rc == GAC_OK && n) {
        size_t off = 0;
        for (int i = 0; i < k && e == hipSuccess; off += (size_t)n * words[i], ++i)
            e = hipMemcpyAsync(out[i], d + off, (size_t)n * words[i] * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (d) hipFree(d);
    if (rc == GAC_OK && e != hipSuccess)
        return gac_fail(GAC_E_HIP, "%s failed: %s", who, hipGetErrorString(e));
    return rc;
}

extern "C" int gac_chain_composition_device(gac_ctx *c, const gac_chainset *cs, int64_t *d_match,
                                            int64_t *d_rep, int64_t *d_total, void *stream) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    return compose_device(c, cs, d_match, d_rep, d_total, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int gac_chain_composition(gac_ctx *c, const gac_chainset *cs, int64_t *match,
                                     int64_t *rep, int64_t *total) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset");
    int64_t *const out[3] = {match, rep, total};
    static const int words[3] = {4, 1, 1};
    return chain_counts_host(c, cs, "gac_chain_composition", 3, out, words,
                             [&](int64_t *d, int64_t n, hipStream_t s) {
                                 return compose_device(c, cs, d, d + 4 * n, d + 5 * n, s);
                             });
}

// ------------------------------------------------------ PSL match counts
// (chainToPsl, chainToPsl.c:106-131; k_psl_counts walks the set as k_compose
// does and reads the target's soft-mask plane only)
static int psl_counts_device(gac_ctx *c, const gac_chainset *cs, int64_t *d_counts, hipStream_t s) {
    if (!c->g[0].final || !c->g[1].final || !c->g[0].lmask)
        return gac_fail(GAC_E_STATE, "gac_chain_psl_counts: the target side needs the soft-mask "
                                     "plane (gac_genome_want_softmask before loading)");
    const int64_t n = cs->n_chains;
    if (n == 0) return GAC_OK;
    if (!d_counts) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)n * 4 * 8, s));
    PslArgs a;
    chain_walk_args(c, cs, a);
    a.counts = (unsigned long long *)d_counts;
    HIPCHK(launch_psl_counts(a, s));
    return GAC_OK;
}

extern "C" int gac_chain_psl_counts_device(gac_ctx *c, const gac_chainset *cs, int64_t *d_counts,
                                           void *stream) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    return psl_counts_device(c, cs, d_counts, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int gac_chain_psl_counts(gac_ctx *c, const gac_chainset *cs, int64_t *counts) {
    gac_clear_error();
    if (!c) return gac_fail(GAC_E_ARG, "NULL context");
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset");
    static const int words[1] = {4};
    return chain_counts_host(c, cs, "gac_chain_psl_counts", 1, &counts, words,
                             [&](int64_t *d, int64_t n, hipStream_t s) {
                                 return psl_counts_device(c, cs, d, s);
                             });
}

// ------------------------------------------------------ alignment text
// (chainToAxt; gac_axtout.hip).  A call runs in two steps with one host wait
// between them: the pieces are checked and counted (k_axt_plan + scan), then
// the kernels sized by the virtual block count run.  Workspace: two grow-only
// arenas per AxtWs (the context's for the host entry points, one per job).
struct AxtArena {
    char *p = nullptr;
    size_t cap = 0;
};

struct AxtWs {
    AxtArena a1, a2, text;
    int64_t *h = nullptr;  // pinned: [0] V, [1] status
};

static hipError_t arena_need(AxtArena &A, size_t bytes, hipStream_t s) {
    if (bytes <= A.cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);  // (work in flight may still use the old one)
    if (e != hipSuccess) return e;
    if (A.p) hipFree(A.p);
    A.p = nullptr;
    A.cap = 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    e = hipMalloc((void **)&A.p, cap);
    if (e == hipSuccess) A.cap = cap;
    return e;
}

static void ws_free(AxtWs &w) {
    for (AxtArena *A : {&w.a1, &w.a2, &w.text}) {
        if (A->p) hipFree(A->p);
        A->p = nullptr;
        A->cap = 0;
    }
    if (w.h) hipHostFree(w.h);
    w.h = nullptr;
}

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Step one.  pieces: in host memory (copied) or already on the device.  On
// return a holds the genome, set and plan fields and a.V; status is zero.
static int axt_plan(gac_ctx *c, const gac_chainset *cs, AxtWs &ws, const gac_window *h_pieces,
                    const gac_window *d_pieces, int64_t n, bool clip, hipStream_t s, AxtArgs &a) {
    if (!c->g[0].final || !c->g[1].final || !c->g[0].lmask || !c->g[1].lmask)
        return gac_fail(GAC_E_STATE, "gac_axt: both genome sides need the soft-mask plane "
                                     "(gac_genome_want_softmask before loading)");
    if (n < 0 || n >= INT32_MAX) return gac_fail(GAC_E_ARG, "gac_axt: bad piece count");
    if (!h_pieces && !d_pieces) return gac_fail(GAC_E_ARG, "NULL buffer");
    if (!ws.h) HIPCHK(hipHostMalloc((void **)&ws.h, 64, hipHostMallocDefault));
    const size_t b_pieces = h_pieces ? up16((size_t)n * sizeof(Window)) : 0;
    const size_t b_pboff = up16((size_t)(n + 1) * 8), b_part = up16((size_t)(n / 2048 + 2) * 8);
    HIPCHK(arena_need(ws.a1, b_pieces + b_pboff + b_part + 16, s));
    char *p = ws.a1.p;
    memset(&a, 0, sizeof(a));
    a.t_planes = c->g[0].planes;
    a.q_planes = c->g[1].planes;
    a.t_nmask = c->g[0].nmask;
    a.q_nmask = c->g[1].nmask;
    a.t_lmask = c->g[0].lmask;
    a.q_lmask = c->g[1].lmask;
    a.chains = cs->chains;
    a.blk = cs->blk;
    a.n_chains = cs->n_chains;
    a.n = n;
    a.clip = clip;
    if (h_pieces) {
        HIPCHK(hipMemcpyAsync(p, h_pieces, (size_t)n * sizeof(Window), hipMemcpyHostToDevice, s));
        a.pieces = (const Window *)p;
        p += b_pieces;
    } else {
        a.pieces = (const Window *)d_pieces;
    }
    a.pboff = (int64_t *)p;
    p += b_pboff;
    a.part = (int64_t *)p;
    p += b_part;
    a.status = (int32_t *)p;
    HIPCHK(hipMemsetAsync(a.status, 0, 16, s));
    HIPCHK(launch_axt_plan(a, s));
    HIPCHK(hipMemcpyAsync(&ws.h[0], a.pboff + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&ws.h[1], a.status, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    a.V = ws.h[0];
    if ((int32_t)ws.h[1] & kAxtBadWindow)
        return gac_fail(GAC_E_ARG, "gac_axt: a piece's blocks lie outside its chain (or its chain "
                                   "index is out of range)");
    if ((int32_t)ws.h[1] & kAxtBadClip)
        return gac_fail(GAC_E_ARG, "gac_axt: a piece's t_start / t_end leave its first or last "
                                   "block empty");
    return GAC_OK;
}

// the status word after a step, on the host
static int axt_status(AxtWs &ws, const AxtArgs &a, hipStream_t s, int32_t *st) {
    HIPCHK(hipMemcpyAsync(&ws.h[1], a.status, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *st = (int32_t)ws.h[1];
    return GAC_OK;
}

static int axt_bad_gap() {
    return gac_fail(GAC_E_ARG, "gac_axt: a piece holds a negative or double-sided gap "
                               "(cut chains with gac_axt_split)");
}

// measure into device arrays; extra: bytes the caller wants after acc in a2
static int axt_measure_dev(gac_ctx *c, const gac_chainset *cs, AxtWs &ws, const gac_window *h_pieces,
                           const gac_window *d_pieces, int64_t n, int32_t *d_score,
                           int64_t *d_match, int64_t *d_ali, int64_t *d_sym, bool own_out,
                           bool clip, hipStream_t s) {
    AxtArgs a;
    int rc = axt_plan(c, cs, ws, h_pieces, d_pieces, n, clip, s, a);
    if (rc != GAC_OK) return rc;
    const size_t b_acc = up16((size_t)n * 32);
    HIPCHK(arena_need(ws.a2, b_acc + (own_out ? 4 * up16((size_t)n * 8) : 0), s));
    a.acc = (unsigned long long *)ws.a2.p;
    if (own_out) {  // the host entry point's results, behind acc
        char *p = ws.a2.p + b_acc;
        d_score = (int32_t *)p;
        d_match = (int64_t *)(p + up16((size_t)n * 8));
        d_ali = (int64_t *)(p + 2 * up16((size_t)n * 8));
        d_sym = (int64_t *)(p + 3 * up16((size_t)n * 8));
    }
    a.score = d_score;
    a.match = d_match;
    a.ali = d_ali;
    a.sym = d_sym;
    HIPCHK(hipMemsetAsync(a.acc, 0, (size_t)n * 32, s));
    HIPCHK(launch_axt_stat(a, s));
    int32_t st = 0;
    rc = axt_status(ws, a, s, &st);
    if (rc != GAC_OK) return rc;
    if (st & kAxtBadGap) return axt_bad_gap();
    return GAC_OK;
}

// render into device text; the pieces' rows are checked against out_bytes
// before anything is written.  Returns with the render kernels enqueued.
static int axt_render_dev(gac_ctx *c, const gac_chainset *cs, AxtWs &ws, const gac_window *h_pieces,
                          const gac_window *d_pieces, int64_t n, const int64_t *h_offsets,
                          const int64_t *d_offsets, char *d_out, int64_t out_bytes, bool clip,
                          hipStream_t s) {
    if (out_bytes < 0) return gac_fail(GAC_E_ARG, "gac_axt_render: negative out_bytes");
    AxtArgs a;
    int rc = axt_plan(c, cs, ws, h_pieces, d_pieces, n, clip, s, a);
    if (rc != GAC_OK) return rc;
    const size_t b_S = up16((size_t)(a.V + 1) * 8), b_part = up16((size_t)(a.V / 2048 + 2) * 8);
    const size_t b_off = up16((size_t)n * 8);
    HIPCHK(arena_need(ws.a2, b_S + b_part + 2 * b_off, s));
    char *p = ws.a2.p;
    a.S = (int64_t *)p;
    p += b_S;
    a.part = (int64_t *)p;
    p += b_part;
    a.off = (int64_t *)p;
    p += b_off;
    if (h_offsets) {
        HIPCHK(hipMemcpyAsync(p, h_offsets, (size_t)n * 8, hipMemcpyHostToDevice, s));
        a.offsets = (const int64_t *)p;
    } else {
        a.offsets = d_offsets;
    }
    a.out = d_out;
    a.out_bytes = out_bytes;
    HIPCHK(launch_axt_place(a, s));
    int32_t st = 0;
    rc = axt_status(ws, a, s, &st);
    if (rc != GAC_OK) return rc;
    if (st & kAxtBadGap) return axt_bad_gap();
    if (st & kAxtBadOut)
        return gac_fail(GAC_E_ARG, "gac_axt_render: a piece's rows do not fit out_bytes (%lld)",
                        (long long)out_bytes);
    if (n && !d_out) return gac_fail(GAC_E_ARG, "NULL buffer");
    HIPCHK(launch_axt_render(a, s));
    return GAC_OK;
}

#define AXT_ENTRY(c, cs)                                                                   \
    gac_clear_error();                                                                     \
    if (!(c)) return gac_fail(GAC_E_ARG, "NULL context");                                  \
    if (!(cs) || (cs)->ctx != (c)) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset"); \
    CTX_LOCK(c);                                                                           \
    HIPCHK(hipSetDevice((c)->device));                                                     \
    if (!(c)->axt) (c)->axt = new AxtWs()

// The entry points; clip: the _clip forms, which read t_start / t_end.
static int axt_measure_device_x(gac_ctx *c, const gac_chainset *cs, const gac_window *d_pieces,
                                int64_t n, int32_t *d_score, int64_t *d_match, int64_t *d_ali,
                                int64_t *d_sym, void *stream, bool clip) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && (!d_pieces || !d_score || !d_match || !d_ali || !d_sym))
        return gac_fail(GAC_E_ARG, "NULL buffer");
    return axt_measure_dev(c, cs, *c->axt, nullptr, d_pieces, n, d_score, d_match, d_ali, d_sym,
                           false, clip, stream ? (hipStream_t)stream : c->stream);
}

static int axt_measure_x(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                         int32_t *score, int64_t *match, int64_t *ali, int64_t *sym, bool clip) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && (!pieces || !score || !match || !ali || !sym))
        return gac_fail(GAC_E_ARG, "NULL buffer");
    hipStream_t s = c->stream;
    int rc = axt_measure_dev(c, cs, *c->axt, pieces, nullptr, n, nullptr, nullptr, nullptr, nullptr,
                             true, clip, s);
    if (rc != GAC_OK) return rc;
    const char *p = c->axt->a2.p + up16((size_t)n * 32);
    const size_t b = up16((size_t)n * 8);
    HIPCHK(hipMemcpyAsync(score, p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(match, p + b, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ali, p + 2 * b, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sym, p + 3 * b, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return GAC_OK;
}

static int axt_render_device_x(gac_ctx *c, const gac_chainset *cs, const gac_window *d_pieces,
                               int64_t n, const int64_t *d_offsets, char *d_out, int64_t out_bytes,
                               void *stream, bool clip) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && !d_pieces) return gac_fail(GAC_E_ARG, "NULL buffer");
    return axt_render_dev(c, cs, *c->axt, nullptr, d_pieces, n, nullptr, d_offsets, d_out, out_bytes,
                          clip, stream ? (hipStream_t)stream : c->stream);
}

static int axt_render_x(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces, int64_t n,
                        const int64_t *offsets, char *out, int64_t out_bytes, bool clip) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && (!pieces || !out)) return gac_fail(GAC_E_ARG, "NULL buffer");
    if (out_bytes < 0) return gac_fail(GAC_E_ARG, "gac_axt_render: negative out_bytes");
    hipStream_t s = c->stream;
    AxtWs &ws = *c->axt;
    // the caller's buffer goes to the device and comes back, so that the
    // bytes between the pieces' rows stay what they were
    HIPCHK(arena_need(ws.text, (size_t)out_bytes + 16, s));
    HIPCHK(hipMemcpyAsync(ws.text.p, out, (size_t)out_bytes, hipMemcpyHostToDevice, s));
    int rc = axt_render_dev(c, cs, ws, pieces, nullptr, n, offsets, nullptr, ws.text.p, out_bytes,
                            clip, s);
    if (rc != GAC_OK) {
        hipStreamSynchronize(s);
        return rc;
    }
    HIPCHK(hipMemcpyAsync(out, ws.text.p, (size_t)out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return GAC_OK;
}

extern "C" int gac_axt_measure_device(gac_ctx *c, const gac_chainset *cs, const gac_window *d_pieces,
                                      int64_t n, int32_t *d_score, int64_t *d_match,
                                      int64_t *d_ali, int64_t *d_sym, void *stream) {
    return axt_measure_device_x(c, cs, d_pieces, n, d_score, d_match, d_ali, d_sym, stream, false);
}

extern "C" int gac_axt_measure_clip_device(gac_ctx *c, const gac_chainset *cs,
                                           const gac_window *d_pieces, int64_t n, int32_t *d_score,
                                           int64_t *d_match, int64_t *d_ali, int64_t *d_sym,
                                           void *stream) {
    return axt_measure_device_x(c, cs, d_pieces, n, d_score, d_match, d_ali, d_sym, stream, true);
}

extern "C" int gac_axt_measure(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces,
                               int64_t n, int32_t *score, int64_t *match, int64_t *ali,
                               int64_t *sym) {
    return axt_measure_x(c, cs, pieces, n, score, match, ali, sym, false);
}

extern "C" int gac_axt_measure_clip(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces,
                                    int64_t n, int32_t *score, int64_t *match, int64_t *ali,
                                    int64_t *sym) {
    return axt_measure_x(c, cs, pieces, n, score, match, ali, sym, true);
}

// Letter-pair counts (lavToAxt -dropSelf): the plan step of measure, then
// k_axt_pairs adding into the zeroed result arrays.
static int axt_pairs_dev(gac_ctx *c, const gac_chainset *cs, AxtWs &ws, const gac_window *h_pieces,
                         const gac_window *d_pieces, int64_t n, int64_t *d_pairs, int64_t *d_ncols,
                         bool own_out, hipStream_t s) {
    AxtPairArgs a;
    int rc = axt_plan(c, cs, ws, h_pieces, d_pieces, n, false, s, a);
    if (rc != GAC_OK) return rc;
    if (own_out) {  // the host entry point's results: pairs, then ncols
        HIPCHK(arena_need(ws.a2, (size_t)n * 17 * 8, s));
        d_pairs = (int64_t *)ws.a2.p;
        d_ncols = d_pairs + n * 16;
    }
    a.pairs = (unsigned long long *)d_pairs;
    a.ncols = (unsigned long long *)d_ncols;
    HIPCHK(hipMemsetAsync(d_pairs, 0, (size_t)n * 16 * 8, s));
    HIPCHK(hipMemsetAsync(d_ncols, 0, (size_t)n * 8, s));
    HIPCHK(launch_axt_pairs(a, s));
    int32_t st = 0;
    rc = axt_status(ws, a, s, &st);
    if (rc != GAC_OK) return rc;
    if (st & kAxtBadGap) return axt_bad_gap();
    return GAC_OK;
}

extern "C" int gac_axt_pair_counts_device(gac_ctx *c, const gac_chainset *cs,
                                          const gac_window *d_pieces, int64_t n, int64_t *d_pairs,
                                          int64_t *d_n_cols, void *stream) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && (!d_pieces || !d_pairs || !d_n_cols)) return gac_fail(GAC_E_ARG, "NULL buffer");
    return axt_pairs_dev(c, cs, *c->axt, nullptr, d_pieces, n, d_pairs, d_n_cols, false,
                         stream ? (hipStream_t)stream : c->stream);
}

extern "C" int gac_axt_pair_counts(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces,
                                   int64_t n, int64_t *pairs, int64_t *n_cols) {
    AXT_ENTRY(c, cs);
    if (n == 0) return GAC_OK;
    if (n > 0 && (!pieces || !pairs || !n_cols)) return gac_fail(GAC_E_ARG, "NULL buffer");
    hipStream_t s = c->stream;
    int rc = axt_pairs_dev(c, cs, *c->axt, pieces, nullptr, n, nullptr, nullptr, true, s);
    if (rc != GAC_OK) return rc;
    const int64_t *p = (const int64_t *)c->axt->a2.p;
    HIPCHK(hipMemcpyAsync(pairs, p, (size_t)n * 16 * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(n_cols, p + n * 16, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return GAC_OK;
}

extern "C" int gac_axt_render_device(gac_ctx *c, const gac_chainset *cs, const gac_window *d_pieces,
                                     int64_t n, const int64_t *d_offsets, char *d_out,
                                     int64_t out_bytes, void *stream) {
    return axt_render_device_x(c, cs, d_pieces, n, d_offsets, d_out, out_bytes, stream, false);
}

extern "C" int gac_axt_render_clip_device(gac_ctx *c, const gac_chainset *cs,
                                          const gac_window *d_pieces, int64_t n,
                                          const int64_t *d_offsets, char *d_out, int64_t out_bytes,
                                          void *stream) {
    return axt_render_device_x(c, cs, d_pieces, n, d_offsets, d_out, out_bytes, stream, true);
}

extern "C" int gac_axt_render(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces,
                              int64_t n, const int64_t *offsets, char *out, int64_t out_bytes) {
    return axt_render_x(c, cs, pieces, n, offsets, out, out_bytes, false);
}

extern "C" int gac_axt_render_clip(gac_ctx *c, const gac_chainset *cs, const gac_window *pieces,
                                   int64_t n, const int64_t *offsets, char *out, int64_t out_bytes) {
    return axt_render_x(c, cs, pieces, n, offsets, out, out_bytes, true);
}

// Ranges to clipped pieces.  Two host waits: for V (the selected blocks, which
// size the flag array and its kernels) and for P (which sizes the result).
extern "C" int gac_axt_cut(gac_ctx *c, const gac_chainset *cs, const gac_range *ranges, int64_t n,
                           int32_t max_gap, gac_window **pieces, int64_t **first,
                           int64_t *n_pieces) {
    if (pieces) *pieces = nullptr;
    if (first) *first = nullptr;
    if (n_pieces) *n_pieces = 0;
    AXT_ENTRY(c, cs);
    if (!pieces || !first || !n_pieces || n < 0 || n >= INT32_MAX || (n > 0 && !ranges))
        return gac_fail(GAC_E_ARG, "gac_axt_cut: bad argument");
    AxtWs &ws = *c->axt;
    hipStream_t s = c->stream;
    if (!ws.h) HIPCHK(hipHostMalloc((void **)&ws.h, 64, hipHostMallocDefault));
    const size_t b_rg = up16((size_t)n * sizeof(Range)), b_rf = up16((size_t)n * 4);
    const size_t b_rboff = up16((size_t)(n + 1) * 8), b_first = b_rboff;
    HIPCHK(arena_need(ws.a1, b_rg + b_rf + b_rboff + b_first + 16, s));
    AxtCutArgs a;
    memset(&a, 0, sizeof(a));
    a.chains = cs->chains;
    a.blk = cs->blk;
    a.n_chains = cs->n_chains;
    a.n = n;
    a.max_gap = max_gap;
    char *p = ws.a1.p;
    a.ranges = (const Range *)p;
    p += b_rg;
    a.rfirst = (int32_t *)p;
    p += b_rf;
    a.rboff = (int64_t *)p;
    p += b_rboff;
    a.first = (int64_t *)p;
    p += b_first;
    a.status = (int32_t *)p;
    // the scans' workgroup totals, first for n and then for V elements, lie in a2
    HIPCHK(arena_need(ws.a2, up16((size_t)(n / 2048 + 2) * 8), s));
    a.part = (int64_t *)ws.a2.p;
    if (n)
        HIPCHK(hipMemcpyAsync((void *)a.ranges, ranges, (size_t)n * sizeof(Range),
                              hipMemcpyHostToDevice, s));
    ws.h[2] = INT32_MAX;
    ws.h[2] <<= 32;  // status[0] = 0, status[1] = INT32_MAX
    HIPCHK(hipMemcpyAsync(a.status, &ws.h[2], 8, hipMemcpyHostToDevice, s));
    HIPCHK(launch_axt_cut_find(a, s));
    HIPCHK(hipMemcpyAsync(&ws.h[0], a.rboff + n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&ws.h[1], a.status, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    a.V = ws.h[0];
    if ((int32_t)ws.h[1] & kAxtBadWindow)
        return gac_fail(GAC_E_ARG, "gac_axt_cut: a range's chain index is out of range");
    const size_t b_pidx = up16((size_t)(a.V + 2) * 8), b_part = up16((size_t)(a.V / 2048 + 2) * 8);
    HIPCHK(arena_need(ws.a2, b_pidx + b_part, s));
    a.pidx = (int64_t *)ws.a2.p;
    a.part = (int64_t *)(ws.a2.p + b_pidx);
    HIPCHK(launch_axt_cut_flag(a, s));
    HIPCHK(hipMemcpyAsync(&ws.h[0], a.pidx + a.V, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&ws.h[1], a.status, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    a.P = ws.h[0];
    if ((int32_t)ws.h[1] & kAxtBadGap) {
        const int64_t r = ws.h[1] >> 32;
        return gac_fail(GAC_E_FORMAT, "chain %d: negative gap between two blocks of range %lld "
                                      "[%d, %d)", (int)ranges[r].chain, (long long)r,
                        (int)ranges[r].t_start, (int)ranges[r].t_end);
    }
    // one allocation for the caller: the pieces, then first[0 .. n] (8-byte aligned)
    const size_t b_pc = ((size_t)a.P * sizeof(Window) + 7) & ~(size_t)7;
    HIPCHK(arena_need(ws.text, (size_t)a.P * sizeof(Window) + 16, s));
    a.pieces = (Window *)ws.text.p;
    char *res = (char *)malloc(b_pc + (size_t)(n + 1) * 8 + 8);
    if (!res) return gac_fail(GAC_E_ARG, "gac_axt_cut: out of memory");
    hipError_t e = launch_axt_cut_emit(a, s);
    if (e == hipSuccess && a.P)
        e = hipMemcpyAsync(res, a.pieces, (size_t)a.P * sizeof(Window), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(res + b_pc, a.first, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        free(res);
        HIPCHK(e);
    }
    *pieces = (gac_window *)res;
    *first = (int64_t *)(res + b_pc);
    *n_pieces = a.P;
    return GAC_OK;
}

// A render in flight (chainToAxt's batches): its own stream, workspace,
// device text and pinned host text, so that two jobs alternate -- the host
// formats one batch while the next is rendered and copied.
struct gac_axt_job {
    gac_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    AxtWs ws;
    char *h_text = nullptr;  // pinned
    int64_t cap = 0, bytes = 0;
};

static void job_release(gac_axt_job *j) {
    if (j->st) {
        hipStreamSynchronize(j->st);
        hipStreamDestroy(j->st);
    }
    j->st = nullptr;
    ws_free(j->ws);
    if (j->h_text) hipHostFree(j->h_text);
    j->h_text = nullptr;
    j->cap = 0;
}

void gac::axt_release(gac_ctx *c) {
    for (gac_axt_job *j : c->axt_jobs) {
        job_release(j);
        j->ctx = nullptr;
    }
    c->axt_jobs.clear();
    if (c->axt) {
        ws_free(*c->axt);
        delete c->axt;
        c->axt = nullptr;
    }
}

static int job_text(gac_axt_job *j, int64_t bytes) {
    if (bytes <= j->cap) return GAC_OK;
    HIPCHK(hipStreamSynchronize(j->st));
    if (j->h_text) hipHostFree(j->h_text);
    j->h_text = nullptr;
    j->cap = 0;
    HIPCHK(hipHostMalloc((void **)&j->h_text, (size_t)bytes, hipHostMallocDefault));
    j->cap = bytes;
    return arena_need(j->ws.text, (size_t)bytes + 16, j->st) == hipSuccess
               ? GAC_OK
               : gac_fail(GAC_E_HIP, "gac_axt_job: no device memory for %lld text bytes",
                          (long long)bytes);
}

extern "C" int gac_axt_job_open(gac_ctx *c, int64_t text_bytes, gac_axt_job **out) {
    gac_clear_error();
    if (!c || !out || text_bytes < 0) return gac_fail(GAC_E_ARG, "gac_axt_job_open: bad argument");
    *out = nullptr;
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    gac_axt_job *j = new gac_axt_job();
    j->ctx = c;
    c->axt_jobs.push_back(j);
    int rc = GAC_OK;
    if (hipStreamCreateWithFlags(&j->st, hipStreamNonBlocking) != hipSuccess)
        rc = gac_fail(GAC_E_HIP, "gac_axt_job_open: no stream");
    if (rc == GAC_OK) rc = job_text(j, text_bytes > 0 ? text_bytes : 1);
    if (rc != GAC_OK) {
        gac_axt_job_close(j);
        return rc;
    }
    *out = j;
    return GAC_OK;
}

static int axt_job_submit_x(gac_axt_job *j, const gac_chainset *cs, const gac_window *pieces,
                            int64_t n, const int64_t *offsets, int64_t bytes, bool clip) {
    gac_clear_error();
    if (!j || !j->ctx) return gac_fail(GAC_E_ARG, "NULL or orphaned job");
    gac_ctx *c = j->ctx;
    if (!cs || cs->ctx != c) return gac_fail(GAC_E_ARG, "NULL or orphaned chainset");
    if (bytes < 0 || n < 0 || (n > 0 && (!pieces || !offsets)))
        return gac_fail(GAC_E_ARG, "gac_axt_job_submit: bad argument");
    CTX_LOCK(c);
    HIPCHK(hipSetDevice(c->device));
    j->bytes = 0;
    if (n == 0 || bytes == 0) return GAC_OK;
    int rc = job_text(j, bytes);
    if (rc != GAC_OK) return rc;
    rc = axt_render_dev(c, cs, j->ws, pieces, nullptr, n, offsets, nullptr, j->ws.text.p, bytes, clip,
                        j->st);
    if (rc != GAC_OK) return rc;
    HIPCHK(hipMemcpyAsync(j->h_text, j->ws.text.p, (size_t)bytes, hipMemcpyDeviceToHost, j->st));
    j->bytes = bytes;
    return GAC_OK;
}

extern "C" int gac_axt_job_submit(gac_axt_job *j, const gac_chainset *cs, const gac_window *pieces,
                                  int64_t n, const int64_t *offsets, int64_t bytes) {
    return axt_job_submit_x(j, cs, pieces, n, offsets, bytes, false);
}

extern "C" int gac_axt_job_submit_clip(gac_axt_job *j, const gac_chainset *cs,
                                       const gac_window *pieces, int64_t n, const int64_t *offsets,
                                       int64_t bytes) {
    return axt_job_submit_x(j, cs, pieces, n, offsets, bytes, true);
}

extern "C" int gac_axt_job_wait(gac_axt_job *j, const char **text, int64_t *bytes) {
    gac_clear_error();
    if (!j || !j->ctx || !text) return gac_fail(GAC_E_ARG, "NULL or orphaned job");
    HIPCHK(hipSetDevice(j->ctx->device));
    HIPCHK(hipStreamSynchronize(j->st));  // (no context lock: the other job may be submitting)
    *text = j->h_text;
    if (bytes) *bytes = j->bytes;
    return GAC_OK;
}

extern "C" void gac_axt_job_close(gac_axt_job *j) {
    if (!j) return;
    if (gac_ctx *c = j->ctx) {
        CTX_LOCK(c);
        hipSetDevice(c->device);
        job_release(j);
        c->axt_jobs.erase(std::remove(c->axt_jobs.begin(), c->axt_jobs.end(), j), c->axt_jobs.end());
    }
    delete j;
}
