"""Python host mirror of the reference's chain-scoring interface, on top of
the libgachain C ABI (include/gachain.h).

Reference interface                          here
-------------------------------------------  --------------------------------
gapCalcFromFile (gapCalc.c:233-255)          GapCosts(name_or_file)
axtScoreSchemeRead/Default (axt.c:423,692)   read_score_scheme(path | None)
twoBitOpen + twoBitReadSeqFrag (twoBit.c)    Engine.load_2bit(side, path)
chainRead loop (chain.c:337)                 chainfile.read_chains -> Engine.upload_chains
chainSubsetOnT + chainCalcScore (+ local)    Engine.score_ranges(chainset, ranges)
scoreChain getChainScore (scoreChain.c:207)  Engine.score_chains(chainset) (gac_score_chains)
twoBitReadSeqFragExt(doMask) (twoBit.c:835)  Engine.load_2bit(..., soft_mask=True), decode_case
chainAntiRepeat's two filters' counts        Engine.chain_composition(chainset)
  (chainAntiRepeat.c:40-117) and decision    antirepeat_pass(score, match, rep, total, minScore)
chainToPsl's four counts (chainToPsl.c:106)  Engine.chain_psl_counts(chainset)
netSyntenic's dupeTree (netSyntenic.c:63)    Engine.depth_count(seq, start, end, delta, threshold)
                                             depth_count_host(...): the same on the CPU
chainPreNet's chainUsed (chainPreNet.c:104)  Engine.prenet_keep(blk_off, t_seq, q_seq, ...)
                                             prenet_keep_host(...): the reference's own pass
filterAxtIdentityEntropy.py's checkAxt (:88) Engine.axt_filter(t_rows, q_rows, ident, entropy, W)
                                             axt_filter_host(...): the same on host threads
pslFromAlign's column loop (psl.c:1716)      Engine.axt_psl(t_rows, q_rows)
                                             axt_psl_host(...): the same on host threads
axtScoreSym, default scheme (axt.c:196)      Engine.axt_score(t_rows, q_rows)
                                             axt_score_host(...): the same on host threads
axtScoreSym, any scheme (lavToAxt -dropSelf) Engine.axt_pair_counts(cs, pieces): letter-pair counts a piece
                                             axt_pair_counts_host(...): the same from two .2bit files
axtScoreUngapped per block (axt.c:186-194)   Engine.score_blocks / score_text_blocks (caller text)
cBlockFindCrossover (chainConnect.c:61-105)  Engine.crossovers / text_crossovers (caller text)
chainBlocks' kd-tree DP (chainBlock.c:400)   Engine.chain_dp_blocks (total, predecessor per block)

Every scoring call runs on the GPU through libgachain; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import GAC_Q, GAC_T, GAC_WANT_LOCAL, ChainsetDesc, GapCalc, check, lib


def _p(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


class GapCosts:
    """Piecewise-linear gap costs (struct gapCalc)."""

    def __init__(self, name_or_file: str = "loose"):
        self._ptr = C.POINTER(GapCalc)()
        check(lib().gac_gapcalc_build(name_or_file.encode(), C.byref(self._ptr)))
        self.name = name_or_file

    @property
    def ptr(self):
        return self._ptr

    def cost(self, dq: int, dt: int) -> int:
        """gapCalcCost on the host (gac_gap_cost)."""
        return int(lib().gac_gap_cost(self._ptr, int(dq), int(dt)))

    def tables(self):
        g = self._ptr.contents
        n, m = g.small_size, g.long_count
        return {
            "small_size": n,
            "q_small": np.ctypeslib.as_array(g.q_small, (n,)).copy(),
            "t_small": np.ctypeslib.as_array(g.t_small, (n,)).copy(),
            "b_small": np.ctypeslib.as_array(g.b_small, (n,)).copy(),
            "long_pos": np.ctypeslib.as_array(g.long_pos, (m,)).copy(),
        }

    def __del__(self):
        try:
            if self._ptr:
                lib().gac_gapcalc_free(self._ptr)
        except Exception:
            pass


def read_score_scheme(path: Optional[str] = None) -> Tuple[np.ndarray, int, int, str]:
    """Returns (mat[4,4] int32 [query][target] in A,C,G,T order, gapOpen,
    gapExtend, extra)."""
    mat = (C.c_int32 * 16)()
    go, ge = C.c_int32(), C.c_int32()
    extra = C.c_void_p()
    check(lib().gac_scheme_read(path.encode() if path else None, mat, C.byref(go),
                                C.byref(ge), C.byref(extra)))
    ex = ""
    if extra.value:
        ex = C.string_at(extra.value).decode()
        C.CDLL(None).free(extra)
    return np.array(mat[:], dtype=np.int32).reshape(4, 4), go.value, ge.value, ex


class ChainSet:
    def __init__(self, engine: "Engine", handle: C.c_void_p, n_chains: int, n_blocks: int,
                 aligned_bases: int):
        self.engine = engine
        self.handle = handle
        self.n_chains = n_chains
        self.n_blocks = n_blocks
        self.aligned_bases = aligned_bases

    def close(self):
        if self.handle:
            lib().gac_chains_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One libgachain context on one MI355X (gfx950) device."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib().gac_open(device, C.byref(h)))
        self.h = h
        self.device = device

    @property
    def arch(self) -> str:
        return lib().gac_device_arch(self.h).decode()

    def close(self):
        if self.h:
            lib().gac_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- scoring scheme
    def set_scoring(self, mat: np.ndarray, gap: GapCosts) -> None:
        m = np.ascontiguousarray(np.asarray(mat, dtype=np.int32).reshape(16))
        check(lib().gac_set_scoring(self.h, m.ctypes.data_as(C.POINTER(C.c_int32)), gap.ptr))
        self._gap = gap

    # ---- genomes
    def load_2bit(self, side: int, path: str, soft_mask: bool = False, keep=None,
                  runs=None) -> None:
        """soft_mask: also keep the file's mask runs as the soft-mask plane
        (chain_composition, decode_case); off, the load is unchanged.
        keep: one flag per sequence of the file, false = not loaded.
        runs: the sparse upload (gac_genome_load_2bit_runs) -- per sequence of
        the file a list of (lo, hi) word runs, 32 bases per word; only these
        words of the planes are uploaded."""
        if soft_mask:
            check(lib().gac_genome_want_softmask(self.h, side))
        if keep is None and runs is None:
            check(lib().gac_genome_load_2bit(self.h, side, path.encode()))
            return
        k = None if keep is None else np.ascontiguousarray(np.asarray(keep, bool), np.uint8)
        off = lo = hi = None
        if runs is not None:
            off = np.zeros(len(runs) + 1, np.int64)
            off[1:] = np.cumsum([len(r) for r in runs])
            flat = np.asarray([x for r in runs for x in r], np.int64).reshape(-1, 2)
            flat = np.concatenate([flat, np.zeros((1, 2), np.int64)])  # (never NULL)
            lo = np.ascontiguousarray(flat[:, 0], np.int32)
            hi = np.ascontiguousarray(flat[:, 1], np.int32)
        check(lib().gac_genome_load_2bit_runs(
            self.h, side, path.encode(), _p(k) if k is not None else None,
            _p(off) if off is not None else None, _p(lo) if lo is not None else None,
            _p(hi) if hi is not None else None))

    def genome_planes(self, side: int):
        """The resident arrays of a finalized side copied back
        (gac_genome_planes): (planes uint32 [n + 4, 2] {bit-0, bit-1 plane},
        nmask uint32 [n + 4], lmask uint32 [n + 4] or None), n the side's word
        count; the four trailing words are the padding scoring windows read."""
        pl, nm, lm = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_int64()
        check(lib().gac_genome_planes(self.h, side, C.byref(pl), C.byref(nm), C.byref(lm),
                                      C.byref(n)))
        m = n.value + 4
        planes = np.zeros((m, 2), np.uint32)
        nmask = np.zeros(m, np.uint32)
        self.d2h(planes, pl.value)
        self.d2h(nmask, nm.value)
        lmask = None
        if lm.value:
            lmask = np.zeros(m, np.uint32)
            self.d2h(lmask, lm.value)
        return planes, nmask, lmask

    def add_sequences(self, side: int, seqs: Iterable, mask_runs=None) -> None:
        """seqs: iterable of (name, size, packed uint8 .2bit payload, n_starts, n_sizes).
        mask_runs: per sequence (starts, sizes) of its soft-mask runs (e.g.
        synth.Genome.mruns): the side is loaded with the soft-mask plane."""
        if mask_runs is not None:
            check(lib().gac_genome_want_softmask(self.h, side))
        for i, (name, size, packed, ns, nz) in enumerate(seqs):
            packed = np.ascontiguousarray(packed, dtype=np.uint8)
            ns = np.ascontiguousarray(ns, dtype=np.int32)
            nz = np.ascontiguousarray(nz, dtype=np.int32)
            if mask_runs is None:
                check(lib().gac_genome_add_seq(self.h, side, name.encode(), int(size),
                                               _p(packed), len(ns), _p(ns), _p(nz)))
                continue
            ms = np.ascontiguousarray(mask_runs[i][0], dtype=np.int32)
            mz = np.ascontiguousarray(mask_runs[i][1], dtype=np.int32)
            check(lib().gac_genome_add_seq_masked(self.h, side, name.encode(), int(size),
                                                  _p(packed), len(ns), _p(ns), _p(nz),
                                                  len(ms), _p(ms), _p(mz)))
        check(lib().gac_genome_finalize(self.h, side))

    def decode_case(self, side: int, idx: int, start: int, end: int) -> str:
        """'ACGTN' / 'acgtn' inside mask runs, as twoBitReadSeqFragExt(doMask=TRUE)."""
        buf = C.create_string_buffer(max(end - start, 1))
        check(lib().gac_genome_decode_case(self.h, side, idx, start, end, buf))
        return buf.raw[: end - start].decode()

    def chain_composition(self, cs: "ChainSet"):
        """chainAntiRepeat's counts of every chain of the set (gac_chain_composition):
        (match int64 [n, 4] by code T, C, A, G; rep int64 [n]; total int64 [n])."""
        n = cs.n_chains
        match = np.zeros((n, 4), np.int64)
        rep = np.zeros(n, np.int64)
        total = np.zeros(n, np.int64)
        check(lib().gac_chain_composition(self.h, cs.handle, _p(match), _p(rep), _p(total)))
        return match, rep, total

    def chain_composition_device(self, cs: "ChainSet", d_match: int, d_rep: int, d_total: int,
                                 stream: int = 0) -> None:
        check(lib().gac_chain_composition_device(
            self.h, cs.handle, C.c_void_p(d_match), C.c_void_p(d_rep), C.c_void_p(d_total),
            C.c_void_p(stream) if stream else None))

    def chain_psl_counts(self, cs: "ChainSet") -> np.ndarray:
        """chainToPsl's counts of every chain of the set (gac_chain_psl_counts):
        int64 [n, 4], columns match, misMatch, repMatch, nCount.  The target
        side must hold the soft-mask plane; '-' block coordinates unshifted."""
        counts = np.zeros((cs.n_chains, 4), np.int64)
        check(lib().gac_chain_psl_counts(self.h, cs.handle, _p(counts)))
        return counts

    def chain_psl_counts_device(self, cs: "ChainSet", d_counts: int, stream: int = 0) -> None:
        check(lib().gac_chain_psl_counts_device(
            self.h, cs.handle, C.c_void_p(d_counts), C.c_void_p(stream) if stream else None))

    # ---- coverage depth (netSyntenic)
    def depth_count(self, seq, start, end, delta, threshold: int = 2) -> np.ndarray:
        """Per range [start, end) of sequence seq: the positions whose summed
        depth (delta of every range of that sequence covering them) is >=
        threshold (gac_depth_count): int32 [n].  netSyntenic's qDup with
        delta +1 for fills, -1 for gaps, threshold 2."""
        a = _depth_args(seq, start, end, delta)
        count = np.zeros(len(a[0]), np.int32)
        check(lib().gac_depth_count(self.h, len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]),
                                    int(threshold), _p(count)))
        return count

    # ---- chains worth netting (chainPreNet)
    def prenet_keep(self, blk_off, t_seq, q_seq, blk_t, blk_q, blk_size, t_sizes, q_sizes,
                    pad: int = 1, max_rounds: int = _lib.GAC_PRENET_MAX_ROUNDS):
        """Which chains chainPreNet writes (gac_prenet_keep): chains in file
        order with their block offsets [n + 1] and target / query sequence
        numbers (-1: skipped), blocks with their raw target and query starts
        and sizes, the sequence sizes per side.  Returns (keep uint8 [n],
        stats): rounds, passes, groups (target, query), fell_back, kept."""
        a = _prenet_args(blk_off, t_seq, q_seq, blk_t, blk_q, blk_size, t_sizes, q_sizes)
        keep = np.zeros(len(a[1]), np.uint8)
        st = _lib.PrenetStats()
        check(lib().gac_prenet_keep(self.h, len(a[1]), _p(a[0]), _p(a[1]), _p(a[2]), len(a[3]),
                                    _p(a[3]), _p(a[4]), _p(a[5]), len(a[6]), _p(a[6]), len(a[7]),
                                    _p(a[7]), int(pad), int(max_rounds), _p(keep), C.byref(st)))
        return keep, _prenet_stats(st)

    # ---- alignments worth chaining (filterAxtIdentityEntropy.py)
    def axt_filter(self, t_rows, q_rows, min_ident: float, min_entropy: float, window: int):
        """Which alignments filterAxtIdentityEntropy.py writes (gac_axt_filter):
        t_rows and q_rows are the target and query rows of the entries (bytes
        or str; a target row may be longer than its query row, whose length
        counts).  Returns (keep uint8 [n], stats): kept, windows,
        host_entries, batches, fell_back."""
        text, t_off, q_off, ln = _axt_filter_args(t_rows, q_rows)
        keep = np.zeros(len(ln), np.uint8)
        st = _lib.AxtFilterStats()
        check(lib().gac_axt_filter(self.h, len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                   float(min_ident), float(min_entropy), int(window), _p(keep),
                                   C.byref(st)))
        return keep, _axt_filter_stats(st)

    # ---- alignments to PSL blocks (axtToPsl)
    def axt_psl(self, t_rows, q_rows):
        """What pslFromAlign makes of alignments' rows (gac_axt_psl): t_rows
        and q_rows are the target and query rows of the entries (bytes or str,
        of equal length).  Returns (entries, blocks, stats): entries a
        structured array [n] with the fields of gac_axtpsl_entry (the eight
        counts, q_head, t_head, q_tail, t_tail, cols, n_blocks, block0),
        blocks int32 [n_blocks, 3] of (q_adv, t_adv, size), stats: blocks,
        columns, host_entries, batches, fell_back."""
        text, t_off, q_off, ln = _axt_psl_args(t_rows, q_rows)
        res = C.POINTER(_lib.AxtPslResult)()
        st = _lib.AxtPslStats()
        check(lib().gac_axt_psl(self.h, len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                C.byref(res), C.byref(st)))
        return _axt_psl_result(res, st)

    # ---- alignments to blastz scores (axtToMaf -score)
    def axt_score(self, t_rows, q_rows):
        """axtScoreDnaDefault of alignments' rows (gac_axt_score): t_rows and
        q_rows as for axt_psl.  Returns (scores, stats): scores int32 [n],
        stats: columns, host_entries, batches, fell_back."""
        text, t_off, q_off, ln = _axt_psl_args(t_rows, q_rows, "axt_score")
        score = np.zeros(len(ln), np.int32)
        st = _lib.AxtScoreStats()
        check(lib().gac_axt_score(self.h, len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                  _p(score), C.byref(st)))
        return score, _axt_score_stats(st)

    # ---- alignment text (chainToAxt)
    @staticmethod
    def axt_split(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size,
                  max_gap: int = 100) -> np.ndarray:
        """chainToAxt's pieces of parsed chains (gac_axt_split; host only, no
        device: callable on the class): int32 [n, 5] gac_window rows (chain,
        tStart, tEnd, first block, blocks)."""
        d, _arrs = Engine._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
        p = C.c_void_p()
        n = C.c_int64()
        check(lib().gac_axt_split(C.byref(d), int(max_gap), C.byref(p), C.byref(n)))
        try:
            out = np.zeros((n.value, 5), np.int32)
            if n.value:
                C.memmove(_p(out), p, n.value * 20)
        finally:
            lib().gac_axt_free(p)
        return out

    def axt_cut(self, cs: "ChainSet", ranges: np.ndarray, max_gap: int = 100):
        """netToAxt's clipped pieces of sub-chain ranges (gac_axt_cut).  ranges:
        int32 [n, 3] (chain, tStart, tEnd).  Returns (pieces int32 [P, 5] with
        the clipped tStart / tEnd, first int64 [n + 1]): range r's pieces are
        pieces[first[r]:first[r + 1]]."""
        rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 3))
        n = rg.shape[0]
        p, f = C.c_void_p(), C.c_void_p()
        m = C.c_int64()
        check(lib().gac_axt_cut(self.h, cs.handle, _p(rg), n, int(max_gap), C.byref(p), C.byref(f),
                                C.byref(m)))
        try:
            pieces = np.zeros((m.value, 5), np.int32)
            first = np.zeros(n + 1, np.int64)
            if m.value:
                C.memmove(_p(pieces), p, m.value * 20)
            C.memmove(_p(first), f, (n + 1) * 8)
        finally:
            lib().gac_axt_free(p)  # (one allocation: first goes with it)
        return pieces, first

    def axt_measure(self, cs: "ChainSet", pieces: np.ndarray, clip: bool = False):
        """(score int32, match, ali, sym int64) of every piece (gac_axt_measure;
        clip: gac_axt_measure_clip, which reads the pieces' tStart / tEnd)."""
        w = np.ascontiguousarray(np.asarray(pieces, dtype=np.int32).reshape(-1, 5))
        n = w.shape[0]
        score = np.zeros(n, np.int32)
        match, ali, sym = (np.zeros(n, np.int64) for _ in range(3))
        fn = lib().gac_axt_measure_clip if clip else lib().gac_axt_measure
        check(fn(self.h, cs.handle, _p(w), n, _p(score), _p(match), _p(ali), _p(sym)))
        return score, match, ali, sym

    def axt_measure_device(self, cs: "ChainSet", d_pieces: int, n: int, d_score: int, d_match: int,
                           d_ali: int, d_sym: int, stream: int = 0, clip: bool = False) -> None:
        fn = lib().gac_axt_measure_clip_device if clip else lib().gac_axt_measure_device
        check(fn(
            self.h, cs.handle, C.c_void_p(d_pieces), n, C.c_void_p(d_score), C.c_void_p(d_match),
            C.c_void_p(d_ali), C.c_void_p(d_sym), C.c_void_p(stream) if stream else None))

    def axt_pair_counts(self, cs: "ChainSet", pieces: np.ndarray):
        """(pairs int64 [n, 16], n_cols int64 [n]) of every piece
        (gac_axt_pair_counts): pairs[p, q * 4 + t] = ungapped columns with query
        letter q over target letter t (A, C, G, T as read_score_scheme's
        matrix), n_cols[p] = those with an N on either side."""
        w = np.ascontiguousarray(np.asarray(pieces, dtype=np.int32).reshape(-1, 5))
        n = w.shape[0]
        pairs = np.zeros((n, 16), np.int64)
        n_cols = np.zeros(n, np.int64)
        check(lib().gac_axt_pair_counts(self.h, cs.handle, _p(w), n, _p(pairs), _p(n_cols)))
        return pairs, n_cols

    def axt_pair_counts_device(self, cs: "ChainSet", d_pieces: int, n: int, d_pairs: int,
                               d_n_cols: int, stream: int = 0) -> None:
        check(lib().gac_axt_pair_counts_device(
            self.h, cs.handle, C.c_void_p(d_pieces), n, C.c_void_p(d_pairs), C.c_void_p(d_n_cols),
            C.c_void_p(stream) if stream else None))

    def axt_render(self, cs: "ChainSet", pieces: np.ndarray, offsets=None, out=None,
                   sym=None, clip: bool = False) -> np.ndarray:
        """The pieces' rows, tSym '\\n' qSym '\\n' '\\n' each (gac_axt_render), into
        the uint8 array `out` at byte `offsets` [n]; both None: packed in order
        into a new array (sym: the pieces' column counts, measured if None).
        clip: gac_axt_render_clip, which reads the pieces' tStart / tEnd."""
        w = np.ascontiguousarray(np.asarray(pieces, dtype=np.int32).reshape(-1, 5))
        n = w.shape[0]
        if out is None:
            if sym is None:
                sym = self.axt_measure(cs, w, clip=clip)[3]
            out = np.zeros(int((2 * np.asarray(sym, np.int64) + 3).sum()), np.uint8)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
        fn = lib().gac_axt_render_clip if clip else lib().gac_axt_render
        check(fn(self.h, cs.handle, _p(w), n, _p(off) if off is not None else None, _p(out), out.size))
        return out

    def axt_render_device(self, cs: "ChainSet", d_pieces: int, n: int, d_offsets: int, d_out: int,
                          out_bytes: int, stream: int = 0, clip: bool = False) -> None:
        fn = lib().gac_axt_render_clip_device if clip else lib().gac_axt_render_device
        check(fn(
            self.h, cs.handle, C.c_void_p(d_pieces), n, C.c_void_p(d_offsets) if d_offsets else None,
            C.c_void_p(d_out), out_bytes, C.c_void_p(stream) if stream else None))

    def seq_index(self, side: int, name: str) -> int:
        return lib().gac_genome_seq_index(self.h, side, name.encode())

    def seq_size(self, side: int, idx: int) -> int:
        return lib().gac_genome_seq_size(self.h, side, idx)

    def seq_count(self, side: int) -> int:
        return lib().gac_genome_seq_count(self.h, side)

    def decode(self, side: int, idx: int, start: int, end: int) -> str:
        buf = C.create_string_buffer(max(end - start, 1))
        check(lib().gac_genome_decode(self.h, side, idx, start, end, buf))
        return buf.raw[: end - start].decode()

    # ---- chains
    def upload_chains(self, ca) -> ChainSet:
        """Upload a chainfile.ChainArrays; sequences are resolved by name."""
        tidx = np.array([self.seq_index(GAC_T, n) for n in ca.tname], dtype=np.int32)
        qidx = np.array([self.seq_index(GAC_Q, n) for n in ca.qname], dtype=np.int32)
        if (tidx < 0).any() or (qidx < 0).any():
            bad = [n for n, i in zip(ca.tname, tidx) if i < 0] + \
                  [n for n, i in zip(ca.qname, qidx) if i < 0]
            raise KeyError(f"sequence(s) not loaded: {sorted(set(bad))[:5]}")
        return self.upload_chain_arrays(tidx, qidx, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q,
                                        ca.blk_size)

    @staticmethod
    def _desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size):
        """(gac_chainset_desc, the arrays it points into: keep them alive)"""
        arrs = [np.ascontiguousarray(t_seq, np.int32), np.ascontiguousarray(q_seq, np.int32),
                np.ascontiguousarray(q_strand, np.uint8), np.ascontiguousarray(blk_off, np.int64),
                np.ascontiguousarray(blk_t, np.int32), np.ascontiguousarray(blk_q, np.int32),
                np.ascontiguousarray(blk_size, np.int32)]
        d = ChainsetDesc()
        d.n_chains = len(arrs[0])
        d.t_seq, d.q_seq, d.q_strand, d.blk_off = (_p(a) for a in arrs[:4])
        d.n_blocks = len(arrs[4])
        d.blk_t, d.blk_q, d.blk_size = (_p(a) for a in arrs[4:])
        return d, arrs

    def upload_chain_arrays(self, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size) -> ChainSet:
        d, arrs = self._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
        h = C.c_void_p()
        check(lib().gac_chains_upload(self.h, C.byref(d), C.byref(h)))
        return ChainSet(self, h, d.n_chains, d.n_blocks, int(arrs[6].sum(dtype=np.int64)))

    def reupload_chain_arrays(self, cs: ChainSet, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q,
                              blk_size) -> ChainSet:
        """gac_chains_reupload: cs now holds these chains (its memory reused)."""
        d, arrs = self._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
        check(lib().gac_chains_reupload(self.h, C.byref(d), cs.handle))
        cs.n_chains, cs.n_blocks = d.n_chains, d.n_blocks
        cs.aligned_bases = int(arrs[6].sum(dtype=np.int64))
        return cs

    def score_ranges_host(self, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size,
                          ranges: np.ndarray, want_local: bool = False):
        """gac_score_ranges_host: ranges of chains held in host memory."""
        d, arrs = self._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 3))
        n = r.shape[0]
        g = np.zeros(n, np.int64)
        ali = np.zeros(n, np.int32)
        loc = np.zeros(n, np.int64) if want_local else None
        check(lib().gac_score_ranges_host(self.h, C.byref(d), _p(r), n,
                                          GAC_WANT_LOCAL if want_local else 0, _p(g),
                                          _p(loc) if want_local else None, _p(ali)))
        return g, loc, ali

    # ---- scoring
    def score_ranges(self, cs: ChainSet, ranges: np.ndarray, want_local: bool = False):
        """ranges: int32 [n, 3] (chain, tStart, tEnd).  Returns (global int64,
        local int64 or None, ali int32)."""
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int32).reshape(-1, 3))
        n = r.shape[0]
        g = np.zeros(n, np.int64)
        ali = np.zeros(n, np.int32)
        loc = np.zeros(n, np.int64) if want_local else None
        check(lib().gac_score_ranges(self.h, cs.handle, _p(r), n,
                                     GAC_WANT_LOCAL if want_local else 0, _p(g),
                                     _p(loc) if want_local else None, _p(ali)))
        return g, loc, ali

    def score_windows(self, cs: ChainSet, windows: np.ndarray, want_local: bool = False):
        """windows: int32 [n, 5] (chain, tStart, tEnd, first block, block count;
        gac_window).  Returns as score_ranges."""
        w = np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1, 5))
        n = w.shape[0]
        g = np.zeros(n, np.int64)
        ali = np.zeros(n, np.int32)
        loc = np.zeros(n, np.int64) if want_local else None
        check(lib().gac_score_windows(self.h, cs.handle, _p(w), n,
                                      GAC_WANT_LOCAL if want_local else 0, _p(g),
                                      _p(loc) if want_local else None, _p(ali)))
        return g, loc, ali

    def full_ranges(self, ca) -> np.ndarray:
        return np.stack([np.arange(ca.n, dtype=np.int32), ca.tstart.astype(np.int32),
                         ca.tend.astype(np.int32)], axis=1)

    def score_chains(self, cs: ChainSet, ca=None, want_local: bool = True):
        """scoreChain: global, local and aligned bases of every chain of the
        set, in order (gac_score_chains: the set's own plan, no ranges)."""
        n = cs.n_chains
        g = np.zeros(n, np.int64)
        ali = np.zeros(n, np.int32)
        loc = np.zeros(n, np.int64) if want_local else None
        check(lib().gac_score_chains(self.h, cs.handle, GAC_WANT_LOCAL if want_local else 0,
                                     _p(g), _p(loc) if want_local else None, _p(ali)))
        return g, loc, ali

    def score_chains_device(self, cs: ChainSet, d_g: int, d_ali: int, d_l: int = 0,
                            want_local: bool = False, stream: int = 0) -> None:
        check(lib().gac_score_chains_device(
            self.h, cs.handle, GAC_WANT_LOCAL if want_local else 0, C.c_void_p(d_g),
            C.c_void_p(d_l) if d_l else None, C.c_void_p(d_ali),
            C.c_void_p(stream) if stream else None))

    # ---- axtChain primitives
    def score_blocks(self, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size) -> np.ndarray:
        """axtScoreUngapped of every block (gac_score_blocks): int32 per block;
        pair p holds blocks [blk_off[p], blk_off[p+1])."""
        d, arrs = self._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
        score = np.zeros(d.n_blocks, np.int32)
        check(lib().gac_score_blocks(self.h, d.n_chains, d.t_seq, d.q_seq, d.q_strand, d.blk_off,
                                     d.blk_t, d.blk_q, d.blk_size, _p(score)))
        return score

    def crossovers(self, t_seq, q_seq, q_strand, lqe, lte, rqs, rts, overlap):
        """cBlockFindCrossover of n overlaps in genome coordinates
        (gac_crossovers): (pos int32, adj int32)."""
        a = [np.ascontiguousarray(t_seq, np.int32), np.ascontiguousarray(q_seq, np.int32),
             np.ascontiguousarray(q_strand, np.uint8)] + \
            [np.ascontiguousarray(x, np.int32) for x in (lqe, lte, rqs, rts, overlap)]
        n = len(a[0])
        pos = np.zeros(n, np.int32)
        adj = np.zeros(n, np.int32)
        check(lib().gac_crossovers(self.h, n, *[_p(x) for x in a], _p(pos), _p(adj)))
        return pos, adj

    @staticmethod
    def _texts(strs):
        """(char*[n] array, the bytes objects it points into: keep them alive)"""
        keep = [bytes(s) for s in strs]
        arr = (C.c_char_p * max(len(keep), 1))(*keep)
        return arr, keep

    def score_text_blocks(self, q, t, mat) -> np.ndarray:
        """chainScoreBlock of n blocks of caller text (gac_score_text_blocks):
        q[i], t[i] bytes of equal length; int64 per block."""
        n = len(q)
        size = np.array([len(x) for x in q], np.int32)
        assert all(len(a) == len(b) for a, b in zip(q, t))
        qa, k1 = self._texts(q)
        ta, k2 = self._texts(t)
        m = np.ascontiguousarray(np.asarray(mat, np.int32).reshape(16))
        score = np.zeros(n, np.int64)
        check(lib().gac_score_text_blocks(self.h, n, qa, ta, _p(size),
                                          m.ctypes.data_as(C.POINTER(C.c_int32)), _p(score)))
        return score

    def text_crossovers(self, lq, lt, rq, rt, mat):
        """cBlockFindCrossover of n overlaps on caller text (gac_text_crossovers):
        four bytes objects of equal length per overlap; (pos int32, adj int32)."""
        n = len(lq)
        ov = np.array([len(x) for x in lq], np.int32)
        assert all(len(a) == len(b) == len(c) == len(d) for a, b, c, d in zip(lq, lt, rq, rt))
        ptrs = [self._texts(x) for x in (lq, lt, rq, rt)]
        m = np.ascontiguousarray(np.asarray(mat, np.int32).reshape(16))
        pos = np.zeros(n, np.int32)
        adj = np.zeros(n, np.int32)
        check(lib().gac_text_crossovers(self.h, n, *[p[0] for p in ptrs], _p(ov),
                                        m.ctypes.data_as(C.POINTER(C.c_int32)), _p(pos), _p(adj)))
        return pos, adj

    def chain_dp_blocks(self, t_seq, q_seq, q_strand, blk_off, box, score, fast: int = 1,
                        lin_k: int = 0, min_entry: int = 0, ov_cap: int = 1024):
        """chainBlocks' kd-tree DP of n pairs from their blocks
        (gac_chain_dp_blocks): box int32 [n_blocks, 4] = {qStart, qEnd, tStart,
        tEnd}.  Returns (leaf_off int64 [n + 1], tord int32 [leaves], total int64
        [n_blocks], pred int32 [n_blocks])."""
        a = [np.ascontiguousarray(t_seq, np.int32), np.ascontiguousarray(q_seq, np.int32),
             np.ascontiguousarray(q_strand, np.uint8), np.ascontiguousarray(blk_off, np.int64),
             np.ascontiguousarray(np.asarray(box, np.int32).reshape(-1, 4)),
             np.ascontiguousarray(score, np.int32)]
        n, nb = len(a[0]), len(a[5])
        leaf_off = np.zeros(n + 1, np.int64)
        tord = np.full(max(nb, 1), -1, np.int32)
        total = np.zeros(nb, np.int64)
        pred = np.full(nb, -2, np.int32)
        check(lib().gac_chain_dp_blocks(self.h, n, *[_p(x) for x in a], int(fast), int(lin_k),
                                        int(min_entry), int(ov_cap), _p(leaf_off), _p(tord),
                                        _p(total), _p(pred)))
        return leaf_off, tord[:int(leaf_off[-1])], total, pred

    def kd_trees(self, t_seq, q_seq, q_strand, blk_off, box):
        """kdTreeMake of n pairs from their blocks (gac_kd_trees).  Returns
        (leaf_off int64 [n + 1], and per pair lists of int32 arrays: tord[p],
        qord[p] (its leaves' pair-local blocks in target / query order),
        lnode[p] (per block its leaf node, -1: no leaf), nodes[p] [2 leaves - 1,
        6] in pre-order with the hi child first)."""
        a = [np.ascontiguousarray(t_seq, np.int32), np.ascontiguousarray(q_seq, np.int32),
             np.ascontiguousarray(q_strand, np.uint8), np.ascontiguousarray(blk_off, np.int64),
             np.ascontiguousarray(np.asarray(box, np.int32).reshape(-1, 4))]
        n = len(a[0])
        cnt = np.diff(a[3]) if n else np.zeros(0, np.int64)
        cap = [max(int(c), 0) for c in cnt]  # (descending offsets are the call's to refuse)
        leaf_off = np.zeros(n + 1, np.int64)
        bufs = [[np.full(max(w * c, 1), -9, np.int32) for c in cap] for w in (1, 1, 1, 12)]
        ptrs = [(C.c_void_p * max(n, 1))(*[b.ctypes.data for b in col]) for col in bufs]
        check(lib().gac_kd_trees(self.h, n, *[_p(x) for x in a], _p(leaf_off), *ptrs))
        nl = np.diff(leaf_off).astype(np.int64)
        tord = [bufs[0][p][:nl[p]] for p in range(n)]
        qord = [bufs[1][p][:nl[p]] for p in range(n)]
        lnode = [bufs[2][p][:cap[p]] for p in range(n)]
        nodes = [bufs[3][p][:6 * max(2 * nl[p] - 1, 0)].reshape(-1, 6) for p in range(n)]
        return leaf_off, tord, qord, lnode, nodes

    # ---- device buffers / timing (bench)
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(lib().gac_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, p: int) -> None:
        check(lib().gac_dev_free(self.h, C.c_void_p(p)))

    def h2d(self, dst: int, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        check(lib().gac_memcpy_h2d(self.h, C.c_void_p(dst), _p(a), a.nbytes))

    def d2h(self, a: np.ndarray, src: int) -> None:
        check(lib().gac_memcpy_d2h(self.h, _p(a), C.c_void_p(src), a.nbytes))

    def score_ranges_device(self, cs: ChainSet, d_ranges: int, n: int, d_g: int, d_ali: int,
                            d_l: int = 0, want_local: bool = False, stream: int = 0) -> None:
        check(lib().gac_score_ranges_device(
            self.h, cs.handle, C.c_void_p(d_ranges), n, GAC_WANT_LOCAL if want_local else 0,
            C.c_void_p(d_g), C.c_void_p(d_l) if d_l else None, C.c_void_p(d_ali),
            C.c_void_p(stream) if stream else None))

    def score_windows_device(self, cs: ChainSet, d_windows: int, n: int, d_g: int, d_ali: int,
                             d_l: int = 0, want_local: bool = False, stream: int = 0) -> None:
        check(lib().gac_score_windows_device(
            self.h, cs.handle, C.c_void_p(d_windows), n, GAC_WANT_LOCAL if want_local else 0,
            C.c_void_p(d_g), C.c_void_p(d_l) if d_l else None, C.c_void_p(d_ali),
            C.c_void_p(stream) if stream else None))

    def synchronize(self) -> None:
        check(lib().gac_synchronize(self.h))

    def prof_enable(self, on: bool = True, kernels=None) -> None:
        """Time launches with HIP events: all kernels, or those in `kernels`
        (GAC_K_* ids)."""
        mask = 0
        if on:
            mask = (1 << 3) - 1 if kernels is None else sum(1 << k for k in kernels)
        check(lib().gac_prof_enable(self.h, mask))

    def prof_reset(self) -> None:
        check(lib().gac_prof_reset(self.h))

    def prof_read(self, k: int):
        ms, n = C.c_double(), C.c_int64()
        check(lib().gac_prof_read(self.h, k, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _depth_args(seq, start, end, delta):
    a = [np.ascontiguousarray(x, dtype=t)
         for x, t in ((seq, np.int32), (start, np.int32), (end, np.int32), (delta, np.int8))]
    if any(x.ndim != 1 or len(x) != len(a[0]) for x in a):
        raise ValueError("depth_count: seq, start, end and delta must be 1-d and of one length")
    return a


def depth_count_host(seq, start, end, delta, threshold: int = 2) -> np.ndarray:
    """Engine.depth_count's result on the CPU (gac_depth_count_host; no device)."""
    a = _depth_args(seq, start, end, delta)
    count = np.zeros(len(a[0]), np.int32)
    check(lib().gac_depth_count_host(len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]),
                                     int(threshold), _p(count)))
    return count


def _prenet_args(blk_off, t_seq, q_seq, blk_t, blk_q, blk_size, t_sizes, q_sizes):
    a = [np.ascontiguousarray(x, dtype=t)
         for x, t in ((blk_off, np.int64), (t_seq, np.int32), (q_seq, np.int32), (blk_t, np.int32),
                      (blk_q, np.int32), (blk_size, np.int32), (t_sizes, np.int32),
                      (q_sizes, np.int32))]
    if any(x.ndim != 1 for x in a) or len(a[2]) != len(a[1]) or len(a[0]) != len(a[1]) + 1 or \
            len(a[4]) != len(a[3]) or len(a[5]) != len(a[3]):
        raise ValueError("prenet_keep: blk_off [n + 1], t_seq and q_seq [n], blk_t, blk_q and "
                         "blk_size of one length, all 1-d")
    return a


def _prenet_stats(st) -> dict:
    return dict(rounds=st.rounds, passes=st.passes, groups=(st.groups[0], st.groups[1]),
                fell_back=st.fell_back, kept=st.kept)


def prenet_keep_host(blk_off, t_seq, q_seq, blk_t, blk_q, blk_size, t_sizes, q_sizes, pad: int = 1):
    """Engine.prenet_keep's result by the reference's sequential bitmap pass
    (gac_prenet_keep_host; no device): (keep uint8 [n], stats)."""
    a = _prenet_args(blk_off, t_seq, q_seq, blk_t, blk_q, blk_size, t_sizes, q_sizes)
    keep = np.zeros(len(a[1]), np.uint8)
    st = _lib.PrenetStats()
    check(lib().gac_prenet_keep_host(len(a[1]), _p(a[0]), _p(a[1]), _p(a[2]), len(a[3]), _p(a[3]),
                                     _p(a[4]), _p(a[5]), len(a[6]), _p(a[6]), len(a[7]), _p(a[7]),
                                     int(pad), _p(keep), C.byref(st)))
    return keep, _prenet_stats(st)


def _axt_filter_args(t_rows, q_rows):
    rows = [[r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in side]
            for side in (t_rows, q_rows)]
    if len(rows[0]) != len(rows[1]):
        raise ValueError("axt_filter: as many target rows as query rows")
    n = len(rows[0])
    ln = np.fromiter((len(q) for q in rows[1]), np.int32, n)
    tl = np.fromiter((len(t) for t in rows[0]), np.int64, n)
    if np.any(tl < ln):
        raise ValueError("axt_filter: a target row shorter than its query row")
    # t0 q0 t1 q1 ...: the query row of entry i follows its whole target row
    sizes = np.stack([tl, ln.astype(np.int64)], axis=1).ravel()
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    text = b"".join(x for pair in zip(rows[0], rows[1]) for x in pair)
    return text, np.ascontiguousarray(starts[0:2 * n:2]), np.ascontiguousarray(starts[1:2 * n:2]), ln


def _axt_filter_stats(st) -> dict:
    return dict(kept=st.kept, windows=st.windows, host_entries=st.host_entries, batches=st.batches,
                fell_back=st.fell_back)


def axt_filter_host(t_rows, q_rows, min_ident: float, min_entropy: float, window: int,
                    nthreads: int = 0):
    """Engine.axt_filter's result with running window counts on host threads
    (gac_axt_filter_host; no device): (keep uint8 [n], stats)."""
    text, t_off, q_off, ln = _axt_filter_args(t_rows, q_rows)
    keep = np.zeros(len(ln), np.uint8)
    st = _lib.AxtFilterStats()
    check(lib().gac_axt_filter_host(len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                    float(min_ident), float(min_entropy), int(window), int(nthreads),
                                    _p(keep), C.byref(st)))
    return keep, _axt_filter_stats(st)


AXT_PSL_ENTRY = np.dtype([(name, {C.c_uint32: np.uint32, C.c_int32: np.int32, C.c_int64: np.int64}[t])
                          for name, t in _lib.AxtPslEntry._fields_])


def _axt_psl_args(t_rows, q_rows, who="axt_psl"):
    rows = [[r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in side]
            for side in (t_rows, q_rows)]
    if len(rows[0]) != len(rows[1]):
        raise ValueError(who + ": as many target rows as query rows")
    n = len(rows[0])
    ln = np.fromiter((len(q) for q in rows[1]), np.int32, n)
    tl = np.fromiter((len(t) for t in rows[0]), np.int32, n)
    if np.any(tl != ln):
        raise ValueError(who + ": a target row and its query row of different lengths")
    # t0 q0 t1 q1 ...
    starts = np.concatenate([[0], np.cumsum(np.repeat(ln.astype(np.int64), 2))]).astype(np.int64)
    text = b"".join(x for pair in zip(rows[0], rows[1]) for x in pair)
    return text, np.ascontiguousarray(starts[0:2 * n:2]), np.ascontiguousarray(starts[1:2 * n:2]), ln


def _axt_psl_result(res, st):
    """copies of a gac_axtpsl_result's arrays; the handle is released"""
    try:
        r = res.contents
        entries = np.zeros(r.n, AXT_PSL_ENTRY)
        blocks = np.zeros((r.n_blocks, 3), np.int32)
        if r.n:
            C.memmove(entries.ctypes.data, r.entry, entries.nbytes)
        if r.n_blocks:
            C.memmove(blocks.ctypes.data, r.block, blocks.nbytes)
    finally:
        lib().gac_axtpsl_free(res)
    return entries, blocks, dict(blocks=st.blocks, columns=st.columns, host_entries=st.host_entries,
                                 batches=st.batches, fell_back=st.fell_back)


def axt_psl_host(t_rows, q_rows, nthreads: int = 0):
    """Engine.axt_psl's result by one sequential pass an entry on host threads
    (gac_axt_psl_host; no device): (entries, blocks, stats)."""
    text, t_off, q_off, ln = _axt_psl_args(t_rows, q_rows)
    res = C.POINTER(_lib.AxtPslResult)()
    st = _lib.AxtPslStats()
    check(lib().gac_axt_psl_host(len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln), int(nthreads),
                                 C.byref(res), C.byref(st)))
    return _axt_psl_result(res, st)


def _axt_score_stats(st):
    return dict(columns=st.columns, host_entries=st.host_entries, batches=st.batches,
                fell_back=st.fell_back)


def axt_score_host(t_rows, q_rows, nthreads: int = 0):
    """Engine.axt_score's result by one pass an entry on host threads
    (gac_axt_score_host; no device): (scores, stats)."""
    text, t_off, q_off, ln = _axt_psl_args(t_rows, q_rows, "axt_score")
    score = np.zeros(len(ln), np.int32)
    st = _lib.AxtScoreStats()
    check(lib().gac_axt_score_host(len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln), int(nthreads),
                                   _p(score), C.byref(st)))
    return score, _axt_score_stats(st)


def axt_pair_counts_host(t_2bit: str, q_2bit: str, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q,
                         blk_size, pieces):
    """Engine.axt_pair_counts' result base by base on the host
    (gac_axt_pair_counts_host; no device): the sequences come from the two
    .2bit files, t_seq / q_seq numbering them in file order."""
    d, _arrs = Engine._desc(t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size)
    w = np.ascontiguousarray(np.asarray(pieces, dtype=np.int32).reshape(-1, 5))
    n = w.shape[0]
    pairs = np.zeros((n, 16), np.int64)
    n_cols = np.zeros(n, np.int64)
    check(lib().gac_axt_pair_counts_host(t_2bit.encode(), q_2bit.encode(), C.byref(d), _p(w), n,
                                         _p(pairs), _p(n_cols)))
    return pairs, n_cols


def antirepeat_pass(score: float, match, rep: int, total: int, min_score: int = 5000) -> bool:
    """chainAntiRepeat's keep/drop decision for one chain from its composition
    (gac_antirepeat_pass: degeneracyFilter then repeatFilter; host only)."""
    m = (C.c_int64 * 4)(*[int(x) for x in match])
    return bool(lib().gac_antirepeat_pass(float(score), m, int(rep), int(total), int(min_score)))


def twobit_mask_runs(path: str, name: str) -> Tuple[np.ndarray, np.ndarray]:
    """(starts, sizes) int32 of the soft-mask runs of one sequence of a .2bit
    file, as the host reader keeps them (gac_twobit_mask_runs)."""
    n = C.c_int32()
    check(lib().gac_twobit_mask_runs(path.encode(), name.encode(), 0, None, None, C.byref(n)))
    st = np.zeros(n.value, np.int32)
    sz = np.zeros(n.value, np.int32)
    check(lib().gac_twobit_mask_runs(path.encode(), name.encode(), n.value, _p(st), _p(sz),
                                     C.byref(n)))
    return st, sz


__all__ = ["Engine", "ChainSet", "GapCosts", "read_score_scheme", "GAC_T", "GAC_Q",
           "antirepeat_pass", "twobit_mask_runs", "depth_count_host", "prenet_keep_host",
           "axt_filter_host", "axt_psl_host", "AXT_PSL_ENTRY", "axt_score_host",
           "axt_pair_counts_host"]
