"""The resident genome planes and the per-block N flags, directly.

Planes: Engine.genome_planes (the device arrays copied back) equals
genome_ref.image word for word -- padding bits, the soft-mask plane and the
four trailing words included -- through every way a genome arrives: sequence
by sequence, from a .2bit file, with a keep list, in more staging windows
than there are pinned buffers, and as the sparse word-run upload.

N flags: the bits kTHasN / kQHasN of the block records have no reader, so
they are observed through every consumer's result on chains whose blocks end,
start and sit exactly on N-run edges (genome_ref.edge_chains; the fixtures'
claims are checked in test_genome_ref_cpu.py).  Every comparison is exact.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import antirepeat_ref as AR
import axt_ref as AX
import genome_ref as GR
import pslout_ref as PS
from conftest import BLASTZ, REPO

pytestmark = pytest.mark.gpu

GAC_E_ARG, GAC_E_FORMAT, GAC_E_STATE = -1, -4, -5


def _diff(got, want, what, sel=None):
    """exact, with the first differing words in the message"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    ne = got != want
    if ne.ndim == 2:
        ne = ne.any(1)
    if sel is not None:
        ne &= sel
    bad = np.flatnonzero(ne)
    assert bad.size == 0, (what, f"{bad.size} of {len(got)} words differ",
                           [(int(w), got[w].tolist(), want[w].tolist()) for w in bad[:6]])


def _same_image(e, side, g, soft, what):
    planes, nmask, lmask = e.genome_planes(side)
    wp, wn, wl, _ = GR.image(g, soft)
    _diff(planes, wp, what + ": planes")
    _diff(nmask, wn, what + ": nmask")
    if soft:
        _diff(lmask, wl, what + ": lmask")
    else:
        assert lmask is None, what


@functools.lru_cache(maxsize=None)
def _genomes():
    return GR.edge_genome(101), GR.edge_genome(202)


# ------------------------------------------------------------------ planes
@pytest.mark.parametrize("soft", [False, True])
def test_planes_from_add_sequences(soft):
    """k_relayout / k_nruns on the edge genome (sequences of 0 .. 140 003
    bases, lanes whose two words lie in three sequences, workgroup steps
    inside a sequence, runs on word, piece and sequence edges), every word;
    then decode / decode_case on sub-ranges at bit 0, bit 31 and across
    words, and the sequence table.  A sequence of size 0 is accepted: it owns
    no word and shares its word offset with the next sequence."""
    from genomealignmenttools_amd._lib import GacError
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    e = Engine(0)
    try:
        with pytest.raises(GacError) as ei:
            e.genome_planes(GAC_T)
        assert ei.value.code == GAC_E_STATE
        with pytest.raises(GacError) as ei:
            e.genome_planes(2)
        assert ei.value.code == GAC_E_ARG
        for side, g in zip((GAC_T, GAC_Q), _genomes()):
            e.add_sequences(side, g.seq_records(), mask_runs=g.mruns if soft else None)
            _same_image(e, side, g, soft, f"add_sequences side {side}")
            assert e.seq_count(side) == len(g.names) and e.seq_index(side, "nope") == -1
            assert e.seq_size(side, len(g.names)) == -1
            for i, n in enumerate(g.names):
                size = len(g.codes[i])
                assert e.seq_index(side, n) == i and e.seq_size(side, i) == size
            for n in ("e0", "e3", "e5", "e7", "e8", "e10", "y150", "nend", "main", "zlast"):
                i = g.index(n)
                size = len(g.codes[i])
                text = g.text(i)
                cased = AR.decode_case(g, i, 0, size)
                for a, b in ((0, 0), (0, 1), (0, 32), (31, 32), (31, 33), (32, 64), (1, 63),
                             (33, 97), (size - 1, size), (size // 2, size), (0, size)):
                    if 0 <= a <= b <= size:
                        assert e.decode(side, i, a, b) == text[a:b], (n, a, b)
                        if soft:
                            assert e.decode_case(side, i, a, b) == cased[a:b], (n, a, b)
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["plain", "soft", "keep", "keep-soft"])
def test_planes_from_2bit_file(mode, tmp_path):
    """The same through the .2bit loader: payloads staged from the mapped
    file (not 8-byte aligned there), records of size 0 included (the reader
    takes them), and a keep list that drops every third sequence."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    soft = "soft" in mode
    e = Engine(0)
    try:
        for side, g in zip((GAC_T, GAC_Q), _genomes()):
            path = os.path.join(str(tmp_path), f"g{side}.2bit")
            synth.write_2bit(g, path)
            keep = None
            if "keep" in mode:
                keep = [i % 3 != 2 for i in range(len(g.names))]
                g = GR.subset(g, [i for i in range(len(g.names)) if keep[i]])
            e.load_2bit(side, path, soft_mask=soft, keep=keep)
            _same_image(e, side, g, soft, f"load_2bit {mode} side {side}")
            assert e.seq_count(side) == len(g.names)
            assert all(e.seq_index(side, n) == i for i, n in enumerate(g.names))
    finally:
        e.close()


# ------------------------------------------------------------------ staging windows
def _staging_child():
    """GAC_PIN_MB=1 (read once per process): more staging windows than pinned buffers."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    g = GR.staging_genome(5)
    total = GR.staging_layout(g)[1]
    path = os.path.join(os.environ["GAC_TEST_TMP"], "stage.2bit")
    synth.write_2bit(g, path)
    e = Engine(0)
    e.add_sequences(GAC_T, g.seq_records(), mask_runs=g.mruns)
    _same_image(e, GAC_T, g, True, "staged add_sequences")
    e.load_2bit(GAC_Q, path)
    _same_image(e, GAC_Q, g, False, "staged load_2bit")
    e.close()
    print(json.dumps({"ok": True, "windows": -(-total // GR.WINDOW), "bytes": total}))


def test_planes_through_many_staging_windows(tmp_path):
    """An 8.4 Mb genome through 1 MB staging windows on 16 threads: three
    windows, so both pinned buffers are used again; the first boundary is a
    tiny payload's start, the second lies inside a large one; thread shares of
    the last window start inside the padding behind tiny payloads and inside
    tiny payloads (test_genome_ref_cpu.py asserts the arithmetic).  In a fresh
    process, because the window size is read once."""
    env = dict(os.environ, GAC_PIN_MB="1", GAC_THREADS=str(GR.STAGE_THREADS),
               GAC_TEST_TMP=str(tmp_path))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_genome as T; T._staging_child()"
            % (os.path.join(REPO, "tests"), REPO))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["windows"] == 3


# ------------------------------------------------------------------ sparse upload
def _run_words(g, runs, woff):
    """bool per plane word: inside one of the (clipped) runs"""
    sel = np.zeros(int(woff[-1]) + (len(g.codes[-1]) + 31) // 32 + 4, bool)
    for i, rr in enumerate(runs):
        nw = (len(g.codes[i]) + 31) // 32
        for lo, hi in rr:
            for w in range(max(lo, 0), min(hi, nw)):
                sel[int(woff[i]) + w] = True
    return sel


def test_sparse_upload_runs(tmp_path):
    """k_scatter: inside the runs the planes equal the image; the N mask does
    everywhere (padding and N runs do not depend on the payload).  Runs of one
    word, a last partial word, adjacent runs, runs clipped at both ends, an
    empty run, sequences without a run; the soft-mask plane is refused."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd._lib import GacError
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    g = _genomes()[0]
    path = os.path.join(str(tmp_path), "t.2bit")
    synth.write_2bit(g, path)
    runs = [[] for _ in g.names]
    nw = lambda n: (len(g.codes[g.index(n)]) + 31) // 32
    runs[g.index("e0")] = [(0, 1)]                         # one word, partial
    runs[g.index("e6")] = [(2, 3)]                         # the last partial word only
    runs[g.index("e9")] = [(0, 5), (5, 9), (9, 10), (30, 40)]  # adjacent; past the end
    runs[g.index("e10")] = [(-3, 2), (7, 7), (9, 8), (100, 129)]  # from below 0; empty runs
    runs[g.index("y10")] = [(0, 3)]
    runs[g.index("big")] = [(0, 1), (1, 2), (2047, 2049), (nw("big") - 1, nw("big") + 5), (3000, 3001)]
    runs[g.index("main")] = [(0, nw("main"))]
    runs[g.index("zlast")] = [(0, 1)]                      # nothing to clip to
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, path, runs=runs)
        planes, nmask, lmask = e.genome_planes(GAC_T)
        wp, wn, _, woff = GR.image(g, False)
        sel = _run_words(g, runs, woff)
        assert sel.sum() > 900 and not sel.all() and lmask is None
        _diff(planes, wp, "sparse planes", sel)
        _diff(nmask, wn, "sparse nmask")
        _diff(planes[-4:], wp[-4:], "sparse trailing planes")
        with pytest.raises(GacError) as ei:
            e.load_2bit(GAC_Q, path, soft_mask=True, runs=runs)
        assert ei.value.code == GAC_E_ARG
    finally:
        e.close()


def test_sparse_upload_grid_stride(tmp_path):
    """70 000 one-word runs: k_scatter's grid holds 16 384 workgroups of four
    waves, one run per wave, so the waves' loop takes a second trip
    (test_genome_ref_cpu.py asserts the counts)."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.gachain import GAC_T, Engine
    g = GR.scatter_genome()
    path = os.path.join(str(tmp_path), "g.2bit")
    synth.write_2bit(g, path)
    n = GR.SCATTER_RUNS
    assert n > GR.SCATTER_WAVES
    runs = [[], [(w, w + 1) for w in range(n)]]
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, path, runs=runs)
        planes, nmask, _ = e.genome_planes(GAC_T)
        wp, wn, _, woff = GR.image(g, False)
        sel = np.zeros(len(wn), bool)
        sel[int(woff[1]):int(woff[1]) + n] = True
        _diff(planes, wp, "grid-stride planes", sel)
        _diff(nmask, wn, "grid-stride nmask")
    finally:
        e.close()


# ------------------------------------------------------------------ errors
def test_refused_sequence_leaves_no_trace():
    """gac_genome_add_seq refuses an N block out of range (negative start,
    past the end, start + size over int32) before it stores anything: the
    count is unchanged, the name is free, and the finalized side is the image
    of the accepted sequences only."""
    import ctypes as C
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd._lib import lib
    from genomealignmenttools_amd.gachain import GAC_T, Engine
    rng = np.random.default_rng(8)
    run = lambda *r: (np.array([a for a, _ in r], np.int32), np.array([l for _, l in r], np.int32))
    g = synth.Genome(["a", "b", "c"], [rng.integers(0, 4, s).astype(np.uint8) for s in (70, 100, 45)],
                     [run((60, 10)), run((10, 5), (90, 10)), run((0, 2))])
    e = Engine(0)

    def add(i, runs):
        ns, nz = (np.ascontiguousarray(x, np.int32) for x in runs)
        p = np.ascontiguousarray(g.packed(i))
        return lib().gac_genome_add_seq(e.h, GAC_T, g.names[i].encode(), len(g.codes[i]),
                                        C.c_void_p(p.ctypes.data), len(ns),
                                        C.c_void_p(ns.ctypes.data), C.c_void_p(nz.ctypes.data))
    try:
        assert add(0, g.nruns[0]) == 0
        for bad in (run((10, 5), (-1, 3)), run((10, 5), (90, 60)), run((95, 6)),
                    run((10, 5), (2**31 - 2, 2**31 - 1)), run((3, -1))):
            assert add(1, bad) == GAC_E_FORMAT, bad
            assert e.seq_count(GAC_T) == 1 and e.seq_index(GAC_T, "b") == -1
        assert add(1, g.nruns[1]) == 0 and add(2, g.nruns[2]) == 0
        assert e.seq_count(GAC_T) == 3
        assert lib().gac_genome_finalize(e.h, GAC_T) == 0
        _same_image(e, GAC_T, g, False, "after refused sequences")
        for i in range(3):
            assert e.decode(GAC_T, i, 0, len(g.codes[i])) == g.text(i)
    finally:
        e.close()


# ------------------------------------------------------------------ N flags
ASYM_RANDOM = np.random.default_rng(300).integers(-300, 301, 16).astype(np.int32)
ASYM_RANDOM[0] = 300  # (test_asymmetric_matrix's matrix at lim = 300)


@functools.lru_cache(maxsize=None)
def _flag_case():
    """The edge chains and every reference result, computed once."""
    from oracle.oracle import OracleScorer, genome_text
    from test_host import subset_windows
    tg, qg = _genomes()
    ca, info, cuts = GR.edge_chains(tg, qg)
    sh = GR.shifted(ca, info, tg, qg)
    R = GR.edge_ranges(ca, cuts)
    assert len(R) > 256 * 8
    first, cnt = subset_windows(ca, R[:, 0], R[:, 1], R[:, 2])
    W = np.concatenate([R, first[:, None], cnt[:, None]], 1).astype(np.int32)
    tt, qt = genome_text(tg), genome_text(qg)
    full = lambda c: np.stack([np.arange(c.n), c.tstart, c.tend], 1).astype(np.int64)
    ref = {}
    for name, mat in (("blastz", BLASTZ), ("asym", ASYM_RANDOM)):
        o = OracleScorer(tt, qt, mat, "loose")
        ref[name] = o.score_ranges(ca, R)
        ref[name + "-shifted"] = o.score_ranges(sh, full(sh))
    tidx = np.array([tg.index(n) for n in ca.tname], np.int32)
    qidx = np.array([qg.index(n) for n in ca.qname], np.int32)
    for name, mat in (("blastz", BLASTZ), ("axt-asym", AX.ASYM)):
        for tag, c in (("", ca), ("-shifted", sh)):
            ref["blocks-" + name + tag] = AX.block_scores(
                tg, qg, mat, tidx, qidx, c.qstrand, c.blk_off, c.blk_t, c.blk_q,
                c.blk_size).astype(np.int32)
    for tag, c in (("", ca), ("-shifted", sh)):
        ref["compose" + tag] = AR.composition(tg, qg, c)
        ref["psl" + tag] = PS.counts(tg, qg, c)
    return tg, qg, ca, sh, R, W, tidx, qidx, ref


def _score_chunked(e, cs, R, want_local):
    """batches of at most 256 ranges (k_small), sizes cycling through edge values"""
    sizes, out, i, k = (1, 7, 64, 255, 256, 100), [], 0, 0
    while i < len(R):
        m = sizes[k % len(sizes)]
        out.append(e.score_ranges(cs, R[i:i + m], want_local=want_local))
        i += m
        k += 1
    cat = lambda j: np.concatenate([o[j] for o in out])
    return cat(0), (cat(1) if want_local else None), cat(2)


def _arrays(ca, tidx, qidx):
    return tidx, qidx, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q, ca.blk_size


@pytest.mark.parametrize("order", ["scoring-first", "chains-first"])
def test_n_flags_through_every_consumer(order):
    """Blocks that end at a, a+1, start at b-1, b, contain, lie inside and are
    single bases on a-1, a, b-1, b of a dozen N runs per side and strand;
    runs in a chain's gap, met by a chain's last base only, ending where the
    next sequence (and a chain) starts; 600 one-block chains in a row
    (k_build_flat's unstaged chain search).  A flag wrongly clear scores an N
    as the random base stored under it, in k_tile (large batches, windows,
    whole chains), k_small (batches of at most 256), chain_walk (composition,
    PSL counts); score_blocks reads the same genome.  Then the set is
    re-uploaded in place with every block moved by one base, and back: stale
    flags would show.  Every consumer is run and all mismatches are reported
    together."""
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine, GapCosts
    tg, qg, ca, sh, R, W, tidx, qidx, ref = _flag_case()
    nfull = ca.n
    bad, checked = {}, []

    def cmp(what, got, want):
        for k, (a, b) in enumerate(zip(got, want)):
            if a is None:
                continue
            checked.append(f"{what}[{k}]")
            a, b = np.asarray(a), np.asarray(b)
            ne = np.flatnonzero((a != b).reshape(len(a), -1).any(1)) if a.shape == b.shape else [-1]
            if len(ne):
                bad[f"{what}[{k}]"] = (len(ne), [int(x) for x in ne[:5]])

    e = Engine(0)
    try:
        e.add_sequences(GAC_T, tg.seq_records(), mask_runs=tg.mruns)
        e.add_sequences(GAC_Q, qg.seq_records(), mask_runs=qg.mruns)
        if order == "scoring-first":
            e.set_scoring(np.asarray(BLASTZ, np.int32), GapCosts("loose"))
        cs = e.upload_chain_arrays(*_arrays(ca, tidx, qidx))
        if order == "chains-first":
            e.set_scoring(np.asarray(BLASTZ, np.int32), GapCosts("loose"))

        def consumers(tag, c, full_only):
            """every consumer on the set now resident (c), BLASTZ then the asymmetric matrix"""
            for name, mat, bname, bmat in (("blastz", BLASTZ, "blastz", BLASTZ),
                                           ("asym", ASYM_RANDOM, "axt-asym", AX.ASYM)):
                e.set_scoring(np.asarray(mat, np.int32), GapCosts("loose"))
                want = ref[name + tag]
                wfull = tuple(x[:nfull] for x in want)
                for local in (True, False):
                    g, l, a = e.score_chains(cs, want_local=local)
                    cmp(f"score_chains {name}{tag} local={local}", (g, l, a), wfull)
                if not full_only:
                    cmp(f"score_ranges {name}", e.score_ranges(cs, R, want_local=True), want)
                    cmp(f"score_ranges<=256 {name}", _score_chunked(e, cs, R, True), want)
                    g, l, a = _score_chunked(e, cs, R, False)
                    cmp(f"score_ranges<=256 no local {name}", (g, None, a), want)
                    cmp(f"score_windows {name}", e.score_windows(cs, W, want_local=True), want)
                else:
                    fr = np.stack([np.arange(c.n), c.tstart, c.tend], 1)
                    cmp(f"score_ranges {name}{tag}", e.score_ranges(cs, fr, want_local=True), want)
                    cmp(f"score_ranges<=256 {name}{tag}", _score_chunked(e, cs, fr[:700], True),
                        tuple(x[:700] for x in want))
                e.set_scoring(np.asarray(bmat, np.int32), GapCosts("loose"))
                cmp(f"score_blocks {bname}{tag}", (e.score_blocks(*_arrays(c, tidx, qidx)),),
                    (ref["blocks-" + bname + tag],))
            cmp("chain_composition" + tag, e.chain_composition(cs), ref["compose" + tag])
            cmp("chain_psl_counts" + tag, (e.chain_psl_counts(cs),), (ref["psl" + tag],))

        consumers("", ca, False)
        e.reupload_chain_arrays(cs, *_arrays(sh, tidx, qidx))
        consumers("-shifted", sh, True)
        e.reupload_chain_arrays(cs, *_arrays(ca, tidx, qidx))
        e.set_scoring(np.asarray(BLASTZ, np.int32), GapCosts("loose"))
        cmp("score_ranges after re-upload", e.score_ranges(cs, R, want_local=True), ref["blastz"])
        cmp("score_chains after re-upload", e.score_chains(cs, want_local=True),
            tuple(x[:nfull] for x in ref["blastz"]))
        cmp("chain_psl_counts after re-upload", (e.chain_psl_counts(cs),), (ref["psl"],))
        cs.close()
    finally:
        e.close()
    for k in checked:  # (shown with a failure)
        print("differs" if k in bad else "equal  ", k, bad.get(k, ""))
    assert not bad, sorted(bad)
