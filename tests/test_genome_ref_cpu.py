"""tests/genome_ref.py (the plain reference of the resident genome layout and
the N-edge fixtures of test_gpu_genome.py) checked against what exists: the
synthetic genome's own text, the soft-mask reference, the .2bit writer and
reader, and the oracle -- so the GPU tests' expectations and the cases they
claim to contain hold without a GPU."""
import functools
import os

import numpy as np

import antirepeat_ref as AR
import genome_ref as GR
from conftest import BLASTZ


@functools.lru_cache(maxsize=None)
def _case():
    tg, qg = GR.edge_genome(101), GR.edge_genome(202)
    return (tg, qg) + GR.edge_chains(tg, qg)


def test_edge_genome_holds_the_shapes():
    tg, qg = _case()[:2]
    for g in (tg, qg):
        sizes = [len(c) for c in g.codes]
        assert sizes[:11] == GR.EDGE_SIZES and sizes[-1] == 0 and sizes.count(0) == 3
        assert set(range(1, 71)) <= set(sizes[11:11 + GR.N_TINY + 1])
        planes, nmask, lmask, woff = GR.image(g, True)
        big, main, nend = (g.index(n) for n in ("big", "main", "nend"))
        # workgroup steps of 2048 words fall inside big; hundreds of starts before it
        assert woff[big] < 2048 and woff[big] + (GR.BIG + 31) // 32 > 4096 and big > 300
        # the run that ends nend ends on main's first base, globally
        assert (woff[nend] + 2) * 32 == woff[main] * 32 and GR.merged_runs(g, "nend") == [(60, 64)]
        assert not GR.block_has_n(g, "main", 0, 5)
        # a lane's two words in three sequences: a one-word sequence between two starts
        nw = (np.asarray(sizes) + 31) // 32
        assert any(nw[i] == 1 and nw[i - 1] >= 1 and nw[i + 1] >= 1 and woff[i] % 2 == 1
                   for i in range(1, len(nw) - 1))
        # unsorted runs, pieces of over 1024 bases, a sequence that is all N, clipped mask runs
        st, sz = g.nruns[big]
        assert (np.diff(st) < 0).any() and {1024, 1025, 2049, 0} <= set(sz.tolist())
        assert len(st) > 2900 and GR.n_bases(g, g.index("e8")).all()
        ms, mz = g.mruns[main]
        assert (ms < 0).any() and (ms.astype(np.int64) + mz > GR.MAIN).any()
    assert not np.array_equal(tg.codes[tg.index("big")], qg.codes[qg.index("big")])


def test_image_decodes_to_the_genome_text():
    for g in _case()[:2]:
        planes, nmask, lmask, woff = GR.image(g, True)
        assert len(nmask) == len(lmask) == len(planes) == \
            sum((len(c) + 31) // 32 for c in g.codes) + 4
        assert (planes[-4:] == 0).all() and (nmask[-4:] == 0xffffffff).all() and \
            (lmask[-4:] == 0).all()
        for i in range(len(g.names)):
            size = len(g.codes[i])
            assert GR.image_text(g, planes, nmask, lmask, woff, i) == g.text(i)
            assert GR.image_text(g, planes, nmask, lmask, woff, i, cased=True) == \
                AR.decode_case(g, i, 0, size)
            if size % 32:  # tail padding: N set, planes and mask clear
                w, pad = int(woff[i]) + size // 32, (0xffffffff << (size % 32)) & 0xffffffff
                assert nmask[w] & pad == pad and not (planes[w] & pad).any() and not lmask[w] & pad
        assert GR.image(g, False)[2] is None


def test_2bit_file_round_trip(tmp_path):
    from genomealignmenttools_amd import synth
    g = _case()[0]
    path = os.path.join(str(tmp_path), "t.2bit")
    synth.write_2bit(g, path)
    back = AR.read_2bit(path)
    assert back.names == g.names
    for i in range(len(g.names)):
        assert np.array_equal(back.codes[i], g.codes[i])
        for a, b in zip(back.nruns[i] + back.mruns[i], g.nruns[i] + g.mruns[i]):
            assert np.array_equal(a, b)
    a, b = GR.image(back, True), GR.image(g, True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _block_scores(tg, qg, ca):
    """the oracle's score of every block alone: its chain cut to the block"""
    from oracle.oracle import OracleScorer, genome_text
    chain = np.repeat(np.arange(ca.n), np.diff(ca.blk_off))
    R = np.stack([chain, ca.blk_t, ca.blk_t.astype(np.int64) + ca.blk_size], 1)
    g, _, a = OracleScorer(genome_text(tg), genome_text(qg), BLASTZ, "loose").score_ranges(ca, R)
    assert np.array_equal(a, ca.blk_size)
    return g


def test_edge_chains_have_teeth():
    """The labels are true per base; a block that touches an N scores
    differently once the N runs are gone (every 1-base block for certain:
    BLASTZ has no zero entry), for every shape, side and strand; the flags of
    most blocks that touch an N flip in the shifted set; the stretch of
    one-block chains leaves k_build_flat's staged chain search."""
    tg, qg, ca, info, cuts = _case()
    assert len(info) == len(ca.blk_t) and ca.n > 1000
    ft, fq = GR.block_flags(tg, qg, ca)
    chain = np.repeat(np.arange(ca.n), np.diff(ca.blk_off))
    for b, (c, side, strand, shape, touch, group) in enumerate(info):
        assert c == chain[b] and strand == ca.qstrand[c]
        own, other = (ft, fq) if side == 0 else (fq, ft)
        assert own[b] == touch and not other[b], (b, info[b])
        f = int(ca.blk_q[b]) if not strand else int(ca.qsize[c] - ca.blk_q[b] - ca.blk_size[b])
        assert GR.block_has_n(tg, ca.tname[c], int(ca.blk_t[b]), int(ca.blk_size[b])) == ft[b]
        assert GR.block_has_n(qg, ca.qname[c], f, int(ca.blk_size[b])) == fq[b]
    with_n = _block_scores(tg, qg, ca)
    no_n = _block_scores(GR.without_n(tg), GR.without_n(qg), ca)
    touches = ft | fq
    assert np.array_equal(with_n[~touches], no_n[~touches])
    one = touches & (ca.blk_size == 1)
    assert one.sum() > 100 and (with_n[one] == 0).all() and (no_n[one] != 0).all()
    differs = {}
    for b, (c, side, strand, shape, touch, group) in enumerate(info):
        if touch:
            k = (side, strand, shape)
            differs[k] = differs.get(k, False) or with_n[b] != no_n[b]
    want = {(s, st, sh) for s in (0, 1) for st in (0, 1)
            for sh in [n for n in GR.ONE_SHAPES if GR.TOUCH[n]] + ["seq_edge", "over", "stretch_on"]}
    assert want <= set(differs) and all(differs.values()), \
        (want - set(differs), [k for k, v in differs.items() if not v])
    # every shape of every chosen run, nothing dropped
    runs = sum(1 for x in info if x[5] == "run" and x[3] == "one_a")
    assert runs == 2 * (12 + 2 * 12)  # one-block chain + the chain of 1-base blocks, per run use
    # the other set of the re-upload test: of the blocks that touch an N in
    # either set, most change their flag
    st, sq = GR.block_flags(tg, qg, GR.shifted(ca, info, tg, qg))
    flips, touching = (st != ft) | (sq != fq), ft | fq | st | sq
    assert 2 * flips.sum() > touching.sum() > 900
    # upload paths: workgroups over more than kStage chains, and one under
    un = GR.unstaged_workgroups(ca.blk_off)
    nwg = (len(ca.blk_t) + 511) // 512
    assert un and len(un) < nwg
    s0 = next(b for b, x in enumerate(info) if x[5] == "stretch")
    assert any(wg * 512 >= s0 and (wg + 1) * 512 <= s0 + GR.STRETCH for wg in un)
    R = GR.edge_ranges(ca, cuts)
    assert len(R) > 4 * ca.n - 2 * GR.STRETCH and (R[:, 1] < R[:, 2]).all()


def test_staging_and_scatter_fixtures_reach_their_paths():
    """The arithmetic of the upload paths the GPU tests claim, with the
    library's own formulas.  Staging (stage_thread_body, 1 MB windows, 16
    threads): three windows, so both pinned buffers are used again; the first
    window boundary is the start of a tiny payload, the second lies inside a
    large one; thread shares start strictly inside the padding behind a tiny
    payload and strictly inside a tiny payload.  Scatter (launch_scatter: at
    most 16 384 workgroups of four waves, one run per wave and trip): more
    runs than waves."""
    sizes = GR.staging_sizes(5)
    off, total = GR._layout_of_sizes(sizes)
    assert -(-total // GR.WINDOW) == 3
    assert GR.WINDOW in off[1:151] and not 2 * GR.WINDOW in off
    k = max(i for i in range(len(off)) if off[i] <= 2 * GR.WINDOW)
    assert sizes[k] > 4_000_000 and off[k] < 2 * GR.WINDOW < off[k] + (sizes[k] + 3) // 4
    pad, tiny, other = GR.share_starts(sizes, GR.STAGE_THREADS)
    assert pad >= 1 and tiny >= 1 and other >= 30
    shares = GR.stage_shares(total)
    assert shares[0][0] == 0 and shares[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(shares, shares[1:]))
    g = GR.staging_genome(5)
    assert [len(c) for c in g.codes] == sizes
    words = (GR.SCATTER_SIZE + 31) // 32
    assert GR.SCATTER_WAVES < GR.SCATTER_RUNS < words
    assert len(GR.scatter_genome().codes[1]) == GR.SCATTER_SIZE
