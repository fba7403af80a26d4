"""The device primitives behind axtChain against the plain references of
tests/axt_ref.py, exactly: gac_score_blocks (k_blocks), gac_crossovers
(k_xover), gac_score_text_blocks / gac_text_crossovers (k_text_blocks,
k_text_xover) and chainConnectCost inside the DP kernels (k_dp, k_dp_spec,
k_dp_fast) through gac_chain_dp_blocks on pairs of two blocks.  The case
sets are the ones tests/test_axt_ref_cpu.py shows to tell the usual bugs
apart; every case runs with BLASTZ and with an asymmetric matrix."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
# torch before libgachain (see the note at the top of tests/test_gpu_antirepeat.py)
import torch  # noqa: F401

from conftest import BLASTZ, REPO

import axt_ref as AX

pytestmark = pytest.mark.gpu

MATS = {"blastz": BLASTZ, "asym": AX.ASYM}
GAC_E_ARG = -1


def _engine(tg, qg, mat=None):
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine, GapCosts
    e = Engine(0)
    e.add_sequences(GAC_T, tg.seq_records())
    e.add_sequences(GAC_Q, qg.seq_records())
    if mat is not None:
        e.set_scoring(mat, GapCosts("loose"))
    return e


def _same(got, want, what, rows=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {got.size} differ",
                           [(int(i), int(got[i]), int(want[i]), None if rows is None else rows(int(i)))
                            for i in bad[:8]])


# ------------------------------------------------------------------ gac_score_blocks
@pytest.fixture(scope="module")
def block_case():
    return AX.block_case_set()


@pytest.fixture(scope="module")
def block_engine(block_case):
    e = _engine(block_case[0], block_case[1], BLASTZ)
    yield e
    e.close()


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_score_blocks_vs_reference(block_case, block_engine, mat):
    """Sizes 0 .. 70 000 at bits 0 and 31 of a word on both sides, the first
    and last bases of the first, the last and an odd-sized sequence, '-'
    windows at forward base 0, N runs at every place of a block, an all-N
    block; several pairs with empty pairs between them; both strands."""
    from genomealignmenttools_amd.gachain import GapCosts
    tg, qg, t_seq, q_seq, q_strand, blk_off, bt, bq, bs = block_case
    assert set(AX.BLOCK_SIZES) <= set(bs.tolist()) and (np.diff(blk_off) == 0).sum() >= 6
    block_engine.set_scoring(MATS[mat], GapCosts("loose"))
    want = AX.block_scores(tg, qg, MATS[mat], t_seq, q_seq, q_strand, blk_off, bt, bq, bs)
    got = block_engine.score_blocks(t_seq, q_seq, q_strand, blk_off, bt, bq, bs)
    pair = np.repeat(np.arange(len(t_seq)), np.diff(blk_off))
    _same(got, want, "gac_score_blocks", lambda i: (int(t_seq[pair[i]]), int(q_seq[pair[i]]),
                                                   int(q_strand[pair[i]]), int(bt[i]), int(bq[i]),
                                                   int(bs[i])))
    assert len(want) > 900 and (want != 0).sum() > 800


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_score_blocks_million_block_batch(block_case, block_engine, mat):
    """A little over 2^20 blocks of 1 to 8 bases: the job fill works in
    2^20-block chunks on threads; a pair boundary and an empty pair sit at
    block 2^20, the first pair is '+', the last '-'."""
    from genomealignmenttools_amd.gachain import GapCosts
    tg, qg = block_case[:2]
    n0, n1 = 1 << 20, 1500
    n = n0 + n1
    rng = np.random.default_rng(77)
    bs = rng.integers(1, 9, n).astype(np.int32)
    bt = rng.integers(0, len(tg.codes[1]) - 8, n).astype(np.int32)
    bq = rng.integers(0, len(qg.codes[1]) - 8, n).astype(np.int32)
    t_seq = np.array([3, 1, 0, 1], np.int32)
    q_seq = np.array([3, 1, 0, 1], np.int32)
    q_strand = np.array([1, 0, 1, 1], np.uint8)
    blk_off = np.array([0, 0, n0, n0, n], np.int64)
    block_engine.set_scoring(MATS[mat], GapCosts("loose"))
    want = AX.block_scores(tg, qg, MATS[mat], t_seq, q_seq, q_strand, blk_off, bt, bq, bs)
    got = block_engine.score_blocks(t_seq, q_seq, q_strand, blk_off, bt, bq, bs)
    _same(got, want, "gac_score_blocks, 2^20 + 1500 blocks",
          lambda i: (int(bt[i]), int(bq[i]), int(bs[i])))


def test_score_blocks_errors(block_case, block_engine):
    """A block one base past its target, past its query, or with a negative
    coordinate is GAC_E_ARG, and the message names the first bad block in
    order -- also when a later chunk of the job fill holds another one."""
    from genomealignmenttools_amd._lib import GacError
    tg, qg = block_case[:2]
    T1, Q1 = len(tg.codes[1]), len(qg.codes[1])
    one = np.array([1], np.int32)

    def run(blocks, strand=0, off=None):
        b = np.asarray(blocks, np.int32).reshape(-1, 3)
        off = np.array([0, len(b)], np.int64) if off is None else off
        k = len(off) - 1
        return block_engine.score_blocks(np.repeat(one, k), np.repeat(one, k),
                                         np.full(k, strand, np.uint8), off, b[:, 0], b[:, 1], b[:, 2])

    good = [(10, 10, 5), (T1 - 5, Q1 - 5, 5), (0, 0, 0), (T1, Q1, 0)]
    for strand in (0, 1):
        assert len(run(good, strand)) == 4
        for bad in ((T1 - 4, 10, 5), (10, Q1 - 4, 5), (-1, 10, 5), (10, -1, 5), (T1 + 1, 0, 0),
                    (0, Q1 + 1, 0), (10, 10, -1)):
            blocks = good[:3] + [bad] + good + [(T1, 0, 1)]  # (a second bad one, later)
            with pytest.raises(GacError) as ei:
                run(blocks, strand)
            assert ei.value.code == GAC_E_ARG
            assert f"block 3 ({bad[0]} {bad[1]} {bad[2]})" in str(ei.value), str(ei.value)
    # across the 2^20-block chunks of the fill, two pairs
    n = (1 << 20) + 10
    big = np.tile(np.array([[10, 10, 1]], np.int32), (n, 1))
    off = np.array([0, 1 << 20, n], np.int64)
    big[(1 << 20) + 5] = (T1, 0, 1)
    with pytest.raises(GacError) as ei:
        run(big, 1, off)
    assert ei.value.code == GAC_E_ARG and f"block {(1 << 20) + 5} (" in str(ei.value), str(ei.value)
    big[7] = (0, Q1, 1)
    with pytest.raises(GacError) as ei:
        run(big, 1, off)
    assert ei.value.code == GAC_E_ARG and "block 7 (" in str(ei.value), str(ei.value)


# ------------------------------------------------------------------ gac_crossovers
@pytest.fixture(scope="module")
def xover_case():
    return AX.xover_case_set()


@pytest.fixture(scope="module")
def xover_engine(xover_case):
    e = _engine(xover_case[0], xover_case[1], BLASTZ)
    yield e
    e.close()


def _xover_ref(tg, qg, mat, jobs):
    M = AX.code_matrix(mat)
    cache = {}
    r = [AX.crossover_at(tg, qg, M, *(int(x) for x in j), _cache=cache) for j in jobs]
    return np.array([p for p, _ in r], np.int64), np.array([a for _, a in r], np.int64)


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_crossovers_vs_reference(xover_case, xover_engine, mat):
    """Overlaps of 0 .. 1000 bases with the crafted difference sequences (no
    maximum, a maximum of exactly 0, ties within and across the 64-base
    segments, a maximum only the carried sum shows or only the last partial
    segment holds), random ones, N on either block and at the winning
    position, overlaps touching base 0 and the last base; '+' and '-'."""
    from genomealignmenttools_amd.gachain import GapCosts
    tg, qg, jobs, _ = xover_case
    assert set(AX.OVS) <= set(jobs[:, 7].tolist()) and set(jobs[:, 2].tolist()) == {0, 1}
    xover_engine.set_scoring(MATS[mat], GapCosts("loose"))
    wpos, wadj = _xover_ref(tg, qg, MATS[mat], jobs)
    pos, adj = xover_engine.crossovers(*jobs.T)
    _same(pos, wpos, "gac_crossovers pos", lambda i: jobs[i].tolist())
    _same(adj, wadj, "gac_crossovers adj", lambda i: jobs[i].tolist())
    # what the crafted sequences are built for (both matrices share the diagonal)
    assert {0, 1, 64, 65, 128, 129, 130, 191, 1000} <= set(wpos.tolist())


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_crossovers_grid_stride(xover_case, xover_engine, mat):
    """40 000 short random overlaps in one call: the launch caps at 8192
    workgroups of four waves, so the waves loop over the jobs."""
    from genomealignmenttools_amd.gachain import GapCosts
    tg, qg = xover_case[:2]
    n = 40_000
    rng = np.random.default_rng(4)
    ov = rng.integers(0, 25, n)
    strand = rng.integers(0, 2, n)
    q_seq = np.where(strand == 1, 2, 1)
    T, Qp, Qm = len(tg.codes[1]), len(qg.codes[1]), len(qg.codes[2])
    qlen = np.where(strand == 1, Qm, Qp)
    jobs = np.stack([np.ones(n, np.int64), q_seq, strand,
                     ov + rng.integers(0, qlen - 24), ov + rng.integers(0, T - 24, n),
                     rng.integers(0, qlen - 24), rng.integers(0, T - 24, n), ov], 1).astype(np.int32)
    xover_engine.set_scoring(MATS[mat], GapCosts("loose"))
    wpos, wadj = _xover_ref(tg, qg, MATS[mat], jobs)
    pos, adj = xover_engine.crossovers(*jobs.T)
    _same(pos, wpos, "gac_crossovers pos (40 000 jobs)", lambda i: jobs[i].tolist())
    _same(adj, wadj, "gac_crossovers adj (40 000 jobs)", lambda i: jobs[i].tolist())
    assert (wpos > 0).sum() > 10_000 and (wpos == 0).sum() > 10_000


def test_crossovers_errors(xover_case, xover_engine):
    """An overlap that leaves its sequence is GAC_E_ARG (and names the job)."""
    from genomealignmenttools_amd._lib import GacError
    tg, qg = xover_case[:2]
    T, Q = len(tg.codes[1]), len(qg.codes[1])
    good = (1, 1, 0, 20, 20, 30, 30, 10)
    assert len(xover_engine.crossovers(*np.array([good], np.int32).T)[0]) == 1
    for bad in ((1, 1, 0, 9, 20, 30, 30, 10), (1, 1, 0, 20, 9, 30, 30, 10),
                (1, 1, 0, 20, 20, Q - 9, 30, 10), (1, 1, 0, 20, 20, 30, T - 9, 10),
                (1, 1, 1, Q + 1, 20, 30, 30, 10), (1, 1, 0, 20, T + 1, 30, 30, 10),
                (1, 1, 0, 20, 20, -1, 30, 10), (1, 1, 0, 20, 20, 30, -1, 10),
                (1, 1, 0, 20, 20, 30, 30, -1), (9, 1, 0, 20, 20, 30, 30, 10)):
        with pytest.raises(GacError) as ei:
            xover_engine.crossovers(*np.array([good, good, bad, good], np.int32).T)
        assert ei.value.code == GAC_E_ARG, bad
        if bad[0] == 1:
            assert "overlap 2 " in str(ei.value), str(ei.value)


# ------------------------------------------------------------------ the text kernels
@pytest.fixture(scope="module")
def plain_engine():
    from genomealignmenttools_amd.gachain import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_text_kernels_vs_reference(plain_engine, mat):
    """The same difference sequences as caller text, upper and lower case
    mixed, with N, n, '-', '.' and a byte >= 0x80 among the bases; size 0 and
    sizes that are no multiple of 64."""
    texts = AX.text_case_set()
    TM = AX.text_matrix(MATS[mat])
    sizes = {len(t[0]) for t in texts}
    assert 0 in sizes and any(s % 64 for s in sizes) and any(s > 128 for s in sizes)
    assert any(0xE9 in t[k] for t in texts for k in range(4))
    want = [AX.crossover(*t, TM) for t in texts]
    pos, adj = plain_engine.text_crossovers(*zip(*texts), MATS[mat])
    _same(pos, [p for p, _ in want], "gac_text_crossovers pos", lambda i: len(texts[i][0]))
    _same(adj, [a for _, a in want], "gac_text_crossovers adj", lambda i: len(texts[i][0]))
    rng = np.random.default_rng(2)
    alphabet = np.frombuffer(b"acgtACGTacgtACGTNn-.\xe9", np.uint8)
    long_q, long_t = (alphabet[rng.integers(0, len(alphabet), 5003)].tobytes() for _ in range(2))
    q = [t[0] for t in texts] + [t[2] for t in texts] + [long_q]
    t = [t[1] for t in texts] + [t[3] for t in texts] + [long_t]
    got = plain_engine.score_text_blocks(q, t, MATS[mat])
    _same(got, [AX.text_block_score(a, b, TM) for a, b in zip(q, t)], "gac_score_text_blocks",
          lambda i: len(q[i]))


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_text_kernels_grid_stride(plain_engine, mat):
    """70 000 short random texts in one call of each text kernel: their
    launches cap at 16384 workgroups of four waves (65536 jobs at once), so
    only more jobs than that make the waves loop."""
    n = 70_000
    rng = np.random.default_rng(8)
    alphabet = np.frombuffer(b"acgtACGTacgtACGTacgtACGTNn-.\xe9", np.uint8)
    ov = rng.integers(0, 17, n)
    off = np.concatenate([[0], np.cumsum(ov)])
    four = []
    for _ in range(4):
        buf = alphabet[rng.integers(0, len(alphabet), int(off[-1]))].tobytes()
        four.append([buf[off[i]:off[i + 1]] for i in range(n)])
    TM = AX.text_matrix(MATS[mat])
    want = [AX.crossover(a, b, c, d, TM) for a, b, c, d in zip(*four)]
    pos, adj = plain_engine.text_crossovers(*four, MATS[mat])
    _same(pos, [p for p, _ in want], "gac_text_crossovers pos (70 000 jobs)")
    _same(adj, [a for _, a in want], "gac_text_crossovers adj (70 000 jobs)")
    got = plain_engine.score_text_blocks(four[0], four[1], MATS[mat])
    _same(got, [AX.text_block_score(a, b, TM) for a, b in zip(four[0], four[1])],
          "gac_score_text_blocks (70 000 jobs)")


# ------------------------------------------------------------------ chainConnectCost in the DP kernels
_MINORANT = {}


def gap_minorant(gap):
    """lin_k: the floor of 1024 x the smallest cost(d) / d over d >= 1 and the
    three kinds of gap (query only, target only, both), minus 1 -- a true
    linear minorant of the gap costs.  Past the last table position the cost
    is linear, so its ratio lies between the last position's and the slope."""
    if gap.name in _MINORANT:
        return _MINORANT[gap.name]
    g = gap.ptr.contents
    last = max(g.q_last_pos, g.t_last_pos, g.b_last_pos) + 2
    best = None
    for d in range(1, last + 1):
        costs = [gap.cost(d, 0), gap.cost(0, d)] + ([gap.cost(1, d - 1)] if d >= 2 else [])
        k = min(1024 * c // d for c in costs)
        best = k if best is None or k < best else best
    for slope in (g.q_last_slope, g.t_last_slope, g.b_last_slope):
        assert slope >= 0
        best = min(best, int(np.floor(1024 * slope)))
    _MINORANT[gap.name] = best - 1
    return best - 1


@pytest.fixture(scope="module")
def dp_case():
    return AX.dp_case_set()


def _dp_check(engine, case, mat, gap, configs):
    """Run gac_chain_dp_blocks on the cases of `case` that survive the pruning
    condition, once per config (fast, lin_k, ov_cap), and compare with the
    two-leaf expectation.  Returns (pairs run, pairs dropped)."""
    tg, qg, t_seq, q_seq, q_strand, _, box, a_first, kind, ov = case
    score, cost, total, pred, keep = AX.dp_expected(tg, qg, MATS[mat], gap.cost, case)
    n = len(keep)
    assert (n - keep.sum()) <= 0.05 * n
    crafted = np.array([k.startswith("ov_") and not k.startswith("ov_skew") for k in kind])
    for o in AX.DP_OVS:
        assert (keep & crafted & (ov == o)).sum() >= 20, o
    sel = np.flatnonzero(keep)
    blk = np.stack([2 * sel, 2 * sel + 1], 1).reshape(-1)
    m = len(sel)
    off = np.arange(0, 2 * m + 1, 2, dtype=np.int64)
    want_tord = np.stack([np.where(a_first[sel], 0, 1), np.where(a_first[sel], 1, 0)], 1).reshape(-1)
    min_entry = min(0, int(np.min(MATS[mat])))
    engine.set_scoring(MATS[mat], gap)
    row = lambda i: (kind[sel[i // 2]], int(ov[sel[i // 2]]), box[blk[i]].tolist(),  # noqa: E731
                     int(cost[sel[i // 2]]))
    for fast, lin_k, ov_cap in configs:
        leaf_off, tord, got_total, got_pred = engine.chain_dp_blocks(
            t_seq[sel], q_seq[sel], q_strand[sel], off, box[blk], score[blk], fast=fast,
            lin_k=lin_k, min_entry=min_entry, ov_cap=ov_cap)
        what = f"{mat} fast={fast} lin_k={lin_k} ov_cap={ov_cap}"
        _same(leaf_off, off, "leaf_off, " + what)
        _same(tord, want_tord, "tord, " + what, row)
        _same(got_total, total[blk], "total, " + what, row)
        _same(got_pred, pred[blk], "pred, " + what, row)
    return m, n - m


@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_dp_connect_cost_vs_reference(dp_case, mat):
    """Two blocks per pair, A strictly before B: gaps on either or both axes,
    abutting blocks, overlaps of 1 .. 200 bases with crafted differences,
    overlaps with dq != dt, overlaps as large as the smaller block (cost
    100000000: no connection).  total / pred / leaf_off / tord of k_dp (fast =
    0) and k_dp_spec (fast = 1; without and with a true linear minorant of the
    gap costs; ov_cap 0 and the default) equal findBestPredecessors on two
    leaves with the plain chainConnectCost."""
    from genomealignmenttools_amd.gachain import GapCosts
    gap = GapCosts("loose")
    lin_k = gap_minorant(gap)
    assert lin_k > 0
    e = _engine(dp_case[0], dp_case[1])
    try:
        configs = [(0, 0, 1024)] + [(1, k, cap) for k in (0, lin_k) for cap in (0, 1024)]
        m, dropped = _dp_check(e, dp_case, mat, gap, configs)
    finally:
        e.close()
    print(f"{mat}: {m} pairs run, {dropped} dropped by the pruning condition, lin_k {lin_k}")
    assert m >= 2000


def _dp_child():
    """k_dp_fast (GAC_DP_WAVES=1, read once per process): both matrices."""
    from genomealignmenttools_amd.gachain import GapCosts
    gap = GapCosts("loose")
    lin_k = gap_minorant(gap)
    case = AX.dp_case_set()
    e = _engine(case[0], case[1])
    out = {}
    for mat in MATS:
        out[mat] = _dp_check(e, case, mat, gap, [(1, k, cap) for k in (0, lin_k) for cap in (0, 1024)])
    e.close()
    print(json.dumps({"ok": True, "pairs": {k: int(v[0]) for k, v in out.items()}}))


def test_dp_connect_cost_one_wave_kernel():
    """The same cases through k_dp_fast, the one-wave fast search: GAC_DP_WAVES
    is read once per process, so in a fresh one."""
    env = dict(os.environ, GAC_DP_WAVES="1", GAC_TIMING="1")
    code = ("import sys; sys.path[:0] = [%r, %r]; import torch; "
            "import test_gpu_axt_primitives as T; T._dp_child()" % (os.path.join(REPO, "tests"), REPO))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["ok"] and min(res["pairs"].values()) >= 2000
    assert "k_dp_fast" in r.stderr and "k_dp_spec" not in r.stderr
