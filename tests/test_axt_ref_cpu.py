"""Pin the plain references of tests/axt_ref.py on the CPU: block scores
against the C oracle, crossover and connect cost against what the reference's
own kent objects print, and the hand-built case sets against deliberately
wrong variants of the references -- so the shapes the GPU tests run
(tests/test_gpu_axt_primitives.py) are known to tell those bugs apart."""
import os
import subprocess

import numpy as np
import pytest

from conftest import BLASTZ, GOLDEN

import axt_ref as AX

MATS = {"blastz": BLASTZ, "asym": AX.ASYM}


def test_asym_matrix_is_asymmetric():
    m = np.array(AX.ASYM)
    comp = [3, 2, 1, 0]  # A<->T, C<->G
    off = ~np.eye(4, dtype=bool)
    assert (m != m.T)[off].all()
    assert (m != m[np.ix_(comp, comp)])[off].all()
    assert (np.diag(m) == np.diag(np.array(BLASTZ))).all()
    for name, M in (("blastz", AX.code_matrix(BLASTZ)), ("asym", AX.code_matrix(AX.ASYM))):
        for pal in (AX.FREE, AX.SHARED_Q, AX.SHARED_T):  # the palettes' differences hold with both
            for d, s in pal.items():
                lq, lt, rq, rt = AX.letters_to_codes(s)
                assert M[lq, lt] - M[rq, rt] == d, (name, s)


# ------------------------------------------------------------------ against the C oracle
@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_block_scores_vs_oracle(mat):
    """block_scores == OracleScorer.score_ranges on one-block chains over their
    full range: both strands, N runs, an asymmetric matrix."""
    from genomealignmenttools_amd.chainfile import ChainArrays
    from oracle.oracle import OracleScorer, genome_text
    tg, qg, t_seq, q_seq, q_strand, blk_off, bt, bq, bs = AX.block_case_set()
    want = AX.block_scores(tg, qg, MATS[mat], t_seq, q_seq, q_strand, blk_off, bt, bq, bs)
    pair = np.repeat(np.arange(len(t_seq)), np.diff(blk_off))
    sel = np.flatnonzero(bs > 0)  # (a chain needs a base)
    n = len(sel)
    ts, qs = t_seq[pair[sel]], q_seq[pair[sel]]
    ca = ChainArrays(
        score=np.zeros(n), tname=[tg.names[i] for i in ts],
        tsize=np.array([len(tg.codes[i]) for i in ts], np.int32), tstart=bt[sel],
        tend=bt[sel] + bs[sel], qname=[qg.names[i] for i in qs],
        qsize=np.array([len(qg.codes[i]) for i in qs], np.int32), qstrand=q_strand[pair[sel]],
        qstart=bq[sel], qend=bq[sel] + bs[sel], id=np.arange(1, n + 1, dtype=np.int64),
        blk_off=np.arange(n + 1, dtype=np.int64), blk_t=bt[sel], blk_q=bq[sel], blk_size=bs[sel])
    R = np.stack([np.arange(n), ca.tstart, ca.tend], 1)
    g, _, a = OracleScorer(genome_text(tg), genome_text(qg), MATS[mat], "loose").score_ranges(ca, R)
    assert np.array_equal(a, bs[sel])
    assert np.array_equal(g, want[sel])
    assert (want[bs == 0] == 0).all()
    assert (q_strand[pair[sel]] == 1).sum() > 300 and len(set(want[sel].tolist())) > 300


# ------------------------------------------------------------------ against the reference
def _letters(c):
    return np.frombuffer(b"tcagn", np.uint8)[c].tobytes()


@pytest.mark.parametrize("seed", [11, 12])
def test_crossover_and_connect_cost_vs_reference(seed):
    """connect_cost, crossover (codes and text) and the block scores reproduce
    every `s`, `c` and `o` line the reference's kent objects print for the
    kent-API workload (oracle/kentapi_workload.inc: chainScoreBlock of every
    block, chainConnectCost of adjacent blocks, and of the right block pulled
    back into an overlap with its cBlockFindCrossover)."""
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GapCosts
    from oracle.oracle import have_ref, ref_tool
    import antirepeat_ref as AR
    if not have_ref():
        pytest.skip("oracle/_ref not built (needs the reference tree)")
    d = os.path.join(GOLDEN, f"synth{seed}")
    nmax = 150
    ref = subprocess.run([ref_tool("kentref"), "kentapi", os.path.join(d, "in.chain"),
                          os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"), "-", "loose",
                          str(nmax)], capture_output=True, text=True, timeout=300)
    assert ref.returncode == 0, ref.stderr[-2000:]
    want = {"s": {}, "c": {}, "o": {}}
    for ln in ref.stdout.splitlines():
        f = ln.split()
        if f[0] in want:
            want[f[0]][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
    tg, qg = AR.read_2bit(os.path.join(d, "t.2bit")), AR.read_2bit(os.path.join(d, "q.2bit"))
    ca = read_chains(os.path.join(d, "in.chain"))
    gap = GapCosts("loose")
    M, TM = AX.code_matrix(BLASTZ), AX.text_matrix(BLASTZ)
    n = min(nmax, ca.n)
    t_seq = np.array([tg.index(x) for x in ca.tname[:n]], np.int32)
    q_seq = np.array([qg.index(x) for x in ca.qname[:n]], np.int32)
    nb = int(ca.blk_off[n])
    sc = AX.block_scores(tg, qg, BLASTZ, t_seq, q_seq, ca.qstrand[:n], ca.blk_off[:n + 1],
                         ca.blk_t[:nb], ca.blk_q[:nb], ca.blk_size[:nb])
    got = {"s": {}, "c": {}, "o": {}}
    cache = {}
    for ci in range(n):
        assert int(ca.qsize[ci]) == len(qg.codes[q_seq[ci]])
        mi = int(ca.qstrand[ci])
        T = cache.setdefault(("t", int(t_seq[ci])), AX.codes(tg, int(t_seq[ci])))
        Q = cache.setdefault(("q", int(q_seq[ci]), bool(mi)), AX.strand_codes(qg, int(q_seq[ci]), mi))
        bt, bq, bs = (x.astype(np.int64) for x in ca.blocks(ci))
        b0 = int(ca.blk_off[ci])

        def xo(lqe, lte, rqs, rts, ov):
            r = AX.crossover_at(tg, qg, M, int(t_seq[ci]), int(q_seq[ci]), mi, lqe, lte, rqs, rts,
                                ov, _cache=cache)
            # the text form on the decoded letters gives the same
            assert r == AX.crossover(_letters(Q[lqe - ov:lqe]), _letters(T[lte - ov:lte]),
                                     _letters(Q[rqs:rqs + ov]).upper(), _letters(T[rts:rts + ov]), TM)
            return r

        for k in range(len(bs)):
            s = int(sc[b0 + k])
            assert s == AX.text_block_score(_letters(Q[bq[k]:bq[k] + bs[k]]),
                                            _letters(T[bt[k]:bt[k] + bs[k]]), TM)
            got["s"][(ci, k)] = (s, s)
        for k in range(len(bs) - 1):
            A = (bq[k], bq[k] + bs[k], bt[k], bt[k] + bs[k])
            B = (bq[k + 1], bq[k + 1] + bs[k + 1], bt[k + 1], bt[k + 1] + bs[k + 1])
            got["c"][(ci, k)] = (AX.connect_cost(A, B, gap.cost, xo),)
            # the workload's forced overlap: half of the smaller block
            asz, bsz = int(bs[k]), int(bs[k + 1])
            ov = min(asz, bsz) // 2
            if ov < 1:
                continue
            sh = int(B[2] - A[3]) + ov
            B2 = tuple(int(x) - sh for x in B)
            if B2[0] <= A[0] or B2[2] <= A[2] or B2[0] < 0:
                continue
            dq, dt = B2[0] - A[1], B2[2] - A[3]
            o = -min(dq, dt)
            pos, adj = -1, 0
            if 0 < o < asz and o < B2[3] - B2[2]:
                pos, adj = xo(int(A[1]), int(A[3]), B2[0], B2[2], int(o))
            got["o"][(ci, k)] = (AX.connect_cost(A, B2, gap.cost, xo), pos, adj)
    for tag in "sco":
        assert len(want[tag]) > 500
        assert got[tag].keys() == want[tag].keys(), tag
        bad = [(k, got[tag][k], want[tag][k]) for k in want[tag] if got[tag][k] != want[tag][k]]
        assert not bad, (tag, bad[:5])
    assert sum(1 for v in want["o"].values() if v[1] > 0) > 50  # real crossovers among them


# ------------------------------------------------------------------ the inputs discriminate
def _loop_ge(l, r):
    r_score, l_score = sum(r), sum(l)
    score = best = r_score
    pos = 0
    for i in range(len(l)):
        score += l[i] - r[i]
        if score >= best:
            best, pos = score, i + 1
    return pos, r_score + l_score - best


def _loop_last_max(l, r):
    r_score, l_score = sum(r), sum(l)
    score = best = r_score
    pos = 0
    for i in range(len(l)):
        score += l[i] - r[i]
        if score > best or (score == best and pos > 0):
            best, pos = score, i + 1
    return pos, r_score + l_score - best


def _loop_best_from_0(l, r):
    r_score, l_score = sum(r), sum(l)
    score, best, pos = r_score, 0, 0
    for i in range(len(l)):
        score += l[i] - r[i]
        if score > best:
            best, pos = score, i + 1
    return pos, r_score + l_score - best


def _loop_restart_64(l, r):
    r_score, l_score = sum(r), sum(l)
    score = best = r_score
    pos = 0
    for i in range(len(l)):
        if i and i % 64 == 0:
            score = r_score  # the carry of the earlier segments is lost
        score += l[i] - r[i]
        if score > best:
            best, pos = score, i + 1
    return pos, r_score + l_score - best


def _q_no_complement(g, i, minus):
    c = AX.codes(g, i)
    return c[::-1] if minus else c


def _q_not_reversed(g, i, minus):
    c = AX.codes(g, i)
    return np.where(c == AX.N_CODE, AX.N_CODE, c ^ 2) if minus else c


def _t_n_as_t(g, i):
    return g.codes[i].astype(np.int64)


def _q_n_as_t(g, i, minus):
    c = g.codes[i].astype(np.int64)
    return (c ^ 2)[::-1] if minus else c


LOOPS = {"ge_instead_of_gt": _loop_ge, "last_maximum": _loop_last_max,
         "best_from_0": _loop_best_from_0, "restart_every_64": _loop_restart_64}
# name -> keyword arguments of block_scores / crossover_at (M: transposed)
VIEWS = {"matrix_transposed": dict(transpose=True), "no_complement": dict(qview=_q_no_complement),
         "not_reversed": dict(qview=_q_not_reversed),
         "n_as_t_query": dict(qview=_q_n_as_t), "n_as_t_target": dict(tview=_t_n_as_t)}


def _xover_all(tg, qg, jobs, mat, loop=AX.crossover_lr, transpose=False, **kw):
    M = AX.code_matrix(mat)
    M = M.T.copy() if transpose else M
    cache = {}
    return [AX.crossover_at(tg, qg, M, *(int(x) for x in j), loop=loop, _cache=cache, **kw)
            for j in jobs]


def _blocks_all(case, mat, transpose=False, **kw):
    M = AX.code_matrix(mat)
    return AX.block_scores(*case[:2], mat, *case[2:], M=M.T.copy() if transpose else M, **kw)


def test_case_sets_discriminate():
    """Every deliberately wrong variant of the plain reference differs from
    the true one on at least one hand-built case -- per kernel family: the
    genome crossovers, the genome blocks, the text crossovers."""
    tg, qg, jobs, strings = AX.xover_case_set()
    bcase = AX.block_case_set()
    texts = AX.text_case_set()
    caught = {}
    true_x = {m: _xover_all(tg, qg, jobs, MATS[m]) for m in MATS}
    true_b = {m: _blocks_all(bcase, MATS[m]) for m in MATS}
    true_t = {m: [AX.crossover(*t, AX.text_matrix(MATS[m])) for t in texts] for m in MATS}
    # the strings the builder reports are what the genomes hold
    for m in MATS:
        M = AX.code_matrix(MATS[m])
        assert true_x[m] == [AX.crossover(*(AX.letters_to_codes(s) for s in four), M)
                             for four in strings]
    for name, loop in LOOPS.items():
        caught["xover/" + name] = any(_xover_all(tg, qg, jobs, MATS[m], loop=loop) != true_x[m]
                                      for m in MATS)
        caught["text/" + name] = any(
            [AX.crossover(*t, AX.text_matrix(MATS[m]), loop=loop) for t in texts] != true_t[m]
            for m in MATS)
    for name, kw in VIEWS.items():
        caught["xover/" + name] = any(_xover_all(tg, qg, jobs, MATS[m], **kw) != true_x[m]
                                      for m in MATS)
        caught["blocks/" + name] = any(
            not np.array_equal(_blocks_all(bcase, MATS[m], **kw), true_b[m]) for m in MATS)
    caught["text/matrix_transposed"] = any(
        [AX.crossover(*t, AX.text_matrix(MATS[m]).T.copy()) for t in texts] != true_t[m]
        for m in MATS)
    print("\n".join(f"{k}: {'caught' if v else 'MISSED'}" for k, v in sorted(caught.items())))
    assert all(caught.values()), [k for k, v in caught.items() if not v]
    assert len(caught) == 2 * len(LOOPS) + 2 * len(VIEWS) + 1
    # BLASTZ alone cannot see a transposition (it is symmetric): the asymmetric
    # matrix is what catches it
    assert _xover_all(tg, qg, jobs, BLASTZ, transpose=True) == true_x["blastz"]
    assert np.array_equal(_blocks_all(bcase, BLASTZ, transpose=True), true_b["blastz"])


def test_crossover_patterns_give_what_they_are_built_for():
    """The crafted difference sequences land where the issue says, with BLASTZ."""
    M = AX.code_matrix(BLASTZ)
    P = dict(AX.xover_patterns())

    def run(name):
        lq, lt, rq, rt = (AX.letters_to_codes(s) for s in AX.build_strings(P[name]))
        pos, adj = AX.crossover(lq, lt, rq, rt, M)
        return pos, adj, int(M[lq, lt].sum())

    for ov in AX.OVS:
        assert run(f"zero{ov}")[0] == 0
        pos, adj, ls = run(f"neg{ov}")
        assert pos == 0 and adj == ls
        assert run(f"pos{ov}")[0] == ov
        assert run(f"max0_{ov}")[0] == 0
        assert run(f"tie{ov}")[0] == (1 if ov else 0)
    assert run("tie200")[0] == 1
    for k in (63, 64, 127, 128):
        assert run(f"first{k}")[0] == k + 1 and run(f"first{k}_again")[0] == k + 1
    assert run("seg0_seg1")[0] == 11 and run("seg0_seg1_edge")[0] == 64
    assert run("last_partial")[0] == 130 and run("last_partial_1")[0] == 130
    # 64 x +9 (576 at k = 63), 63 x -9 (9), 64 x +9: 585 at k = 190 -- above 576
    # only when the first two segments' sums are carried along
    assert run("carry")[0] == 191


# ------------------------------------------------------------------ the DP cases survive the pruning
@pytest.mark.parametrize("mat", ["blastz", "asym"])
def test_dp_cases_survive_pruning(mat):
    """At most 5 % of the two-block DP cases fall to the condition that the
    reference's pruning cannot interfere, and every overlap length and every
    relation of A and B survives; both outcomes (connected or not) occur."""
    from genomealignmenttools_amd.gachain import GapCosts
    case = AX.dp_case_set()
    tg, qg = case[:2]
    kind, ov = case[8], case[9]
    score, cost, total, pred, keep = AX.dp_expected(tg, qg, MATS[mat], GapCosts("loose").cost, case)
    n = len(keep)
    print(f"{mat}: {n} pairs, {n - int(keep.sum())} dropped ({100.0 * (n - keep.sum()) / n:.2f} %)")
    assert n >= 2000 and (n - keep.sum()) <= 0.05 * n
    assert score.min() > 0 and np.median(score) > 5000
    kinds = np.array(kind)
    for k in sorted(set(kind)):
        assert keep[kinds == k].any(), k
    crafted = np.array([k.startswith("ov_") and not k.startswith("ov_skew") for k in kind])
    for o in AX.DP_OVS:
        assert (keep & crafted & (ov == o)).sum() >= 20, o
    has = pred.reshape(-1, 2).max(axis=1) >= 0
    assert (has & keep).sum() > 200 and (~has & keep).sum() > 100
    assert (cost[keep & (kinds == "enclosed")] >= AX.BIG_OVERLAP).all()
    assert not has[kinds == "enclosed"].any()
