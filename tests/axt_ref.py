"""Plain numpy / Python restatements of the reference operations behind
axtChain's device primitives, and the hand-built case sets the CPU and GPU
tests share (tests/test_axt_ref_cpu.py, tests/test_gpu_axt_primitives.py).

Written from the reference's text:
  axtScoreUngapped / chainScoreBlock   kent/src/lib/axt.c:186-194, chainConnect.c:14-22
  cBlockFindCrossover                  kent/src/lib/chainConnect.c:61-105 (the loop :91-104)
  chainConnectCost                     kent/src/lib/chainConnect.c:114-149
  bestPredecessor / findBestPredecessors  kent/src/lib/chainBlock.c:207-304

Sequences are synth.Genome codes (T=0 C=1 A=2 G=3) with N = 4 laid over the
N runs; a '-' query in strand coordinates is the reverse complement, base x =
comp(fwd[qSize - 1 - x]) (reverseComplement, kent/src/lib/dnautil.c:404-462).
The score matrix is mat[query][target] in A, C, G, T order (axt.c:423-458);
N scores 0 against everything.  Everything is exact integers.
"""
import numpy as np

from genomealignmenttools_amd import synth

N_CODE = 4
# An asymmetric matrix ([query][target], A C G T): mat[q][t] != mat[t][q] and
# != mat[comp q][comp t], so a transposition or a missing complement shows
# (BLASTZ hides both).  The diagonal and the entries the palettes below use
# keep BLASTZ's differences (+-9), so the crafted ties stay ties.
ASYM = [[91, -114, -31, -123], [-104, 100, -135, -41], [-21, -120, 100, -99],
        [-113, -36, -124, 91]]
_LETTER_CODE = {"T": 0, "C": 1, "A": 2, "G": 3, "N": 4}
_CODE_LETTER = "TCAGN"


# ------------------------------------------------------------------ matrices
def code_matrix(mat):
    """[query code][target code] int64 5 x 5: N (4) scores 0."""
    m = np.zeros((5, 5), np.int64)
    m[:4, :4] = synth.matrix_by_code(np.asarray(mat, np.int64).reshape(4, 4))
    return m


def text_matrix(mat):
    """kent's matrix[256][256] (axt.c:402-458, propagateCase): acgt in either
    case score mat[q][t], every other byte scores 0."""
    mat = np.asarray(mat, np.int64).reshape(4, 4)
    m = np.zeros((256, 256), np.int64)
    for i, a in enumerate("acgt"):
        for j, b in enumerate("acgt"):
            for x in (a, a.upper()):
                for y in (b, b.upper()):
                    m[ord(x), ord(y)] = mat[i, j]
    return m


def _idx(s):
    """bytes / latin-1 str / integer sequence -> index array"""
    if isinstance(s, str):
        s = s.encode("latin-1")
    if isinstance(s, (bytes, bytearray)):
        return np.frombuffer(bytes(s), np.uint8).astype(np.int64)
    return np.asarray(s, np.int64)


# ------------------------------------------------------------------ sequences
def codes(g, i):
    """forward codes of sequence i, N = 4 over the N runs"""
    c = g.codes[i].astype(np.int64)
    for a, l in zip(*g.nruns[i]):
        c[a:a + l] = N_CODE
    return c


def strand_codes(g, i, minus):
    """the sequence in strand coordinates: '-' is the reverse complement
    (T<->A, C<->G: code ^ 2; N stays N)"""
    c = codes(g, i)
    if minus:
        c = c[::-1]
        c = np.where(c == N_CODE, N_CODE, c ^ 2)
    return c


def _flat_index(start, size):
    size = np.asarray(size, np.int64)
    tot = int(size.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    first = np.repeat(np.asarray(start, np.int64), size)
    return first + np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(size) - size, size)


# ------------------------------------------------------------------ block scores
def block_scores(tg, qg, mat, t_seq, q_seq, q_strand, blk_off, blk_t, blk_q, blk_size,
                 qview=strand_codes, M=None, tview=codes):
    """axtScoreUngapped (axt.c:186-194) of every block: score = sum over i <
    size of matrix[q[i]][t[i]], q in the pair's strand coordinates.  Pair p
    holds blocks [blk_off[p], blk_off[p+1]).  int64 per block.
    (qview / tview / M: only the deliberately wrong variants of the CPU test pass them.)"""
    M = code_matrix(mat) if M is None else M
    blk_t, blk_q, blk_size = (np.asarray(x, np.int64) for x in (blk_t, blk_q, blk_size))
    out = np.zeros(len(blk_size), np.int64)
    tcache, qcache = {}, {}
    for p in range(len(t_seq)):
        b0, b1 = int(blk_off[p]), int(blk_off[p + 1])
        if b0 == b1:
            continue
        ts, qs, mi = int(t_seq[p]), int(q_seq[p]), bool(q_strand[p])
        if ts not in tcache:
            tcache[ts] = tview(tg, ts)
        if (qs, mi) not in qcache:
            qcache[(qs, mi)] = qview(qg, qs, mi)
        T, Q = tcache[ts], qcache[(qs, mi)]
        sz = blk_size[b0:b1]
        v = M[Q[_flat_index(blk_q[b0:b1], sz)], T[_flat_index(blk_t[b0:b1], sz)]]
        cs = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
        end = np.cumsum(sz)
        out[b0:b1] = cs[end] - cs[end - sz]
    assert (np.abs(out) < 2 ** 31).all()  # the reference's int
    return out


def text_block_score(q, t, TM):
    """chainScoreBlock / axtScoreUngapped on caller text (chainConnect.c:14-22)."""
    q, t = _idx(q), _idx(t)
    assert len(q) == len(t)
    return int(TM[q, t].sum())


# ------------------------------------------------------------------ crossover
def crossover_lr(l, r):
    """The loop of cBlockFindCrossover (chainConnect.c:91-104) on the per-base
    scores of the left block's last and the right block's first `overlap`
    bases: (pos, adj)."""
    r_score = sum(r)
    l_score = sum(l)
    score = best = r_score
    pos = 0
    for i in range(len(l)):
        score += l[i]
        score -= r[i]
        if score > best:
            best = score
            pos = i + 1
    return pos, r_score + l_score - best


def crossover(lq, lt, rq, rt, M, loop=crossover_lr):
    """cBlockFindCrossover on four equal-length strings: genome codes with
    code_matrix, or text with text_matrix.  (pos, adj)."""
    lq, lt, rq, rt = _idx(lq), _idx(lt), _idx(rq), _idx(rt)
    assert len(lq) == len(lt) == len(rq) == len(rt)
    return loop(M[lq, lt].tolist(), M[rq, rt].tolist())


def crossover_at(tg, qg, M, t_seq, q_seq, strand, lqe, lte, rqs, rts, ov, qview=strand_codes,
                 loop=crossover_lr, _cache=None, tview=codes):
    """cBlockFindCrossover in genome coordinates: the left block ends at
    (lqe, lte), the right one starts at (rqs, rts), query in strand coordinates
    (chainConnect.c:69-72)."""
    if _cache is None:
        _cache = {}
    kt, kq = ("t", t_seq), ("q", q_seq, bool(strand))
    if kt not in _cache:
        _cache[kt] = tview(tg, t_seq)
    if kq not in _cache:
        _cache[kq] = qview(qg, q_seq, bool(strand))
    T, Q = _cache[kt], _cache[kq]
    assert 0 <= lqe - ov and lqe <= len(Q) and 0 <= rqs and rqs + ov <= len(Q)
    assert 0 <= lte - ov and lte <= len(T) and 0 <= rts and rts + ov <= len(T)
    return crossover(Q[lqe - ov:lqe], T[lte - ov:lte], Q[rqs:rqs + ov], T[rts:rts + ov], M, loop)


# ------------------------------------------------------------------ connect cost
BIG_OVERLAP = 100000000


def connect_cost(a, b, gap_cost, xover):
    """chainConnectCost (chainConnect.c:114-149).  a, b = (qStart, qEnd,
    tStart, tEnd); gap_cost(dq, dt) = gapCalcCost; xover(lqe, lte, rqs, rts,
    overlap) -> (pos, adj) = cBlockFindCrossover of the two blocks."""
    aqs, aqe, ats, ate = (int(x) for x in a)
    bqs, bqe, bts, bte = (int(x) for x in b)
    dq, dt = bqs - aqe, bts - ate
    adj = 0
    assert aqs < bqs and ats < bts, "a not strictly before b"  # (:124-128 errAbort)
    if dq < 0 or dt < 0:
        b_size, a_size = bqe - bqs, aqe - aqs
        overlap = -min(dq, dt)
        if overlap >= b_size or overlap >= a_size:
            adj = BIG_OVERLAP
        else:
            _, adj = xover(aqe, ate, bqs, bts, overlap)
            dq += overlap
            dt += overlap
    return adj + gap_cost(dq, dt)


def dp_two_blocks(sa, sb, c):
    """findBestPredecessors (chainBlock.c:281-304) on two leaves, A strictly
    before B: (total[A], pred of A, total[B], B's predecessor is A).
    bestPredecessor (:236-246) offers score[A] + score[B] - c, kept when it is
    > 0 (noBest) and then when it beats B's own score (:293)."""
    cand = sa + sb - c
    if cand > 0 and cand > sb:
        return sa, False, cand, True
    return sa, False, sb, False


def dp_prune_ok(sa, sb, dq, dt, c, gap_cost):
    """The reference prunes A's branch when score[A] + score[B] - gapCost(dq,
    dt) (negative distances count 0; chainBlock.c:222-232) falls below the best
    so far; the two-leaf expectation above needs that bound to be >= 0 and >=
    the connected score."""
    bound = sa + sb - gap_cost(max(dq, 0), max(dt, 0))
    return bound >= 0 and bound >= sa + sb - c


# ------------------------------------------------------------------ case builder
# Per-base differences d = left - right with the BLASTZ matrix, as the four
# letters (left q, left t, right q, right t).  FREE: the four strings are
# independent.  SHARED_Q / SHARED_T: both blocks read the same query / target
# bases (a real overlap on that axis), so the letters of that axis agree.
FREE = {0: "AAAA", 9: "CCAA", -9: "AACC"}
SHARED_Q = {0: "AAAA", 9: "ACAT", -9: "ATAC"}   # M[A][C] - M[A][T] = -114 + 123
SHARED_T = {0: "AAAA", 9: "CATA", -9: "TACA"}   # M[C][A] - M[T][A] = -114 + 123
# letters for the random sequences: matches, both kinds of mismatch (an
# asymmetric matrix tells (q, t) from (t, q)), N on each of the four strings
RANDOM_FREE = ["AAAA", "CCAA", "AACC", "ACCA", "CAAC", "GTTG", "TGGT", "AGGG", "TTCT",
               "NAAA", "ANAA", "AANA", "AAAN", "CCCC", "GGTT"]
RANDOM_SHARED_Q = ["AAAA", "ACAT", "ATAC", "CCCG", "CGCC", "GAGG", "TTTC", "NANA", "ANAA", "AAAN"]
RANDOM_SHARED_T = ["AAAA", "CATA", "TACA", "CCGC", "GCCC", "AGGG", "TTCT", "ANAN", "NAAA", "AANA"]


def build_strings(ds, palette=FREE):
    """ds: per overlap base an int (looked up in the palette) or four
    letters.  Returns (lq, lt, rq, rt) as upper-case ACGTN strings."""
    cols = [palette[d] if not isinstance(d, str) else d for d in ds]
    assert all(len(c) == 4 for c in cols)
    return tuple("".join(c[k] for c in cols) for k in range(4))


def letters_to_codes(s):
    return np.array([_LETTER_CODE[ch] for ch in s], np.int64)


def codes_to_letters(c):
    return "".join(_CODE_LETTER[int(x)] for x in c)


class Draft:
    """Genome under construction: random bases, then strings laid down at
    chosen coordinates; N letters become N runs."""

    def __init__(self, sizes, seed):
        rng = np.random.default_rng(seed)
        self.names = list(sizes)
        self.codes = [rng.integers(0, 4, n).astype(np.uint8) for n in sizes.values()]
        self.nmask = [np.zeros(n, bool) for n in sizes.values()]

    def size(self, i):
        return len(self.codes[i])

    def put(self, i, start, c5):
        """forward codes (N = 4) at [start, start + len)"""
        c5 = np.asarray(c5, np.int64)
        assert 0 <= start and start + len(c5) <= self.size(i)
        n = c5 == N_CODE
        self.codes[i][start:start + len(c5)] = np.where(n, 0, c5)  # (.2bit stores N as T)
        self.nmask[i][start:start + len(c5)] = n

    def put_strand(self, i, minus, start, c5):
        """codes in strand coordinates: '-' lays the reverse complement on the
        forward strand"""
        c5 = np.asarray(c5, np.int64)
        if not minus:
            return self.put(i, start, c5)
        rc = np.where(c5 == N_CODE, N_CODE, c5 ^ 2)[::-1]
        self.put(i, self.size(i) - start - len(c5), rc)

    def get(self, i, start, end):
        return np.where(self.nmask[i][start:end], N_CODE, self.codes[i][start:end]).astype(np.int64)

    def n_run(self, i, start, end):
        self.nmask[i][start:end] = True
        self.codes[i][start:end] = 0

    def genome(self):
        nr = []
        for m in self.nmask:
            e = np.flatnonzero(np.diff(np.concatenate([[0], m.astype(np.int8), [0]])))
            nr.append((e[0::2].astype(np.int32), (e[1::2] - e[0::2]).astype(np.int32)))
        return synth.Genome(self.names, [c.copy() for c in self.codes], nr)


# ------------------------------------------------------------------ crossover cases
OVS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000]


def _fit(pat, ov):
    return (pat * (ov // len(pat) + 1))[:ov]


def xover_patterns(seed=5, palette=FREE, random_letters=RANDOM_FREE):
    """[(name, ds)]: the hand-built difference sequences (ints: BLASTZ
    differences from the palette; strings: explicit letters)."""
    rng = np.random.default_rng(seed)
    P = []
    for ov in OVS:
        P.append((f"zero{ov}", [0] * ov))                 # pos 0
        P.append((f"neg{ov}", [-9] * ov))                 # pos 0, adj = lScore
        P.append((f"pos{ov}", [9] * ov))                  # pos = ov
        P.append((f"max0_{ov}", _fit([-9, 9], ov)))       # the maximum is exactly 0: pos 0
        P.append((f"tie{ov}", _fit([9, -9], ov)))         # the maximum 9 first at k = 0
        P.append((f"rand{ov}", [random_letters[k] for k in rng.integers(0, len(random_letters), ov)]))
        P.append((f"walk{ov}", [int(x) for x in rng.choice([-9, 0, 9], ov)]))
    P.append(("tie200", [9, -9] * 100))                   # k = 0 wins against later segments
    for k in (63, 64, 127, 128):                          # first maximum at k
        P.append((f"first{k}", [0] * k + [9] + [0] * 5))
        P.append((f"first{k}_again", [0] * k + [9, -9, 9] + [0] * 70 + [-9, 9]))
    P.append(("seg0_seg1", [0] * 10 + [9, -9] + [0] * 60 + [9] + [0] * 20))  # equal maxima, two segments
    P.append(("seg0_seg1_edge", [0] * 63 + [9, -9, 9]))                      # k = 63 and k = 65
    P.append(("last_partial", [9, -9] + [0] * 126 + [9, 9]))                 # larger only at k = 128, 129
    P.append(("last_partial_1", [9, -9] * 64 + [9, 9]))
    P.append(("carry", [9] * 64 + [-9] * 63 + [9] * 64 + [-9] * 10))         # a maximum only the carry shows
    if palette is FREE:
        P.append(("n_left", ["NAAA", "ANAA"] + [9] * 3 + ["NCAA"] * 2 + [0] * 4))
        P.append(("n_right", ["AANA", "AAAN"] + [-9] * 3 + ["AANC"] * 2 + [9] * 70))
        P.append(("n_at_win", [0, 0, "NCAA", -9, 9, 9, "CNAA", -9, -9] + [0] * 60 + ["CCNA"]))
        P.append(("n_only", ["NNNN"] * 70))
    return [(n, list(ds)) for n, ds in P]


def xover_case_set(seed=5):
    """The crossover cases laid into a target and a query genome, '+' and '-'.
    Returns (tg, qg, jobs, strings): jobs int32 [n, 8] = (t_seq, q_seq, strand,
    lqe, lte, rqs, rts, ov), strings[n] = the four letter strings of the job.
    Target sequences: edge_a (130 bases: one overlap of 65 touches base 0 and
    the last base, and the size is no multiple of 32), main, edge_z (the last
    sequence, 66 bases).  Query: the same shapes, '+' jobs on main_p, '-' jobs
    on main_m (so the two strands never share bases)."""
    pats = xover_patterns(seed)
    total = sum(2 * len(ds) + 3 for _, ds in pats) + 64
    td = Draft({"edge_a": 130, "main": total, "edge_z": 66}, seed + 1)
    qd = Draft({"edge_a": 130, "main_p": total, "main_m": total + 37, "edge_z": 66}, seed + 2)
    jobs, strings = [], []

    def lay(strs, minus, tseq, qseq, lt0, rt0, lq0, rq0):
        lq, lt, rq, rt = (letters_to_codes(s) for s in strs)
        ov = len(lq)
        td.put(tseq, lt0, lt)
        td.put(tseq, rt0, rt)
        qd.put_strand(qseq, minus, lq0, lq)
        qd.put_strand(qseq, minus, rq0, rq)
        jobs.append((tseq, qseq, int(minus), lq0 + ov, lt0 + ov, rq0, rt0, ov))
        strings.append(strs)

    for minus in (False, True):
        tc, qc = 7, 11  # (different phases of the 32-base words on the two sides)
        for _, ds in pats:
            strs = build_strings(ds)
            ov = len(ds)
            # target: left then right; query: right then left (order is free)
            lay(strs, minus, 1, 2 if minus else 1, tc, tc + ov + 1, qc + ov + 2, qc)
            tc += 2 * ov + 3
            qc += 2 * ov + 3
    # overlaps touching base 0 and the last base of their sequences: the two
    # strands' jobs cover the same whole sequences, so the '-' pass overwrites
    # what the '+' pass laid down (the strings are read back below)
    for minus in (False, True):
        r = np.random.default_rng(seed + 3 + minus)
        for tseq, qseq, ov in ((0, 0, 65), (2, 3, 33)):
            ds = [RANDOM_FREE[k] for k in r.integers(0, 9, ov)]  # (the entries without N)
            lay(build_strings(ds), minus, tseq, qseq, 0, ov, 0, ov)
    tg, qg = td.genome(), qd.genome()
    jobs = np.asarray(jobs, np.int32)
    # the strings as the genomes finally hold them (the edge sequences are
    # written twice): read back through the strand view
    cache = {}
    out = []
    for j in jobs:
        ts, qs, mi, lqe, lte, rqs, rts, ov = (int(x) for x in j)
        T = cache.setdefault(("t", ts), codes(tg, ts))
        Q = cache.setdefault(("q", qs, mi), strand_codes(qg, qs, mi))
        out.append(tuple(codes_to_letters(x) for x in
                         (Q[lqe - ov:lqe], T[lte - ov:lte], Q[rqs:rqs + ov], T[rts:rts + ov])))
        assert ts != 1 or out[-1] == strings[len(out) - 1]  # (main: exactly what was laid down)
    return tg, qg, jobs, out


# ------------------------------------------------------------------ block cases
BLOCK_SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 4095, 4096, 70000]


def block_case_set(seed=9):
    """The gac_score_blocks cases: (tg, qg, t_seq, q_seq, q_strand, blk_off,
    blk_t, blk_q, blk_size), several pairs with empty pairs between them.
    Sequences: 0 the first (33 / 37 bases), 1 the long one, 2 one whose size
    is no multiple of 32 followed by another, 3 the last one."""
    tsz = {"t0": 33, "t1": 70300, "t2": 4229, "t3": 45}
    qsz = {"q0": 37, "q1": 70200, "q2": 4197, "q3": 33}
    td, qd = Draft(tsz, seed), Draft(qsz, seed + 1)
    # N runs: single bases, a run across a 32-base word, a run longer than a
    # 64-base block (the all-N block), runs at the sequences' ends
    for d, n in ((td, 70300), (qd, 70200)):
        for a, b in ((1000, 1001), (1099, 1100), (1040, 1046), (1030, 1034), (2000, 2070),
                     (5000, 5003), (n - 1300, n - 1299), (n - 1201, n - 1200), (n - 1260, n - 1254),
                     (n - 1270, n - 1266), (n - 2070, n - 2000), (40000, 40700)):
            d.n_run(1, a, b)
        d.n_run(0, 0, 2)
        d.n_run(2, d.size(2) - 3, d.size(2))
        d.n_run(3, 0, 1)
        d.n_run(3, d.size(3) - 1, d.size(3))
    tg, qg = td.genome(), qd.genome()
    T = [len(c) for c in tg.codes]
    Q = [len(c) for c in qg.codes]
    rng = np.random.default_rng(seed + 2)
    pairs = []  # (t_seq, q_seq, minus, [(bt, bq, size)])

    def fits(ts, qs, bt, bq, size):
        return 0 <= bt and 0 <= bq and bt + size <= T[ts] and bq + size <= Q[qs]

    for mi in (0, 1):
        # every size at bit 0 and bit 31 of a word, both sides independently;
        # on '-' also with the forward window at bit 0 / 31
        blks = []
        for size in BLOCK_SIZES:
            qstarts = [64, 95] + ([Q[1] - size - 64, Q[1] - size - 95] if mi else [])
            for bt in (64, 95):
                for bq in qstarts:
                    if fits(1, 1, bt, bq, size):
                        blks.append((bt, bq, size))
        pairs.append((1, 1, mi, blks))
        pairs.append((0, 0, mi, []))  # an empty pair
        # N runs at a block's first base, last base, inside, across a 32-base
        # step, and the all-N block -- on the target, on the query (strand
        # coordinates: '-' reads the runs near the far end), on both
        blks = []
        for base_t, base_q in ((1000, 300), (300, 1000), (1000, 1000), (T[1] - 1300, Q[1] - 1300)):
            for off, size in ((0, 100), (-5, 105), (40, 6), (1, 99), (30, 4), (-2, 64), (35, 70)):
                blks.append((base_t + off, base_q + off, size))
        for bt, bq in ((2000, 2000), (2003, 300), (300, 2003), (T[1] - 2070, Q[1] - 2070),
                       (T[1] - 2066, 300), (300, Q[1] - 2066)):
            blks.append((bt, bq, 64))
        blks.append((40000, 40000, 700))
        blks.append((39990, 39000, 720))
        pairs.append((1, 1, mi, blks))
        # the first and last bases of every sequence: whole overlaps, and
        # blocks ending at the last target / query base ('-': bq + size =
        # qSize is forward base 0; bq = 0 is the last forward base)
        for s in (0, 2, 3, 1):
            m = min(T[s], Q[s])
            blks = [(0, 0, m), (T[s] - m, Q[s] - m, m)]
            for size in (1, 2, 31, 32, 33):
                if size <= m:
                    blks += [(T[s] - size, Q[s] - size, size), (0, Q[s] - size, size),
                             (T[s] - size, 0, size), (0, 0, size)]
            pairs.append((s, s, mi, blks))
            if s == 2:
                pairs.append((3, 3, mi, []))
                pairs.append((3, 3, 1 - mi, []))
        # mixed sequences (a short target against the long query and back)
        pairs.append((2, 1, mi, [(T[2] - 40, 0, 40), (T[2] - 33, Q[1] - 33, 33), (0, 12345, 4229)]))
        pairs.append((1, 2, mi, [(0, Q[2] - 40, 40), (T[1] - 33, 0, 33), (777, 0, 4197)]))
        # random blocks
        blks = []
        for _ in range(300):
            size = int(rng.integers(0, 200))
            blks.append((int(rng.integers(0, T[1] - size + 1)), int(rng.integers(0, Q[1] - size + 1)), size))
        pairs.append((1, 1, mi, blks))
    t_seq = np.array([p[0] for p in pairs], np.int32)
    q_seq = np.array([p[1] for p in pairs], np.int32)
    q_strand = np.array([p[2] for p in pairs], np.uint8)
    blk_off = np.concatenate([[0], np.cumsum([len(p[3]) for p in pairs])]).astype(np.int64)
    flat = np.array([b for p in pairs for b in p[3]], np.int32).reshape(-1, 3)
    for p in pairs:
        for bt, bq, size in p[3]:
            assert fits(p[0], p[1], bt, bq, size), (p[:3], bt, bq, size)
    return tg, qg, t_seq, q_seq, q_strand, blk_off, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy()


# ------------------------------------------------------------------ DP cases
DP_OVS = [1, 31, 63, 64, 65, 200]


def _dp_patterns(ov, rng, palette, letters):
    """On a shared axis a +-9 base is a mismatch in both blocks (about -120
    each) and a 0 base a match (+91): the +-9 stand two bases apart, so the
    overlap still scores above 0 in both blocks -- a negative adjustment would
    put the connected score above the reference's pruning bound (dp_prune_ok)."""
    P = [("zero", [0] * ov), ("pos", _fit([0, 0, 9], ov)), ("neg", _fit([0, 0, -9], ov)),
         ("max0", _fit([0, 0, -9, 0, 0, 9], ov)),      # the maximum is exactly 0
         ("tie", _fit([0, 0, 9, 0, 0, -9], ov)),       # the maximum 9 first at k = 2
         ("walk", [int(x) for x in rng.choice([-9, 0, 0, 0, 0, 0, 0, 9], ov)]),
         ("rand", [letters[k] if rng.random() < 0.15 else 0 for k in rng.integers(0, len(letters), ov)])]
    if ov > 2:
        P.append(("late", [0] * (ov - 1) + [9]))       # the last base
        P.append(("early", [0, 0, 9] + [0] * (ov - 3)))
    if ov > 64:
        P.append(("seg", [0] * 10 + [9, 0, -9] + [0] * 51 + [9] + [0] * (ov - 65)))  # k = 10 and k = 64
        P.append(("at63", [0] * 63 + [9] + [0] * (ov - 64)))
        P.append(("at64", [0] * 64 + [9] + [0] * (ov - 65)))
    return P


def dp_case_set(seed=21, reps=6):
    """Pairs of exactly two blocks A, B (A strictly before B on both axes) for
    chainConnectCost inside the DP kernels.  Query bases under every block are
    a copy of the target's; overlaps carry crafted difference patterns.
    Returns (tg, qg, t_seq, q_seq, q_strand, blk_off, box int32 [2 n, 4] =
    {qStart, qEnd, tStart, tEnd} in list order, a_first bool [n] (A is the
    pair's block 0), kind [n] (name), ov int [n] (-min(dq, dt), <= 0: none))."""
    rng = np.random.default_rng(seed)
    n_seq, seq_len = 8, 200_000
    td = Draft({f"t{i}": seq_len - 17 * i for i in range(n_seq)}, seed + 1)
    qd = Draft({f"q{i}": seq_len - 13 * i - 5 for i in range(n_seq)}, seed + 2)
    cur = {}  # (seq, minus) -> cursors: the strands of a query sequence use its two halves
    rows = []

    def alloc(tlen, qlen, minus):
        for s in range(n_seq):
            tc = cur.setdefault(("t", s), 3)
            qc = cur.setdefault(("q", s, minus), 5)
            # '+' jobs take strand coordinates [0, half), '-' jobs too: on the
            # forward strand those are the two different halves
            if tc + tlen + 2 <= td.size(s) and qc + qlen + 2 <= qd.size(s) // 2:
                cur[("t", s)] = tc + tlen + 2
                cur[("q", s, minus)] = qc + qlen + 2
                return s, tc, qc
        raise AssertionError("dp_case_set: genomes full")

    def add(kind, minus, asz, bsz, dq, dt, strs=None, shared=None, periodic=False):
        """A of asz bases, B of bsz, B.qStart - A.qEnd = dq, B.tStart - A.tEnd = dt"""
        ov = -min(dq, dt)
        tlen = asz + dt + bsz
        qlen = asz + dq + bsz
        s, t0, q0 = alloc(max(tlen, asz, bsz) + 1, max(qlen, asz, bsz) + 1, minus)
        A = (q0, q0 + asz, t0, t0 + asz)
        B = (q0 + asz + dq, q0 + asz + dq + bsz, t0 + asz + dt, t0 + asz + dt + bsz)
        assert A[0] < B[0] and A[2] < B[2]
        if periodic:
            # both axes overlap with dq != dt: the two blocks pair a query
            # base with target bases dt - dq apart; a target of that period
            # under the overlap lets both blocks match there
            per = abs(dt - dq)
            lo, hi = A[3] - ov, max(A[3], B[2] + ov)
            assert dq < 0 and dt < 0 and per and A[2] <= lo and hi <= B[3]
            td.put(s, lo, rng.integers(0, 4, per)[np.arange(hi - lo) % per])
        # plant: A's copy, then B's (B wins where the query ranges overlap)
        qd.put_strand(s, minus, A[0], td.get(s, A[2], A[3]))
        qd.put_strand(s, minus, B[0], td.get(s, B[2], B[3]))
        if strs is not None:
            lq, lt, rq, rt = (letters_to_codes(x) for x in strs)
            if shared == "q":   # dq = -ov: both blocks read query [B.qStart, A.qEnd)
                assert dq == -ov and dt >= 0 and (lq == rq).all()
                qd.put_strand(s, minus, B[0], lq)
                td.put(s, A[3] - ov, lt)
                td.put(s, B[2], rt)
            else:               # dt = -ov: both read target [B.tStart, A.tEnd)
                assert dt == -ov and dq >= 0 and (lt == rt).all()
                td.put(s, B[2], lt)
                qd.put_strand(s, minus, A[1] - ov, lq)
                qd.put_strand(s, minus, B[0], rq)
        first = bool(rng.integers(0, 2))
        rows.append((s, int(minus), A, B, first, kind, ov))

    for rep in range(reps):
        for minus in (False, True):
            big = lambda: int(rng.integers(120, 220))  # noqa: E731
            for _ in range(6):
                g1, g2 = int(rng.integers(1, 60)), int(rng.integers(1, 1500))
                add("gap_q", minus, big(), big(), g1, 0)
                add("gap_t", minus, big(), big(), 0, g1)
                add("gap_both", minus, big(), big(), g1, int(rng.integers(1, 60)))
                add("gap_q_long", minus, big(), big(), g2, 0)
                add("gap_both_long", minus, big(), big(), g2, int(rng.integers(1, 1500)))
                add("abut", minus, big(), big(), 0, 0)
                # a weak A: whether it pays to connect depends on the cost
                add("weak_a", minus, int(rng.integers(2, 9)), big(), int(rng.integers(0, 400)),
                    int(rng.integers(0, 400)))
                add("weak_a_ov", minus, int(rng.integers(3, 9)), big(), -1, int(rng.integers(0, 300)),
                    build_strings([0], SHARED_Q), "q")
            for ov in DP_OVS:
                for shared, pal, letters in (("q", SHARED_Q, RANDOM_SHARED_Q),
                                             ("t", SHARED_T, RANDOM_SHARED_T)):
                    for name, ds in _dp_patterns(ov, rng, pal, letters):
                        other = int(rng.choice([0, 5, 300]))
                        dq, dt = (-ov, other) if shared == "q" else (other, -ov)
                        add(f"ov_{name}_{shared}", minus, ov + big(), ov + big(), dq, dt,
                            build_strings(ds, pal), shared)
                # dq != dt, both negative: the two blocks' bases are tied to
                # each other on both axes, so only planted copies -- over a
                # periodic target (both blocks match in the overlap) and, in
                # every third round, over the random one
                per = ov > 1 and rep % 3 != 2
                add("ov_skew", minus, ov + big(), ov + big(), -ov, min(3 - ov, 0), periodic=per)
                add("ov_skew", minus, ov + big(), ov + big(), -(ov // 2), -ov, periodic=per)
                # the overlap reaches the smaller block's size: cost 100000000
                add("enclosed", minus, ov + big(), ov, -ov, int(rng.integers(0, 50)))
                add("enclosed", minus, ov + big(), max(ov // 2, 1), int(rng.integers(0, 50)), -ov)
    tg, qg = td.genome(), qd.genome()
    n = len(rows)
    t_seq = np.array([r[0] for r in rows], np.int32)
    q_strand = np.array([r[1] for r in rows], np.uint8)
    box = np.zeros((2 * n, 4), np.int32)
    a_first = np.array([r[4] for r in rows], bool)
    for i, (_, _, A, B, first, _, _) in enumerate(rows):
        box[2 * i], box[2 * i + 1] = (A, B) if first else (B, A)
    blk_off = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    return (tg, qg, t_seq, t_seq.copy(), q_strand, blk_off, box, a_first,
            [r[5] for r in rows], np.array([r[6] for r in rows], np.int64))


def dp_expected(tg, qg, mat, gap_cost, case):
    """Block scores (block_scores), connect costs (connect_cost) and the two-leaf
    DP's result for every pair of a dp_case_set; pairs where the reference's
    pruning could interfere are flagged in `keep` (False)."""
    _, _, t_seq, q_seq, q_strand, blk_off, box, a_first, kind, ov = case
    M = code_matrix(mat)
    score = block_scores(tg, qg, mat, t_seq, q_seq, q_strand, blk_off, box[:, 2], box[:, 0],
                         box[:, 1] - box[:, 0])
    n = len(t_seq)
    total = score.copy()
    pred = np.full(2 * n, -1, np.int32)
    keep = np.ones(n, bool)
    cost = np.zeros(n, np.int64)
    cache = {}
    for p in range(n):
        ia, ib = (2 * p, 2 * p + 1) if a_first[p] else (2 * p + 1, 2 * p)
        A, B = box[ia], box[ib]
        xo = lambda lqe, lte, rqs, rts, o: crossover_at(  # noqa: E731
            tg, qg, M, int(t_seq[p]), int(q_seq[p]), int(q_strand[p]), lqe, lte, rqs, rts, o,
            _cache=cache)
        c = connect_cost(A, B, gap_cost, xo)
        cost[p] = c
        sa, sb = int(score[ia]), int(score[ib])
        keep[p] = sa > 0 and sb > 0 and dp_prune_ok(sa, sb, int(B[0] - A[1]), int(B[2] - A[3]), c,
                                                    gap_cost)
        _, _, tb, has = dp_two_blocks(sa, sb, c)
        total[ib] = tb
        if has:
            pred[ib] = ia - 2 * p
    return score, cost, total, pred, keep


# ------------------------------------------------------------------ text cases
_JUNK = [ord("N"), ord("n"), ord("-"), ord("."), 0xE9]


def text_case_set(seed=13):
    """The crossover patterns as caller text for gac_text_crossovers: [(lq, lt,
    rq, rt)] bytes, upper and lower case mixed, and in every third case N, n,
    '-', '.' and a byte >= 0x80 among the bases (each scores 0)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (_, ds) in enumerate(xover_patterns(seed)):
        four = []
        for s in build_strings(ds):
            b = np.frombuffer(s.encode(), np.uint8).copy()
            b[rng.random(len(b)) < 0.5] |= 0x20
            if k % 3 == 0 and len(b):
                hit = rng.random(len(b)) < 0.08
                b[hit] = rng.choice(_JUNK, int(hit.sum()))
            four.append(b.tobytes())
        out.append(tuple(four))
    return out
