"""chainBlocks' kd-tree DP restated in plain Python integers and lists, and
the crafted multi-leaf case set the CPU and GPU tests share
(tests/test_dp_ref_cpu.py, tests/test_gpu_dp_multileaf.py).

Written from the algorithm of the reference:
  kdBuild / medianVal / splitList        kent/src/lib/chainBlock.c:66-159
  kdTreeMake (the two leaf orders)       kent/src/lib/chainBlock.c:161-198
  bestPredecessor, updateScoresOnWay,
  findBestPredecessors                   kent/src/lib/chainBlock.c:207-309
  chainBlocks' leaf list                 kent/src/lib/chainBlock.c:423-441
  axtChain's block order                 kent/src/hg/mouseStuff/axtChain/axtChain.c:85-101,
                                         :173-197, :425-428
The connect cost, the crossover, the block scores and the gap costs are the
pieces of tests/axt_ref.py.  Nothing here is shaped like the kernels: one
pair at a time, recursion where the reference recurses.

A pair's blocks are box[g] = (qStart, qEnd, tStart, tEnd) in the caller's
list order and score[g]; every result speaks of pair-local blocks g.
"""
import functools

import numpy as np

import axt_ref as AX

SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200, 300]
RING = 64          # the slots of the speculating kernel's ring
SEED_W = 16        # its widest seed window: predecessors 64 - 16 .. 63 leaves back
STRUCTURES = ["diagonal", "braid", "far", "tie", "tie_starts", "overlap", "noise", "degenerate"]
PSL_STRUCTURES = ["diagonal", "braid", "far", "tie_starts", "overlap"]
PSL_SIZES = [1, 2, 3, 17, 48, 65, 200]
BATCH_P = [1, 2, 255, 256, 257, 1023, 1024, 1025]


# ------------------------------------------------------------------ leaves and tree
def leaf_orders(box):
    """(tord, qord): the leaves -- blocks with tStart != tEnd -- in target and
    in query order.  The leaf list is built head first (so in reverse input
    order), sorted by tStart, and the query list is that list sorted by
    qStart; both sorts keep the order of equal keys."""
    leaves = [g for g in range(len(box) - 1, -1, -1) if box[g][2] != box[g][3]]
    tord = sorted(leaves, key=lambda g: box[g][2])
    qord = sorted(tord, key=lambda g: box[g][0])
    return tord, qord


def _cut_half(n):
    return n // 2


def kd_build(box, qord, tord, cut_at=_cut_half):
    """kdBuild as nested lists: a leaf is [g]; a branch is [dim, cut, lo, hi].
    The first cut_at(n) leaves of the list of the branch's dimension are the
    lo side (marked by position), the cut is the coordinate of the last of
    them, both lists are split keeping their order, lo is built before hi."""
    def build(Q, T, dim):
        n = len(Q)
        if n == 1:
            return [Q[0]]
        half = cut_at(n)
        D = Q if dim == 0 else T
        hit = set(D[:half])
        cut = box[D[half - 1]][0 if dim == 0 else 2]
        lo = build([g for g in Q if g in hit], [g for g in T if g in hit], 1 - dim)
        hi = build([g for g in Q if g not in hit], [g for g in T if g not in hit], 1 - dim)
        return [dim, cut, lo, hi]
    return build(list(qord), list(tord), 0)


def number_nodes(box, tree):
    """The tree as rows of six ints in pre-order with the hi child first:
    [lo, hi, -1, cut, maxQ, maxT] for a branch, [qStart, tStart, g, 0, qEnd,
    tEnd] for a leaf; dims[v] = the branch's dimension (-1: leaf); lnode[g] =
    the node of leaf g."""
    nodes, dims, lnode = [], [], {}

    def walk(t):
        v = len(nodes)
        nodes.append(None)
        dims.append(-1)
        if len(t) == 1:
            g = t[0]
            nodes[v] = [box[g][0], box[g][2], g, 0, box[g][1], box[g][3]]
            lnode[g] = v
            return v
        dim, cut, lo, hi = t
        dims[v] = dim
        h = walk(hi)
        l = walk(lo)
        nodes[v] = [l, h, -1, cut, max(nodes[l][4], nodes[h][4]), max(nodes[l][5], nodes[h][5])]
        return v
    walk(tree)
    return nodes, dims, lnode


def update_path(nodes, dims, b, strict=False):
    """The nodes updateScoresOnWay reaches for a leaf with box b, in the order
    its recursion reaches them (lo before hi): coord <= cut goes lo, coord >=
    cut goes hi, so a leaf on a cut goes both ways.  (strict: the wrong
    variant with < and >.)"""
    out = []

    def walk(v, dim):
        out.append(v)
        if dims[v] < 0:
            return
        coord, cut = (b[0] if dim == 0 else b[2]), nodes[v][3]
        if coord < cut or (coord == cut and not strict):
            walk(nodes[v][0], 1 - dim)
        if coord > cut or (coord == cut and not strict):
            walk(nodes[v][1], 1 - dim)
    walk(0, 0)
    return out


# ------------------------------------------------------------------ the DP of one pair
def chain_pair(box, score, gap_cost, xover, exhaustive=True, tie_later=False, clamp=True,
               cut_at=_cut_half, strict_update=False):
    """findBestPredecessors on one pair.  box: rows (qStart, qEnd, tStart,
    tEnd); score: ints; gap_cost(dq, dt) = gapCalcCost; xover(lqe, lte, rqs,
    rts, overlap) -> (pos, adj).  Returns a dict:
      total[g], pred[g] (pair-local block or -1; a non-leaf: score, -1)
      tord, qord, lnode[g] (-1: no leaf), nodes (rows of six, see number_nodes)
      path[i]   the update path of leaf tord[i] in node order (the nodes are
                numbered hi first, the reference's recursion reaches lo first:
                the same set, and taking a maximum does not ask for an order)
      ovl[i]    the set of leaves j (blocks) with ts_j < ts, qs_j < qs and
                qs - qe_j < 0 or ts - te_j < 0
      back[i]   how many leaves back in target order the predecessor lies (0: none)
      ties, clamped, pruned_differs: lists of leaf positions i
    (tie_later, clamp, cut_at, strict_update: only the deliberately wrong
    variants of the CPU test pass them.)"""
    box = [tuple(int(x) for x in b) for b in box]
    score = [int(s) for s in score]
    nb = len(box)
    total = list(score)
    pred = [-1] * nb
    tord, qord = leaf_orders(box)
    n = len(tord)
    res = dict(total=total, pred=pred, tord=tord, qord=qord, lnode=[-1] * nb, nodes=[], path=[],
               ovl=[], back=[], ties=[], clamped=[], pruned_differs=[])
    if n == 0:
        return res
    nodes, dims, lnode = number_nodes(box, kd_build(box, qord, tord, cut_at))
    for g, v in lnode.items():
        res["lnode"][g] = v
    res["nodes"] = nodes
    max_score = [0] * len(nodes)
    costs = {}

    def cost(a, b):
        if (a, b) not in costs:
            costs[(a, b)] = AX.connect_cost(box[a], box[b], gap_cost, xover)
        return costs[(a, b)]

    for i, g in enumerate(tord):
        qs, _, ts, _ = box[g]
        sc = score[g]
        tied = [False]

        def best_pred(v, dim, bs, bn):
            ms = max_score[v] + sc
            if ms < bs:
                return bs, bn
            ms -= gap_cost(max(qs - nodes[v][4], 0), max(ts - nodes[v][5], 0))
            if ms < bs:
                return bs, bn
            if dims[v] < 0:
                a = nodes[v][2]
                if box[a][0] < qs and box[a][2] < ts:
                    s = total[a] + sc - cost(a, g)
                    if s > bs or (tie_later and s == bs and bn >= 0):
                        return s, v
                    if s == bs and bn >= 0:
                        tied[0] = True
                return bs, bn
            coord = qs if dim == 0 else ts
            if coord > nodes[v][3]:
                bs, bn = best_pred(nodes[v][1], 1 - dim, bs, bn)
            return best_pred(nodes[v][0], 1 - dim, bs, bn)

        bs, bn = best_pred(0, 0, 0, -1)     # noBest = {NULL, 0}
        if bs > total[g]:
            if bn < 0:
                res["clamped"].append(i)
            if bn >= 0 or clamp:
                total[g] = bs
            if bn >= 0:
                pred[g] = nodes[bn][2]
        if tied[0]:
            res["ties"].append(i)
        reach = update_path(nodes, dims, box[g], strict_update)
        for v in reach:
            if max_score[v] < total[g]:
                max_score[v] = total[g]
        res["path"].append(sorted(reach))
        res["back"].append(i - tord.index(pred[g]) if pred[g] >= 0 else 0)
        res["ovl"].append({a for a in tord[:i] if box[a][2] < ts and box[a][0] < qs and
                           (qs - box[a][1] < 0 or ts - box[a][3] < 0)})

    if exhaustive:  # every earlier leaf offered, no bound consulted
        ex = list(score)
        for i, g in enumerate(tord):
            best = 0
            for a in tord[:i]:
                if box[a][0] < box[g][0] and box[a][2] < box[g][2]:
                    best = max(best, ex[a] + score[g] - cost(a, g))
            if best > ex[g]:
                ex[g] = best
            if ex[g] != total[g]:
                res["pruned_differs"].append(i)
    return res


def dp_nodes(res):
    """The same tree in the DP kernels' layout: na int32 [N, 4] = {maxQ, maxT,
    cut, lo} / {qEnd, tEnd, qStart, tStart}, nb int32 [N, 2] = {end of the
    subtree, dim} / {v + 1, ~(leaf position in target order)}."""
    nodes = res["nodes"]
    N = len(nodes)
    na = np.zeros((N, 4), np.int32)
    nbb = np.zeros((N, 2), np.int32)
    pos = {g: i for i, g in enumerate(res["tord"])}
    end = [0] * N

    def walk(v, dim):
        nd = nodes[v]
        if nd[2] >= 0:
            na[v] = (nd[4], nd[5], nd[0], nd[1])
            nbb[v] = (v + 1, ~pos[nd[2]])
            end[v] = v + 1
        else:
            walk(nd[1], 1 - dim)
            walk(nd[0], 1 - dim)
            end[v] = end[nd[0]]
            na[v] = (nd[4], nd[5], nd[3], nd[0])
            nbb[v] = (end[v], dim)
        return end[v]
    if N:
        walk(0, 0)
    return na, nbb


# ------------------------------------------------------------------ a batch of pairs
def xover_for(tg, qg, M, t_seq, q_seq, strand, cache):
    return lambda lqe, lte, rqs, rts, ov: AX.crossover_at(
        tg, qg, M, int(t_seq), int(q_seq), int(strand), lqe, lte, rqs, rts, ov, _cache=cache)


def chain_batch(tg, qg, mat, gap_cost, t_seq, q_seq, q_strand, blk_off, box, score, pairs=None,
                **kw):
    """chain_pair of every pair (or of `pairs`): a list of result dicts."""
    M = AX.code_matrix(mat)
    cache = {}
    out = []
    for p in (range(len(t_seq)) if pairs is None else pairs):
        b0, b1 = int(blk_off[p]), int(blk_off[p + 1])
        out.append(chain_pair(box[b0:b1], score[b0:b1], gap_cost,
                              xover_for(tg, qg, M, t_seq[p], q_seq[p], q_strand[p], cache), **kw))
    return out


def counters(results):
    """The counts the case set's conditions are stated in."""
    c = dict(pairs=len(results), leaves=0, ties=0, far=0, window=0, clamped=0, ovl=0, ovl_gt2=0,
             ovl_gt8=0, pruned_differs=0, with_pred=0)
    for r in results:
        c["leaves"] += len(r["tord"])
        c["ties"] += len(r["ties"])
        c["far"] += sum(b >= RING for b in r["back"])
        c["window"] += sum(RING - SEED_W <= b < RING for b in r["back"])
        c["with_pred"] += sum(b > 0 for b in r["back"])
        c["clamped"] += len(r["clamped"])
        c["ovl"] += sum(len(s) > 0 for s in r["ovl"])
        c["ovl_gt2"] += sum(len(s) > 2 for s in r["ovl"])
        c["ovl_gt8"] += sum(len(s) > 8 for s in r["ovl"])
        c["pruned_differs"] += len(r["pruned_differs"])
    return c


# ------------------------------------------------------------------ axtChain's front end
def read_psl_pairs(path):
    """in.psl -> {(tName, qName, strand): [(qStart, qEnd, tStart, tEnd)]} in
    the order axtChain hands the blocks to chainBlocks: the records' blocks in
    file order, sorted by (qStart, tStart) keeping that order, blocks with
    equal starts folded into the first (the larger ends)."""
    pairs = {}
    with open(path) as f:
        for line in f:
            w = line.rstrip("\n").split("\t")
            if len(w) < 21 or not w[0].isdigit():
                continue
            sizes, qst, tst = ([int(x) for x in w[k].rstrip(",").split(",")] for k in (18, 19, 20))
            lst = pairs.setdefault((w[13], w[9], w[8]), [])
            for s, q, t in zip(sizes, qst, tst):
                lst.append([q, q + s, t, t + s])
    out = {}
    for key, lst in pairs.items():
        lst = sorted(lst, key=lambda b: (b[0], b[2]))
        kept = []
        for b in lst:
            if kept and kept[-1][0] == b[0] and kept[-1][2] == b[2]:
                kept[-1][1] = max(kept[-1][1], b[1])
                kept[-1][3] = max(kept[-1][3], b[3])
            else:
                kept.append(list(b))
        out[key] = [tuple(b) for b in kept]
    return out


def read_details(path):
    """-details file -> {(tName, qName, strand): sorted list of (score, total,
    tStart, qStart, size, has_pred, dt, dq)} (chainBlock.c:349-381)."""
    out = {}
    cur = None
    with open(path) as f:
        for line in f:
            if line.startswith("chain"):
                w = line.split()
                cur = out.setdefault((w[2], w[7], w[9]), [])
            elif line.startswith(" gap"):
                w = line.split()
                cur[-1] = cur[-1][:5] + (1, int(w[1]), int(w[2]))
            elif line.strip():
                w = line.split()
                tot = float(w[1])
                assert tot == int(tot)
                cur.append((int(w[0]), int(tot), int(w[2]), int(w[3]), int(w[4]), 0, 0, 0))
    return {k: sorted(v) for k, v in out.items()}


def details_of(box, score, res):
    """the same multiset from a chain_pair result"""
    rows = []
    for g in res["tord"]:
        b, a = box[g], res["pred"][g]
        rows.append((int(score[g]), int(res["total"][g]), int(b[2]), int(b[0]), int(b[1] - b[0])) +
                    ((0, 0, 0) if a < 0 else (1, int(b[2] - box[a][3]), int(b[0] - box[a][1]))))
    return sorted(rows)


def psl_details(tg, qg, mat, gap_cost, psl_path, **kw):
    """{pair: details multiset} of dp_ref on a PSL input over (tg, qg)."""
    pairs = read_psl_pairs(psl_path)
    keys = list(pairs)
    t_seq = [tg.names.index(k[0]) for k in keys]
    q_seq = [qg.names.index(k[1]) for k in keys]
    strand = [int(k[2] == "-") for k in keys]
    blk_off = np.concatenate([[0], np.cumsum([len(pairs[k]) for k in keys])]).astype(np.int64)
    box = np.array([b for k in keys for b in pairs[k]], np.int64).reshape(-1, 4)
    score = AX.block_scores(tg, qg, mat, t_seq, q_seq, strand, blk_off, box[:, 2], box[:, 0],
                            box[:, 1] - box[:, 0])
    res = chain_batch(tg, qg, mat, gap_cost, t_seq, q_seq, strand, blk_off, box, score, **kw)
    out = {}
    for p, k in enumerate(keys):
        b0, b1 = int(blk_off[p]), int(blk_off[p + 1])
        out[k] = details_of(box[b0:b1], score[b0:b1], res[p])
    return out, res


# ------------------------------------------------------------------ the crafted structures
# Each returns (blocks, flags): blocks = [(q, t, size)] from the pair's origin,
# flags[k] = "copy" (the query under the block is a copy of the target),
# "weak" (left random) or an int (ABI only: the score passed in).
def _diagonal(n, rng):
    out, q, t = [], 3, 5
    for _ in range(n):
        size = int(rng.integers(12, 40))
        out.append((q, t, size))
        kind = int(rng.integers(0, 3))
        g1, g2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        q += size + (g1 if kind != 1 else 0)
        t += size + (g2 if kind != 0 else 0)
    return out, ["copy"] * n


def _braid(n, rng):
    """two or three diagonals 300 bases apart; along the target one of them
    holds the long blocks for a stretch, then another"""
    nd = 2 + int(rng.integers(0, 2)) if n > 2 else 2
    out, fl, t, k = [], [], 4, 0
    while len(out) < n:
        strong = (k // 3) % nd
        for d in range(nd):
            if len(out) == n:
                break
            if d != strong and rng.random() < 0.3:
                continue
            size = int(rng.integers(30, 45)) if d == strong else int(rng.integers(6, 14))
            out.append((t + 300 * d + int(rng.integers(0, 4)), t + int(rng.integers(0, 4)), size))
            fl.append("copy")
        t += 50 + int(rng.integers(0, 30))
        k += 1
    return out, fl


def _far(n, rng):
    """a strong early leaf E; then m short leaves that start before E on the
    query (none of them can follow E, none can follow another: the query
    falls as the target rises); then k leaves after E on both axes, again
    falling on the query, so E is the only good predecessor of each"""
    if n < 3:
        return _diagonal(n, rng)
    k = max(1, min(n // 4, 40)) if not 100 <= n < 150 else n - 51  # (m = 50: 51 .. n - 1 back)
    m = n - 1 - k
    out = [(8 * m + 20, 2, 150)]
    for i in range(m):
        out.append((8 * (m - i), 160 + 8 * i, 6))
    t0, q0 = 170 + 8 * m, 8 * m + 180
    for j in range(k):
        out.append((q0 + 36 * (k - j), t0 + 36 * j, 30))
    return out, ["copy"] * n


def _tie(n, rng):
    """groups of three: A and its mirror image across the diagonal A', equal
    scores passed in, then S on the diagonal -- A and A' reach S with equal
    totals and equal gap costs from different subtrees"""
    out, fl, o = [], [], 2
    while len(out) < n:
        s = int(rng.integers(1500, 2500))
        for blk, f in (((o, o + 40, 20), s), ((o + 40, o, 20), s), ((o + 100, o + 100, 20), s + 7)):
            if len(out) < n:
                out.append(blk)
                fl.append(f)
        o += 200
    return out, fl


def _tie_starts(n, rng):
    """runs of up to eight leaves sharing one tStart (qStart rising), then
    eight sharing one qStart (tStart rising), and so on along the diagonal"""
    out = []
    for i in range(n):
        g, j = divmod(i, 8)
        size = int(rng.integers(10, 40))
        out.append((g * 400 + j * 45 + 1, g * 400 + 1, size) if g % 2 == 0 else
                   (g * 400 + 1, g * 400 + j * 45 + 1, size))
    return out, ["copy"] * n


_STEPS = [(7, 9), (20, 20), (30, 3), (3, 30), (61, 5), (5, 61), (5, 6), (2, 3), (40, 40)]
_LENS = [60, 60, 60, 25, 6]


def _overlap(n, rng):
    """a staircase: each leaf starts (sq, st) after the one before and is
    long enough to overlap several earlier ones, on one axis, on both with dq
    != dt, on the same diagonal; short leaves are enclosed by long ones"""
    out, q, t = [], 2, 2
    step = _STEPS[0]
    for i in range(n):
        if i % 6 == 0:
            step = _STEPS[int(rng.integers(0, len(_STEPS)))]
        out.append((q, t, _LENS[int(rng.integers(0, len(_LENS)))]))
        q += step[0]
        t += step[1]
    return out, ["copy"] * n


def _noise(n, rng):
    w = 30 * n + 100
    out, fl, seen = [], [], set()
    while len(out) < n:
        size = int(rng.integers(1, 40))
        q, t = int(rng.integers(0, w - size)), int(rng.integers(0, w - size))
        if (q, t) in seen:
            continue
        seen.add((q, t))
        out.append((q, t, size))
        fl.append(0 if rng.random() < 0.1 else int(rng.integers(-3000, 5000)))
    return out, fl


def _degenerate(n, rng):
    """a diagonal with zero-length blocks first, in the middle and last, and
    (two leaves or more) one box twice"""
    d, f = _diagonal(n - 1 if n > 1 else n, rng)
    if n > 1:
        d.insert(n // 2, d[n // 3])
    z = [(d[0][0], d[0][1], 0), (d[len(d) // 2][0] + 1, d[len(d) // 2][1] + 1, 0),
         (d[-1][0] + d[-1][2], d[-1][1] + d[-1][2], 0)]
    return [z[0]] + d[:len(d) // 2] + [z[1]] + d[len(d) // 2:] + [z[2]], ["copy"] * (len(d) + 3)


_MAKE = dict(diagonal=_diagonal, braid=_braid, far=_far, tie=_tie, tie_starts=_tie_starts,
             overlap=_overlap, noise=_noise, degenerate=_degenerate)
_KEEP_ORDER = {"degenerate"}  # (the zero-length blocks stay first, in the middle and last)


class CaseSet:
    """tg, qg (synth.Genome), t_seq, q_seq, q_strand, blk_off, box int32 [B,
    4], kind[p] (structure name), leaves[p] (the size asked for), fixed int64
    [B] (the score passed in, or NO_SCORE: from the bases), batches = [(name,
    pair indices)]."""
    NO_SCORE = -(1 << 40)

    def scores(self, mat):
        s = AX.block_scores(self.tg, self.qg, mat, self.t_seq, self.q_seq, self.q_strand,
                            self.blk_off, self.box[:, 2], self.box[:, 0],
                            self.box[:, 1] - self.box[:, 0])
        return np.where(self.fixed == self.NO_SCORE, s, self.fixed).astype(np.int64)

    def select(self, pairs):
        """(t_seq, q_seq, q_strand, blk_off, block indices) of a sub-batch"""
        pairs = np.asarray(pairs, np.int64)
        cnt = (self.blk_off[pairs + 1] - self.blk_off[pairs]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        blk = AX._flat_index(self.blk_off[pairs], cnt)
        return self.t_seq[pairs], self.q_seq[pairs], self.q_strand[pairs], off, blk


@functools.lru_cache(maxsize=None)
def case_set(seed=31, psl=False):
    """The crafted pairs.  Every size of SIZES in every structure of
    STRUCTURES (psl: PSL_SIZES x PSL_STRUCTURES, one pair per (target, query,
    strand), no passed-in scores, small genomes), both strands, five target
    and five query sequences including the last; a pair of only zero-length
    blocks and empty pairs between the others; 1024 pairs of 1 to 3 leaves
    and the batches built from them (BATCH_P pairs each, the 300-leaf pair
    inside; pair boundaries around multiples of 64 and 256 packed leaves).
    Each pair owns its bases, so the pairs do not disturb each other."""
    rng = np.random.default_rng(seed)
    n_t = n_q = 5 if not psl else 6
    plan = []   # (kind, leaves asked, blocks, flags)
    sizes, structs = (PSL_SIZES, PSL_STRUCTURES) if psl else (SIZES, STRUCTURES)
    for kind in structs:
        for n in sizes:
            blocks, flags = _MAKE[kind](n, rng)
            if kind not in _KEEP_ORDER and rng.random() < 0.8:
                order = rng.permutation(len(blocks))
                blocks, flags = [blocks[i] for i in order], [flags[i] for i in order]
            plan.append((kind, n, blocks, flags))
            if not psl and n in (3, 64):
                plan.append(("empty", 0, [], []))
    small0 = len(plan)
    batches = []
    if not psl:
        plan.append(("degenerate", 0, [(5, 5, 0), (9, 3, 0), (2, 7, 0)], ["copy"] * 3))
        plan.append(("empty", 0, [], []))
        small0 = len(plan)
        for _ in range(1024):
            blocks, flags = _diagonal(int(rng.integers(1, 4)), rng)
            plan.append(("small", len(blocks), blocks[::-1] if rng.random() < 0.5 else blocks, flags))
        big = next(i for i, p in enumerate(plan) if p[0] == "braid" and p[1] == 300)
        for P in BATCH_P:
            sm = list(range(small0, small0 + P - 1))
            batches.append((f"P{P}", sm[:P // 2] + [big] + sm[P // 2:]))
        # pair boundaries at, just before and just after multiples of 64 and
        # 256 packed leaves; a whole block of 256 leaves inside one pair
        want = [63, 1, 1, 63, 127, 1, 1, 255, 300, 212, 64, 64, 128, 129, 127, 256, 255, 2, 255]
        diag = {p[1]: i for i, p in enumerate(plan) if p[0] == "diagonal"}
        for n in sorted(set(want) - set(diag)):
            blocks, flags = _diagonal(n, rng)
            diag[n] = len(plan)
            plan.append(("diagonal", n, blocks, flags))
        batches.append(("edges", [diag[n] for n in want]))
    # ---- lay the pairs into the sequences
    tcur, qcur = [7] * n_t, [[11, 13] for _ in range(n_q)]
    place = []
    combos = [(t, q, s) for s in (0, 1) for t in range(n_t) for q in range(n_q)]
    if psl:
        combos = [combos[i] for i in rng.permutation(len(combos))]
        assert len(plan) <= len(combos)
    for k, (kind, n, blocks, flags) in enumerate(plan):
        if psl:
            ts, qs, mi = combos[k]
        else:
            ts, qs, mi = (k % n_t, (k // 2) % n_q, (k // 3) % 2) if kind != "small" else \
                (int(rng.integers(0, n_t)), int(rng.integers(0, n_q)), int(rng.integers(0, 2)))
        te = max([t + s for _, t, s in blocks], default=0) + 3
        qe = max([q + s for q, _, s in blocks], default=0) + 3
        place.append((ts, qs, mi, tcur[ts], qcur[qs][mi]))
        tcur[ts] += te
        qcur[qs][mi] += qe
    td = AX.Draft({f"dt{i}": tcur[i] + 29 + i for i in range(n_t)}, seed + 1)
    qd = AX.Draft({f"dq{i}": sum(qcur[i]) + 31 + 2 * i for i in range(n_q)}, seed + 2)
    box, fixed = [], []
    for (kind, n, blocks, flags), (ts, qs, mi, t0, q0) in zip(plan, place):
        for (q, t, s), f in zip(blocks, flags):
            box.append((q0 + q, q0 + q + s, t0 + t, t0 + t + s))
            fixed.append(f if isinstance(f, int) else CaseSet.NO_SCORE)
        for (q, t, s), f in sorted(zip(blocks, flags), key=lambda x: x[0][1]):
            if f != "weak" and s:
                qd.put_strand(qs, bool(mi), q0 + q, td.get(ts, t0 + t, t0 + t + s))
    c = CaseSet()
    c.tg, c.qg = td.genome(), qd.genome()
    c.t_seq = np.array([p[0] for p in place], np.int32)
    c.q_seq = np.array([p[1] for p in place], np.int32)
    c.q_strand = np.array([p[2] for p in place], np.uint8)
    c.blk_off = np.concatenate([[0], np.cumsum([len(p[2]) for p in plan])]).astype(np.int64)
    c.box = np.array(box, np.int32).reshape(-1, 4)
    c.fixed = np.array(fixed, np.int64)
    c.kind = [p[0] for p in plan]
    c.leaves = [p[1] for p in plan]
    c.batches = batches
    c.crafted = list(range(small0))
    for p in range(len(plan)):   # every block inside its sequences
        b = c.box[c.blk_off[p]:c.blk_off[p + 1]]
        assert not len(b) or (b.min() >= 0 and b[:, 3].max() <= td.size(c.t_seq[p]) and
                              b[:, 1].max() <= qd.size(c.q_seq[p]))
    return c


def psl_records(c):
    """the pairs of a psl case set as PSL records of 1 to 16 blocks each, the
    blocks dealt out in a seeded order: (qName, strand, tName, [(t, q, size)])"""
    rng = np.random.default_rng(97)
    recs = []
    for p in range(len(c.t_seq)):
        blks = [(int(t), int(q), int(qe - q)) for q, qe, t, _ in
                c.box[int(c.blk_off[p]):int(c.blk_off[p + 1])]]
        blks = [blks[i] for i in rng.permutation(len(blks))]
        while blks:
            k = int(rng.integers(1, 17))
            recs.append((c.qg.names[c.q_seq[p]], "+-"[c.q_strand[p]], c.tg.names[c.t_seq[p]], blks[:k]))
            blks = blks[k:]
    return [recs[i] for i in rng.permutation(len(recs))]
