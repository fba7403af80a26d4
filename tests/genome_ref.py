"""Plain per-base reference of the resident genome layout, and the edge
fixtures of the genome-upload and N-flag tests (numpy only; shares no code
with the library).

Layout (csrc/gac_kernels.h): 32 bases per word, every sequence starts on a
word boundary, base 32w+i sits at bit i.  planes[w] = {x, y}: x the bit-0
plane and y the bit-1 plane of the .2bit code T=0 C=1 A=2 G=3 (the stored
code, also under an N run).  nmask: set for a base in any N run and for the
tail padding of a sequence's last word; plane bits of padding are 0.  lmask:
set for the mask runs clipped to [0, size), padding 0.  Four trailing words:
planes 0, nmask 0xffffffff, lmask 0 (scoring windows read word w + 1).
"""
import numpy as np

from genomealignmenttools_amd import synth
from genomealignmenttools_amd.chainfile import ChainArrays

K_UP_PER, K_STAGE = 2, 256  # k_build_flat: 256 * K_UP_PER blocks per workgroup, chains staged


# ---------------------------------------------------------------- the image
def _run_bases(size, runs, clip):
    """bool per base: inside any of the raw runs (starts, sizes) -- unsorted,
    overlapping, touching, zero-size as given; clip: a run may pass [0, size)."""
    out = np.zeros(size, bool)
    for a, l in zip(*runs):
        a, e = int(a), int(a) + int(l)
        if clip:
            a, e = max(a, 0), min(e, size)
        else:
            assert 0 <= a and e <= size, (a, e, size)
        for p in range(a, e):
            out[p] = True
    return out


def n_bases(g, i):
    return _run_bases(len(g.codes[i]), g.nruns[i], False)


def mask_bases(g, i):
    if i >= len(g.mruns):
        return np.zeros(len(g.codes[i]), bool)
    return _run_bases(len(g.codes[i]), g.mruns[i], True)


def _words(bits):
    """bool [32 k] -> uint32 [k], base i of a word at bit i"""
    b = np.ascontiguousarray(bits.reshape(-1, 32)[:, ::-1])
    out = np.zeros(len(b), np.uint64)
    for i in range(32):
        out = (out << np.uint64(1)) | b[:, i].astype(np.uint64)
    return out.astype(np.uint32)


def image(genome, soft_mask):
    """(planes uint32 [n + 4, 2], nmask uint32 [n + 4], lmask uint32 [n + 4] or
    None, woff int64 [sequences]) of a synth.Genome."""
    px, py, nm, lm, woff = [], [], [], [], []
    w = 0
    for i in range(len(genome.names)):
        size = len(genome.codes[i])
        nw = (size + 31) // 32
        woff.append(w)
        w += nw
        code = np.zeros(nw * 32, np.uint8)
        code[:size] = genome.codes[i]
        isn = np.ones(nw * 32, bool)   # padding counts as N
        isn[:size] = n_bases(genome, i)
        low = np.zeros(nw * 32, bool)
        low[:size] = mask_bases(genome, i)
        px.append(_words((code & 1).astype(bool)))
        py.append(_words((code >> 1).astype(bool)))
        nm.append(_words(isn))
        lm.append(_words(low))
    z4 = np.zeros(4, np.uint32)
    planes = np.stack([np.concatenate(px + [z4]), np.concatenate(py + [z4])], 1)
    nmask = np.concatenate(nm + [np.full(4, 0xffffffff, np.uint32)])
    lmask = np.concatenate(lm + [z4]) if soft_mask else None
    return planes.astype(np.uint32), nmask.astype(np.uint32), lmask, np.asarray(woff, np.int64)


def image_text(genome, planes, nmask, lmask, woff, i, cased=False):
    """sequence i decoded back from an image, per base: 'acgtn', or with
    cased 'ACGTN' / 'acgtn' inside the mask plane"""
    out = []
    for p in range(len(genome.codes[i])):
        w, b = int(woff[i]) + p // 32, p % 32
        if (int(nmask[w]) >> b) & 1:
            ch = "n"
        else:
            ch = "tcag"[((int(planes[w, 1]) >> b) & 1) << 1 | ((int(planes[w, 0]) >> b) & 1)]
        if cased and not (int(lmask[w]) >> b) & 1:
            ch = ch.upper()
        out.append(ch)
    return "".join(out)


def block_has_n(genome, seq, start, size):
    """does [start, start + size) of sequence seq (forward) hold an N base?"""
    i = genome.index(seq) if isinstance(seq, str) else seq
    isn = _isn(genome, i)
    for p in range(start, start + size):
        if isn[p]:
            return True
    return False


_ISN = {}


def _isn(genome, i):
    """n_bases, kept per (genome, sequence): the fixtures ask block by block"""
    hit = _ISN.get((id(genome), i))
    if hit is None or hit[0] is not genome:
        hit = _ISN[(id(genome), i)] = (genome, n_bases(genome, i))
    return hit[1]


def without_n(genome):
    """the same genome with no N runs (what a missed N is scored as)"""
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    return synth.Genome(list(genome.names), genome.codes, [e for _ in genome.names],
                        list(genome.mruns))


def subset(genome, idx):
    return synth.Genome([genome.names[i] for i in idx], [genome.codes[i] for i in idx],
                        [genome.nruns[i] for i in idx], [genome.mruns[i] for i in idx])


# ---------------------------------------------------------------- the edge genome
EDGE_SIZES = [1, 31, 32, 33, 63, 64, 65, 0, 5, 1000, 4099]
N_TINY = 300
BIG, MAIN = 140_003, 30_011
RUN_ZONE = 12_000           # main's N and mask runs lie below (and on its last base)
CLEAN_HI = MAIN - 64        # main's [RUN_ZONE, CLEAN_HI) holds no N: the partners' place
SHORT0 = 9_000              # big's short runs start past here


def _arr(runs, rng):
    """run list -> (starts, sizes) int32 in shuffled (unsorted) order"""
    if not runs:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    r = np.asarray(runs, np.int64)[rng.permutation(len(runs))]
    return r[:, 0].astype(np.int32), r[:, 1].astype(np.int32)


def _edge_runs(size, first_base=True):
    """the edge shapes that fit a sequence: first and last base, a whole word,
    a run across a word boundary (overlapping the whole word), a touching and
    an overlapping pair, a zero-size run, runs across the 1024-base pieces"""
    cand = [(0, 1), (size - 1, 1), (32, 32), (62, 4), (100, 10), (110, 10), (200, 30), (220, 20),
            (300, 0), (1000, 1024), (3000, 1025), (5000, 2049)]
    return [(a, l) for a, l in cand if a >= 0 and a + l <= size and (first_base or a > 0)]


def short_runs(size=BIG):
    """big's additional short runs (1..5 bases, gaps 20..40), sorted [a, b)"""
    rng = np.random.default_rng(77)
    out, pos = [], SHORT0
    for _ in range(3000):
        pos += int(rng.integers(20, 41))
        ln = int(rng.integers(1, 6))
        if pos + ln + 200 > size:
            break
        out.append((pos, pos + ln))
        pos += ln
    assert len(out) > 2900
    return out


def edge_genome(seed):
    """One side's genome of sequence-, word- and run-edge shapes (see the
    tests' docstrings); codes are random also under the N runs."""
    rng = np.random.default_rng(seed)
    names, sizes = [], []
    for k, s in enumerate(EDGE_SIZES):
        names.append(f"e{k}")
        sizes.append(s)
    tiny = [int(x) for x in rng.integers(1, 71, N_TINY)]
    tiny[:70] = range(1, 71)  # every size at least once
    tiny = [tiny[i] for i in rng.permutation(N_TINY)]
    tiny.insert(N_TINY // 2, 0)
    for k, s in enumerate(tiny):
        names.append(f"y{k}")
        sizes.append(s)
    names += ["big", "nend", "main", "zlast"]
    sizes += [BIG, 64, MAIN, 0]
    codes, nr, mr = [], [], []
    for name, size in zip(names, sizes):
        codes.append(rng.integers(0, 4, size).astype(np.uint8))
        if size == 0:
            n, m = [], []
        elif name == "e8":          # entirely N
            n, m = [(0, size)], [(0, size)]
        elif name == "nend":        # its last four bases: the run ends where main starts
            n, m = [(60, 4)], [(60, 4)]
        elif name == "main":
            n = _edge_runs(size, first_base=False)
            m = [(a + 7, l) for a, l in _edge_runs(size) if a + 7 + l <= RUN_ZONE]
        elif name == "big":
            n = _edge_runs(size) + [(a, b - a) for a, b in short_runs(size)]
            m = _edge_runs(size) + [(a - 1, b - a + 1) for a, b in short_runs(size)[::3]]
        elif name.startswith("e") or int(name[1:]) % 5 == 0:
            n, m = _edge_runs(size), _edge_runs(size)
        else:
            n, m = [], []
        if size > 0:                # clipped: one past the end, one from below 0
            m = m + [(size - 3, 10), (-4, 9)]
        nr.append(_arr(n, rng))
        mr.append(_arr(m, rng))
    return synth.Genome(names, codes, nr, mr)


def merged_runs(genome, seq):
    """the N bases of a sequence as sorted, maximal [a, b)"""
    isn = n_bases(genome, genome.index(seq))
    d = np.diff(np.r_[0, isn.astype(np.int8), 0])
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


# ---------------------------------------------------------------- the edge chains
ONE_SHAPES = ("end_a", "end_a1", "start_b1", "start_b", "contain", "inside",
              "one_am1", "one_a", "one_bm1", "one_b")
TOUCH = {"end_a": False, "end_a1": True, "start_b1": True, "start_b": False, "contain": True,
         "inside": True, "one_am1": False, "one_a": True, "one_bm1": True, "one_b": False}
L = 5  # flank of the shapes


def _shape(a, b, name):
    third = (b - a) // 3
    return {"end_a": (a - L, a), "end_a1": (a - L, a + 1), "start_b1": (b - 1, b + L),
            "start_b": (b, b + L), "contain": (a - 3, b + 3),
            "inside": (a + third, max(a + third + 1, b - third)),
            "one_am1": (a - 1, a), "one_a": (a, a + 1), "one_bm1": (b - 1, b),
            "one_b": (b, b + 1)}[name]


def _run_chains(a, b):
    """the chains of one run [a, b): lists of (x0, x1, shape, touches) in
    ascending forward order"""
    S = lambda n: _shape(a, b, n) + (n, TOUCH[n])
    out = [[S(n)] for n in ONE_SHAPES]
    out.append([S("end_a"), S("start_b")])       # the run lies in the gap
    out.append([S("end_a1"), S("start_b")])
    out.append([S("end_a"), S("start_b1")])
    ones = [S("one_am1"), S("one_a")] + ([S("one_bm1")] if b - 1 > a else []) + [S("one_b")]
    out.append(ones)
    out.append([(a - L, a - 3, "lead", False), S("contain")])
    out.append([(a - L, a - 1, "lead", False), S("inside"), (b + 1, b + L, "trail", False)])
    out.append([(a - 12, a - 9, "lead", False), S("end_a1")])  # met by the last base only
    return out


class _Builder:
    def __init__(self, tg, qg):
        self.g = (tg, qg)
        self.rows = []    # per chain: (tname, qname, strand)
        self.blocks = []  # per chain: list of (t, q, size)
        self.info = []    # per block: (chain, side, strand, shape, touches, group)
        self.cuts = []    # per chain: target positions worth cutting at

    def add(self, side, strand, seq, fblocks, group, run=None):
        """a chain whose blocks lie at forward [x0, x1) of `seq` on `side`
        (0 target, 1 query); the other side's bases come from main's N-free
        stretch, 2 bases apart."""
        tg, qg = self.g
        own, other = self.g[side], self.g[1 - side]
        S = len(own.codes[own.index(seq)])
        if side == 1 and strand:
            fblocks = fblocks[::-1]
        c, cum, blk = len(self.rows), 0, []
        for x0, x1, shape, touch in fblocks:
            z = x1 - x0
            assert z > 0 and 0 <= x0 and x1 <= S, (seq, x0, x1, shape)
            assert block_has_n(own, seq, x0, z) == touch, (side, seq, x0, x1, shape)
            if side == 0:
                t = x0
                q = RUN_ZONE + cum if not strand else MAIN - CLEAN_HI + cum
                pf = q if not strand else MAIN - q - z
            else:
                q = x0 if not strand else S - x1
                t = pf = RUN_ZONE + cum
            assert RUN_ZONE <= pf and pf + z <= CLEAN_HI and not block_has_n(other, "main", pf, z)
            blk.append((t, q, z))
            self.info.append((c, side, strand, shape, touch, group))
            cum += z + 2
        for (t0, q0, z0), (t1, q1, _) in zip(blk, blk[1:]):
            assert t1 >= t0 + z0 and q1 >= q0 + z0 and (t1 > t0 + z0 or q1 > q0 + z0)
        self.rows.append((seq if side == 0 else "main", "main" if side == 0 else seq, strand))
        self.blocks.append(blk)
        cut = []
        if run is not None and side == 0:
            cut = [run[0], run[0] + 1, run[1] - 1, run[1]]
        for t, _, z in blk:
            cut += [t + 1, t + z - 1, t, t + z]
        self.cuts.append(cut)

    def arrays(self):
        tg, qg = self.g
        n = len(self.rows)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(b) for b in self.blocks])
        flat = np.asarray([x for b in self.blocks for x in b], np.int64)
        first, last = off[:-1], off[1:] - 1
        tsz, qsz = tg.sizes, qg.sizes
        return ChainArrays(
            score=np.zeros(n), tname=[r[0] for r in self.rows],
            tsize=np.array([tsz[r[0]] for r in self.rows], np.int32),
            tstart=flat[first, 0].astype(np.int32),
            tend=(flat[last, 0] + flat[last, 2]).astype(np.int32),
            qname=[r[1] for r in self.rows],
            qsize=np.array([qsz[r[1]] for r in self.rows], np.int32),
            qstrand=np.array([r[2] for r in self.rows], np.uint8),
            qstart=flat[first, 1].astype(np.int32),
            qend=(flat[last, 1] + flat[last, 2]).astype(np.int32),
            id=np.arange(1, n + 1, dtype=np.int64), blk_off=off,
            blk_t=flat[:, 0].astype(np.int32), blk_q=flat[:, 1].astype(np.int32),
            blk_size=flat[:, 2].astype(np.int32))


def chosen_runs(genome):
    """a dozen runs with room for every shape: main's word-, pair- and
    piece-edge runs, and six of big's short runs"""
    m = [("main", a, b) for a, b in merged_runs(genome, "main") if a >= 12 and b + L <= RUN_ZONE]
    assert [(a, b) for _, a, b in m] == [(32, 66), (100, 120), (200, 240), (1000, 2024),
                                         (3000, 4025), (5000, 7049)]
    sh = short_runs()
    return m + [("big",) + sh[k] for k in (0, 1, 500, 1500, len(sh) - 2, len(sh) - 1)]


STRETCH = 600


def edge_chains(tg, qg):
    """(ChainArrays, info, cuts): the N-edge chains of the two edge genomes.
    info: per block (chain, side 0 target / 1 query, strand, shape, touches an
    N on that side, group); the other side of every block is N-free.  cuts: per
    chain the target positions edge_ranges cuts at."""
    B = _Builder(tg, qg)
    # more one-block chains in a row than k_build_flat stages per workgroup
    sh = short_runs()
    for j in range(STRETCH):
        a, b = sh[100 + j]
        side = 1 if j % 10 == 5 else 0
        if j % 5 == 0:
            B.add(side, (j // 10) & 1, "big", [(a - 1, a + 2, "stretch_on", True)], "stretch")
        else:
            B.add(side, (j >> 1) & 1, "big", [(b + 5, b + 8, "stretch_off", False)], "stretch")
    for side in (0, 1):
        g = B.g[side]
        for k, (seq, a, b) in enumerate(chosen_runs(g)):
            for strand in ((k & 1,) if side == 0 else (0, 1)):
                for ch in _run_chains(a, b):
                    B.add(side, strand, seq, ch, "run", (a, b))
        for strand in (0, 1):
            # sequence edges: big's first and last base are N, main's last; main's
            # base 0 follows the N run that ends nend (the global run end = the start)
            for seq in ("big", "main"):
                S = len(g.codes[g.index(seq)])
                n0 = seq == "big"
                for x0, x1, touch in ((0, 1, n0), (0, L, n0), (1, 1 + L, False), (S - 1, S, True),
                                      (S - L, S, True), (S - 1 - L, S - 1, False)):
                    B.add(side, strand, seq, [(x0, x1, "seq_edge", touch)], "edge")
            # among the short runs: 30 blocks over 30 consecutive runs
            sh = short_runs()[1000:1030]
            ch = [(a - 2, b + 2, "over", True) if i % 3 == 0 else (b + 3, b + 9, "between", False)
                  for i, (a, b) in enumerate(sh)]
            B.add(side, strand, "big", ch, "short")
    return B.arrays(), B.info, B.cuts


def edge_ranges(ca, cuts, per_chain=6):
    """the full range of every chain, then ranges cut at the run's a, a+1,
    b-1, b (target-side chains) and at the block edges +-1: int64 [n, 3]"""
    R = [(c, int(ca.tstart[c]), int(ca.tend[c])) for c in range(ca.n)]
    for c in range(ca.n):
        s, e, seen = int(ca.tstart[c]), int(ca.tend[c]), []
        for x in cuts[c]:
            if s < x < e and x not in seen:
                seen.append(x)
        for x in seen[:per_chain]:
            R += [(c, s, x), (c, x, e)]
    return np.asarray(R, np.int64)


def shifted(ca, info, tg, qg):
    """the same chains with every block's own-side window moved by one base,
    each chain forwards or backwards, whichever changes more of its blocks' N
    flags (and stays inside the sequence).  Blocks that lie deep inside a run
    or in N-free sequence keep their flag either way; of the blocks that touch
    an N in either set, most flip."""
    side = {}
    for c, s, *_ in info:
        side[c] = s
    bt, bq = ca.blk_t.astype(np.int64).copy(), ca.blk_q.astype(np.int64).copy()
    for c in range(ca.n):
        o0, o1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
        own, seq, S = (tg, ca.tname[c], int(ca.tsize[c])) if side[c] == 0 else \
            (qg, ca.qname[c], int(ca.qsize[c]))
        z = ca.blk_size[o0:o1].astype(np.int64)
        if side[c] == 0:
            x0 = bt[o0:o1]
        else:  # the forward window of a '-' block
            x0 = S - bq[o0:o1] - z if ca.qstrand[c] else bq[o0:o1]
        best, flips = 0, -1
        for d in (1, -1):
            if (x0 + d).min() < 0 or (x0 + d + z).max() > S:
                continue
            n = sum(block_has_n(own, seq, int(a), int(l)) != block_has_n(own, seq, int(a) + d, int(l))
                    for a, l in zip(x0, z))
            if n > flips:
                best, flips = d, n
        assert best
        if side[c] == 0:
            bt[o0:o1] += best
        else:  # forward +1 is strand -1 on '-'
            bq[o0:o1] += -best if ca.qstrand[c] else best
    first, last = ca.blk_off[:-1], ca.blk_off[1:] - 1
    out = ChainArrays(
        score=ca.score, tname=ca.tname, tsize=ca.tsize, tstart=bt[first].astype(np.int32),
        tend=(bt[last] + ca.blk_size[last]).astype(np.int32), qname=ca.qname, qsize=ca.qsize,
        qstrand=ca.qstrand, qstart=bq[first].astype(np.int32),
        qend=(bq[last] + ca.blk_size[last]).astype(np.int32), id=ca.id, blk_off=ca.blk_off,
        blk_t=bt.astype(np.int32), blk_q=bq.astype(np.int32), blk_size=ca.blk_size)
    assert (out.blk_t >= 0).all() and (out.tend <= out.tsize).all()
    assert (out.blk_q >= 0).all() and (out.qend <= out.qsize).all()
    return out


def block_flags(tg, qg, ca):
    """(t has N, q has N) bool per block, by per-base scan"""
    tn = {n: n_bases(tg, i) for i, n in enumerate(tg.names) if n in set(ca.tname)}
    qn = {n: n_bases(qg, i) for i, n in enumerate(qg.names) if n in set(ca.qname)}
    ft, fq = np.zeros(len(ca.blk_t), bool), np.zeros(len(ca.blk_t), bool)
    for c in range(ca.n):
        for b in range(int(ca.blk_off[c]), int(ca.blk_off[c + 1])):
            t, q, z = int(ca.blk_t[b]), int(ca.blk_q[b]), int(ca.blk_size[b])
            f = int(ca.qsize[c]) - q - z if ca.qstrand[c] else q
            ft[b] = tn[ca.tname[c]][t:t + z].any()
            fq[b] = qn[ca.qname[c]][f:f + z].any()
    return ft, fq


def unstaged_workgroups(blk_off):
    """the k_build_flat workgroups (256 * K_UP_PER blocks each) whose blocks
    belong to more than K_STAGE chains: they take the unstaged chain search"""
    off = np.asarray(blk_off, np.int64)
    nb, n = int(off[-1]), len(off) - 1
    ntiles = (nb + 63) >> 6
    owner = lambda b: int(np.searchsorted(off[:n], b, side="right")) - 1  # last chain at or before b
    tile_c0 = [owner(t << 6) for t in range(ntiles)] + [n - 1]
    out = []
    for wg in range((nb + 256 * K_UP_PER - 1) // (256 * K_UP_PER)):
        t0 = wg * 4 * K_UP_PER
        t1 = min(t0 + 4 * K_UP_PER, ntiles)
        if tile_c0[t1] - tile_c0[t0] + 1 > K_STAGE:
            out.append(wg)
    return out


# ---------------------------------------------------------------- staging windows
WINDOW = 1 << 20  # GAC_PIN_MB=1


def staging_layout(genome):
    """(byte offset of every payload, total bytes) of the upload's staging
    layout: payloads in sequence order, each 8-byte aligned"""
    return _layout_of_sizes([len(c) for c in genome.codes])


STAGE_THREADS = 16  # the child runs with GAC_THREADS=16


def stage_shares(total, nt=STAGE_THREADS, window=WINDOW):
    """the byte ranges [a, b) the staging threads copy, window by window:
    share t of window [lo, hi) is lo + min(len, per t) .. lo + min(len, per (t + 1)),
    per = ceil(len / nt)"""
    out = []
    for lo in range(0, total, window):
        hi = min(total, lo + window)
        ln = hi - lo
        per = (ln + nt - 1) // nt
        for t in range(nt):
            a, b = lo + min(ln, per * t), lo + min(ln, per * (t + 1))
            if a < b:
                out.append((a, b))
    return out


def share_starts(sizes, nt=STAGE_THREADS):
    """where the thread shares of a staging layout start: (strictly inside the
    alignment padding behind a payload, strictly inside a payload of at most
    18 bytes, elsewhere), as counts"""
    off, total = _layout_of_sizes(sizes)
    end = [o + (s + 3) // 4 for o, s in zip(off, sizes)]
    nxt = off[1:] + [total]
    pad = tiny = other = 0
    for a, _ in stage_shares(total, nt):
        k = max(i for i in range(len(off)) if off[i] <= a)
        if end[k] < a < nxt[k]:
            pad += 1
        elif off[k] < a < end[k] and end[k] - off[k] <= 18:
            tiny += 1
        else:
            other += 1
    return pad, tiny, other


def staging_sizes(seed):
    """About 8.4 Mb: a large sequence that ends just below the first 1 MB
    window boundary of the staging layout, 150 tiny ones across it (payloads
    and windows are 8-byte aligned, so the boundary is a payload's start), a
    large one that ends just past the second boundary, then 150 tiny ones and
    a short one: the last window is a few kilobytes, and its sixteen thread
    shares (no multiple of 8 bytes) start inside tiny payloads and inside the
    padding behind them.  The last size is searched for that; none found is
    an error."""
    rng = np.random.default_rng(seed)
    tiny = [int(x) for x in rng.integers(1, 71, N_TINY)]
    h = N_TINY // 2
    for last in range(301, 901):
        sizes = [4 * (WINDOW - 900) + 3] + tiny[:h] + [4 * (WINDOW + 900) + 1] + tiny[h:] + [last]
        pad, small, _ = share_starts(sizes)
        if pad >= 2 and small >= 2:
            break
    else:
        raise AssertionError("no thread share starts in padding and in a tiny payload")
    off, total = _layout_of_sizes(sizes)
    assert off[1] < WINDOW < off[h] and off[h + 1] < 2 * WINDOW < off[h + 2] < total
    assert 2 * WINDOW < total <= 3 * WINDOW
    return sizes


def staging_genome(seed):
    """staging_sizes as a genome, N and mask runs on every sequence they fit"""
    sizes = staging_sizes(seed)
    rng = np.random.default_rng(seed + 1)
    names = [f"s{k}" for k in range(len(sizes))]
    codes, nr, mr = [], [], []
    for size in sizes:
        codes.append(rng.integers(0, 4, size).astype(np.uint8))
        runs = _edge_runs(size) if size > 70 else ([(size - 1, 1)] if size % 4 == 0 else [])
        nr.append(_arr(runs, rng))
        mr.append(_arr([(a + 3, l) for a, l in runs if a + 3 + l <= size], rng))
    return synth.Genome(names, codes, nr, mr)


# ---------------------------------------------------------------- sparse scatter
SCATTER_RUNS = 70_000          # one-word runs of the grid-stride case
SCATTER_WAVES = 16384 * 4      # k_scatter's grid at most: one run per wave and trip
SCATTER_SIZE = 2_300_011


def scatter_genome(seed=3):
    rng = np.random.default_rng(seed)
    z = (np.zeros(0, np.int32), np.zeros(0, np.int32))
    return synth.Genome(["a", "b"], [rng.integers(0, 4, 77).astype(np.uint8),
                                     rng.integers(0, 4, SCATTER_SIZE).astype(np.uint8)],
                        [z, (np.array([64_000], np.int32), np.array([1500], np.int32))], [z, z])


def _layout_of_sizes(sizes):
    off, pos = [], 0
    for s in sizes:
        pos = (pos + 7) & ~7
        off.append(pos)
        pos += (s + 3) // 4
    return off, pos
