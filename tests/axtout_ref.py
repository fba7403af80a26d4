"""numpy restatement of chainToAxt (kent/src/hg/mouseStuff/chainToAxt/
chainToAxt.c, kent/src/lib/chainToAxt.c, axtWrite / axtScoreSym /
axtScoreSchemeDefault of kent/src/lib/axt.c), shared by the fixture generator
(tests/golden/make_axtout_golden.py) and the tests.

Pieces: a chain is cut before block b (previous block a, dq = b.qStart -
a.qEnd, dt = b.tStart - a.tEnd) when (dq > 0 and dt > 0) or dt > maxGap or
dq > maxGap.  The tool passes BIGNUM for the library's maxChain, so -maxChain
changes nothing.  Rows: per inner gap dt columns (target bases, '-') or dq
columns ('-', query bases), then the block on both rows; text as
twoBitReadSeqFragExt(doMask=TRUE) gives it, a '-' query reverse-complemented
inside the .2bit sequence (loadSeqStrand flips with nibTwoGetSize, the .2bit
size, not the header's qSize).  Score: blastz default matrix on the letters,
case-blind, 0 with an N; a gap run costs 400 + 30 for its first column and 30
for each further one; C int.  Identity: columns without a dash, letters equal
case-blind (N against N is a match); 0.0 when nothing matches.

`wrong` (a set of names from WRONG) turns on one deliberate mistake each, so
that the tests can show the fixtures catch it.
"""
import numpy as np

import antirepeat_ref as AR

WRONG = ("cut_ge", "no_open", "nn_no_match", "ix_on_dropped", "no_case", "max_chain")
BIGNUM = 0x3FFFFFFF

# blastz default by .2bit code T=0 C=1 A=2 G=3 (axt.c:434-452)
_M = np.zeros((6, 6), np.int64)
for _a, _b, _v in (("A", "A", 91), ("A", "C", -114), ("A", "G", -31), ("A", "T", -123),
                   ("C", "C", 100), ("C", "G", -125), ("C", "T", -31), ("G", "G", 100),
                   ("G", "T", -114), ("T", "T", 91)):
    _M["TCAG".index(_a), "TCAG".index(_b)] = _v
    _M["TCAG".index(_b), "TCAG".index(_a)] = _v
_CODE = np.full(256, 4, np.uint8)  # N / n: 4, '-': 5
for _i, _c in enumerate("TCAG"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("-")] = 5


class Text:
    """Cased text of every sequence of a synth.Genome: forward, and reverse
    complement (indexed by strand coordinate) on demand."""

    def __init__(self, g):
        self.g = g
        self.idx = {n: i for i, n in enumerate(g.names)}
        self._f, self._r = {}, {}

    def fwd(self, name):
        if name not in self._f:
            code, lower = AR.cased(self.g, self.idx[name])
            up = np.frombuffer(b"TCAGN", np.uint8)[code]
            self._f[name] = np.where(lower, up | 0x20, up).astype(np.uint8)
        return self._f[name]

    def rev(self, name):
        if name not in self._r:
            comp = np.arange(256, dtype=np.uint8)
            for a, b in ("AT", "TA", "CG", "GC", "at", "ta", "cg", "gc"):
                comp[ord(a)] = ord(b)
            self._r[name] = comp[self.fwd(name)[::-1]]
        return self._r[name]


def split(ca, max_gap=100, max_chain=BIGNUM, wrong=()):
    """int32 [n, 5] pieces (chain, tStart, tEnd, first block, blocks), file order."""
    out = []
    for c in range(ca.n):
        b0, b1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
        if b1 == b0:
            continue
        t = ca.blk_t[b0:b1].astype(np.int64)
        q = ca.blk_q[b0:b1].astype(np.int64)
        z = ca.blk_size[b0:b1].astype(np.int64)
        dt = t[1:] - (t[:-1] + z[:-1])
        dq = q[1:] - (q[:-1] + z[:-1])
        if (dt < 0).any() or (dq < 0).any():
            raise ValueError("chain %d: negative gap" % c)
        if "cut_ge" in wrong:
            cut = ((dq > 0) & (dt > 0)) | (dt >= max_gap) | (dq >= max_gap)
        else:
            cut = ((dq > 0) & (dt > 0)) | (dt > max_gap) | (dq > max_gap)
        start = 0
        for b in range(1, b1 - b0 + 1):
            brk = b == b1 - b0 or cut[b - 1]
            if not brk and "max_chain" in wrong and t[b] + z[b] - t[start] > max_chain:
                brk = True
            if brk:
                out.append((c, t[start], t[b - 1] + z[b - 1], start, b - start))
                start = b
    return np.asarray(out, np.int32).reshape(-1, 5)


def rows(tt, qt, ca, piece):
    """(tSym, qSym) uint8 arrays of one piece.  tt / qt: Text of the two sides."""
    c, _, _, first, nb = (int(x) for x in piece)
    b0 = int(ca.blk_off[c]) + first
    tseq = tt.fwd(ca.tname[c])
    qseq = qt.rev(ca.qname[c]) if ca.qstrand[c] else qt.fwd(ca.qname[c])
    ts, qs = [], []
    for b in range(b0, b0 + nb):
        t, q, z = int(ca.blk_t[b]), int(ca.blk_q[b]), int(ca.blk_size[b])
        if b > b0:
            pt = int(ca.blk_t[b - 1]) + int(ca.blk_size[b - 1])
            pq = int(ca.blk_q[b - 1]) + int(ca.blk_size[b - 1])
            dt, dq = t - pt, q - pq
            assert dt >= 0 and dq >= 0 and not (dt > 0 and dq > 0)
            if dq == 0:
                ts.append(tseq[pt:t])
                qs.append(np.full(dt, ord("-"), np.uint8))
            else:
                ts.append(np.full(dq, ord("-"), np.uint8))
                qs.append(qseq[pq:q])
        ts.append(tseq[t:t + z])
        qs.append(qseq[q:q + z])
    return np.concatenate(ts), np.concatenate(qs)


def measure_rows(tsym, qsym, wrong=()):
    """(score as C int, match, ali, sym) of two rows."""
    tc, qc = _CODE[tsym], _CODE[qsym]
    gap = (tc == 5) | (qc == 5)
    prev = np.concatenate([[False], gap[:-1]])
    score = int(_M[np.minimum(qc, 5), np.minimum(tc, 5)][~gap].sum()) - 30 * int(gap.sum())
    if "no_open" not in wrong:
        score -= 400 * int((gap & ~prev).sum())
    score = int(np.array(score, np.int64).astype(np.int32))
    ali = int((~gap).sum())
    same = (tsym | 0x20) == (qsym | 0x20)
    if "nn_no_match" in wrong:
        same &= tc != 4
    match = int((same & ~gap).sum())
    return score, match, ali, len(tsym)


def measure(tt, qt, ca, pieces, wrong=()):
    """(score int32, match, ali, sym int64) arrays over pieces."""
    n = len(pieces)
    out = np.zeros((n, 4), np.int64)
    for i in range(n):
        out[i] = measure_rows(*rows(tt, qt, ca, pieces[i]), wrong=wrong)
    return out[:, 0].astype(np.int32), out[:, 1], out[:, 2], out[:, 3]


def render(tt, qt, ca, pieces, offsets=None, out=None):
    """The rows as gac_axt_render lays them out: tSym '\\n' qSym '\\n' '\\n' per
    piece at offsets[p] (None: packed).  Returns (uint8 buffer, offsets)."""
    rr = [rows(tt, qt, ca, p) for p in pieces]
    if offsets is None:
        sizes = np.array([2 * len(t) + 3 for t, _ in rr], np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if len(rr) else \
            np.zeros(0, np.int64)
        out = np.zeros(int(sizes.sum()), np.uint8)
    for (t, q), o in zip(rr, offsets):
        o, s = int(o), len(t)
        out[o:o + s] = t
        out[o + s] = 10
        out[o + s + 1:o + 2 * s + 1] = q
        out[o + 2 * s + 1:o + 2 * s + 3] = 10
    return out, offsets


def f32(x):
    """kent's optionFloat returns float."""
    return float(np.float32(float(x)))


def tool_output(tt, qt, ca, max_gap=100, max_chain=BIGNUM, min_score=0.0, min_id=0.0, bed=False,
                wrong=()):
    """The bytes chainToAxt writes for chain arrays ca."""
    min_score = f32(min_score)
    min_ratio = f32(min_id) / 100.0
    pieces = split(ca, max_gap, max_chain, wrong)
    out = []
    ix = 0
    for p in pieces:
        c = int(p[0])
        if not float(ca.score[c]) >= min_score:
            continue
        tsym, qsym = rows(tt, qt, ca, p)
        if "no_case" in wrong:
            up = lambda a: np.where((a >= 97) & (a <= 122), a & 0xDF, a).astype(np.uint8)
            tsym, qsym = up(tsym), up(qsym)
        score, match, ali, _ = measure_rows(tsym, qsym, wrong)
        ratio = 0.0 if match == 0 else float(match) / float(ali)
        if not min_ratio <= ratio:
            if "ix_on_dropped" in wrong:
                ix += 1
            continue
        b0 = int(ca.blk_off[c]) + int(p[3])
        b1 = b0 + int(p[4]) - 1
        ts, te = int(ca.blk_t[b0]), int(ca.blk_t[b1]) + int(ca.blk_size[b1])
        qs, qe = int(ca.blk_q[b0]), int(ca.blk_q[b1]) + int(ca.blk_size[b1])
        strand = "-" if ca.qstrand[c] else "+"
        if bed:
            out.append(("%s\t%d\t%d\t%s\t%d\t%s\n" % (ca.tname[c], ts, te, ca.qname[c],
                                                      int(ratio * 1000), strand)).encode())
            continue
        out.append(("%d %s %d %d %s %d %d %s %d\n" % (ix, ca.tname[c], ts + 1, te, ca.qname[c],
                                                      qs + 1, qe, strand, score)).encode())
        ix += 1
        out.append(tsym.tobytes() + b"\n" + qsym.tobytes() + b"\n\n")
    return b"".join(out)


def upload(engine, ca):
    """Upload ca for axt_measure / axt_render (sequences by name; '-' strand
    coordinates as they are: the reference flips with the .2bit size)."""
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T
    tidx = np.array([engine.seq_index(GAC_T, n) for n in ca.tname], np.int32)
    qidx = np.array([engine.seq_index(GAC_Q, n) for n in ca.qname], np.int32)
    assert (tidx >= 0).all() and (qidx >= 0).all()
    return engine.upload_chain_arrays(tidx, qidx, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q,
                                      ca.blk_size)
