"""numpy restatement of chainToPsl and chainToPslBasic
(kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c, chainToPslBasic/
chainToPslBasic.c), shared by the fixture generator
(tests/golden/make_psl_golden.py) and the tests.

Sequence semantics are twoBitReadSeqFragExt(doMask=TRUE), as
antirepeat_ref.cased gives them.  Per aligned base (chainToPsl.c:101-124), in
this order: nCount if either base is N; else, bases equal ignoring case, match
when the TARGET base is upper case and repMatch when it is lower case; else
misMatch.  The query's case is never read.  A '-' query is the reverse
complement of the whole sequence with the .2bit sequence's own size (:55-56),
not the chain header's qSize.

`wrong` (a set of names from WRONG) turns on one deliberate mistake each.
"""
import gzip
import os

import numpy as np

import antirepeat_ref as AR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
PSL_DIR = os.path.join(GOLDEN, "psl")
BUILT = os.path.join(GOLDEN, "antirepeat", "built")
# set -> (directory of t.2bit / q.2bit, chain file)
SETS = {
    "built": (BUILT, os.path.join(BUILT, "in.chain")),
    "synth11": (os.path.join(GOLDEN, "synth11"), os.path.join(GOLDEN, "synth11", "in.chain")),
    "synth12": (os.path.join(GOLDEN, "synth12"), os.path.join(GOLDEN, "synth12", "in.chain")),
    "edge": (BUILT, os.path.join(PSL_DIR, "edge.chain")),
}
WRONG = ("q_case_counts",          # a lower-case query base makes a repMatch too
         "n_as_base",              # N compared by its packed code (T)
         "lower_mismatch_is_rep",  # a mismatch on a lower-case target counted as repMatch
         "header_qsize_flip",      # '-' flipped with the header's qSize
         "shifted_q")              # chainAntiRepeat's shift by S - qSize applied to '-' blocks
CLASSES = ("minus_chains", "match_upper", "rep_match", "mismatch_lower", "n_target_only",
           "n_query_only", "n_in_mask")
GZ_ABOVE = 16 << 10  # a fixture larger than this is stored gzipped, as the axtout fixtures are


def fixture(name):
    """bytes of tests/golden/psl/<name> (stored plain or as <name>.gz)."""
    p = os.path.join(PSL_DIR, name)
    if os.path.exists(p + ".gz"):
        return gzip.open(p + ".gz", "rb").read()
    return open(p, "rb").read()


def load(name):
    """(target Genome, query Genome, ChainArrays) of a set."""
    from genomealignmenttools_amd.chainfile import read_chains
    d, chain = SETS[name]
    return (AR.read_2bit(os.path.join(d, "t.2bit")), AR.read_2bit(os.path.join(d, "q.2bit")),
            read_chains(chain))


def _sides(tg, qg, wrong):
    def one(g, i):
        code, lower = AR.cased(g, i)
        if "n_as_base" in wrong:
            code = g.codes[i].copy()
        return code, lower
    return ({n: one(tg, i) for i, n in enumerate(tg.names)},
            {n: one(qg, i) for i, n in enumerate(qg.names)})


def _aligned(tc, qc, ca, c, wrong):
    """(t code, t lower, q code on the chain's strand, q lower) of chain c's aligned bases"""
    b0, b1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
    bs = ca.blk_size[b0:b1]
    ti = AR._flat_index(ca.blk_t[b0:b1], bs)
    qi = AR._flat_index(ca.blk_q[b0:b1], bs)
    tcode, tlow = tc[ca.tname[c]]
    qcode, qlow = qc[ca.qname[c]]
    if not ca.qstrand[c]:
        return tcode[ti], tlow[ti], qcode[qi], qlow[qi]
    S = len(qcode)
    if "shifted_q" in wrong:
        qi = qi + (S - int(ca.qsize[c]))
    f = (int(ca.qsize[c]) if "header_qsize_flip" in wrong else S) - 1 - qi
    if wrong:
        f = np.clip(f, 0, S - 1)  # (a mistaken flip may leave the sequence)
    q = qcode[f]
    return tcode[ti], tlow[ti], np.where(q == AR.N_CODE, AR.N_CODE, q ^ 2), qlow[f]


def counts(tg, qg, ca, wrong=()):
    """int64 [n, 4]: match, misMatch, repMatch, nCount of every chain."""
    tc, qc = _sides(tg, qg, wrong)
    out = np.zeros((ca.n, 4), np.int64)
    for c in range(ca.n):
        t, tl, q, ql = _aligned(tc, qc, ca, c, wrong)
        isn = (t == AR.N_CODE) | (q == AR.N_CODE)
        eq = (t == q) & ~isn
        low = (tl | ql) if "q_case_counts" in wrong else tl
        rep = eq & low
        if "lower_mismatch_is_rep" in wrong:
            rep = ~isn & low
        out[c] = ((eq & ~rep).sum(), (~isn & ~eq & ~rep).sum(), rep.sum(), isn.sum())
    return out


def classes(tg, qg, ca):
    """The bases of a set by class: what the counts depend on."""
    tc, qc = _sides(tg, qg, ())
    k = dict.fromkeys(CLASSES, 0)
    k["minus_chains"] = int(np.count_nonzero(ca.qstrand))
    for c in range(ca.n):
        t, tl, q, ql = _aligned(tc, qc, ca, c, ())
        tn, qn = t == AR.N_CODE, q == AR.N_CODE
        eq = (t == q) & ~tn & ~qn
        k["match_upper"] += int((eq & ~tl).sum())
        k["rep_match"] += int((eq & tl).sum())
        k["mismatch_lower"] += int((~eq & ~tn & ~qn & tl).sum())
        k["n_target_only"] += int((tn & ~qn).sum())
        k["n_query_only"] += int((qn & ~tn).sum())
        k["n_in_mask"] += int(((tn | qn) & tl).sum())  # an N position on a lower-case target
    return k


def inserts(ca, basic=False):
    """int64 [n, 4]: qNumInsert, qBaseInsert, tNumInsert, tBaseInsert -- between
    adjacent blocks whose end and next start differ (chainToPsl.c:81-93), or
    with basic where the next start is greater (chainToPslBasic.c:36-48)."""
    out = np.zeros((ca.n, 4), np.int64)
    for c in range(ca.n):
        bt, bq, bs = (np.asarray(x, np.int64) for x in ca.blocks(c))
        dq = bq[1:] - (bq[:-1] + bs[:-1])
        dt = bt[1:] - (bt[:-1] + bs[:-1])
        mq, mt = (dq > 0, dt > 0) if basic else (dq != 0, dt != 0)
        out[c] = (mq.sum(), dq[mq].sum(), mt.sum(), dt[mt].sum())
    return out


def psl_text(ca, cnt, ins):
    """The 21 columns of chainToPsl.c:130-176 (pslTabOut's for these values),
    one line per chain."""
    out = []
    for c in range(ca.n):
        bt, bq, bs = ca.blocks(c)
        qsize, qs, qe = int(ca.qsize[c]), int(ca.qstart[c]), int(ca.qend[c])
        if ca.qstrand[c]:
            qs, qe = qsize - qe, qsize - qs
        cols = [*cnt[c], *ins[c], "-" if ca.qstrand[c] else "+", ca.qname[c], qsize, qs, qe,
                ca.tname[c], int(ca.tsize[c]), int(ca.tstart[c]), int(ca.tend[c]), len(bs)]
        cols += ["".join("%d," % v for v in lst) for lst in (bs, bq, bt)]
        out.append("\t".join(str(v) for v in cols) + "\n")
    return "".join(out).encode()


def tool_output(tg, qg, ca, wrong=()):
    """chainToPsl's output file."""
    return psl_text(ca, counts(tg, qg, ca, wrong), inserts(ca))


def basic_output(ca):
    """chainToPslBasic's output file: match = the aligned bases, no other count."""
    cnt = np.zeros((ca.n, 4), np.int64)
    cnt[:, 0] = [int(ca.blocks(c)[2].sum(dtype=np.int64)) for c in range(ca.n)]
    return psl_text(ca, cnt, inserts(ca, basic=True))
