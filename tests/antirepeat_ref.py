"""numpy restatement of what chainAntiRepeat counts and decides
(kent/src/hg/mouseStuff/chainAntiRepeat/chainAntiRepeat.c), shared by the
fixture generator (tests/golden/make_antirepeat_golden.py) and the tests.

Sequence semantics are twoBitReadSeqFragExt(doMask=TRUE)
(kent/src/lib/twoBit.c:835-874): N runs override the packed bits, everything
upper case, then the mask runs lower-cased (an N inside a run included).  A
'-' query is the reverse complement of [qSize - qEnd, qSize - qStart) with the
chain HEADER's qSize; case travels with the base.
"""
import struct

import numpy as np

from genomealignmenttools_amd import synth

N_CODE = 4


def read_2bit(path):
    """A version-0/1 little-endian .2bit file as a synth.Genome (with mruns)."""
    raw = open(path, "rb").read()
    sig, ver, n, _ = struct.unpack_from("<IIII", raw, 0)
    assert sig == 0x1A412743 and ver in (0, 1)
    off = 16
    names, offs = [], []
    for _ in range(n):
        nl = raw[off]
        names.append(raw[off + 1:off + 1 + nl].decode())
        off += 1 + nl
        if ver == 1:
            offs.append(struct.unpack_from("<Q", raw, off)[0])
            off += 8
        else:
            offs.append(struct.unpack_from("<I", raw, off)[0])
            off += 4
    codes, nr, mr = [], [], []
    for p in offs:
        size, nc = struct.unpack_from("<II", raw, p)
        p += 8
        ns = np.frombuffer(raw, "<u4", nc, p).astype(np.int32)
        nz = np.frombuffer(raw, "<u4", nc, p + 4 * nc).astype(np.int32)
        p += 8 * nc
        mc = struct.unpack_from("<I", raw, p)[0]
        p += 4
        ms = np.frombuffer(raw, "<u4", mc, p).astype(np.int32)
        mz = np.frombuffer(raw, "<u4", mc, p + 4 * mc).astype(np.int32)
        p += 8 * mc + 4
        b = np.frombuffer(raw, np.uint8, (size + 3) // 4, p)
        c = np.empty(b.size * 4, np.uint8)
        c[0::4] = b >> 6
        c[1::4] = (b >> 4) & 3
        c[2::4] = (b >> 2) & 3
        c[3::4] = b & 3
        codes.append(c[:size].copy())
        nr.append((ns, nz))
        mr.append((ms, mz))
    return synth.Genome(names, codes, nr, mr)


def cased(g, i):
    """(code uint8: T=0 C=1 A=2 G=3 N=4, lower bool) of sequence i."""
    code = g.codes[i].copy()
    for a, l in zip(*g.nruns[i]):
        code[a:a + l] = N_CODE
    lower = np.zeros(len(code), bool)
    if i < len(g.mruns):
        for a, l in zip(*g.mruns[i]):
            lower[max(a, 0):a + l] = True
    return code, lower


def decode_case(g, i, start, end):
    """'ACGTN' / 'acgtn' text of [start, end) of sequence i."""
    code, lower = cased(g, i)
    up = np.frombuffer(b"TCAGN", np.uint8)[code[start:end]]
    return np.where(lower[start:end], up | 0x20, up).astype(np.uint8).tobytes().decode()


def _flat_index(start, size):
    """concatenated aranges start[k] .. start[k] + size[k]"""
    size = np.asarray(size, np.int64)
    tot = int(size.sum())
    if tot == 0:
        return np.zeros(0, np.int64)
    first = np.repeat(np.asarray(start, np.int64), size)
    within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(size) - size, size)
    return first + within


def composition(tg, qg, ca):
    """(match int64 [n, 4], rep int64 [n], total int64 [n]) of every chain of a
    chainfile.ChainArrays: degeneracyFilter's counts[0..3] (:53-66) and
    repeatFilter's repCount / total (:102-114)."""
    tc = {n: cased(tg, i) for i, n in enumerate(tg.names)}
    qc = {n: cased(qg, i) for i, n in enumerate(qg.names)}
    n = len(ca.score)
    match = np.zeros((n, 4), np.int64)
    rep = np.zeros(n, np.int64)
    total = np.zeros(n, np.int64)
    for c in range(n):
        b0, b1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
        bt, bq, bs = ca.blk_t[b0:b1], ca.blk_q[b0:b1], ca.blk_size[b0:b1]
        ti = _flat_index(bt, bs)
        qi = _flat_index(bq, bs)
        tcode, tlow = tc[ca.tname[c]]
        qcode, qlow = qc[ca.qname[c]]
        t, tl = tcode[ti], tlow[ti]
        if ca.qstrand[c]:
            f = int(ca.qsize[c]) - 1 - qi  # forward position, header qSize
            q = qcode[f]
            q = np.where(q == N_CODE, N_CODE, q ^ 2)  # complement: T<->A, C<->G
            ql = qlow[f]
        else:
            q, ql = qcode[qi], qlow[qi]
        eq = (t == q) & (t != N_CODE)
        match[c] = np.bincount(t[eq], minlength=4)[:4]
        rep[c] = int((tl | ql).sum())
        total[c] = int(np.asarray(bs, np.int64).sum())
    return match, rep, total


DEG_OK, DEG_ADJ_KEPT, DEG_DROP, NOMATCH_DROP = "deg_ok", "deg_adj_kept", "deg_drop", "nomatch_drop"


def decide(score, match, rep, total, min_score=5000):
    """(keep, degeneracy branch, repeat filter result or None) -- the two
    filters in the reference's operation order (Python floats are doubles)."""
    c = [int(x) for x in match]
    tm = sum(c)
    best2 = max(c[0] + c[1], c[0] + c[2], c[0] + c[3], c[1] + c[2], c[1] + c[3], c[2] + c[3])
    score = float(score)
    if tm == 0:
        return False, NOMATCH_DROP, None  # 0/0: NaN, neither comparison holds
    over = float(best2) / float(tm) - 0.80
    if over <= 0:
        branch = DEG_OK
    else:
        adj = score * (1.01 - over / (1.0 - 0.80))
        if not adj >= min_score:
            return False, DEG_DROP, None
        branch = DEG_ADJ_KEPT
    if total == 0:
        return False, branch, False
    keep = (score * 2.0 * float(int(total) - int(rep)) / float(int(total))) >= min_score
    return bool(keep), branch, bool(keep)


def shifted_blk_q(ca, q_sizes):
    """blk_q for an upload: a '-' chain whose header qSize differs from the
    .2bit size S is shifted by S - qSize (the engine flips with S)."""
    bq = ca.blk_q.astype(np.int64).copy()
    for c in range(len(ca.score)):
        if ca.qstrand[c]:
            d = int(q_sizes[ca.qname[c]]) - int(ca.qsize[c])
            if d:
                bq[int(ca.blk_off[c]):int(ca.blk_off[c + 1])] += d
    return bq.astype(np.int32)


def upload(engine, ca, q_sizes):
    """Upload ca for chain_composition (sequences by name, '-' shift applied)."""
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T
    tidx = np.array([engine.seq_index(GAC_T, n) for n in ca.tname], np.int32)
    qidx = np.array([engine.seq_index(GAC_Q, n) for n in ca.qname], np.int32)
    assert (tidx >= 0).all() and (qidx >= 0).all()
    return engine.upload_chain_arrays(tidx, qidx, ca.qstrand, ca.blk_off, ca.blk_t,
                                      shifted_blk_q(ca, q_sizes), ca.blk_size)
