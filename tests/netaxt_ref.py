"""numpy / Python restatement of netToAxt (kent/src/hg/mouseStuff/netToAxt/
netToAxt.c, chainNetRead / cnFillRead of kent/src/hg/lib/chainNet.c:152-265,
chainSwap and chainSubsetOnT of kent/src/lib/chain.c:348-390,471-558), shared
by the fixture generator (tests/golden/make_netaxt_golden.py) and the tests.

The net is parsed into its tree, the ranges are enumerated in the reference's
order (rConvert: a fill's own ranges, then its children's; splitWrite: a fill
is cut at each child gap that has children of its own), and EVERY SUB-CHAIN IS
MATERIALISED AS A CHAIN OF ITS OWN with its first and last block clipped to
the range (the query following).  From there on it is axtout_ref unchanged:
split, rows, measure.  Nothing here shares the device's clip logic.

-qChain: every chain is swapped first -- t and q exchanged; for a '-' chain
both sides reversed with the HEADER's sizes and the block order reversed.  The
'-' query text is still flipped inside the .2bit sequence (the .2bit size).

'#' lines of the net file are copied to the output when the reference's
reader meets them: chainNetRead reads on to the next "net" line, so a comment
anywhere after net k's "net" line and before the next one comes out before
net k's records (comments before the first net too).

`wrong` (a set of names from WRONG) turns on one deliberate mistake each.
"""
import gzip
import os

import numpy as np

import axtout_ref as AX
from genomealignmenttools_amd.chainfile import ChainArrays

WRONG = ("no_clip", "no_insert_split", "split_every_gap", "children_first", "swap_no_reverse",
         "swap_2bit_sizes", "meta_after")

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT = os.path.join(HERE, "netaxt")
SETS = {"built": os.path.join(HERE, "antirepeat", "built"), "synth11": os.path.join(HERE, "synth11"),
        "synth12": os.path.join(HERE, "synth12")}
# (set, tag) -> (tool options, restatement keywords)
CASES = {
    ("synth11", "default"): ([], {}),
    ("synth11", "nosplit"): (["-noSplit"], dict(no_split=True)),
    ("synth11", "maxgap100000"): (["-maxGap=100000"], dict(max_gap=100000)),
    ("synth11", "maxgap100000_nosplit"): (["-maxGap=100000", "-noSplit"],
                                          dict(max_gap=100000, no_split=True)),
    ("synth11", "maxgap10"): (["-maxGap=10"], dict(max_gap=10)),
    ("synth11", "qchain"): (["-qChain"], dict(q_chain=True)),
    ("synth12", "default"): ([], {}),
    ("synth12", "qchain"): (["-qChain"], dict(q_chain=True)),
    ("built", "default"): ([], {}),
    ("built", "qchain"): (["-qChain"], dict(q_chain=True)),
}
CATEGORIES = ("head_cut", "tail_cut", "one_block_both", "insert_split", "minus", "has_N", "has_n",
              "t_dash", "q_dash", "negative", "multi_net", "meta_between")


def net_path(name, q_chain):
    """the net file of a case: the synth sets' committed nets, built's fixtures"""
    side = "q" if q_chain else "t"
    if name == "built":
        return os.path.join(OUT, f"built.{side}.net.gz")
    return os.path.join(SETS[name], f"plain.{side}.net")


def chain_path(name):
    return os.path.join(OUT, "built.chain.gz") if name == "built" else os.path.join(SETS[name], "in.chain")


def read_maybe_gz(path):
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if path.endswith(".gz") else data


def row_categories(text):
    lines = [ln for ln in text.split(b"\n") if not ln.startswith(b"#")]
    cnt = dict(minus=0, has_N=0, has_n=0, t_dash=0, q_dash=0, negative=0)
    for i in range(0, len(lines) - 1, 4):
        h, t, q = lines[i].split(), lines[i + 1], lines[i + 2]
        cnt["minus"] += h[7] == b"-"
        cnt["has_N"] += b"N" in t or b"N" in q
        cnt["has_n"] += b"n" in t or b"n" in q
        cnt["t_dash"] += b"-" in t
        cnt["q_dash"] += b"-" in q
        cnt["negative"] += int(h[8]) < 0
    return cnt


class Fill:
    __slots__ = ("tstart", "tsize", "id", "children")

    def __init__(self, tstart, tsize, cid):
        self.tstart, self.tsize, self.id, self.children = tstart, tsize, cid, []


class Net:
    def __init__(self, name, size):
        self.name, self.size, self.fills, self.meta = name, size, [], []


def parse_net(text):
    """[Net] of the bytes of a .net file, with the '#' lines each read emits."""
    nets, lead, stack = [], [], []
    for raw in text.split(b"\n"):
        if raw[:1] == b"#":  # (only a '#' in column 0 is copied)
            (nets[-1].meta if nets else lead).append(raw)
            continue
        body = raw.lstrip()
        if not body or body[:1] == b"#":
            continue
        if raw.startswith(b"net "):
            w = raw.split()
            nets.append(Net(w[1].decode(), int(w[2])))
            nets[-1].meta, lead = (lead if len(nets) == 1 else []), []
            stack = []
            continue
        assert nets, "fill before the first net"
        d = len(raw) - len(raw.lstrip(b" "))
        w = body.split()
        cid = int(w[w.index(b"id") + 1]) if b"id" in w[7:] else 0
        f = Fill(int(w[1]), int(w[2]), cid)
        if not stack:
            stack = [(d, nets[-1].fills)]
        while stack[-1][0] > d:
            stack.pop()
        if d > stack[-1][0]:
            stack.append((d, stack[-1][1][-1].children))
        stack[-1][1].append(f)
    return nets


def ranges(fills, split=True, wrong=()):
    """[(chain id, tStart, tEnd)] in the reference's order."""
    out = []

    def own(f):
        if not split or "no_insert_split" in wrong:
            return [(f.id, f.tstart, f.tstart + f.tsize)]
        r, s = [], f.tstart
        for g in f.children:
            if g.children or "split_every_gap" in wrong:
                r.append((f.id, s, g.tstart))
                s = g.tstart + g.tsize
        r.append((f.id, s, f.tstart + f.tsize))
        return r

    def rec(lst):
        for f in lst:
            mine = own(f) if f.id else []
            if "children_first" in wrong:
                rec(f.children)
                out.extend(mine)
            else:
                out.extend(mine)
                rec(f.children)

    rec(fills)
    return out


def swap(ca, wrong=(), sizes=None):
    """chainSwap of every chain.  sizes: (new t sizes by name, new q sizes by
    name) of the .2bit files, used only by the wrong variant."""
    n = ca.n
    bt, bq, bs = ca.blk_q.copy(), ca.blk_t.copy(), ca.blk_size.copy()
    tstart, tend = ca.qstart.copy(), ca.qend.copy()
    qstart, qend = ca.tstart.copy(), ca.tend.copy()
    tsize, qsize = ca.qsize.copy(), ca.tsize.copy()
    for c in range(n):
        if not ca.qstrand[c] or "swap_no_reverse" in wrong:
            continue
        ts, qs = int(tsize[c]), int(qsize[c])
        if "swap_2bit_sizes" in wrong:
            ts, qs = sizes[0][ca.qname[c]], sizes[1][ca.tname[c]]
        b0, b1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
        z = bs[b0:b1][::-1].copy()
        bt[b0:b1] = ts - (bt[b0:b1][::-1] + z)
        bq[b0:b1] = qs - (bq[b0:b1][::-1] + z)
        bs[b0:b1] = z
        tstart[c], tend[c] = ts - tend[c], ts - tstart[c]
        qstart[c], qend[c] = qs - qend[c], qs - qstart[c]
    return ChainArrays(score=ca.score, tname=list(ca.qname), tsize=tsize, tstart=tstart, tend=tend,
                       qname=list(ca.tname), qsize=qsize, qstrand=ca.qstrand, qstart=qstart,
                       qend=qend, id=ca.id, blk_off=ca.blk_off, blk_t=bt, blk_q=bq, blk_size=bs)


def subchains(ca, rg, wrong=()):
    """The sub-chains of ranges rg = int [n, 3] (chain index, tStart, tEnd) as a
    ChainArrays of their own (chainSubsetOnT's clipped blocks); a range that
    selects no block gives a chain without blocks.  Also returns the chain-local
    first block of every range."""
    T, Q, Z, off, first = [], [], [], [0], []
    for c, s, e in np.asarray(rg, np.int64).reshape(-1, 3):
        b0, b1 = int(ca.blk_off[c]), int(ca.blk_off[c + 1])
        t = ca.blk_t[b0:b1].astype(np.int64)
        q = ca.blk_q[b0:b1].astype(np.int64)
        z = ca.blk_size[b0:b1].astype(np.int64)
        # from the first block with tEnd > s (chain.c:482-486) up to the first
        # with tStart >= e (:510); blocks ascend on the target.  A range with
        # s >= e selects nothing (the reference would make a block without bases)
        lo = int(np.searchsorted(t + z, s, side="right"))
        hi = max(lo, int(np.searchsorted(t, e, side="left"))) if s < e else lo
        t, q, te = t[lo:hi].copy(), q[lo:hi].copy(), (t + z)[lo:hi].copy()
        qe = q + (te - t)
        if "no_clip" not in wrong:
            for k in range(len(t)):
                if t[k] < s:
                    q[k] += s - t[k]
                    t[k] = s
                if te[k] > e:
                    qe[k] -= te[k] - e
                    te[k] = e
        T.append(t)
        Q.append(q)
        Z.append(te - t)
        off.append(off[-1] + len(t))
        first.append(lo)
    cat = lambda a: (np.concatenate(a) if a else np.zeros(0)).astype(np.int32)
    idx = np.asarray(rg, np.int64).reshape(-1, 3)[:, 0]
    n = len(idx)
    z32 = np.zeros(n, np.int32)
    sub = ChainArrays(score=ca.score[idx], tname=[ca.tname[c] for c in idx], tsize=ca.tsize[idx],
                      tstart=z32, tend=z32, qname=[ca.qname[c] for c in idx], qsize=ca.qsize[idx],
                      qstrand=ca.qstrand[idx], qstart=z32, qend=z32, id=ca.id[idx],
                      blk_off=np.asarray(off, np.int64), blk_t=cat(T), blk_q=cat(Q), blk_size=cat(Z))
    return sub, np.asarray(first, np.int32)


def cut(ca, rg, max_gap=100):
    """What gac_axt_cut gives for ranges rg: (pieces int32 [P, 5] with chain-local
    blocks of the ORIGINAL chain and the clipped span, first int64 [n + 1]), and
    the materialised sub-chains with their own pieces for measure / render."""
    rg = np.asarray(rg, np.int32).reshape(-1, 3)
    sub, lo = subchains(ca, rg)
    sp = AX.split(sub, max_gap)
    first = np.searchsorted(sp[:, 0], np.arange(len(rg) + 1)).astype(np.int64)
    pieces = sp.copy()
    if len(sp):
        pieces[:, 0] = rg[sp[:, 0], 0]
        pieces[:, 3] = sp[:, 3] + lo[sp[:, 0]]
    return pieces, first, sub, sp


def tool_output(net_text, ca, tt, qt, q_chain=False, max_gap=100, no_split=False, wrong=()):
    """(axt bytes, -gapOut bytes, counts) of netToAxt.  tt / qt: axtout_ref.Text of
    the tool's target.2bit / query.2bit arguments."""
    if q_chain:
        ca = swap(ca, wrong, ({n: len(tt.fwd(n)) for n in tt.idx}, {n: len(qt.fwd(n)) for n in qt.idx}))
    by_id = {}
    for c, i in enumerate(ca.id):
        if int(i) in by_id:
            raise ValueError("Duplicate chain %d" % i)
        by_id[int(i)] = c
    out, gaps = [], []
    cnt = dict(nets=0, ranges=0, records=0, head_cut=0, tail_cut=0, one_block_both=0,
               insert_split=0, meta_between=0)
    ix = 0
    nets = parse_net(net_text)
    for net in nets:
        cnt["nets"] += 1
        if "meta_after" not in wrong:
            out.extend(m + b"\n" for m in net.meta)
        if len(tt.fwd(net.name)) != net.size:
            raise ValueError("Size mismatch on %s" % net.name)
        rl = ranges(net.fills, not no_split, wrong)
        rg = np.array([(by_id[i], s, e) for i, s, e in rl], np.int32).reshape(-1, 3)
        sub, _ = subchains(ca, rg, wrong)
        full, _ = subchains(ca, rg, ("no_clip",))
        sp = AX.split(sub, max_gap)
        nblk = np.diff(sub.blk_off)
        if (nblk == 0).any():
            r = int(np.flatnonzero(nblk == 0)[0])
            raise ValueError("null subchain in chain ID %d" % rl[r][0])
        cnt["ranges"] += len(rl)
        for r in range(len(rl)):
            b0, b1 = int(sub.blk_off[r]), int(sub.blk_off[r + 1])
            head = int(sub.blk_t[b0]) != int(full.blk_t[b0])
            tail = int(sub.blk_t[b1 - 1] + sub.blk_size[b1 - 1]) != \
                int(full.blk_t[b1 - 1] + full.blk_size[b1 - 1])
            cnt["head_cut"] += head
            cnt["tail_cut"] += tail
            cnt["one_block_both"] += head and tail and b1 - b0 == 1
            t, q, z = (a[b0:b1].astype(np.int64) for a in (sub.blk_t, sub.blk_q, sub.blk_size))
            gaps.extend(b"%d\t%d\n" % (dt, dq) for dt, dq in
                        zip(t[1:] - (t + z)[:-1], q[1:] - (q + z)[:-1]))
        for p in sp:
            c = int(p[0])
            tsym, qsym = AX.rows(tt, qt, sub, p)
            score = AX.measure_rows(tsym, qsym)[0]
            b0 = int(sub.blk_off[c]) + int(p[3])
            b1 = b0 + int(p[4]) - 1
            out.append(b"%d %s %d %d %s %d %d %s %d\n" % (
                ix, sub.tname[c].encode(), int(sub.blk_t[b0]) + 1,
                int(sub.blk_t[b1]) + int(sub.blk_size[b1]), sub.qname[c].encode(),
                int(sub.blk_q[b0]) + 1, int(sub.blk_q[b1]) + int(sub.blk_size[b1]),
                b"-" if sub.qstrand[c] else b"+", score))
            ix += 1
            out.append(tsym.tobytes() + b"\n" + qsym.tobytes() + b"\n\n")
        if "meta_after" in wrong:
            out.extend(m + b"\n" for m in net.meta)
    cnt["records"] = ix
    # a comment that stands between two "net" lines of the file
    cnt["meta_between"] = sum(len(n.meta) for n in nets[:-1]) - _lead(net_text) if len(nets) > 1 else 0
    cnt["insert_split"] = _insert_splits(nets, no_split)
    return b"".join(out), b"".join(gaps), cnt


def _lead(text):
    n = 0
    for raw in text.split(b"\n"):
        if raw.startswith(b"net "):
            break
        n += raw[:1] == b"#"
    return n


def _insert_splits(nets, no_split):
    """fills that splitWrite cuts into more than one range"""
    if no_split:
        return 0
    n = 0

    def rec(lst):
        nonlocal n
        for f in lst:
            n += bool(f.id) and any(g.children for g in f.children)
            rec(f.children)

    for net in nets:
        rec(net.fills)
    return n


_SETS = {}


def load_set(name):
    """(Text of t.2bit, Text of q.2bit, ChainArrays) of a fixture set, read once."""
    if name not in _SETS:
        import antirepeat_ref as AR
        from genomealignmenttools_amd import chainfile
        d = SETS[name]
        _SETS[name] = (AX.Text(AR.read_2bit(os.path.join(d, "t.2bit"))),
                       AX.Text(AR.read_2bit(os.path.join(d, "q.2bit"))),
                       chainfile.read_chains(chain_path(name)))
    return _SETS[name]


def case_inputs(name, q_chain):
    """(net bytes, ChainArrays, target Text, query Text) as the tool gets them:
    with -qChain the two .2bit arguments change places."""
    tt, qt, ca = load_set(name)
    net = read_maybe_gz(net_path(name, q_chain))
    return (net, ca, qt, tt) if q_chain else (net, ca, tt, qt)


def golden(name, tag):
    return read_maybe_gz(os.path.join(OUT, f"{name}.{tag}.gz"))
