"""netSyntenic restated in numpy / plain Python, for the tests and for the
golden generator (tests/golden/make_netsyn_golden.py asserts that this
restatement equals the reference binary before it writes a fixture).

  parse(text, fname)     chainNetRead / cnFillRead / cnFillFromLine
                         (kent/src/hg/lib/chainNet.c:86-185, 244-264) with the
                         reference's error messages (NetError)
  classify(nets)         rCalcDupes + rNetSyn
                         (kent/src/hg/mouseStuff/netSyntenic/netSyntenic.c:184-271)
  write(meta, nets)      chainNetWrite / cnFillWrite (chainNet.c:187-242)
  net_syntenic(text)     the three together: the tool's output
  depth_count            the coverage count by sort and cumsum
  depth_count_brute      the same per base (small coordinate spaces)
  SHAPES, BAD_ARGS       the coverage count's test inputs, with
  shape_id_width, shape_delta_range, random_small_cases (the small inputs of
                         the per-base checks) and stride_net_text (a net of
                         more records than one grid of the depth kernels)
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NETSYN_DIR = os.path.join(HERE, "golden", "netsyn")
NETFILTER_DIR = os.path.join(HERE, "golden", "netfilter")

# input -> expected output, the five nets of the tool tests
CASES = {
    "synth11": (os.path.join(NETFILTER_DIR, "synth11.net"), os.path.join(NETFILTER_DIR, "synth11.syn.net")),
    "cleaner": (os.path.join(NETFILTER_DIR, "cleaner.net"), os.path.join(NETFILTER_DIR, "cleaner.syn.net")),
    # (its own output again: idempotence)
    "big": (os.path.join(NETFILTER_DIR, "big.syn.net"), os.path.join(NETFILTER_DIR, "big.syn.net")),
    "edge": (os.path.join(NETSYN_DIR, "edge.net"), os.path.join(NETSYN_DIR, "edge.syn.net")),
    "indent": (os.path.join(NETSYN_DIR, "indent.net"), os.path.join(NETSYN_DIR, "indent.syn.net")),
}

INT_FIELDS = ("ali", "tN", "qN", "tR", "qR", "tNewR", "qNewR", "tOldR", "qOldR", "tTrf", "qTrf",
              "qOver", "qFar", "qDup")
TAIL_FIELDS = ("tN", "qN", "tR", "qR", "tNewR", "qNewR", "tOldR", "qOldR", "tTrf", "qTrf")


class NetError(Exception):
    """errAbort: the message the reference prints (exit status 255)."""


def _need_num(words, ix, line_no, fname):
    """lineFileNeedNum (kent/src/lib/linefile.c:1015-1025): '-' or a digit
    first, then atoi."""
    t = words[ix]
    if not (t[0] == "-" or t[0] in "0123456789"):
        raise NetError(f"Expecting number field {ix + 1} line {line_no} of {fname}, got {t}")
    m = re.match(r"-?[0-9]+", t)
    return int(m.group(0)) if m else 0


def _fill_from_line(line, line_no, fname):
    words = line.split()[:64]
    if len(words) < 7:
        raise NetError(f"Expecting at least 7 words line {line_no} of {fname} got {len(words)}")
    f = {k: -1 for k in INT_FIELDS}
    f.update(ali=0, id=0, score=0.0, type=None, children=[])
    f["tStart"] = _need_num(words, 1, line_no, fname)
    f["tSize"] = _need_num(words, 2, line_no, fname)
    f["qName"] = words[3]
    f["qStrand"] = words[4][0]
    f["qStart"] = _need_num(words, 5, line_no, fname)
    f["qSize"] = _need_num(words, 6, line_no, fname)
    for i in range(7, len(words), 2):
        name = words[i]
        if i + 1 >= len(words):  # (the reference reads past the line's words)
            raise NetError(f"Field {name} without a value line {line_no} of {fname}")
        if name == "score":
            f["score"] = float(re.match(r"[-+]?[0-9]*\.?[0-9]*(?:[eE][-+]?[0-9]+)?", words[i + 1]).group(0) or 0)
        elif name == "type":
            f["type"] = words[i + 1]
        else:
            v = _need_num(words, i + 1, line_no, fname)
            if name == "id" or name in INT_FIELDS:
                f[name] = v
    return f


def parse(text, fname="in.net"):
    """(meta lines, nets); a net is (name, size, top-level records)."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    meta = [s for s in lines if s.startswith("#")]
    real = [i for i, s in enumerate(lines) if s.strip() and not s.strip().startswith("#")]
    pos = [0]  # index into real

    def read_list():  # cnFillRead
        out, depth = [], 0
        while pos[0] < len(real):
            i = real[pos[0]]
            d = len(lines[i]) - len(lines[i].lstrip(" "))
            if not out:
                depth = d
            if d < depth:
                break
            if d > depth:
                out[-1]["children"] = read_list()  # (replaces a list it already had)
                continue
            pos[0] += 1
            out.append(_fill_from_line(lines[i], i + 1, fname))
        return out

    nets = []
    while pos[0] < len(real):
        i = real[pos[0]]
        pos[0] += 1
        if not lines[i].startswith("net "):
            raise NetError(f"Expecting 'net' first word of line {i + 1} of {fname}")
        words = lines[i].split()[:3]
        if len(words) < 3:
            raise NetError(f"Expecting at least 3 words line {i + 1} of {fname} got {len(words)}")
        size = _need_num(words, 2, i + 1, fname)
        nets.append((words[1], size, read_list()))
    return meta, nets


def preorder(nets):
    """(record, parent record or None, level) of every record, in output order."""
    out = []

    def walk(lst, parent, level):
        for f in lst:
            out.append((f, parent, level))
            walk(f["children"], f, level + 1)

    for _name, _size, top in nets:
        walk(top, None, 1)
    return out


def depth_count(seq, start, end, delta, threshold):
    """count[i] = positions of [start[i], end[i]) of seq[i] under a summed
    depth >= threshold; int32 [n].  Sort of the 2n range ends + cumsum."""
    seq = np.asarray(seq, np.int64)
    start = np.asarray(start, np.int64)
    end = np.asarray(end, np.int64)
    delta = np.asarray(delta, np.int64)
    n = len(seq)
    if n == 0:
        return np.zeros(0, np.int32)
    key = np.concatenate([(seq << 32) | start, (seq << 32) | end])
    d = np.concatenate([delta, -delta])
    order = np.argsort(key, kind="stable")
    k = key[order]
    depth = np.cumsum(d[order])
    length = np.zeros(2 * n, np.int64)
    same = (k[1:] >> 32) == (k[:-1] >> 32)
    length[:-1] = np.where(same & (depth[:-1] >= threshold), k[1:] - k[:-1], 0)
    before = np.concatenate([[0], np.cumsum(length)[:-1]])
    where = np.empty(2 * n, np.int64)
    where[order] = np.arange(2 * n)
    return (before[where[n:]] - before[where[:n]]).astype(np.int32)


def depth_count_brute(seq, start, end, delta, threshold):
    """The same, one counter per base of every sequence."""
    seq = np.asarray(seq, np.int64)
    start = np.asarray(start, np.int64)
    end = np.asarray(end, np.int64)
    delta = np.asarray(delta, np.int64)
    count = np.zeros(len(seq), np.int32)
    for s in np.unique(seq):
        ix = np.nonzero(seq == s)[0]
        depth = np.zeros(int(end[ix].max()) + 1, np.int64)
        for i in ix:
            depth[start[i]:end[i]] += delta[i]
        for i in ix:
            count[i] = int((depth[start[i]:end[i]] >= threshold).sum())
    return count


def classify(nets):
    """qDup, type, qOver, qFar of every fill, in place."""
    recs = preorder(nets)
    names = {}
    seq = [names.setdefault(f["qName"], len(names)) for f, _p, _l in recs]
    start = [f["qStart"] for f, _p, _l in recs]
    end = [f["qStart"] + f["qSize"] for f, _p, _l in recs]
    delta = [1 if f["id"] else -1 for f, _p, _l in recs]
    dup = depth_count(seq, start, end, delta, 2)
    for (f, parent, _level), q in zip(recs, dup):
        if not f["id"]:
            continue
        f["qDup"] = int(q)
        if parent is None:
            f["type"] = "top"
        elif parent["qName"] != f["qName"]:
            f["type"] = "nonSyn"
        else:
            x = (min(f["qStart"] + f["qSize"], parent["qStart"] + parent["qSize"])
                 - max(f["qStart"], parent["qStart"]))
            f["qOver"], f["qFar"] = (x, 0) if x > 0 else (0, -x)
            f["type"] = "syn" if parent["qStrand"] == f["qStrand"] else "inv"


def write(meta, nets):
    out = [s + "\n" for s in meta]
    for name, size, top in nets:
        out.append(f"net {name} {size}\n")
        for f, _parent, level in preorder([(name, size, top)]):
            s = " " * level + ("fill" if f["id"] else "gap")
            s += f" {f['tStart']} {f['tSize']} {f['qName']} {f['qStrand']} {f['qStart']} {f['qSize']}"
            if f["id"]:
                s += f" id {f['id']}"
            if f["score"] > 0:
                s += " score %1.0f" % f["score"]
            if f["ali"] > 0:
                s += f" ali {f['ali']}"
            for k in ("qOver", "qFar", "qDup"):
                if f[k] >= 0:
                    s += f" {k} {f[k]}"
            if f["type"] is not None:
                s += f" type {f['type']}"
            for k in TAIL_FIELDS:
                if f[k] >= 0:
                    s += f" {k} {f[k]}"
            out.append(s + "\n")
    return "".join(out)


def net_syntenic(text, fname="in.net"):
    meta, nets = parse(text, fname)
    classify(nets)
    return write(meta, nets)


# ---- the coverage count's test shapes (tests/test_netsyn_cpu.py, tests/test_gpu_netsyn.py)
def shape_ref_test_block():
    """the seven ranges of the reference's own TEST block (netSyntenic.c:161-167)"""
    start = [10, 30, 15, 5, 35, 0, 5]
    end = [20, 40, 35, 45, 50, 25, 55]
    return [0] * 7, start, end, [1, 1, 1, 1, 1, 1, -1]


def shape_dense():
    """70 001 ranges over 3 sequences in [0, 5000): many coincident ends,
    mixed signs, one in ten of length 0, more events than a sort tile"""
    rng = np.random.default_rng(11)
    n = 70001
    seq = rng.integers(0, 3, n)
    start = rng.integers(0, 5000, n)
    end = np.minimum(start + rng.integers(1, 400, n), 5000)
    end[::10] = start[::10]
    delta = np.where(rng.random(n) < 0.3, -1, 1)
    return seq, start, end, delta


def shape_sparse():
    """70 000 sequences with one or two ranges each, sparse ids, shuffled"""
    rng = np.random.default_rng(12)
    ids = rng.choice(2**31 - 1, 70000, replace=False)
    seq = np.concatenate([ids, ids[::2]])
    start = rng.integers(0, 1 << 20, len(seq))
    end = start + rng.integers(0, 1 << 20, len(seq))
    delta = np.ones(len(seq), np.int64)
    p = rng.permutation(len(seq))
    return seq[p], start[p], end[p], delta[p]


def shape_wide():
    """four sequences, each under two ranges [0, 2^31 - 1): every count is
    2^31 - 1 and the covered lengths sum past 2^32"""
    seq = np.repeat([3, 70000, 5, 2**31 - 1], 2)
    return seq, np.zeros(8, np.int64), np.full(8, 2**31 - 1), np.ones(8, np.int64)


STRIDE_N = 2048 * 256 + 77  # one full grid of ranges (two of range ends) and a tail


def shape_stride():
    """524 365 ranges (1 048 730 events) over 5 sequences: more than the
    kernels' largest grid (2048 workgroups of 256) holds, so the loops over
    the events take a second full trip and a third for the last 154, and the
    loop over the ranges a second for the last 77"""
    rng = np.random.default_rng(21)
    n = STRIDE_N
    seq = rng.integers(0, 5, n)
    start = rng.integers(0, 1 << 20, n)
    end = start + rng.integers(1, 3000, n)
    end[::10] = start[::10]
    delta = np.where(rng.random(n) < 0.3, -1, 1)
    return seq, start, end, delta


def _ties(positions, ids, n=3000, seed=22):
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, np.int64)
    a, b = pos[rng.integers(0, len(pos), n)], pos[rng.integers(0, len(pos), n)]
    seq = np.asarray(ids, np.int64)[rng.integers(0, len(ids), n)]
    delta = rng.choice([-1, 1, 1], n)
    return seq, np.minimum(a, b), np.maximum(a, b), delta


def shape_ties():
    """3000 ranges whose starts and ends all lie on 0, 7, 8, 2^31 - 2 and
    2^31 - 1 of the sequences 0 and 2^31 - 1: many starts, ends and
    zero-length ranges of mixed sign on each position"""
    return _ties([0, 7, 8, 2**31 - 2, 2**31 - 1], [0, 2**31 - 1])


def shape_ties_small():
    """the same on positions 0, 7, 8, 40 and 41, small enough for the
    per-base count"""
    return _ties([0, 7, 8, 40, 41], [0, 2**31 - 1])


def ties_thresholds():
    """the depths, counted per base, that the stretches between ties_small's
    positions lie under (ties' are the same, drawn alike), and each plus 1:
    at threshold 2 every stretch is far above it, at these the counts change"""
    seq, start, end, delta = shape_ties_small()
    found = set()
    for s in np.unique(seq):
        depth = np.zeros(41, np.int64)
        for i in np.nonzero(seq == s)[0]:
            depth[start[i]:end[i]] += delta[i]
        found |= {int(d) for d in depth if d >= 1}
    return sorted(found | {d + 1 for d in found})


def shape_id_width(k):
    """seven overlapping ranges on the sequence ids 2^k, 2^k - 1 and 0: the
    largest id is an exact power of two, bit k is the sort key's top bit, and
    without it the ranges of id 2^k fall on those of id 0"""
    hi = 1 << k
    seq = [hi, hi - 1, 0, hi, hi - 1, hi, 0]
    start = [0, 50, 10, 40, 60, 99, 90]
    end = [100, 150, 95, 100, 70, 400, 91]
    return seq, start, end, [1] * 7


ID_WIDTHS = range(31)

DELTA_THRESHOLDS = (1, 2, 127, 128, 255, 1000, 2**31 - 1)


def shape_delta_range():
    """500 ranges on 2 sequences below position 420 with deltas over the
    whole int8 range, -128 (whose negation is no int8) and 0 among them"""
    rng = np.random.default_rng(22)
    n = 500
    seq = rng.integers(0, 2, n)
    start = rng.integers(0, 300, n)
    end = start + rng.integers(0, 120, n)
    delta = rng.choice([-128, -127, -2, -1, 0, 1, 2, 127], n)
    return seq, start, end, delta


def random_small_cases():
    """the 200 random cases (n < 40, 3 sequences, positions below 90) of the
    restatement's own check against the per-base count"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        seq = rng.integers(0, 3, n)
        start = rng.integers(0, 60, n)
        end = start + rng.integers(0, 30, n)
        delta = rng.choice([-2, -1, 1, 1, 1, 3], n)
        yield seq, start, end, delta


SHAPES = {"ref_test": shape_ref_test_block, "dense": shape_dense, "sparse": shape_sparse,
          "wide": shape_wide, "stride": shape_stride, "ties": shape_ties,
          "ties_small": shape_ties_small}

def stride_net_text(tops_per_net=3100):
    """A net file of 3 nets and 29 records per top-level fill (269 700 with the
    default, more than the 262 144 one grid of the depth kernels takes), four
    levels deep, over the query names chrA..chrD: a fill, its 4 gaps (one in
    eight of query size 0), 2 fills in each (one in four placed anywhere on
    any query name), a gap in each of those and a fill in that, placed
    anywhere.  Returns (text, the text of its first net, records)."""
    rng = np.random.default_rng(23)
    names = ["chrA", "chrB", "chrC", "chrD"]
    out, first_len, fid = [], 0, 0

    def anywhere(size):
        return names[rng.integers(0, 4)], "+-"[rng.integers(0, 2)], int(rng.integers(0, 1 << 25)), size

    def fill(level, t, t_size, q):
        nonlocal fid
        fid += 1
        out.append(f"{' ' * level}fill {t} {t_size} {q[0]} {q[1]} {q[2]} {q[3]} id {fid} "
                   f"score {1000 + fid % 977} ali {max(t_size - 3, 1)}\n")

    def gap(level, t, t_size, q):
        out.append(f"{' ' * level}gap {t} {t_size} {q[0]} {q[1]} {q[2]} {q[3]}\n")

    for net in range(3):
        out.append(f"net chr{net + 1} {tops_per_net * 20000}\n")
        for j in range(tops_per_net):
            t0 = j * 20000
            name, strand, q0, _ = top = anywhere(16000)
            fill(1, t0, 16000, top)
            for g in range(4):
                tg, qg = t0 + 1000 + g * 3500, q0 + 1000 + g * 3500
                gap(2, tg, 3000, (name, strand, qg, 0 if rng.integers(0, 8) == 0 else 3000))
                for c in range(2):
                    tc, qc = tg + 200 + c * 1400, qg + 200 + c * 1400
                    child = anywhere(1000) if rng.integers(0, 4) == 0 else (name, strand, qc, 1000)
                    fill(3, tc, 1000, child)
                    gap(4, tc + 300, 400, (child[0], child[1], child[2] + 300, 400))
                    fill(5, tc + 400, 200, anywhere(200))
        if net == 0:
            first_len = len(out)
    return "".join(out), "".join(out[:first_len]), len(out) - 3


BAD_ARGS = {  # each GAC_E_ARG case: (seq, start, end, delta, threshold)
    "end_before_start": ([0, 0], [5, 9], [6, 8], [1, 1], 2),
    "negative_seq": ([0, -1], [5, 5], [6, 6], [1, 1], 2),
    "negative_start": ([0, 0], [5, -5], [6, 6], [1, 1], 2),
    "threshold_zero": ([0], [5], [6], [1], 0),
}
