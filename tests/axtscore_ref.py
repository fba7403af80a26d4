"""axtToMaf and axtSort restated in plain Python, and what the axtmaf tests share.

score(t, q) is axtScoreSym (kent/src/lib/axt.c:196-229) under
axtScoreSchemeDefault (:423-458) in numpy: a column is a gap column iff either
character is '-'; a gap column costs 30, and 400 more when the column before it
is no gap column (column 0 included); any other column adds the blastz matrix
on its two letters, case-blind, 0 for a character outside acgtACGT; the sum
wraps as a 32-bit int.

to_maf is axtToMaf.c:74-145 over mafWrite (kent/src/lib/maf.c:281-361), and
sort_axt is axtSort.c:24-47 over axtWrite (axt.c:101-120); both read as axtRead
does, with every line that starts with '#' noted where lineFileNext meets it.

BadInput is raised where the reference aborts."""
import json
import os

import numpy as np

import axtpsl_ref as AP
from axtpsl_ref import BadInput  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
AXTMAF_DIR = os.path.join(HERE, "golden", "axtmaf")

GAP_OPEN, GAP_EXTEND = 400, 30
MATRIX = np.array([[91, -114, -31, -123, 0],
                   [-114, 100, -125, -31, 0],
                   [-31, -125, 100, -114, 0],
                   [-123, -31, -114, 91, 0],
                   [0, 0, 0, 0, 0]], np.int64)
CLASS = np.full(256, 4, np.int64)
for _k, _c in enumerate("acgt"):
    CLASS[ord(_c)] = CLASS[ord(_c.upper())] = _k


def _bytes(row):
    return row.encode("latin-1") if isinstance(row, str) else bytes(row)


def wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def score(t, q):
    t = np.frombuffer(_bytes(t), np.uint8)
    q = np.frombuffer(_bytes(q), np.uint8)
    assert len(t) == len(q)
    if len(t) == 0:
        return 0
    gap = (t == ord("-")) | (q == ord("-"))
    prev = np.concatenate([[False], gap[:-1]])
    total = int(MATRIX[CLASS[t], CLASS[q]][~gap].sum())
    total -= GAP_EXTEND * int(gap.sum()) + GAP_OPEN * int((gap & ~prev).sum())
    return wrap32(total)


def scores(t_rows, q_rows):
    return np.array([score(t, q) for t, q in zip(t_rows, q_rows)], np.int32)


# ------------------------------------------------------------ reading
def read_axt(data):
    """(records, tail): records as axtRead fills them, each with the '#' lines
    lineFileNext met while it was read ("meta": before and inside it); tail:
    the '#' lines after the last record"""
    lines, at, out, meta = AP.split_lines(data), 0, [], []

    def take():
        nonlocal at
        ln = lines[at]
        at += 1
        if ln[:1] == b"#":
            meta.append(ln)
        return ln

    while True:
        w = None
        while at < len(lines):
            ln = take()
            if ln[:1] == b"#":
                continue
            w = AP.chop_by_white(ln, 10)
            if w:
                break
            w = None
        if w is None:
            return out, meta
        if len(w) < 8:
            raise BadInput("Expecting at least 8 words got %d" % len(w))
        r = dict(q_name=w[4], q_start=AP.need_num(w[5]) - 1, q_end=AP.need_num(w[6]), strand=w[7][:1],
                 t_name=w[1], t_start=AP.need_num(w[2]) - 1, t_end=AP.need_num(w[3]))
        r["score"] = AP.need_num(w[8]) if len(w) > 8 else 0
        if at + 2 > len(lines):
            raise BadInput("Unexpected end of file")
        r["t_sym"], r["q_sym"] = take(), take()
        if len(r["t_sym"]) != len(r["q_sym"]):
            raise BadInput("Symbol count %d != %d" % (len(r["t_sym"]), len(r["q_sym"])))
        if at < len(lines):
            take()
        r["meta"], meta = meta, []
        out.append(r)


def rows_of(data):
    recs, _ = read_axt(data)
    return [r["t_sym"] for r in recs], [r["q_sym"] for r in recs]


# ------------------------------------------------------------ axtToMaf
def digits(x):
    return len("%d" % x)  # digitsBaseTen counts the minus sign


def maf_block(r, t_sizes, q_sizes, q_prefix=b"", t_prefix=b"", rescore=False, score_zero=False):
    s = r["score"]
    if rescore or (score_zero and s == 0):
        s = score(r["t_sym"], r["q_sym"])
    comps = []
    for prefix, name, sizes, strand, start, end, text in (
            (t_prefix, r["t_name"], t_sizes, b"+", r["t_start"], r["t_end"], r["t_sym"]),
            (q_prefix, r["q_name"], q_sizes, r["strand"], r["q_start"], r["q_end"], r["q_sym"])):
        src = prefix + name
        if len(src) >= 256:
            raise BadInput("buffer overflow")
        if name not in sizes:
            raise BadInput("%r not found" % name)
        comps.append((b"defaultName" if src == b"." else src, start, end - start, strand, sizes[name], text))
    # (the query's size is looked up first there; either way the record aborts)
    w = [max(len(c[0]) for c in comps)] + [max(digits(c[k]) for c in comps) for k in (1, 2, 4)]
    out = b"a score=%f\n" % float(s)
    for src, start, size, strand, src_size, text in comps:
        out += b"s %-*s %*d %*d %s %*d %s\n" % (w[0], src, w[1], start, w[2], size, strand, w[3], src_size, text)
    return out + b"\n"


HEAD = b"##maf version=1 scoring=blastz\n"


def to_maf(data, t_sizes_data, q_sizes_data, q_prefix=b"", t_prefix=b"", t_split=False, rescore=False,
           score_zero=False):
    """the output file's bytes, or with t_split {file name: bytes}"""
    t_sizes, q_sizes = AP.read_sizes(t_sizes_data), AP.read_sizes(q_sizes_data)
    recs, tail = read_axt(data)
    kw = dict(q_prefix=q_prefix, t_prefix=t_prefix, rescore=rescore, score_zero=score_zero)
    if not t_split:
        out = HEAD
        for r in recs:
            out += b"".join(m + b"\n" for m in r["meta"]) + maf_block(r, t_sizes, q_sizes, **kw)
        return out + b"".join(m + b"\n" for m in tail)
    files, name = {}, b""
    for r in recs:
        block = maf_block(r, t_sizes, q_sizes, **kw)
        if r["t_name"] != name:
            name = r["t_name"]
            if name + b".maf" in files:
                raise BadInput("isn't sorted")
            files[name + b".maf"] = HEAD
        files[name + b".maf"] += block
    return files


# ------------------------------------------------------------ axtSort
def sort_axt(data, by_query=False, by_score=False):
    recs, tail = read_axt(data)
    if by_score:
        key = lambda r: -r["score"]  # noqa: E731
    elif by_query:
        key = lambda r: (r["q_name"], r["q_start"])  # noqa: E731
    else:
        key = lambda r: (r["t_name"], r["t_start"])  # noqa: E731
    # slAddHead reverses the list; slSort is stable (bytes compare as strcmp does)
    order = sorted(reversed(recs), key=key)
    out = b"".join(m + b"\n" for r in recs for m in r["meta"]) + b"".join(m + b"\n" for m in tail)
    for ix, r in enumerate(order):
        out += b"%d %s %d %d %s %d %d %s %d\n" % (ix, r["t_name"], r["t_start"] + 1, r["t_end"], r["q_name"],
                                                  r["q_start"] + 1, r["q_end"], r["strand"], r["score"])
        out += r["t_sym"] + b"\n" + r["q_sym"] + b"\n\n"
    return out


# ------------------------------------------------------------ shared inputs
def edge_rows():
    """(t_rows, q_rows): the scoring rules one by one"""
    pairs = [
        ("", ""), ("A", "A"), ("-", "A"), ("A", "-"), ("-", "-"),
        ("-ACGT", "AACGT"), ("ACGT-", "ACGTA"), ("AC--GT", "ACTTGT"),
        ("AC--GT", "AC-TGT"), ("AC-TGT", "ACT-GT"), ("AC-AGT", "ACT-GT"),   # runs that change rows
        ("AC-T-GT", "ACT-TGT"), ("A-C-G", "ATCTG"),                        # two runs
        ("AC.GT", "AC-GT"), ("AC-.-GT", "ACT.TGT"), ("AC-=-GT", "ACT=TGT"), ("AC-_-GT", "ACT_TGT"),
        ("acgtACGT", "ACGTacgt"), ("ACGTNnXx*19", "NNNNACGTACG"), ("AAAACCCCGGGGTTTT", "ACGTACGTACGTACGT"),
        ("aaaaccccggggtttt", "ACGTACGTACGTACGT"), ("------", "ACGTAC"), ("---", "---"),
    ]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def random_rows(seed=20261021, n=400, max_len=300):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTacgtACGTACGT----Nn.=_x", np.uint8)
    t_rows, q_rows = [], []
    for _ in range(n):
        ln = int(rng.integers(0, max_len + 1))
        t_rows.append(alphabet[rng.integers(0, len(alphabet), ln)].tobytes())
        q_rows.append(alphabet[rng.integers(0, len(alphabet), ln)].tobytes())
    return t_rows, q_rows


def read_input(path):
    with open(path, "rb") as f:
        return f.read()


def load_cases():
    with open(os.path.join(AXTMAF_DIR, "cases.json")) as f:
        return json.load(f)


def load_errors():
    with open(os.path.join(AXTMAF_DIR, "errors.json")) as f:
        return json.load(f)
