"""axtToPsl restated in plain Python, and what the axtpsl tests share.

The rule (the reference's kent/src/hg/mouseStuff/axtToPsl/axtToPsl.c over
axtRead, kent/src/lib/axt.c:52-92, pslFromAlign, kent/src/lib/psl.c:1626-1806,
and pslTabOut, psl.c:175-254):

Lines are lineFile's: the first '\\n' or '\\r' of a file decides whether lines
end with '\\n', with '\\r\\n' (a '\\r' before the '\\n' is dropped) or with '\\r';
a last line without an end counts.  A record is the next line that does not
start with '#' and has a word (its first eight words at least: words 3, 4, 6, 7
and, if present, 9 must start with '-' or a digit and are read by atoi; the
strand is the first character of word 8), then two lines taken as they are,
target row and query row, of equal length, then one more line, whatever it
holds.  A sizes file is lines of two words at least, '#' lines and blank lines
skipped; the last line of a name counts.

qStart / qEnd are flipped to the plus strand for '-', the trim moves the
psl's qStart / tStart for leading one-sided columns and qEnd / tEnd for
trailing ones (in those flipped coordinates: on '-' the wrong end moves, as in
the reference), nothing is written when qStart == qEnd or tStart == tEnd after
it, and the blocks start from the flipped-back qStart.  Columns with a gap
('-', '.', '=', '_') in both rows are skipped and are not a "previous" column.

BadInput is raised where the reference aborts."""
import gzip
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
AXTPSL_DIR = os.path.join(GOLDEN, "axtpsl")

DEL = frozenset(b"-.=_")
SPACE = frozenset(b" \t\n\v\f\r")


class BadInput(Exception):
    pass


# ------------------------------------------------------------ lineFile
def split_lines(data):
    """the lines lineFileNext returns for a file's bytes"""
    first = next((c for c in data if c in (10, 13)), None)
    if first is None:
        return [data] if data else []
    sep, dos = b"\n", False
    if first == 13:
        i = data.index(b"\r")
        if data[i + 1:i + 2] == b"\n":
            dos = True
        else:
            sep = b"\r"
    lines = data.split(sep)
    if lines[-1] == b"":
        lines.pop()
    if dos:
        lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]
    # (the lines are zero-terminated strings there: a NUL ends one early)
    return [ln.split(b"\0")[0] for ln in lines]


def chop_by_white(line, max_words):
    words, i, n = [], 0, len(line)
    while len(words) < max_words:
        while i < n and line[i] in SPACE:
            i += 1
        if i == n:
            break
        a = i
        while i < n and line[i] not in SPACE:
            i += 1
        words.append(line[a:i])
    return words


def need_num(word):
    """lineFileNeedNum: a '-' or a digit first, then atoi"""
    if not (word[:1] == b"-" or word[:1].isdigit()):
        raise BadInput("Expecting number, got %r" % word)
    i = 1 if word[:1] == b"-" else 0
    j = i
    while j < len(word) and 48 <= word[j] <= 57:
        j += 1
    v = int(word[i:j] or b"0")
    return -v if i else v


def chop_next(lines, at, max_words):
    """lineFileChopNext: (words, index after the line) or (None, len)"""
    while at < len(lines):
        ln = lines[at]
        at += 1
        if ln[:1] == b"#":
            continue
        words = chop_by_white(ln, max_words)
        if words:
            return words, at
    return None, at


def read_sizes(data):
    sizes, lines, at = {}, split_lines(data), 0
    while True:
        words, at = chop_next(lines, at, 2)
        if words is None:
            return sizes
        if len(words) < 2:
            raise BadInput("Expecting 2 words got %d" % len(words))
        sizes[words[0]] = need_num(words[1])  # hashAdd puts the newest first: the last line counts


def read_axt(data):
    """[(qName, qStart, qEnd, strand, tName, tStart, tEnd, tSym, qSym)] as axtRead fills them"""
    lines, at, out = split_lines(data), 0, []
    while True:
        w, at = chop_next(lines, at, 10)
        if w is None:
            return out
        if len(w) < 8:
            raise BadInput("Expecting at least 8 words got %d" % len(w))
        q_start, q_end = need_num(w[5]) - 1, need_num(w[6])
        t_start, t_end = need_num(w[2]) - 1, need_num(w[3])
        if len(w) > 8:
            need_num(w[8])
        if at + 2 > len(lines):
            raise BadInput("Unexpected end of file")
        t_sym, q_sym = lines[at], lines[at + 1]
        if len(t_sym) != len(q_sym):
            raise BadInput("Symbol count %d != %d" % (len(t_sym), len(q_sym)))
        at += 3  # the rows and one more line, if there is one
        out.append((w[4], q_start, q_end, w[7][:1], w[1], t_start, t_end, t_sym, q_sym))


# ------------------------------------------------------------ pslFromAlign
def _upper(c):
    return c - 32 if 97 <= c <= 122 else c


def psl_from_align(q_size, q_start, q_end, q_str, t_start, t_end, t_str, minus):
    """the psl's numbers, or None: dict(counts=[match, misMatch, repMatch,
    nCount, qNumInsert, qBaseInsert, tNumInsert, tBaseInsert], qStart, qEnd,
    tStart, tEnd, blocks=[(size, qStart, tStart)], cols)"""
    assert len(q_str) == len(t_str)
    lo, n = 0, len(q_str)
    while n > 0 and (q_str[lo] in DEL or t_str[lo] in DEL):  # trimAlignment
        if q_str[lo] not in DEL:
            q_start += 1
        elif t_str[lo] not in DEL:
            t_start += 1
        lo += 1
        n -= 1
    while n > 0 and (q_str[lo + n - 1] in DEL or t_str[lo + n - 1] in DEL):
        if q_str[lo + n - 1] not in DEL:
            q_end -= 1
        elif t_str[lo + n - 1] not in DEL:
            t_end -= 1
        n -= 1
    if q_start == q_end or t_start == t_end:
        return None
    qs, qe = (q_size - q_end, q_size - q_start) if minus else (q_start, q_end)
    ts = t_start
    qe, te = qs, ts
    match = mis = rep = ncount = q_num = q_base = t_num = t_base = 0
    blocks, either, prev_q, prev_t = [], False, 0, 0
    for i in range(lo, lo + n):
        q, t = q_str[i], t_str[i]
        qd, td = q in DEL, t in DEL
        if qd and td:
            continue
        if qd or td:
            if not either:
                blocks.append((qe - qs, qs, ts))
                either = True
            qe += not qd
            te += not td
        else:
            if either:
                qs, ts, either = qe, te, False
            qe += 1
            te += 1
        if not qd and not td:  # accumCounts
            if q == 78 or t == 78:
                ncount += 1
            elif _upper(q) == _upper(t):
                if _upper(q) != q or _upper(t) != t:
                    rep += 1
                else:
                    match += 1
            else:
                mis += 1
        elif qd:
            t_base += 1
            t_num += prev_q not in DEL
        else:
            q_base += 1
            q_num += prev_t not in DEL
        prev_q, prev_t = q, t
    blocks.append((qe - qs, qs, ts))
    return dict(counts=[match, mis, rep, ncount, q_num, q_base, t_num, t_base], qStart=q_start,
                qEnd=q_end, tStart=t_start, tEnd=t_end, blocks=blocks, cols=n)


def _u(v):
    return b"%d" % (v & 0xffffffff)


def _d(v):
    v &= 0xffffffff
    return b"%d" % (v - (1 << 32) if v >> 31 else v)


def psl_line(p, strand, q_name, q_size, t_name, t_size):
    """pslTabOut"""
    c = p["counts"]
    f = [_u(c[0]), _u(c[1]), _u(c[2]), _u(c[3]), _u(c[4]), _d(c[5]), _u(c[6]), _d(c[7]), strand,
         q_name, _u(q_size), _u(p["qStart"]), _u(p["qEnd"]), t_name, _u(t_size), _u(p["tStart"]),
         _u(p["tEnd"]), _u(len(p["blocks"]))]
    for k in range(3):
        f.append(b"".join(_u(b[k]) + b"," for b in p["blocks"]))
    return b"\t".join(f) + b"\n"


def convert(axt, t_sizes, q_sizes):
    """axtToPsl's output for the three files' bytes"""
    ts, qs = read_sizes(t_sizes), read_sizes(q_sizes)
    out = []
    for q_name, q_start, q_end, strand, t_name, t_start, t_end, t_sym, q_sym in read_axt(axt):
        if q_name not in qs:
            raise BadInput("%r not found" % q_name)
        q_size = qs[q_name]
        minus = strand == b"-"
        if minus:
            q_start, q_end = q_size - q_end, q_size - q_start
        if t_name not in ts:
            raise BadInput("%r not found" % t_name)
        p = psl_from_align(q_size, q_start, q_end, q_sym, t_start, t_end, t_sym, minus)
        if p is not None:
            out.append(psl_line(p, strand, q_name, q_size, t_name, ts[t_name]))
    return b"".join(out)


# ------------------------------------------------------------ the library's view
BIG = 1 << 40


def entry_result(t_row, q_row):
    """what gac_axt_psl returns for one entry: (counts[8], (q_head, t_head,
    q_tail, t_tail), cols, [(q_adv, t_adv, size)]), through psl_from_align on
    coordinates wide enough never to be empty"""
    p = psl_from_align(0, 0, BIG, q_row, 0, BIG, t_row, False)
    qh, th = p["qStart"], p["tStart"]
    blocks = [(q - qh, t - th, s) for s, q, t in p["blocks"]]
    return p["counts"], (qh, th, BIG - p["qEnd"], BIG - p["tEnd"]), p["cols"], blocks


def as_bytes(rows):
    return [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]


def results(t_rows, q_rows):
    return [entry_result(t, q) for t, q in zip(as_bytes(t_rows), as_bytes(q_rows))]


# ------------------------------------------------------------ fixtures
def load_cases():
    """{case: (axt path, tSizes path, qSizes path, expected psl path)}"""
    with open(os.path.join(AXTPSL_DIR, "cases.json")) as f:
        cases = json.load(f)
    return {k: tuple(os.path.join(AXTPSL_DIR, c[x]) for x in ("axt", "t_sizes", "q_sizes", "psl"))
            for k, c in cases.items()}


def load_errors():
    with open(os.path.join(AXTPSL_DIR, "errors.json")) as f:
        return json.load(f)


def read_input(path):
    """a file's bytes, a .gz file's decompressed"""
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        return f.read()


def golden_rows():
    """(target rows, query rows) of every entry of every golden input"""
    t_rows, q_rows = [], []
    for axt, _t, _q, _psl in load_cases().values():
        for e in read_axt(read_input(axt)):
            t_rows.append(e[7])
            q_rows.append(e[8])
    return t_rows, q_rows


ALPHABET = "ACGTacgtNn-.=_"


def random_rows(seed=20261021, n=2000):
    """seeded (target, query) rows of 1..300 columns over ACGTacgtNn-.=_: half
    the entries draw every character from the alphabet, the others are a
    mutated copy with gap runs, as alignments are"""
    r = random.Random(seed)
    t_rows, q_rows = [], []
    for k in range(n):
        L = r.randint(1, 300)
        if k % 2 == 0:
            t = "".join(r.choice(ALPHABET) for _ in range(L))
            q = "".join(r.choice(ALPHABET) for _ in range(L))
        else:
            t = [r.choice("ACGTacgtNn") for _ in range(L)]
            q = [c if r.random() > 0.2 else r.choice("ACGTacgtNn") for c in t]
            for _ in range(r.randint(0, 6)):
                a = r.randrange(L)
                b = min(L, a + r.randint(1, 12))
                side, g = r.choice((t, q, None)), r.choice("-.=_")
                for j in range(a, b):
                    if side is None:
                        t[j] = q[j] = g
                    else:
                        side[j] = g
            t, q = "".join(t), "".join(q)
        t_rows.append(t)
        q_rows.append(q)
    return t_rows, q_rows
