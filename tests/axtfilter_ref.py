"""filterAxtIdentityEntropy.py restated in plain Python, and what the axtfilter
tests share.

The rule (the reference's src/filterAxtIdentityEntropy.py): every line of the
input is read, lines starting with '#' are dropped wherever they stand, then
lines that are empty after stripping are skipped and three lines are taken at a
time, each stripped: header, target row, query row.  The header needs five
words, the third an integer.  L = len(query row); the target row may be longer.
With both characters lower-cased a column is a match when they are equal, and
the target adds to the count of a, c, g or t when it is one of them.  An entry
is written iff some start s with target[s] != '-' and s + W <= L has, over
columns [s, s + W), 100.0 * matches / W >= minSeqIdent and H >= minEntropy,
where H = 0.0 without a counted base and else, with p = k / n for the counts k
in the order a, c, g, t (zero counts skipped), e = 0.0; e -= p * log(p); H = e /
log(2).  The arithmetic here is the script's: Python floats and math.log, in
that order.

read_entries raises BadInput where the script dies (a truncated last entry, a
bad header, a target row shorter than the query row)."""
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
AXTF_DIR = os.path.join(GOLDEN, "axtfilter")


class BadInput(Exception):
    pass


def entropy(a, c, g, t):
    n = a + c + g + t
    if n == 0:
        return 0.0
    e = 0.0
    for k in (a, c, g, t):
        if k != 0:
            p = float(k) / float(n)
            e -= p * math.log(p)
    return e / math.log(2)


def identity(m, w):
    return 100.0 * m / w


def entry_passes(target, query, min_ident, min_entropy, w):
    """target and query: str; only the first len(query) columns of target count"""
    L = len(query)
    if w < 1:
        raise BadInput("window size")
    if len(target) < L:
        raise BadInput("target row shorter than the query row")
    t, q = target[:L].lower(), query.lower()
    pre = [(0, 0, 0, 0, 0)]
    for i in range(L):
        a, c, g, tt, m = pre[-1]
        ch = t[i]
        pre.append((a + (ch == "a"), c + (ch == "c"), g + (ch == "g"), tt + (ch == "t"),
                    m + (ch == q[i])))
    for s in range(L - w + 1):
        if target[s] == "-":
            continue
        lo, hi = pre[s], pre[s + w]
        if identity(hi[4] - lo[4], w) >= min_ident and \
                entropy(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], hi[3] - lo[3]) >= min_entropy:
            return True
    return False


def read_entries(text):
    """[(header, target, query)] of an input's text (newlines already universal)"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    lines = [ln for ln in lines if not ln.startswith("#")]
    out = []
    i = 0
    while i < len(lines):
        if lines[i].strip() == "":
            i += 1
            continue
        if i + 2 >= len(lines):
            raise BadInput("truncated entry")
        info, target, query = lines[i].strip(), lines[i + 1].strip(), lines[i + 2].strip()
        words = info.split()
        if len(words) < 5:
            raise BadInput("header of fewer than five words")
        try:
            int(words[2])
        except ValueError:
            raise BadInput("header's third word")
        out.append((info, target, query))
        i += 3
    return out


def read_text(path):
    """a file's text as the script reads it: '\\n', '\\r\\n' and '\\r' end a line"""
    with open(path, newline=None, encoding="latin-1") as f:
        return f.read()


def filter_entries(entries, min_ident, min_entropy, w):
    return [entry_passes(t, q, min_ident, min_entropy, w) for _h, t, q in entries]


def filter_text(text, min_ident, min_entropy, w):
    """the output file's text"""
    if w < 1:
        raise BadInput("window size")
    entries = read_entries(text)
    keep = filter_entries(entries, min_ident, min_entropy, w)
    return "".join(h + "\n" + t + "\n" + q + "\n\n" for (h, t, q), k in zip(entries, keep) if k)


# ------------------------------------------------------------ fixtures
def load_cases():
    """{run: (input path, [minSeqIdent, minEntropy, windowSize] as the command
    line has them, expected output path)}"""
    with open(os.path.join(AXTF_DIR, "cases.json")) as f:
        cases = json.load(f)
    return {k: (os.path.join(AXTF_DIR, c["input"]), list(c["args"]), os.path.join(AXTF_DIR, c["output"]))
            for k, c in cases.items()}


def load_errors():
    with open(os.path.join(AXTF_DIR, "errors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------ random rows
WINDOWS = (1, 2, 4, 6, 30)
ALPHABET = "ACGTacgtNn-"


def random_rows(seed, n=400):
    """seeded (target, query) rows over ACGTacgtNn-, L in 0..200: queries are
    mutated copies of their targets, a third of the targets of low complexity"""
    r = random.Random(seed)
    t_rows, q_rows = [], []
    for _ in range(n):
        L = r.choice((0, 1, 2, 5, 29, 30, 31)) if r.random() < 0.15 else r.randint(0, 200)
        kind = r.random()
        letters = ALPHABET if kind > 0.33 else r.choice(("AaCc-", "Tt", "ACGNn", "Gg-A"))
        t = "".join(r.choice(letters) for _ in range(L))
        rate = r.choice((0.0, 0.05, 0.2, 0.5))
        q = "".join(ch if r.random() >= rate else r.choice(ALPHABET) for ch in t)
        if r.random() < 0.1:
            t += "".join(r.choice(ALPHABET) for _ in range(r.randint(1, 9)))  # a longer target row
        t_rows.append(t)
        q_rows.append(q)
    return t_rows, q_rows


# thresholds of the random set per window: some entries pass, some do not
RANDOM_THRESHOLDS = {1: (100.0, 0.0), 2: (100.0, 1.0), 4: (75.0, 1.5), 6: (80.0, 1.25), 30: (70.0, 1.2)}
