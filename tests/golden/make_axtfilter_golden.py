#!/usr/bin/env python3
"""Generate tests/golden/axtfilter/ with the REFERENCE filterAxtIdentityEntropy.py.

Run in the build container (needs /root/reference; REF=path otherwise):
    python tests/golden/make_axtfilter_golden.py

The reference is a Python 2 script.  Its text is read, two mechanical shims are
applied in memory by regular expression -- the xrange( calls become range(,
and the print statement with a string becomes a call -- and the result is
written into a temporary directory and run there with python3.  Nothing of
the script, shimmed or not, is kept.

Fixtures (data only, written here):
  *.axt                  inputs, purpose-built (see the comments at each)
  *.out.axt              the reference's output of a run
  cases.json             per run: the input, the three arguments minSeqIdent
                         minEntropy windowSize as given on the command line, the
                         output.  Thresholds of the tie runs are computed here
                         (the value itself: kept; the next double above: dropped)
                         and stored by repr
  errors.json            per case: the arguments ("{in}": the input's path,
                         "{out}": a scratch file) and the reference's exit status

Before anything is kept the generator asserts that the restatement
(tests/axtfilter_ref.py) gives the reference's output byte for byte on every
run and dies where the reference dies, and that each run holds what it is
for."""
import itertools
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import axtfilter_ref as AR  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
OUT = AR.AXTF_DIR


def shimmed_reference(tmp):
    with open(os.path.join(REF, "src", "filterAxtIdentityEntropy.py")) as f:
        text = f.read()
    text, n_range = re.subn(r"\bxrange\(", "range(", text)
    text, n_print = re.subn(r'(?m)^(\s*)print\s+(".*")\s*$', r"\1print(\2)", text)
    assert n_range >= 1 and n_print >= 1, (n_range, n_print)
    path = os.path.join(tmp, "reference_py3.py")
    with open(path, "w") as f:
        f.write(text)
    return path


def run_ref(script, args):
    return subprocess.run([sys.executable, script] + args, capture_output=True, text=True)


def hdr(k, size=30):
    return "%d chrT %d %d chrQ %d %d + %d" % (k, 100 * k + 1, 100 * k + size, 7 * k + 1, 7 * k + size,
                                              1000 + k)


def axt(entries, start=0):
    """entries: (target, query)"""
    return "".join("%s\n%s\n%s\n\n" % (hdr(start + k, len(q)), t, q) for k, (t, q) in enumerate(entries))


# ------------------------------------------------------------ the inputs
# rules.axt, for W = 10, minSeqIdent 100, minEntropy 0 (kept = K, dropped = D):
RULES = [
    ("ACGTNNACGT", "ACGTnnACGT"),        # K  N / n columns match
    ("ACGTNNACGT", "ACGTaaACGT"),        # D  N against a base does not
    ("ACG--TACGT", "acg--tacgt"),        # K  - / - columns match, case is ignored
    ("ACGTACGTACGGGGG", "ACGTACGTAC"),   # K  a longer target row: accepted, written whole
    ("ACGTACGTA", "ACGTACGTA"),          # D  L = 9 < W
    ("-ACGTACGTAC", "-ACGTACGTAG"),      # D  the only passing window starts on a target gap
    ("CACGTACGTAC", "CACGTACGTAG"),      # K  the same window starting on a base
    ("ACGTACGTACGTACGTACGT", "ACGTACGTAGCTACGTACGT"),  # D  no window of 10 without a mismatch
    ("AAAAAAAAAAAA", "AAAAAAAAAAAA"),    # K  (entropy 0: dropped by the runs that ask for some)
    ("acgtacgtacNNNNNNNNNN", "acgtacgtacNNNNNNNNNN"),  # K
    ("----------ACGTACGTAC", "----------ACGTACGTAC"),  # K  by the window at 10 only
    ("", ""),                            # D  L = 0 (blank rows are lines like any other)
]
RULES_WANT = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0]


def rules_text():
    out = ""
    for k, (t, q) in enumerate(RULES):
        out += "%s\n%s\n%s\n\n" % (hdr(k, len(q)), t, q)
    return out


HASH_TEXT = (
    "##matrix=axtChain 16 91,-114,-31,-123\n"
    "# a comment before the first entry\n"
    + hdr(0, 12) + "\n"
    "# a comment between the header and the target row\n"
    "ACGTACGTACGT\n"
    "#ACGTACGTACGT (a row that starts with the comment sign is a comment)\n"
    "ACGTACGTACGT\n"
    "\n"
    + hdr(1, 12) + "\n"
    "ACGTTTGTACGT\n"
    "ACGTACGTACCC\n"
    "# a comment where the blank line would be\n"
    + hdr(2, 12) + "\n"
    "GGGTACGTACGT\n"
    "GGGTACGTACGT\n"
    "# the last line is a comment"
)

# CRLF ends, blanks and tabs around every line, runs of blank lines, two
# entries without a blank line between them, no newline at the end
CRLF_TEXT = (
    "\r\n\r\n  " + hdr(0, 12) + " \t\r\n"
    "\tACGTACGTACGT  \r\n"
    "ACGTACGTACGT\t \r\n"
    " \t \r\n"
    "\r\n"
    + hdr(1, 12) + "\r\n"
    "ACGTTTGTACGT\r\n"
    "ACGTACGTACCC\r\n"
    + hdr(2, 12) + "   \r\n"
    "  GGGTACGTACGT\r\n"
    "GGGTACGTACGT  "
)

# a lone carriage return ends a line too
CR_TEXT = CRLF_TEXT.replace("\r\n", "\r")


def tie_inputs():
    """{name: (text, W, which threshold, value)}: the threshold at the value keeps
    the first entry, the next double above drops it"""
    t = {}
    # identity 100.0 * 18 / 30: 18 of 30 columns match
    tgt = "ACGTACGTACGTACGTACGTACGTACGTAC"
    qry = tgt[:18] + "".join("A" if c != "A" else "C" for c in tgt[18:])
    t["tie_ident60"] = (axt([(tgt, qry)]), 30, "ident", AR.identity(18, 30))
    t["tie_ident33"] = (axt([("ACG", "ATT")]), 3, "ident", AR.identity(1, 3))
    t["tie_ent1111"] = (axt([("ACGT", "TTTT")]), 4, "entropy", AR.entropy(1, 1, 1, 1))
    t["tie_ent15_15"] = (axt([("A" * 15 + "C" * 15, "A" * 30)]), 30, "entropy", AR.entropy(15, 15, 0, 0))
    t["tie_ent10_10_10"] = (axt([("A" * 10 + "C" * 10 + "G" * 10, "A" * 30)]), 30, "entropy",
                            AR.entropy(10, 10, 10, 0))
    # counts (0, 1, 2, 3) in a, c, g, t order, and the same counts given to other
    # bases: an assignment whose sum, in a, c, g, t order, comes out lower
    want = AR.entropy(0, 1, 2, 3)
    lower = [p for p in itertools.permutations((0, 1, 2, 3)) if AR.entropy(*p) < want]
    assert lower, "no assignment of the counts 0 1 2 3 sums lower"
    a, c, g, tt = lower[0]
    t["tie_ent0123"] = (axt([("CGGTTT", "CGGTTT"), ("A" * a + "C" * c + "G" * g + "T" * tt, "AAAAAA")]), 6,
                        "entropy", want)
    return t


def main():
    tmp = tempfile.mkdtemp()
    try:
        script = shimmed_reference(tmp)
        if os.path.isdir(OUT):
            shutil.rmtree(OUT)
        os.makedirs(OUT)
        inputs = {"rules": rules_text(), "hash": HASH_TEXT, "crlf": CRLF_TEXT, "cr": CR_TEXT, "empty": "",
                  "comments_only": "# nothing\n# but comments\n"}
        runs = {  # run: (input, minSeqIdent, minEntropy, windowSize)
            "rules_w10": ("rules", "100", "0", "10"),
            "rules_w10_entropy": ("rules", "100", "1.9", "10"),
            "rules_w10_loose": ("rules", "85.5", "1.5", "10"),
            "rules_w1": ("rules", "100", "0", "1"),
            "rules_w12_negative": ("rules", "-5", "-1", "12"),
            "rules_w2000": ("rules", "0", "0", "2000"),
            "hash_w12": ("hash", "100", "1.5", "12"),
            "hash_w4": ("hash", "100", "2", "4"),
            "crlf_w12": ("crlf", "100", "1.5", "12"),
            "crlf_w4": ("crlf", "100", "2", "4"),
            "cr_w12": ("cr", "100", "1.5", "12"),
            "empty_w10": ("empty", "50", "1", "10"),
            "comments_only_w10": ("comments_only", "50", "1", "10"),
        }
        ties = tie_inputs()
        for name, (text, w, which, value) in ties.items():
            inputs[name] = text
            above = math.nextafter(value, math.inf)
            for tag, v in (("at", value), ("above", above)):
                runs["%s_%s" % (name, tag)] = (name, repr(v) if which == "ident" else "0",
                                               repr(v) if which == "entropy" else "0", str(w))
        for name, text in inputs.items():
            with open(os.path.join(OUT, name + ".axt"), "wb") as f:
                f.write(text.encode("latin-1"))

        cases = {}
        for run, (inp, ident, ent, w) in sorted(runs.items()):
            src = os.path.join(OUT, inp + ".axt")
            dst = os.path.join(OUT, run + ".out.axt")
            r = run_ref(script, [src, ident, ent, w, dst])
            assert r.returncode == 0, (run, r.stderr)
            mine = AR.filter_text(AR.read_text(src), float(ident), float(ent), int(w))
            with open(dst, newline="") as f:
                got = f.read()
            assert mine == got, run
            cases[run] = dict(input=inp + ".axt", args=[ident, ent, w], output=run + ".out.axt")

        def kept(run):
            with open(os.path.join(OUT, run + ".out.axt")) as f:
                heads = [ln.split()[0] for ln in f.read().split("\n")[0::4] if ln]
            return [int(h) for h in heads]

        # what the runs are for
        assert kept("rules_w10") == [k for k, w in enumerate(RULES_WANT) if w], kept("rules_w10")
        assert 0 < len(kept("rules_w10_entropy")) < len(kept("rules_w10"))
        assert kept("rules_w2000") == [] and len(kept("rules_w12_negative")) >= 3
        assert kept("hash_w12") == [0, 2] and kept("crlf_w12") == [0, 2] and kept("cr_w12") == [0, 2]
        assert kept("hash_w4") == [0, 1, 2] and kept("crlf_w4") == [0, 1, 2]
        with open(os.path.join(OUT, "rules_w10.out.axt")) as f:
            assert "ACGTACGTACGGGGG\n" in f.read()  # the longer target row, whole
        for name in ties:
            assert kept(name + "_at")[:1] == [0] and 0 not in kept(name + "_above"), name
        assert kept("tie_ent0123_at") == [0]  # the other assignment of the same counts stays below

        # ---- the error table
        bad_inputs = {
            "err_truncated": hdr(0, 12) + "\nACGTACGTACGT\nACGTACGTACGT\n\n" + hdr(1, 12) + "\nACGTACGTACGT\n",
            "err_header4": "0 chrT 1 12\nACGTACGTACGT\nACGTACGTACGT\n\n",
            "err_header_int": "0 chrT one 12 chrQ 1 12 + 100\nACGTACGTACGT\nACGTACGTACGT\n\n",
            "err_target_short": hdr(0, 12) + "\nACGTACGTAC\nACGTACGTACGT\n\n",
        }
        for name, text in bad_inputs.items():
            with open(os.path.join(OUT, name + ".axt"), "w") as f:
                f.write(text)
        errors = {
            "truncated": dict(input="err_truncated.axt", args=["{in}", "50", "1", "10", "{out}"]),
            "header4": dict(input="err_header4.axt", args=["{in}", "50", "1", "10", "{out}"]),
            "header_int": dict(input="err_header_int.axt", args=["{in}", "50", "1", "10", "{out}"]),
            "target_short": dict(input="err_target_short.axt", args=["{in}", "50", "1", "10", "{out}"]),
            "window0": dict(input="rules.axt", args=["{in}", "50", "1", "0", "{out}"]),
            "args4": dict(input="rules.axt", args=["{in}", "50", "1", "10"]),
            "args6": dict(input="rules.axt", args=["{in}", "50", "1", "10", "{out}", "extra"]),
            "args0": dict(input="rules.axt", args=[]),
            "ok": dict(input="rules.axt", args=["{in}", "50", "1", "10", "{out}"]),
        }
        for name, e in sorted(errors.items()):
            src = os.path.join(OUT, e["input"])
            scratch = os.path.join(tmp, name + ".out")
            r = run_ref(script, [{"{in}": src, "{out}": scratch}.get(a, a) for a in e["args"]])
            e["status"] = r.returncode
            assert r.returncode in (0, 1), (name, r.returncode, r.stderr)
            assert (name == "ok") == (r.returncode == 0), (name, r.stderr)
            if len(e["args"]) == 5 and name != "window0":  # the restatement dies there too
                died = False
                try:
                    AR.filter_text(AR.read_text(src), float(e["args"][1]), float(e["args"][2]),
                                   int(e["args"][3]))
                except AR.BadInput:
                    died = True
                assert died == (r.returncode != 0), name
            if len(e["args"]) != 5:
                assert r.stdout.startswith("Usage") and r.stderr == "", name
        with open(os.path.join(OUT, "cases.json"), "w") as f:
            json.dump(cases, f, indent=1, sort_keys=True)
            f.write("\n")
        with open(os.path.join(OUT, "errors.json"), "w") as f:
            json.dump(errors, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %d runs, %d error cases to %s" % (len(cases), len(errors), OUT))
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
