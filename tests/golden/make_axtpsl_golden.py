#!/usr/bin/env python3
"""Generate tests/golden/axtpsl/ with the REFERENCE axtToPsl.

Run in the build container (needs /root/reference and oracle/ref.mk's kent
archive, `make ref`):
    python tests/golden/make_axtpsl_golden.py

The reference tool is compiled into oracle/_ref/axtToPsl from
kent/src/hg/mouseStuff/axtToPsl/axtToPsl.c with oracle/ref.mk's tool flags
(GAC_REF_AXTTOPSL=path uses an existing binary instead).  Nothing of its
program text is kept.

Fixtures (data only):
  blockBug.axt / .sizes / .psl   the reference's own test (input and expected
                         output, copied; the output is made again here and
                         must equal the expected one)
  *.axt t.sizes q.sizes dup.sizes   purpose-built inputs (written here), one
                         file a subject: both strands; leading and trailing
                         one-sided columns on '+' and on '-'; columns with a
                         gap in both rows at the head, inside an insert and
                         between an insert and an aligned run; each of the
                         gap characters; the count rule's branches; records
                         that trim to nothing, of gaps only, of one column;
                         header coordinates that disagree with the rows; 8-
                         and 9-word headers; '#' lines before a header and
                         where a row is expected; a file without a final
                         blank line and one without a final line end; '\\r\\n'
                         lines; duplicated names in a sizes file
  s5.t.sizes s5.q.sizes  the sizes of tests/golden/axtchain/s5's sequences: its in.axt.gz
                         (610 records against t.2bit and q.2bit) is the case chain_s5,
                         whose output axtChain -psl can chain
  *.psl                  the reference's output
  cases.json             per case: the three inputs and the output
  err_*                  inputs of the error table
  errors.json            per case: the arguments ("{in}" "{t}" "{q}": the
                         inputs' paths, "{out}": a scratch file), the
                         reference's exit status, the first line of its stderr
                         with the paths replaced by their tags, and whether it
                         left output behind

Before anything is kept the generator asserts that the restatement
(tests/axtpsl_ref.py) gives the reference's output byte for byte on every
case, and raises BadInput exactly where the reference dies.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import axtpsl_ref as AR  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/ref.mk
OUT = AR.AXTPSL_DIR


def ref_binary():
    if os.environ.get("GAC_REF_AXTTOPSL"):
        return os.environ["GAC_REF_AXTTOPSL"]
    lib = os.path.join(REPO, "oracle", "_ref", "jkweb.a")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", REPO, "-f", "oracle/ref.mk", "oracle/_ref/jkweb.a", "-j8"],
                       check=True)
    k = os.path.join(REF, "kent", "src")
    exe = os.path.join(REPO, "oracle", "_ref", "axtToPsl")
    subprocess.run(["gcc", "-O2", "-fcommon", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE",
                    "-D_GNU_SOURCE", "-DMACHTYPE_x86_64", f"-I{k}/inc", f"-I{k}/hg/inc", "-w",
                    f"{k}/hg/mouseStuff/axtToPsl/axtToPsl.c", "-o", exe, lib,
                    "-lm", "-lz", "-lssl", "-lcrypto", "-pthread",
                    "-Wl,--warn-unresolved-symbols"], check=True, stderr=subprocess.DEVNULL)
    return exe


T_SIZES = "chrT\t100000\nchrT2\t5000\n"
Q_SIZES = "# query sizes\nchrQ\t90000\n\nchrQ2 4000 extra words\n"
DUP_SIZES = "chrT\t111\nchrQ\t222\nchrT\t100000\nchrQ\t90000\nchrT2\t5000\nchrQ2\t4000\n"


class Axt:
    def __init__(self):
        self.out = []
        self.k = 0

    def rec(self, t, q, strand="+", t_start=1001, q_start=2001, t_name="chrT", q_name="chrQ", score="3500",
            t_end=None, q_end=None, after="\n"):
        """a record whose header agrees with the rows, unless ends are given"""
        assert len(t) == len(q)
        nt = sum(c not in "-.=_" for c in t)
        nq = sum(c not in "-.=_" for c in q)
        t_end = t_start + nt - 1 if t_end is None else t_end
        q_end = q_start + nq - 1 if q_end is None else q_end
        head = "%d %s %d %d %s %d %d %s" % (self.k, t_name, t_start, t_end, q_name, q_start, q_end, strand)
        if score is not None:
            head += " " + score
        self.out.append(head + "\n" + t + "\n" + q + "\n" + after)
        self.k += 1
        return self

    def raw(self, s):
        self.out.append(s)
        return self

    def text(self):
        return "".join(self.out)


def built_inputs():
    f = {}
    a = Axt()
    for s in "+-":
        a.rec("ACGTACGTAC", "ACGTACGTAC", s)
        a.rec("ACGT--ACGTAC", "ACGTTTAC--AC", s)
        a.rec("ACGTACGTACGTACGT", "AC--AC--ACGT--GT", s, t_name="chrT2", q_name="chrQ2", t_start=1, q_start=1)
        a.rec("AC--GT--AC", "ACGTGTACAC", s, q_start=89990)
    f["strands.axt"] = a.text()

    a = Axt()
    for s in "+-":
        a.rec("--ACGTAC", "GGACGTAC", s)          # leading query-only columns
        a.rec("GGACGTAC", "--ACGTAC", s)          # leading target-only columns
        a.rec("ACGTAC---", "ACGTACTTT", s)        # trailing query-only
        a.rec("ACGTACTTT", "ACGTAC---", s)        # trailing target-only
        a.rec("--GGACG-TAC--TT", "CC--ACGATACGG--", s)   # both kinds at both ends
        a.rec("-G-ACGTAC", "C-CACGTAC", s)        # alternating at the head
        a.rec("ACGTAC-T-", "ACGTACG-G", s)        # alternating at the tail
    f["trims.axt"] = a.text()

    a = Axt()
    for s in "+-":
        a.rec("--ACGT", "--ACGT", s)              # both-gap at the head
        a.rec("-.G-ACGT", "_=-CACGT", s)          # both-gap, then one-sided, at the head
        a.rec("ACG--T-TTACG", "ACGAA--TTACG", s)  # a target insert next to a query insert
        a.rec("ACGTT-TTTACG", "ACG---TT-ACG", s)  # both-gap inside a target insert
        a.rec("ACG---TTACG", "ACGA-ATTACG", s)    # both-gap inside a query insert
        a.rec("ACGTT-ACG", "ACG---ACG", s)        # both-gap between an insert and an aligned run
        a.rec("ACG-TTACG", "ACG---ACG", s)        # both-gap between an aligned run and an insert
        a.rec("ACG-ACG", "ACG-ACG", s)            # both-gap inside an aligned run: one block
        a.rec("ACGT-A-CG", "ACG--ATCG", s)        # target insert, both-gap, aligned, query insert
        a.rec("ACG-.-ACG--", "ACG_=-ACG--", s)    # both-gap runs in the middle and at the tail
    f["bothgap.axt"] = a.text()

    a = Axt()
    for g in "-.=_":
        a.rec("ACG" + g + "TACGT" + g + g + "ACG", "ACGT" + g + g + "CGTAAACG")
        a.rec(g + "ACGT" + g, "A" + g + "CGTA", "-")
    a.rec("AC-GT.AC=GT_AC", "A_CG=TA.CG-TAC")
    f["gapchars.axt"] = a.text()

    a = Axt()
    pairs = ["AA", "aa", "aA", "Aa", "AC", "ac", "aC", "Ac", "NN", "NA", "AN", "Na", "nN", "nn", "nA", "An", "na",
             "an", "nc", "Nn", "XX", "xx", "xX", "Xy", "**", "*A", "1a"]
    for s in "+-":
        a.rec("".join(p[0] for p in pairs), "".join(p[1] for p in pairs), s)
        for p in pairs:
            a.rec("A" + p[0] + "C", "A" + p[1] + "C", s)
    f["counts.axt"] = a.text()

    a = Axt()
    for s in "+-":
        a.rec("ACG---", "---ACG", s)              # trims to nothing, coordinates used up
        a.rec("------", "ACGTAC", s)              # the same, one side only
        a.rec("ACGTAC", "------", s)
        a.rec("----", "-._=", s, t_end=1000, q_end=2000)   # gaps only, empty ranges
        a.rec("A", "A", s)                        # one column
        a.rec("A", "-", s)
        a.rec("-", "a", s)
        a.rec("-", "-", s, t_end=1000, q_end=2000)
        a.rec("", "", s, t_end=1000, q_end=2000)  # empty rows
    f["empty.axt"] = a.text()

    a = Axt()
    for s in "+-":
        a.rec("ACGTAC", "ACGTAC", s, t_end=1100, q_end=2200)      # ranges longer than the rows
        a.rec("ACGTACGTAC", "ACGTACGTAC", s, t_end=1003, q_end=2002)   # shorter
        a.rec("AC--GTAC", "ACGTGT--", s, t_end=1001, q_end=2050)
        a.rec("----", "----", s, t_end=1010, q_end=2010)          # gaps only, ranges not empty: a block of 0
        a.rec("--", "AC", s, t_end=1010, q_end=2010)              # trims to nothing, ranges left over
        a.rec("ACGT", "ACGT", s, t_start=0, q_start=0, t_end=3, q_end=3)   # starts of -1
        a.rec("ACGT", "ACGT", s, t_start=99990, q_start=89995)    # past the sequences' ends
        a.rec("ACGT", "ACGT", s, t_start=-5, q_start=-7, t_end=-2, q_end=-4)
        a.rec("ACGT", "AC-T", s, t_end=1004, q_end=2001)          # qStart == qEnd after nothing is trimmed
    f["disagree.axt"] = a.text()

    a = Axt()
    a.rec("ACGTAC", "ACGTAC", score=None)                 # 8 words
    a.rec("ACGTAC", "ACG-AC", score="-17")                # 9 words
    a.rec("ACGTAC", "ACGTAC", score="12 and more words")  # more: chopped at 10
    a.rec("ACGTAC", "ACTTAC", "-x", score="9x")           # atoi stops at the x; the strand's first character
    a.rec("ACGTAC", "AC-TAC", "?", score=None)
    a.raw("  7\tchrT   11 16\tchrQ 21 26  +   \nACGTAC\nACGTAC\n\n")   # white space of all kinds
    a.raw("8 chrT 11x 16.5 chrQ 021 26e3 -\nACGTAC\nACGTAC\n\n")       # atoi's numbers
    f["words.axt"] = a.text()

    a = Axt()
    a.raw("##matrix=axtChain 16 91 -114 -31 -123\n# a note\n\n")
    a.rec("ACGTAC", "ACGTAC")
    a.raw("# between records\n#\n")
    a.rec("#CGTAC", "A-GTAC")                     # a '#' line where the target row is expected
    a.rec("ACGTAC", "#-GTAC")                     # and where the query row is
    a.rec("ACGTAC", "ACGTAC", after="# the line after the rows is taken, whatever it holds\n")
    a.rec("ACGTAC", "ACGTAC", after="9 chrT 1 6 chrQ 1 6 + 1\n")   # a header there is taken too, and lost
    a.raw("\n \n\t\n")                            # blank lines of all kinds
    a.rec("ACG-AC", "ACGTAC")
    a.raw("# after the last record\n")
    f["comments.axt"] = a.text()
    a = Axt()
    a.rec("ACGTAC", "ACGTAC")
    a.rec("ACG-AC", "ACGTAC", after="")           # no line after the last rows
    f["nofinal.axt"] = a.text()
    f["nofinal_nonl.axt"] = a.text()[:-1]         # and no line end after the last row
    a = Axt()
    a.rec("ACGTAC", "AC-TAC").rec("AC--AC", "ACGTAC", "-")
    f["crlf.axt"] = a.text().replace("\n", "\r\n")
    f["dup.axt"] = f["strands.axt"]
    return f


# case -> (axt, tSizes, qSizes)
CASES = {
    "blockBug": ("blockBug.axt", "blockBug.sizes", "blockBug.sizes"),
    "strands": ("strands.axt", "t.sizes", "q.sizes"),
    "trims": ("trims.axt", "t.sizes", "q.sizes"),
    "bothgap": ("bothgap.axt", "t.sizes", "q.sizes"),
    "gapchars": ("gapchars.axt", "t.sizes", "q.sizes"),
    "counts": ("counts.axt", "t.sizes", "q.sizes"),
    "empty": ("empty.axt", "t.sizes", "q.sizes"),
    "disagree": ("disagree.axt", "t.sizes", "q.sizes"),
    "words": ("words.axt", "t.sizes", "q.sizes"),
    "comments": ("comments.axt", "t.sizes", "q.sizes"),
    "nofinal": ("nofinal.axt", "t.sizes", "q.sizes"),
    "nofinal_nonl": ("nofinal_nonl.axt", "t.sizes", "q.sizes"),
    "crlf": ("crlf.axt", "t.sizes", "q.sizes"),
    "dup_sizes": ("dup.axt", "dup.sizes", "dup.sizes"),
    "chain_s5": ("../axtchain/s5/in.axt.gz", "s5.t.sizes", "s5.q.sizes"),
}
S5_T_SIZES = "chrT1\t300000\nchrT2\t120000\n"
S5_Q_SIZES = "chrQ1\t250000\nchrQ2\t90000\n"

GOOD = "0 chrT 11 16 chrQ 21 26 + 100\nACGTAC\nACGTAC\n\n"
ERR_INPUTS = {
    "err_few_words.axt": GOOD + "1 chrT 11 16 chrQ 21 26\nACGTAC\nACGTAC\n\n",
    "err_number.axt": GOOD + "1 chrT 11 x16 chrQ 21 26 + 100\nACGTAC\nACGTAC\n\n",
    "err_score.axt": GOOD + "1 chrT 11 16 chrQ 21 26 + high\nACGTAC\nACGTAC\n\n",
    "err_rows.axt": GOOD + "1 chrT 11 16 chrQ 21 26 + 100\nACGTAC\nACGTA\n\n",
    "err_eof_header.axt": GOOD + "1 chrT 11 16 chrQ 21 26 + 100\n",
    "err_eof_row.axt": GOOD + "1 chrT 11 16 chrQ 21 26 + 100\nACGTAC\n",
    "err_tname.axt": GOOD + "1 chrU 11 16 chrQ 21 26 + 100\nACGTAC\nACGTAC\n\n",
    "err_qname.axt": GOOD + "1 chrT 11 16 chrU 21 26 + 100\nACGTAC\nACGTAC\n\n",
    "err_width.sizes": "chrT\t100000\nchrQ\n",
    "err_size.sizes": "chrT\t100000\nchrQ\tmany\n",
}

# name -> (arguments, axt, tSizes, qSizes)
ERRORS = {
    "few_words": (["{in}", "{t}", "{q}", "{out}"], "err_few_words.axt", "t.sizes", "q.sizes"),
    "not_a_number": (["{in}", "{t}", "{q}", "{out}"], "err_number.axt", "t.sizes", "q.sizes"),
    "score_not_a_number": (["{in}", "{t}", "{q}", "{out}"], "err_score.axt", "t.sizes", "q.sizes"),
    "unequal_rows": (["{in}", "{t}", "{q}", "{out}"], "err_rows.axt", "t.sizes", "q.sizes"),
    "eof_after_header": (["{in}", "{t}", "{q}", "{out}"], "err_eof_header.axt", "t.sizes", "q.sizes"),
    "eof_after_row": (["{in}", "{t}", "{q}", "{out}"], "err_eof_row.axt", "t.sizes", "q.sizes"),
    "target_name": (["{in}", "{t}", "{q}", "{out}"], "err_tname.axt", "t.sizes", "q.sizes"),
    "query_name": (["{in}", "{t}", "{q}", "{out}"], "err_qname.axt", "t.sizes", "q.sizes"),
    "sizes_width": (["{in}", "{t}", "{q}", "{out}"], "strands.axt", "t.sizes", "err_width.sizes"),
    "sizes_number": (["{in}", "{t}", "{q}", "{out}"], "strands.axt", "err_size.sizes", "q.sizes"),
    "argcount": (["{in}", "{t}", "{q}"], "strands.axt", "t.sizes", "q.sizes"),
    "argcount_option": (["-foo=1", "{in}"], "strands.axt", "t.sizes", "q.sizes"),
}


def read(name):
    return AR.read_input(os.path.join(OUT, name))


def main():
    os.makedirs(OUT, exist_ok=True)
    tests = os.path.join(REF, "kent", "src", "hg", "mouseStuff", "axtToPsl", "tests")
    shutil.copyfile(os.path.join(tests, "input", "blockBug.axt"), os.path.join(OUT, "blockBug.axt"))
    shutil.copyfile(os.path.join(tests, "input", "blockBug.sizes"), os.path.join(OUT, "blockBug.sizes"))
    texts = built_inputs()
    texts.update({"t.sizes": T_SIZES, "q.sizes": Q_SIZES, "dup.sizes": DUP_SIZES, "s5.t.sizes": S5_T_SIZES,
                  "s5.q.sizes": S5_Q_SIZES})
    texts.update(ERR_INPUTS)
    for name, body in texts.items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(body.encode("latin-1"))
    exe = ref_binary()
    cases, made = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.psl")
        for case, (axt, ts, qs) in CASES.items():
            r = subprocess.run([exe] + [os.path.join(OUT, x) for x in (axt, ts, qs)] + [out], capture_output=True)
            assert r.returncode == 0, (case, r.stderr)
            with open(out, "rb") as f:
                got = f.read()
            mine = AR.convert(read(axt), read(ts), read(qs))
            assert mine == got, (case, mine, got)
            made[case] = got
            cases[case] = dict(axt=axt, t_sizes=ts, q_sizes=qs, psl=case + ".psl")
            print(f"{case}: {got.count(10)} lines of {len(AR.read_axt(read(axt)))} records")
        with open(os.path.join(tests, "expected", "blockBug.psl"), "rb") as f:
            assert made["blockBug"] == f.read()
        errors = {}
        for name, (args, src, ts, qs) in ERRORS.items():
            paths = {"{in}": os.path.join(OUT, src), "{t}": os.path.join(OUT, ts),
                     "{q}": os.path.join(OUT, qs), "{out}": out}
            if os.path.exists(out):
                os.remove(out)
            r = subprocess.run([exe] + [paths.get(a, a) for a in args], capture_output=True)
            assert r.returncode == 255, (name, r.returncode)
            first = r.stderr.decode().split("\n")[0]
            for tag, p in paths.items():
                first = first.replace(p, tag)
            empty = not os.path.exists(out) or os.path.getsize(out) == 0
            if len(args) == 4:
                try:
                    AR.convert(read(src), read(ts), read(qs))
                    raise AssertionError(name + ": the restatement does not die")
                except AR.BadInput:
                    pass
            errors[name] = dict(args=args, input=src, t_sizes=ts, q_sizes=qs, status=r.returncode,
                                stderr=first, output_empty=empty)
            print(name, r.returncode, first, "" if empty else "(output left behind)")
    for case, got in made.items():
        with open(os.path.join(OUT, case + ".psl"), "wb") as f:
            f.write(got)
    for name, obj in (("cases.json", cases), ("errors.json", errors)):
        with open(os.path.join(OUT, name), "w") as f:
            json.dump(obj, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
