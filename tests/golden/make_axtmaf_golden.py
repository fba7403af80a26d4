#!/usr/bin/env python3
"""Generate tests/golden/axtmaf/ with the REFERENCE axtToMaf and axtSort.

    python tests/golden/make_axtmaf_golden.py

The two reference tools (kent/src/hg/mouseStuff/axtToMaf, .../axtSort) are
compiled into oracle/_ref/ against oracle/_ref/jkweb.a with the flags of
oracle/ref.mk; only data is kept here: small purpose-built .axt and sizes
inputs, what the reference wrote for them, and two tables,
  cases.json   name -> tool, options, input, t_sizes, q_sizes, output (a file,
               or for -tSplit a directory and its files)
  errors.json  name -> tool, args ({in} {t} {q} {out} stand for the paths),
               status, the first line of stderr with the paths tagged, and
               whether the reference left output behind.

Before anything is kept the restatement (tests/axtscore_ref.py) must give the
reference's bytes for every case -- with them every score -score and
-scoreZero printed -- and raise BadInput for every error row that is about the
input.

The inputs hold: both strands; headers of 8 and of 9 words; scores that are 0,
positive and negative, each under no option, -score and -scoreZero; prefixes;
the name "."; values at which a column gets wider (start 0 and -1, 9 / 10,
99,999 / 100,000); '#' lines at the head, between records, inside a record's
four lines and at the end; \\r\\n lines; no final blank line; sizes files with
a name twice; -tSplit on sorted and on unsorted input; and for axtSort a file
with ties on every key and names that differ only in strcmp order.  Scores
whose difference does not fit an int, and bytes >= 0x80, are left out: the
reference's behaviour there is undefined.
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

import axtscore_ref as AS  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/ref.mk
OUT = AS.AXTMAF_DIR


def ref_binary(tool):
    lib = os.path.join(REPO, "oracle", "_ref", "jkweb.a")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", REPO, "-f", "oracle/ref.mk", "oracle/_ref/jkweb.a", "-j8"],
                       check=True)
    k = os.path.join(REF, "kent", "src")
    exe = os.path.join(REPO, "oracle", "_ref", tool)
    subprocess.run(["gcc", "-O2", "-fcommon", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE",
                    "-D_GNU_SOURCE", "-DMACHTYPE_x86_64", f"-I{k}/inc", f"-I{k}/hg/inc", "-w",
                    f"{k}/hg/mouseStuff/{tool}/{tool}.c", "-o", exe, lib,
                    "-lm", "-lz", "-lssl", "-lcrypto", "-pthread",
                    "-Wl,--warn-unresolved-symbols"], check=True, stderr=subprocess.DEVNULL)
    return exe


T_SIZES = "chrT\t100000\nchrT2\t5000\n.\t777\nchr10\t2000000\nchr2\t3000000\n"
Q_SIZES = "# query sizes\nchrQ\t90000\n\nchrQ2 4000 extra words\n.\t12\nscaffold_123456\t1234567\n"
DUP_SIZES = ("chrT\t111\nchrQ\t222\nchrT\t100000\nchrQ\t90000\nchrT2\t5000\nchrQ2\t4000\n.\t1\n.\t777\n"
             "chr10\t2000000\nchr2\t3000000\nscaffold_123456\t7\nscaffold_123456\t1234567\n")


class Axt:
    def __init__(self):
        self.out = []
        self.k = 0

    def rec(self, t, q, strand="+", t_start=1001, q_start=2001, t_name="chrT", q_name="chrQ", score="3500",
            after="\n", inside=""):
        """a record whose header agrees with the rows; inside: text between the rows"""
        assert len(t) == len(q)
        t_end = t_start + sum(c != "-" for c in t) - 1
        q_end = q_start + sum(c != "-" for c in q) - 1
        head = "%d %s %d %d %s %d %d %s" % (self.k, t_name, t_start, t_end, q_name, q_start, q_end, strand)
        if score is not None:
            head += " " + score
        self.out.append(head + "\n" + t + "\n" + inside + q + "\n" + after)
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
    a.raw("# made by hand\n##matrix=16 91 -114\n")
    a.rec("ACGTACGTAC", "ACGTACGTAC")                                   # 9 words, a score that is kept
    a.rec("ACGT--ACGTAC", "ACGTTTAC--AC", "-", score="0")               # a score of 0
    a.rec("ACGTACGTACGTACGT", "AC--AC--ACGT--GT", "-", t_name="chrT2", q_name="chrQ2", t_start=1, q_start=1,
          score=None)                                                   # 8 words; start 0
    a.raw("# between records\n\n")
    a.rec("AC--GT--AC", "ACGTGTACAC", q_start=89990, score="-250")      # a negative score
    a.rec("acgtnNACGT", "ACGTACgtxa", t_start=10, q_start=11)           # 9 / 10
    a.rec("ACGTACGTAC" * 3, "ACGTACG-AC" * 3, t_start=99991, q_start=10, score="0")   # ends at 100,000 + 20
    a.rec("ACGTAC", "AC-TAC", t_start=100000, q_start=100000 - 99990 + 9, q_name="scaffold_123456")
    a.rec("ACG-T", "ACGTT", t_name=".", q_name=".", t_start=5, q_start=0, score="0")  # the name "."; start -1
    a.rec("AC-.=_GT", "ACT.=_-T", "-", score="12")                      # '.', '=', '_' are no gaps
    a.rec("---A", "C---", score="0")                                    # a run that changes rows
    a.raw("# at the end\n#\n")
    f["basic.axt"] = a.text()
    f["crlf.axt"] = f["basic.axt"].replace("\n", "\r\n")

    a = Axt()
    a.rec("ACGT", "ACGT", score="0")
    a.rec("AC-T", "ACGT", "-", score=None, after="")
    f["nofinal.axt"] = a.text()
    f["nofinal_nl.axt"] = f["nofinal.axt"][:-1]                         # and no line end either

    a = Axt()
    a.rec("ACGT", "ACGT", after="#the fourth line of a record\n")
    a.raw("#before a header\n")
    a.rec("#CGT", "ACGT", score="0")                                    # a target row that starts with '#'
    a.rec("ACGT", "A-GT", after="not blank and not read\n")
    f["meta.axt"] = a.text()

    a = Axt()
    for name, start in (("chr10", 500), ("chr10", 20), ("chr2", 7), ("chr2", 7), ("chrT", 1)):
        a.rec("ACGTACGT", "ACG-ACGT", t_name=name, t_start=start, score="0" if start == 7 else "77")
    a.raw("# split inputs keep no comment\n")
    f["split_sorted.axt"] = a.text()
    a.rec("ACGT", "ACGT", t_name="chr10", t_start=9)
    f["split_unsorted.axt"] = a.text()

    # axtSort: ties on every key; chr10 < chr2 in strcmp order
    a = Axt()
    a.raw("# sort me\n")
    rows = [("chr2", 100, "chrQ", 50, "10"), ("chr10", 100, "chrQ2", 50, "30"), ("chr2", 100, "chrQ", 50, "30"),
            ("chr10", 5, "chrQ", 7, "10"), ("chr2", 20, "chrQ2", 50, "-5"), ("chr10", 100, "chrQ", 7, None),
            ("chr2", 100, "chrQ2", 9, "30"), ("chrT", 1, "chrQ", 50, "0"), ("chr10", 5, "chrQ2", 9, "10")]
    for k, (tn, ts, qn, qs, sc) in enumerate(rows):
        t = "ACGT" + "ACGT"[k % 4] * (k + 1)
        a.rec(t, t.lower() if k % 2 else t, "-" if k % 3 == 0 else "+", t_name=tn, t_start=ts, q_name=qn, q_start=qs,
              score=sc)
        if k == 4:
            a.raw("# in the middle\n")
    a.raw("# the last line\n")
    f["sort.axt"] = a.text()
    f["sort_crlf.axt"] = f["sort.axt"].replace("\n", "\r\n")
    f["empty.axt"] = "# nothing but a comment\n\n"

    # errors
    f["short_head.axt"] = Axt().rec("ACGT", "ACGT").text() + "1 chrT 1 4 chrQ 1 4\nACGT\nACGT\n\n"
    f["bad_number.axt"] = Axt().rec("ACGT", "ACGT").text() + "1 chrT x1 4 chrQ 1 4 +\nACGT\nACGT\n\n"
    f["unequal.axt"] = Axt().rec("ACGT", "ACGT").text() + "1 chrT 1 4 chrQ 1 3 + 10\nACGT\nACG\n\n"
    f["truncated.axt"] = Axt().rec("ACGT", "ACGT").text() + "1 chrT 1 4 chrQ 1 4 + 10\nACGT\n"
    f["no_tname.axt"] = Axt().rec("ACGT", "ACGT").rec("ACGT", "ACGT", t_name="chrNone").text()
    f["no_qname.axt"] = Axt().rec("ACGT", "ACGT").rec("ACGT", "ACGT", q_name="chrNone").text()

    f["t.sizes"] = T_SIZES
    f["q.sizes"] = Q_SIZES
    f["dup.sizes"] = DUP_SIZES
    f["one_word.sizes"] = "chrT\t100000\nchrQ\n"
    return f


MAF_CASES = {  # name: (input, t_sizes, q_sizes, options)
    "basic": ("basic.axt", "t.sizes", "q.sizes", []),
    "basic_score": ("basic.axt", "t.sizes", "q.sizes", ["-score"]),
    "basic_scorezero": ("basic.axt", "t.sizes", "q.sizes", ["-scoreZero"]),
    "basic_prefix": ("basic.axt", "t.sizes", "q.sizes", ["-tPrefix=hg38.", "-qPrefix=mm10.", "-scoreZero"]),
    "basic_dup_sizes": ("basic.axt", "dup.sizes", "dup.sizes", ["-score"]),
    "crlf": ("crlf.axt", "t.sizes", "q.sizes", []),
    "crlf_score": ("crlf.axt", "t.sizes", "q.sizes", ["-score"]),
    "nofinal": ("nofinal.axt", "t.sizes", "q.sizes", ["-scoreZero"]),
    "nofinal_nl": ("nofinal_nl.axt", "t.sizes", "q.sizes", ["-score"]),
    "meta": ("meta.axt", "t.sizes", "q.sizes", []),
    "meta_score": ("meta.axt", "t.sizes", "q.sizes", ["-score"]),
    "empty": ("empty.axt", "t.sizes", "q.sizes", ["-score"]),
    "split": ("split_sorted.axt", "t.sizes", "q.sizes", ["-tSplit"]),
    "split_score": ("split_sorted.axt", "t.sizes", "q.sizes", ["-tSplit", "-scoreZero", "-tPrefix=x."]),
}
SORT_CASES = {  # name: (input, options)
    "sort_target": ("sort.axt", []),
    "sort_query": ("sort.axt", ["-query"]),
    "sort_score": ("sort.axt", ["-byScore"]),
    "sort_score_query": ("sort.axt", ["-byScore", "-query"]),
    "sort_any_option": ("sort.axt", ["-whatever=3"]),
    "sort_crlf": ("sort_crlf.axt", ["-query"]),
    "sort_basic": ("basic.axt", []),
    "sort_meta": ("meta.axt", ["-query"]),
    "sort_empty": ("empty.axt", []),
}
ERRORS = {  # name: (tool, args, input, t_sizes, q_sizes)
    "argcount_maf_few": ("axtToMaf", ["{in}", "{t}", "{q}"]),
    "argcount_maf_many": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}", "extra"]),
    "argcount_sort_few": ("axtSort", ["{in}"]),
    "argcount_sort_many": ("axtSort", ["{in}", "{out}", "extra"]),
    "maf_short_head": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "short_head.axt"),
    "maf_bad_number": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "bad_number.axt"),
    "maf_unequal": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "unequal.axt"),
    "maf_truncated": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "truncated.axt"),
    "maf_no_tname": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "no_tname.axt"),
    "maf_no_qname": ("axtToMaf", ["-score", "{in}", "{t}", "{q}", "{out}"], "no_qname.axt"),
    "maf_long_prefix": ("axtToMaf", ["-qPrefix=" + "p" * 252, "{in}", "{t}", "{q}", "{out}"], "basic.axt"),
    "maf_one_word_sizes": ("axtToMaf", ["{in}", "{t}", "{q}", "{out}"], "basic.axt", "one_word.sizes"),
    "maf_split_unsorted": ("axtToMaf", ["-tSplit", "{in}", "{t}", "{q}", "{out}"], "split_unsorted.axt"),
    "sort_short_head": ("axtSort", ["{in}", "{out}"], "short_head.axt"),
    "sort_unequal": ("axtSort", ["-byScore", "{in}", "{out}"], "unequal.axt"),
    "sort_truncated": ("axtSort", ["{in}", "{out}"], "truncated.axt"),
}
INPUT_ERRORS = {"maf_short_head", "maf_bad_number", "maf_unequal", "maf_truncated", "maf_no_tname", "maf_no_qname",
                "maf_long_prefix", "maf_one_word_sizes", "maf_split_unsorted", "sort_short_head", "sort_unequal",
                "sort_truncated"}


def restated_maf(files, inp, ts, qs, opts):
    kw = {}
    for o in opts:
        if o.startswith("-tPrefix="):
            kw["t_prefix"] = o[9:].encode()
        elif o.startswith("-qPrefix="):
            kw["q_prefix"] = o[9:].encode()
        else:
            kw[{"-tSplit": "t_split", "-score": "rescore", "-scoreZero": "score_zero"}[o]] = True
    return AS.to_maf(files[inp].encode(), files[ts].encode(), files[qs].encode(), **kw)


def restated_sort(files, inp, opts):
    return AS.sort_axt(files[inp].encode(), by_query="-query" in opts, by_score="-byScore" in opts)


def main():
    maf, sort = ref_binary("axtToMaf"), ref_binary("axtSort")
    exe = {"axtToMaf": maf, "axtSort": sort}
    files = built_inputs()
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for name, text in files.items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(text.encode())
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (inp, ts, qs, opts) in MAF_CASES.items():
            out = os.path.join(tmp, name)
            r = subprocess.run([maf] + opts + [os.path.join(OUT, inp), os.path.join(OUT, ts), os.path.join(OUT, qs), out],
                               capture_output=True)
            assert r.returncode == 0, (name, r.stderr)
            want = restated_maf(files, inp, ts, qs, opts)
            if "-tSplit" in opts:
                got = {fn.encode(): AS.read_input(os.path.join(out, fn)) for fn in sorted(os.listdir(out))}
                assert got == want, name
                os.makedirs(os.path.join(OUT, name + ".out"))
                for fn, data in got.items():
                    with open(os.path.join(OUT, name + ".out", fn.decode()), "wb") as f:
                        f.write(data)
                output = {"dir": name + ".out", "files": sorted(fn.decode() for fn in got)}
            else:
                got = AS.read_input(out)
                assert got == want, (name, got, want)
                shutil.copy(out, os.path.join(OUT, name + ".maf"))
                output = name + ".maf"
            cases[name] = dict(tool="axtToMaf", options=opts, input=inp, t_sizes=ts, q_sizes=qs, output=output)
        for name, (inp, opts) in SORT_CASES.items():
            out = os.path.join(tmp, name)
            r = subprocess.run([sort] + opts + [os.path.join(OUT, inp), out], capture_output=True)
            assert r.returncode == 0, (name, r.stderr)
            got = AS.read_input(out)
            assert got == restated_sort(files, inp, opts), name
            shutil.copy(out, os.path.join(OUT, name + ".axt.sorted"))
            cases[name] = dict(tool="axtSort", options=opts, input=inp, output=name + ".axt.sorted")

        errors = {}
        for name, row in ERRORS.items():
            tool, args = row[0], row[1]
            inp = row[2] if len(row) > 2 else "basic.axt"
            ts = row[3] if len(row) > 3 else "t.sizes"
            qs = row[4] if len(row) > 4 else "q.sizes"
            out = os.path.join(tmp, "err_" + name)
            paths = {"{in}": os.path.join(OUT, inp), "{t}": os.path.join(OUT, ts), "{q}": os.path.join(OUT, qs),
                     "{out}": out}
            r = subprocess.run([exe[tool]] + [paths.get(a, a) for a in args], capture_output=True, text=True)
            assert r.returncode == 255, (name, r.returncode, r.stderr)
            first = r.stderr.split("\n")[0]
            for tag, p in paths.items():
                first = first.replace(p, tag)
            left = os.path.exists(out) and (os.path.isdir(out) or os.path.getsize(out) > 0)
            errors[name] = dict(tool=tool, args=args, input=inp, t_sizes=ts, q_sizes=qs, status=r.returncode,
                                stderr=first, left_output=bool(left))
            if name in INPUT_ERRORS:
                opts = [a for a in args if a.startswith("-")]
                try:
                    if tool == "axtToMaf":
                        restated_maf(files, inp, ts, qs, opts)
                    else:
                        restated_sort(files, inp, opts)
                except AS.BadInput:
                    pass
                else:
                    raise AssertionError("the restatement accepts " + name)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d error rows in %s" % (len(cases), len(errors), OUT))


if __name__ == "__main__":
    main()
