#!/usr/bin/env python3
"""Generate tests/golden/prenet/ with the REFERENCE chainPreNet.

Run in the build container (needs /root/reference and oracle/ref.mk's kent
archive, `make ref`):
    python tests/golden/make_prenet_golden.py

The reference tool is compiled into a temporary directory from
kent/src/hg/mouseStuff/chainPreNet/chainPreNet.c with oracle/ref.mk's tool
flags (GAC_REF_PRENET=path uses an existing binary instead).

Fixtures (data only):
  in.chain t.sizes q.sizes   a purpose-built set (written here) with chains
                         kept, dropped, dropped by a pad only, kept only
                         because an earlier chain was dropped, haplotype
                         queries, '-' queries at raw coordinates, one name on
                         both sides, equal scores, an id-less and an id-0
                         header, '#' lines at the start, in the middle and at
                         the end
  built.*.chain          the reference's output on it with the defaults, -pad=0,
                         -pad=5 and -inclHap
  synth11.chain synth12.chain c1.chain   its output on the chain files that
                         exist already (c1 with the packaged sizes)
  err_*                  inputs of the error table
  errors.json            per case: the arguments ("{in}" "{t}" "{q}": the
                         inputs' paths, "{out}": a scratch file), the
                         reference's exit status, the first line of its stderr
                         with the paths replaced by their tags, and whether
                         its output is empty

Before anything is kept the generator asserts that the restatement's keep set
(tests/prenet_ref.py) equals the reference's output on every case, and that
the built set has at least 3 chains in every category named above.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import prenet_ref as PR  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/ref.mk
OUT = PR.PRENET_DIR


def ref_binary(tmp):
    if os.environ.get("GAC_REF_PRENET"):
        return os.environ["GAC_REF_PRENET"]
    lib = os.path.join(REPO, "oracle", "_ref", "jkweb.a")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", REPO, "-f", "oracle/ref.mk", "oracle/_ref/jkweb.a", "-j8"],
                       check=True)
    k = os.path.join(REF, "kent", "src")
    exe = os.path.join(tmp, "chainPreNet")
    subprocess.run(["gcc", "-O2", "-fcommon", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE",
                    "-D_GNU_SOURCE", "-DMACHTYPE_x86_64", f"-I{k}/inc", f"-I{k}/hg/inc", "-w",
                    f"{k}/hg/mouseStuff/chainPreNet/chainPreNet.c", "-o", exe, lib,
                    "-lm", "-lz", "-lssl", "-lcrypto", "-pthread",
                    "-Wl,--warn-unresolved-symbols"], check=True, stderr=subprocess.DEVNULL)
    return exe


# ------------------------------------------------------------ the built set
T_SIZES = {"chrT1": 5000, "chrT2": 3000, "chrS": 2000}
Q_SIZES = {"chrQ1": 4000, "chrQ2": 2500, "chrS": 1500, "chrQ6_hap1": 1000, "chr9_alt2": 800}


class Built:
    def __init__(self):
        self.chains = []  # dicts in file order
        self.score = 900000

    def add(self, tag, blocks, tname="chrT1", qname="chrQ1", minus=False, cid="auto", same_score=False,
            meta=()):
        """blocks: (tStart, qStart, size), the query start as the file has it"""
        if not same_score:
            self.score -= 1000
        if cid == "auto":
            cid = 100 + len(self.chains)
        self.chains.append(dict(tag=tag, blocks=blocks, tname=tname, qname=qname, minus=minus, id=cid,
                                score=self.score, meta=list(meta)))

    def text(self):
        out = ["##matrix=16 91 -114 -31 -123 -114 100 -125 -31 -31 -125 100 -114 -123 -31 -114 91\n",
               "# a note before the first chain\n"]
        for c in self.chains:
            out += [m + "\n" for m in c["meta"]]
            b = c["blocks"]
            head = "chain %d %s %d + %d %d %s %d %s %d %d" % (
                c["score"], c["tname"], T_SIZES[c["tname"]], b[0][0], b[-1][0] + b[-1][2], c["qname"],
                Q_SIZES[c["qname"]], "-" if c["minus"] else "+", b[0][1], b[-1][1] + b[-1][2])
            if c["id"] is not None:
                head += " %d" % c["id"]
            out.append(head + "\n")
            for k in range(len(b) - 1):
                out.append("%d\t%d\t%d\n" % (b[k][2], b[k + 1][0] - b[k][0] - b[k][2],
                                             b[k + 1][1] - b[k][1] - b[k][2]))
            out.append("%d\n\n" % b[-1][2])
        out.append("# a note after the last chain\n")
        return "".join(out)


def build_set():
    B = Built()
    # clusters on chrT1 / chrQ1, 100 bases apart: a base chain A of two blocks
    # and its followers
    for k in range(4):
        t, q = 100 + 200 * k, 150 + 200 * k
        minus = k % 2 == 1
        B.add("kept", [(t, q, 20), (t + 25, q + 30, 20)], minus=minus,
              meta=["# between chains %d" % k] if k else ())
        B.add("dropped", [(t + 3, q + 3, 10)], minus=minus)               # inside A
        B.add("pad_drop", [(t + 20, q + 20, 1)], minus=minus)             # in A's pad only
        B.add("fixpoint", [(t + 21, q + 21, 1)], minus=minus)             # in the pad of the one before
        B.add("pad_drop", [(t + 24, q + 29, 1), (t + 45, q + 50, 1)], minus=not minus)
    # '-' query at raw coordinates: inside a '+' chain's raw query range
    for k in range(3):
        t, q = 1500 + 100 * k, 1700 + 100 * k
        B.add("kept", [(t, q, 30)])
        B.add("dropped", [(t + 5, q + 5, 20)], minus=True)  # (flipped it would lie elsewhere)
    # equal scores
    B.add("kept", [(2500, 2600, 15)])
    B.add("dropped", [(2502, 2602, 5)], same_score=True)
    B.add("kept", [(2530, 2630, 15)], same_score=True)
    # one name on both sides: two maps
    B.add("kept", [(0, 100, 50)], tname="chrS", qname="chrS")
    B.add("kept", [(100, 0, 50)], tname="chrS", qname="chrS")
    B.add("dropped", [(10, 110, 20)], tname="chrS", qname="chrS")
    # haplotype queries: skipped, and what they would cover with -inclHap
    for k in range(3):
        t = 3000 + 100 * k
        B.add("hap", [(t, 50 + 100 * k, 40)], qname="chrQ6_hap1")
        B.add("hap", [(t + 5, 55 + 100 * k, 10)], qname="chrQ6_hap1", minus=True)
        B.add("kept", [(t + 10, 160 + 200 * k, 5)])  # target under the hap chain, query under cluster k
    B.add("hap", [(3500, 10, 40)], qname="chr9_alt2", meta=["# before an alt chain"])
    # other sequences, ends of sequences
    B.add("kept", [(0, 0, 10), (2990, 2490, 10)], tname="chrT2", qname="chrQ2")
    B.add("dropped", [(1, 1, 9)], tname="chrT2", qname="chrQ2")
    B.add("pad_drop", [(10, 10, 1)], tname="chrT2", qname="chrQ2")
    B.add("pad_drop", [(2989, 2489, 1)], tname="chrT2", qname="chrQ2", minus=True)
    B.add("kept", [(4000, 3000, 12)], cid=None)   # no id field
    B.add("kept", [(4100, 3100, 12)], cid=0)      # id 0: chainWrite numbers it
    B.add("dropped", [(4101, 3101, 3)], cid=None)
    return B


def categories(B, text):
    """the built chains by what decides them, from the restatement"""
    k1 = PR.file_keep(text, T_SIZES, Q_SIZES, 1, False)
    k0 = PR.file_keep(text, T_SIZES, Q_SIZES, 0, False)
    # what "every earlier chain covers" would keep: the chains open under all counted chains
    a = PR.chain_arrays(PR.parse_chain_text(text), T_SIZES, Q_SIZES, False)
    naive = np.zeros(len(k1), np.uint8)
    for i in range(len(k1)):
        if a[1][i] >= 0:
            naive[i] = _open_under_all(a, i)
    cnt = dict(kept=0, dropped=0, pad_drop=0, fixpoint=0, hap=0, minus=0)
    for i, c in enumerate(B.chains):
        skipped = PR.haplotype(c["qname"])
        cnt["hap"] += skipped
        cnt["minus"] += c["minus"]
        if skipped:
            assert c["tag"] == "hap" and not k1[i], i
            continue
        cnt["kept"] += int(k1[i])
        cnt["dropped"] += int(not k1[i])
        cnt["pad_drop"] += int(not k1[i] and k0[i])
        cnt["fixpoint"] += int(k1[i] and not naive[i])
        want = {"kept": k1[i] and naive[i], "dropped": not k1[i] and not k0[i],
                "pad_drop": not k1[i] and k0[i], "fixpoint": k1[i] and not naive[i]}[c["tag"]]
        assert want, (i, c["tag"], int(k1[i]), int(k0[i]), int(naive[i]))
    return cnt


def _open_under_all(a, i, pad=1):
    """is chain i open when every counted chain before it has set its padded blocks"""
    off, ts, qs, bt, bq, bz, tz, qz = a
    tb, qb = np.zeros(int(tz[ts[i]]), bool), np.zeros(int(qz[qs[i]]), bool)
    for j in range(i):
        for b in range(off[j], off[j + 1]):
            if ts[j] == ts[i]:
                tb[max(bt[b] - pad, 0):min(bt[b] + bz[b] + pad, len(tb))] = True
            if qs[j] == qs[i]:
                qb[max(bq[b] - pad, 0):min(bq[b] + bz[b] + pad, len(qb))] = True
    return int(any(not qb[bq[b]:bq[b] + bz[b]].all() or not tb[bt[b]:bt[b] + bz[b]].all()
                   for b in range(off[i], off[i + 1])))


# name -> (arguments, {tag: file under prenet/})
ERRORS = {
    "unsorted": (["{in}", "{t}", "{q}", "{out}"], "err_unsorted.chain", "t.sizes", "q.sizes"),
    "no_query": (["{in}", "{t}", "{q}", "{out}"], "err_noquery.chain", "t.sizes", "q.sizes"),
    "no_target": (["{in}", "{t}", "{q}", "{out}"], "err_notarget.chain", "t.sizes", "q.sizes"),
    "name_before_order": (["{in}", "{t}", "{q}", "{out}"], "err_both.chain", "t.sizes", "q.sizes"),
    "sizes_words": (["{in}", "{t}", "{q}", "{out}"], "in.chain", "err_words.sizes", "q.sizes"),
    "sizes_number": (["{in}", "{t}", "{q}", "{out}"], "in.chain", "t.sizes", "err_number.sizes"),
    "argcount": (["{in}", "{t}", "{q}"], "in.chain", "t.sizes", "q.sizes"),
    "argcount_pad": (["-pad=7", "{in}"], "in.chain", "t.sizes", "q.sizes"),
    "option": (["-foo", "{in}", "{t}", "{q}", "{out}"], "in.chain", "t.sizes", "q.sizes"),
    "empty": (["{in}", "{t}", "{q}", "{out}"], "err_empty.chain", "t.sizes", "q.sizes"),
}

ERR_INPUTS = {
    "err_unsorted.chain": "# out of order\nchain 5000 chrT1 5000 + 10 20 chrQ1 4000 + 10 20 1\n10\n\n"
                          "chain 4000 chrT1 5000 + 30 45 chrQ1 4000 + 30 45 2\n5\t5\t5\n5\n\n"
                          "\nchain 4500 chrT1 5000 + 50 60 chrQ1 4000 + 50 60 3\n10\n\n",
    "err_noquery.chain": "chain 5000 chrT1 5000 + 10 20 chrQ1 4000 + 10 20 1\n10\n\n"
                         "chain 4000 chrT1 5000 + 30 40 chrQ7 4000 + 30 40 2\n10\n\n",
    "err_notarget.chain": "chain 5000 chrT9 5000 + 10 20 chrQ1 4000 + 10 20 1\n10\n\n",
    "err_both.chain": "chain 5000 chrT1 5000 + 10 20 chrQ1 4000 + 10 20 1\n10\n\n"
                      "chain 4000 chrT9 5000 + 30 40 chrQ1 4000 + 30 40 2\n10\n\n"
                      "chain 4500 chrT1 5000 + 50 60 chrQ1 4000 + 50 60 3\n10\n\n",
    "err_words.sizes": "chrT1\t5000\nchrT2\n",
    "err_number.sizes": "chrQ1\tmany\n",
    "err_empty.chain": "",
}


def run_case(exe, case, out):
    src, ts, qs, opts, _want = PR.CASES[case]
    r = subprocess.run([exe] + opts + [src, ts, qs, out], capture_output=True)
    assert r.returncode == 0, (case, r.stderr)
    got = open(out, "rb").read()
    text = open(src).read()
    pad, hap = PR.case_options(opts)
    mine = PR.file_keep(text, PR.read_sizes(ts), PR.read_sizes(qs), pad, hap)
    theirs = PR.kept_mask(text, got.decode())
    assert np.array_equal(mine, theirs), (case, np.flatnonzero(mine != theirs))
    print(f"{case}: reference kept {int(theirs.sum())} of {len(theirs)}")
    return got


def main():
    os.makedirs(OUT, exist_ok=True)
    B = build_set()
    text = B.text()
    cnt = categories(B, text)
    print("built:", cnt)
    assert all(v >= 3 for v in cnt.values()), cnt
    assert text.count("\n#") >= 3 and text.startswith("#") and text.rstrip("\n").split("\n")[-1][0] == "#"
    with open(os.path.join(OUT, "in.chain"), "w") as f:
        f.write(text)
    for name, sizes in (("t.sizes", T_SIZES), ("q.sizes", Q_SIZES)):
        with open(os.path.join(OUT, name), "w") as f:
            f.write("".join(f"{k}\t{v}\n" for k, v in sizes.items()))
    for name, body in ERR_INPUTS.items():
        with open(os.path.join(OUT, name), "w") as f:
            f.write(body)
    with tempfile.TemporaryDirectory() as tmp:
        exe = ref_binary(tmp)
        out = os.path.join(tmp, "out.chain")
        made = {case: run_case(exe, case, out) for case in PR.CASES}
        errors = {}
        for name, (args, src, ts, qs) in ERRORS.items():
            paths = {"{in}": os.path.join(OUT, src), "{t}": os.path.join(OUT, ts),
                     "{q}": os.path.join(OUT, qs), "{out}": out}
            if os.path.exists(out):
                os.remove(out)
            r = subprocess.run([exe] + [paths.get(a, a) for a in args], capture_output=True)
            first = r.stderr.decode().split("\n")[0] if r.returncode else ""
            for tag, p in paths.items():
                first = first.replace(p, tag)
            empty = not os.path.exists(out) or os.path.getsize(out) == 0
            errors[name] = dict(args=args, input=src, t_sizes=ts, q_sizes=qs, status=r.returncode,
                                stderr=first, output_empty=empty)
            print(name, r.returncode, first)
    for case, got in made.items():
        with open(PR.CASES[case][4], "wb") as f:
            f.write(got)
    with open(os.path.join(OUT, "errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
