#!/usr/bin/env python3
"""Generate tests/golden/psl/ with the REFERENCE chainToPsl and chainToPslBasic.

Run in the build container (needs /root/reference and oracle/ref.mk's kent
archive, `make ref`):
    python tests/golden/make_psl_golden.py

The reference tools are compiled into a temporary directory from
kent/src/hg/mouseStuff/chainToPsl/chainToPsl.c and chainToPslBasic/
chainToPslBasic.c with oracle/ref.mk's tool flags, and run on the existing sets
antirepeat/built, synth11 and synth12 and on the hand-written psl/edge.chain
(over antirepeat/built's genomes).

Fixtures (data only), per set:
  <set>.psl          chainToPsl's output (tSizes / qSizes given as paths that
                     do not exist: the reference never opens them)
  <set>.basic.psl    chainToPslBasic's output
  <set>.counts.npz   per chain: counts [n, 4] (match, misMatch, repMatch,
                     nCount: the first four columns of <set>.psl), inserts
                     [n, 4], and `classes`, the set's bases by class
                     (pslout_ref.CLASSES)
A file larger than pslout_ref.GZ_ABOVE is stored gzipped.

Before anything is written the generator asserts that the numpy restatement
(tests/pslout_ref.py) reproduces every output byte for byte, that every class
of bases is present in built, synth11 and synth12, and that each deliberately
wrong restatement (pslout_ref.WRONG) changes at least one output.
"""
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import pslout_ref as PS  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/ref.mk


def ref_binary(tmp, tool):
    lib = os.path.join(REPO, "oracle", "_ref", "jkweb.a")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", REPO, "-f", "oracle/ref.mk", "oracle/_ref/jkweb.a", "-j8"],
                       check=True)
    k = os.path.join(REF, "kent", "src")
    exe = os.path.join(tmp, tool)
    subprocess.run(["gcc", "-O2", "-fcommon", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE",
                    "-D_GNU_SOURCE", "-DMACHTYPE_x86_64", f"-I{k}/inc", f"-I{k}/hg/inc", "-w",
                    f"{k}/hg/mouseStuff/{tool}/{tool}.c", "-o", exe, lib,
                    "-lm", "-lz", "-lssl", "-lcrypto", "-pthread",
                    "-Wl,--warn-unresolved-symbols"], check=True, stderr=subprocess.DEVNULL)
    return exe


def store(name, data):
    p = os.path.join(PS.PSL_DIR, name)
    for old in (p, p + ".gz"):
        if os.path.exists(old):
            os.remove(old)
    if len(data) > PS.GZ_ABOVE:
        with open(p + ".gz", "wb") as f:  # (no file name or time in the header: reproducible)
            with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as g:
                g.write(data)
    else:
        with open(p, "wb") as f:
            f.write(data)


def main():
    os.makedirs(PS.PSL_DIR, exist_ok=True)
    made = {}
    with tempfile.TemporaryDirectory() as tmp:
        psl, basic = ref_binary(tmp, "chainToPsl"), ref_binary(tmp, "chainToPslBasic")
        for name, (d, chain) in PS.SETS.items():
            out, outb = os.path.join(tmp, "o.psl"), os.path.join(tmp, "b.psl")
            subprocess.run([psl, chain, os.path.join(tmp, "no.t.sizes"), os.path.join(tmp, "no.q.sizes"),
                            os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"), out], check=True,
                           stderr=subprocess.DEVNULL)
            subprocess.run([basic, chain, outb], check=True)
            made[name] = (open(out, "rb").read(), open(outb, "rb").read())
    data = {name: PS.load(name) for name in PS.SETS}
    save = {}
    for name, (tg, qg, ca) in data.items():
        cnt, ins = PS.counts(tg, qg, ca), PS.inserts(ca)
        assert PS.psl_text(ca, cnt, ins) == made[name][0], name
        assert PS.basic_output(ca) == made[name][1], name
        assert len(made[name][0].splitlines()) == ca.n
        cls = PS.classes(tg, qg, ca)
        print(name, ca.n, "chains", cls)
        if name != "edge":
            assert all(v > 0 for v in cls.values()), (name, cls)
        save[name] = dict(counts=cnt, inserts=ins, classes=np.array([cls[k] for k in PS.CLASSES], np.int64))
    for w in PS.WRONG:
        changed = [name for name, (tg, qg, ca) in data.items()
                   if PS.tool_output(tg, qg, ca, wrong={w}) != made[name][0]]
        print("wrong", w, "changes", changed)
        assert changed, w
    for name in PS.SETS:
        store(f"{name}.psl", made[name][0])
        store(f"{name}.basic.psl", made[name][1])
        np.savez_compressed(os.path.join(PS.PSL_DIR, f"{name}.counts.npz"), **save[name])


if __name__ == "__main__":
    main()
