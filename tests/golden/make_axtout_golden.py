#!/usr/bin/env python3
"""Generate tests/golden/axtout/ with the REFERENCE chainToAxt.

Run in the build container (needs the reference tree and oracle/ref.mk's kent
archive, `make ref`):
    python tests/golden/make_axtout_golden.py

The reference tool is compiled into a temporary directory from
kent/src/hg/mouseStuff/chainToAxt/chainToAxt.c with oracle/ref.mk's tool
flags (GAC_REF_CHAINTOAXT=path uses an existing binary instead).

Fixtures (data only, gzip with a zero time stamp):
  built.<tag>.gz     the reference's output on tests/golden/antirepeat/built
                     for the four option sets of OPTS
  synth11.default.gz, synth12.default.gz
                     its default output on the two synth sets
The generator asserts that the numpy restatement (tests/axtout_ref.py)
reproduces every file byte for byte, that -maxChain=50 changes nothing, and
that the default output on `built` holds every record category the tests
rely on.
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import antirepeat_ref as AR  # noqa: E402
import axtout_ref as AX  # noqa: E402
from genomealignmenttools_amd import chainfile  # noqa: E402

REF = os.environ.get("REF", "/root/reference")  # as oracle/ref.mk
OUT = os.path.join(HERE, "axtout")
OPTS = {
    "default": [],
    "opts": ["-maxGap=10", "-minId=90", "-minScore=3000"],
    "bed": ["-bed", "-minId=70"],
    "maxchain": ["-maxChain=50"],
}
KW = {
    "default": {},
    "opts": dict(max_gap=10, min_id=90, min_score=3000),
    "bed": dict(bed=True, min_id=70),
    "maxchain": dict(max_chain=50),
}
SETS = {"built": os.path.join(HERE, "antirepeat", "built"), "synth11": os.path.join(HERE, "synth11"),
        "synth12": os.path.join(HERE, "synth12")}


def ref_binary(tmp):
    if os.environ.get("GAC_REF_CHAINTOAXT"):
        return os.environ["GAC_REF_CHAINTOAXT"]
    lib = os.path.join(REPO, "oracle", "_ref", "jkweb.a")
    if not os.path.exists(lib):
        subprocess.run(["make", "-C", REPO, "-f", "oracle/ref.mk", "oracle/_ref/jkweb.a", "-j8"],
                       check=True)
    k = os.path.join(REF, "kent", "src")
    exe = os.path.join(tmp, "chainToAxt")
    subprocess.run(["gcc", "-O2", "-fcommon", "-D_FILE_OFFSET_BITS=64", "-D_LARGEFILE_SOURCE",
                    "-D_GNU_SOURCE", "-DMACHTYPE_x86_64", f"-I{k}/inc", f"-I{k}/hg/inc", "-w",
                    f"{k}/hg/mouseStuff/chainToAxt/chainToAxt.c", "-o", exe, lib,
                    "-lm", "-lz", "-lssl", "-lcrypto", "-pthread",
                    "-Wl,--warn-unresolved-symbols"], check=True, stderr=subprocess.DEVNULL)
    return exe


def categories(text):
    """record counts of a default axt output by what the rows hold"""
    lines = text.split(b"\n")
    cnt = dict(records=0, minus=0, has_N=0, has_n=0, t_dash=0, q_dash=0, negative=0)
    for i in range(0, len(lines) - 1, 4):
        h, t, q = lines[i].split(), lines[i + 1], lines[i + 2]
        cnt["records"] += 1
        cnt["minus"] += h[7] == b"-"
        cnt["has_N"] += b"N" in t or b"N" in q
        cnt["has_n"] += b"n" in t or b"n" in q
        cnt["t_dash"] += b"-" in t
        cnt["q_dash"] += b"-" in q
        cnt["negative"] += int(h[8]) < 0
    return cnt


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = ref_binary(tmp)
        for name, d in SETS.items():
            t2, q2, chain = (os.path.join(d, f) for f in ("t.2bit", "q.2bit", "in.chain"))
            tt, qt = AX.Text(AR.read_2bit(t2)), AX.Text(AR.read_2bit(q2))
            ca = chainfile.read_chains(chain)
            got = {}
            for tag, opts in OPTS.items():
                if name != "built" and tag != "default":
                    continue
                outp = os.path.join(tmp, "out")
                subprocess.run([exe, chain, t2, q2, outp] + opts, check=True)
                got[tag] = open(outp, "rb").read()
                mine = AX.tool_output(tt, qt, ca, **KW[tag])
                assert mine == got[tag], (name, tag, "the restatement differs from the reference")
                with open(os.path.join(OUT, f"{name}.{tag}.gz"), "wb") as f:
                    with gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
                        z.write(got[tag])
                print(f"{name} {tag}: {len(got[tag])} bytes")
            if name == "built":
                assert got["maxchain"] == got["default"], "-maxChain changed the output"
                assert got["opts"] != got["default"] and got["bed"]
                cnt = categories(got["default"])
                print(name, cnt)
                assert all(v > 0 for v in cnt.values()), cnt


if __name__ == "__main__":
    main()
