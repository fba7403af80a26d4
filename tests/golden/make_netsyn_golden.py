#!/usr/bin/env python3
"""Generate tests/golden/netsyn/ with the REFERENCE netSyntenic.

Run in the build container (needs oracle/_ref/netSyntenic, `make ref`):
    python tests/golden/make_netsyn_golden.py

The inputs are hand-written and live beside the outputs:
  edge.net     stale qOver / qFar / qDup / type on a top fill, an unknown
               integer field, a gap with tR and qDup, qSize 0 on a gap and on a
               fill, a fill under a gap of another query sequence, a far
               (qFar > 0) and a touching (qOver 0 qFar 0) fill, scores 1234.6
               and 0, a '#' line between nets, two nets on one query sequence
  indent.net   3-space steps, an indented '#' line, a blank line, a line
               indented between two levels (it replaces a child list)
  empty.net, err_*.net   the error table's inputs

Fixtures written (data only):
  edge.syn.net, indent.syn.net   the reference's outputs
  errors.json  per case: the arguments ("{in}": the input's path, "{out}": a
               scratch file), the reference's exit status, the first line of
               its stderr with the input's path replaced by "{in}", and
               whether its output is empty

Before anything is written the generator asserts that the restatement
(tests/netsyn_ref.py) reproduces the reference byte for byte on edge.net,
indent.net and the three nets of tests/golden/netfilter/, and raises the
reference's message for every error input.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import netsyn_ref as NS  # noqa: E402

REF_BIN = os.path.join(REPO, "oracle", "_ref", "netSyntenic")

# name -> (arguments, input file or None)
ERRORS = {
    "nofills": (["{in}", "{out}"], "err_nofills.net"),
    "notnet": (["{in}", "{out}"], "err_notnet.net"),
    "nonnum": (["{in}", "{out}"], "err_nonnum.net"),
    "nonnum_opt": (["{in}", "{out}"], "err_nonnum_opt.net"),
    "shortnet": (["{in}", "{out}"], "err_shortnet.net"),
    "argcount": (["{out}"], None),
    "option": (["-foo", "{in}", "{out}"], "empty.net"),
    "empty": (["{in}", "{out}"], "empty.net"),
}


def run_ref(args):
    return subprocess.run([REF_BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def main():
    assert os.path.exists(REF_BIN), "make ref first"
    made = {}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.net")
        for name, (src, _want) in NS.CASES.items():
            r = run_ref([src, out])
            assert r.returncode == 0, (name, r.stderr)
            got = open(out, "rb").read()
            assert NS.net_syntenic(open(src).read(), src).encode() == got, name
            made[name] = got
        for name in ("synth11", "cleaner", "big"):  # the fixtures that exist already
            assert made[name] == open(NS.CASES[name][1], "rb").read(), name
        errors = {}
        for name, (args, src) in ERRORS.items():
            path = os.path.join(NS.NETSYN_DIR, src) if src else None
            if os.path.exists(out):
                os.remove(out)
            r = run_ref([a.replace("{in}", path or "").replace("{out}", out) for a in args])
            # (a run that succeeds prints only its "memory usage" line, which the tool drops)
            first = r.stderr.decode().split("\n")[0] if r.returncode else ""
            if path:
                first = first.replace(path, "{in}")
            status = r.returncode
            empty = not os.path.exists(out) or os.path.getsize(out) == 0
            errors[name] = dict(args=args, input=src, status=status, stderr=first, output_empty=empty)
            print(name, status, first)
            if src and args[0] == "{in}":  # the restatement raises the same message
                try:
                    text = NS.net_syntenic(open(path).read(), "{in}")
                    assert status == 0 and text == "", name
                except NS.NetError as e:
                    assert status == 255 and str(e) == first, (name, str(e), first)
    for name in ("edge", "indent"):
        with open(NS.CASES[name][1], "wb") as f:
            f.write(made[name])
    with open(os.path.join(NS.NETSYN_DIR, "errors.json"), "w") as f:
        json.dump(errors, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
