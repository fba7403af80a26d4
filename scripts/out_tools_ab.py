#!/usr/bin/env python3
"""The text output of two more tools that write through gac_par_output, on the
whole C5 set (bench.py's files): bin/scoreChain and bin/chainToPsl of another
build (the parent commit's bin directory) against this tree's, alternating, 3
runs each with GAC_TIMING: wall time, the "write output" stage line and the
output path's own line; outputs sha-compared.
usage: out_tools_ab.py PARENT_BIN_DIR"""
import hashlib
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

PARENT = os.path.abspath(sys.argv[1])
sys.argv = [sys.argv[0]]
args = bench.parse()
d, _ = bench.c5_files(args)
p = lambda x: os.path.join(d, x)
builds = {"parent": PARENT, "new": os.path.dirname(bench.TOOL)}
tools = {"scoreChain": lambda o: [p("in.chain"), p("t.2bit"), p("q.2bit"), o, "-linearGap=loose"],
         "chainToPsl": lambda o: [p("in.chain"), p("t.sizes"), p("q.sizes"), p("t.2bit"), p("q.2bit"), o]}
def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()
for tool, mk in tools.items():
    shas = {}
    for rep in range(3):
        for tag, bd in builds.items():
            o = p(f"tools_ab.{tag}.out")
            if os.path.exists(o):
                os.remove(o)
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(bd, tool)] + mk(o) + ["-verbose=2"], capture_output=True, text=True,
                               env=dict(os.environ, GAC_TIMING="1"), timeout=200)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                print(tool, tag, "rc", r.returncode, r.stderr[-1500:], flush=True)
                sys.exit(1)
            print(f"{tool} {tag} rep {rep}: {dt*1e3:.0f} ms, {os.path.getsize(o)} bytes", flush=True)
            for ln in r.stderr.splitlines():
                if ln.startswith("[stage]") or "gac_par_output" in ln or "every run formatted" in ln:
                    print("   " + ln, flush=True)
            if rep == 0:
                shas[tag] = sha(o)
            os.remove(o)
    print(f"== {tool}: outputs identical {shas['parent'] == shas['new']} ({shas['new'][:16]})", flush=True)
