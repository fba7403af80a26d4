#!/usr/bin/env python3
"""The netting stage of the headline tool (bin/chainNet -rescore on C5,
bench.py's files) under variants, alternating, every run with GAC_TIMING:
per rep the [stage] lines (netting: wall and CPU) and the [gac_net_build]
laps (set-up, addChainT/Q, finishNet skeletons / subtrees / index, the arena
MB) and the stages after it (fill list, write nets, free), then the medians
and, against the first variant, the reps in which the netting stage's wall and
CPU were both lower and, lap by lap, the pairs in which each was lower.  scripts/c5_ab.py times the whole step; this
one attributes it.
usage: net_laps.py REPS tag:ENV=v,@TOOL=path ...   (as c5_ab.py)"""
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

LAPS = [("netting", r"\[stage\] netting\s+([\d.]+) s"), ("netting cpu", r"\[stage\] netting.*\(cpu ([\d.]+) s"),
        ("set-up", r"\] set-up ([\d.]+) s"), ("addChainT/Q", r"\] addChainT/Q ([\d.]+) s"),
        ("skeletons", r"finishNet skeletons ([\d.]+) s"), ("subtrees", r"subtrees ([\d.]+) s"),
        ("index", r"index ([\d.]+) s"), ("finishNet", r"\] finishNet ([\d.]+) s \("),
        ("fill list", r"\[stage\] fill list\s+([\d.]+) s"), ("write nets", r"\[stage\] write nets\s+([\d.]+) s"),
        ("free", r"\[stage\] free nets and chains\s+([\d.]+) s"),
        ("arenas MB", r"fill/gap arenas ([\d.]+) MB")]


def main():
    reps = int(sys.argv[1])
    variants = []
    for sp in sys.argv[2:]:
        tag, _, kv = sp.partition(":")
        env = dict(os.environ, GAC_TIMING="1")
        tool = None
        for x in filter(None, kv.split(",")):
            k, _, v = x.partition("=")
            if k == "@TOOL":
                tool = v
            else:
                env[k] = v
        variants.append((tag, env, tool))
    sys.argv = [sys.argv[0]]
    args = bench.parse()
    d, _ = bench.c5_files(args)
    out = os.path.join(d, "laps")
    outs = [out + ".t.net", out + ".q.net"]
    base = bench.tool_cmd(d, out, 1, 0)
    bench.run_tool(base, outs)  # warm the page cache
    got = {tag: {k: [] for k, _ in LAPS} for tag, _, _ in variants}
    for rep in range(reps):
        for tag, env, tool in variants:
            cmd = ([tool] + base[1:] if tool else base) + ["-verbose=2"]
            r = bench.run_tool(cmd, outs, env=env)
            for line in r.stderr.splitlines():
                if line.startswith("[gac_net_build] side "):
                    continue
                if line.startswith(("[stage]", "[gac_net_build]")):
                    print(f"{tag} rep {rep}: {line}", flush=True)
                for k, rx in LAPS:
                    m = re.search(rx, line)
                    if m:
                        got[tag][k].append(float(m.group(1)))
    first = variants[0][0]
    for tag, _, _ in variants:
        for k, _ in LAPS:
            v = got[tag][k]
            if v:
                print(f"== {tag}: {k} median {statistics.median(v):.3f} s, all "
                      f"{' '.join(f'{x:.3f}' for x in v)}", flush=True)
        if tag != first and got[first]["netting"]:
            a, b = got[first], got[tag]
            low = [r for r in range(reps) if b["netting"][r] < a["netting"][r] and
                   b["netting cpu"][r] < a["netting cpu"][r]]
            print(f"== {tag}: netting stage and its CPU below {first}'s in {len(low)} of {reps} "
                  f"pairs (reps {' '.join(map(str, low))})", flush=True)
            for k, _ in LAPS:  # each lap on its own: the pairs it was lower in
                if len(a[k]) == reps and len(b[k]) == reps:
                    print(f"== {tag}: {k} below {first}'s in "
                          f"{sum(b[k][r] < a[k][r] for r in range(reps))} of {reps} pairs", flush=True)


if __name__ == "__main__":
    main()
