"""chainToPsl's kernel on the whole C5 chain set: k_psl_counts beside k_compose
(which shares its walk, gac_compose.hip) on the same uploaded set, for the
A/B and rocprofv3 runs of scripts/chaintopsl_profile.sh.  Prints one
"PROF_JSON {...}" line: the set, the traffic models' bytes (DESIGN.md 7.6,
7.9) and the calls' wall times (ROUNDS rounds of CALLS enqueued calls ending
in a device synchronise: per-call ms of every round, their median and minimum).

With GAC_LIB_VARIANT naming a library built before ABI minor 3 (an earlier
commit's sources, `make variant VSRC=...`) only k_compose is timed: that is
the A side of the shared-walk comparison.

    python scripts/chaintopsl_profile.py <C5 directory of bench.py>"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from genomealignmenttools_amd import _lib  # noqa: E402

PSL = ("gac_chain_psl_counts", "gac_chain_psl_counts_device")
has_psl = hasattr(ctypes.CDLL(_lib.LIB_PATH), PSL[0])
if not has_psl:
    assert os.environ.get("GAC_LIB_VARIANT"), "libgachain without the PSL entry points"
    for name in PSL:
        _lib._PROTOS.pop(name)
from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine  # noqa: E402

ROUNDS, CALLS = 7, 10
d = sys.argv[1]
ch = bench.load_chains_bin(d)
n = int(ch["n"])
bs = ch["bs"]
e = Engine(0)
e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"), soft_mask=True)  # (k_compose needs it; k_psl_counts does not read it)
names = lambda path: [ln.split()[0] for ln in open(path) if ln.strip()]
tmap = np.array([e.seq_index(GAC_T, x) for x in names(os.path.join(d, "t.sizes"))], np.int32)
qmap = np.array([e.seq_index(GAC_Q, x) for x in names(os.path.join(d, "q.sizes"))], np.int32)
cs = e.upload_chain_arrays(tmap[ch["tseq"]], qmap[ch["qseq"]], ch["strand"], ch["off"], ch["bt"],
                           ch["bq"], bs)
d_c = e.dev_alloc(48 * n + 8)
d_p = e.dev_alloc(32 * n + 8)
res = {"lib": os.environ.get("GAC_LIB_VARIANT", "tree"), "chains": n, "blocks": int(len(bs)),
       "bases": int(bs.sum(dtype=np.int64)), "rounds": ROUNDS, "calls_per_round": CALLS}
calls = [("composition", lambda: e.chain_composition_device(cs, d_c, d_c + 32 * n, d_c + 40 * n))]
if has_psl:
    calls.append(("psl_counts", lambda: e.chain_psl_counts_device(cs, d_p)))
for name, call in calls:
    for _ in range(3):
        call()
    e.synchronize()
    per = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        e.synchronize()
        per.append((time.perf_counter() - t0) / CALLS * 1e3)
    res[name + "_wall_ms"] = [round(x, 4) for x in per]
    res[name + "_median_ms"] = round(float(np.median(per)), 4)
    res[name + "_min_ms"] = round(min(per), 4)
# traffic models: per block its 16-B record + ceil(size/32) words x (8 + 8 B
# of planes + 4 B per soft-mask plane read); nmask words only for flagged
# blocks (not counted); 48 / 32 B of sums per chain
words = int(((bs.astype(np.int64) + 31) // 32).sum())
res["model_bytes_compose"] = int(16 * len(bs) + 24 * words + 48 * n)
res["model_bytes_psl"] = int(16 * len(bs) + 20 * words + 32 * n)
m = np.zeros(6 * n, np.int64)
e.d2h(m, d_c)
res["match_sum"] = int(m[:4 * n].sum())
res["rep_sum"] = int(m[4 * n:5 * n].sum())
res["total_sum"] = int(m[5 * n:].sum())
if has_psl:
    p = np.zeros((n, 4), np.int64)
    e.d2h(p, d_p)
    res["psl_sums"] = [int(x) for x in p.sum(0)]
    res["psl_median_over_compose_median"] = round(res["psl_counts_median_ms"] / res["composition_median_ms"], 4)
    # the two kernels count the same equal bases and the same aligned bases
    assert int(p[:, 0].sum() + p[:, 2].sum()) == res["match_sum"] and int(p.sum()) == res["total_sum"]
print("PROF_JSON " + json.dumps(res), flush=True)
cs.close()
e.close()
