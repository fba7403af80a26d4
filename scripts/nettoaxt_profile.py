"""netToAxt's kernels on C5, for one rocprofv3 --kernel-trace --stats run
(scripts/nettoaxt_profile.sh): gac_axt_cut on one whole-chain range per chain
(the k_cut_* kernels), then k_axt_stat / k_axt_render in clip mode next to the
unclipped kernels on the SAME whole-chain pieces.  Prints one "PROF_JSON {...}"
line with the counts and the calls' wall times.

    python scripts/nettoaxt_profile.py <C5 directory of bench.py>"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine  # noqa: E402

d = sys.argv[1]
ch = bench.load_chains_bin(d)
n = int(ch["n"])
off, bt, bq, bs = ch["off"].astype(np.int64), ch["bt"], ch["bq"], ch["bs"]
e = Engine(0)
e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"), soft_mask=True)
names = lambda path: [ln.split()[0] for ln in open(path) if ln.strip()]
tmap = np.array([e.seq_index(GAC_T, x) for x in names(os.path.join(d, "t.sizes"))], np.int32)
qmap = np.array([e.seq_index(GAC_Q, x) for x in names(os.path.join(d, "q.sizes"))], np.int32)
tseq, qseq = tmap[ch["tseq"]], qmap[ch["qseq"]]
cs = e.upload_chain_arrays(tseq, qseq, ch["strand"], off, bt, bq, bs)
# one range per chain, equal to its span: the cut gives gac_axt_split's pieces
rg = np.stack([np.arange(n, dtype=np.int32), bt[off[:-1]], bt[off[1:] - 1] + bs[off[1:] - 1]], 1)
rg = np.ascontiguousarray(rg, np.int32)
res = {"chains": n, "blocks": int(len(bs)), "ranges": n}
for k in range(3):
    t0 = time.perf_counter()
    pieces, first = e.axt_cut(cs, rg, 100)
    res["axt_cut_wall_ms_%d" % k] = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
want = e.axt_split(tseq, qseq, ch["strand"], off, bt, bq, bs, 100)
res["split_host_ms"] = (time.perf_counter() - t0) * 1e3
res["cut_equals_split"] = bool(np.array_equal(pieces, want))
npc = len(pieces)
score, match, ali, sym = e.axt_measure(cs, pieces, clip=True)
text = int((2 * sym + 3).sum())
res.update(pieces=npc, text_bytes=text, score_sum=int(score.astype(np.int64).sum()))
d_w = e.dev_alloc(20 * npc + 8)
e.h2d(d_w, np.ascontiguousarray(pieces))
d_r = e.dev_alloc(32 * npc + 8)
d_t = e.dev_alloc(text + 16)
for clip in (False, True, False, True):  # alternating, so that drift shows in both
    tag = "clip" if clip else "plain"
    for name, call in (("measure", lambda: e.axt_measure_device(cs, d_w, npc, d_r, d_r + 8 * npc, d_r + 16 * npc,
                                                                d_r + 24 * npc, clip=clip)),
                       ("render", lambda: e.axt_render_device(cs, d_w, npc, 0, d_t, text, clip=clip))):
        call()
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            call()
        e.synchronize()
        res.setdefault("%s_%s_wall_ms" % (name, tag), []).append((time.perf_counter() - t0) / 5 * 1e3)
print("PROF_JSON " + json.dumps(res), flush=True)
cs.close()
e.close()
