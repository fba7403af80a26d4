"""chainToAxt's kernels on C5 (all chains, -maxGap=100): k_axt_stat and
k_axt_render beside k_compose on the same uploaded set, for one rocprofv3
--kernel-trace --stats run (scripts/chaintoaxt_profile.sh).  Prints one
"PROF_JSON {...}" line: the set, the pieces, the text bytes written, the
traffic model's bytes and the calls' wall times.

    python scripts/chaintoaxt_profile.py <C5 directory of bench.py>"""
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
t0 = time.perf_counter()
pieces = e.axt_split(tseq, qseq, ch["strand"], off, bt, bq, bs, 100)
split_ms = (time.perf_counter() - t0) * 1e3
npc = len(pieces)
score, match, ali, sym = e.axt_measure(cs, pieces)
text = int((2 * sym + 3).sum())
res = {"chains": n, "blocks": int(len(bs)), "bases": int(bs.sum(dtype=np.int64)), "pieces": npc,
       "columns": int(sym.sum()), "text_bytes": text, "split_host_ms": split_ms}
d_w = e.dev_alloc(20 * npc + 8)
e.h2d(d_w, np.ascontiguousarray(pieces))
d_r = e.dev_alloc(32 * npc + 8)
d_t = e.dev_alloc(text + 16)
d_c = e.dev_alloc(48 * n + 8)
for name, call in (("composition", lambda: e.chain_composition_device(cs, d_c, d_c + 32 * n, d_c + 40 * n)),
                   ("axt_measure", lambda: e.axt_measure_device(cs, d_w, npc, d_r, d_r + 8 * npc,
                                                                d_r + 16 * npc, d_r + 24 * npc)),
                   ("axt_render", lambda: e.axt_render_device(cs, d_w, npc, 0, d_t, text))):
    for _ in range(2):
        call()
    e.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        call()
    e.synchronize()
    res[name + "_wall_ms"] = (time.perf_counter() - t0) / 5 * 1e3
# traffic model: k_compose as scripts/antirepeat_profile.py; k_axt_render reads, per
# 16-byte window of a row, two plane words (16 B) and two words of each mask
# (16 B), per block its record and scan entries, and writes the text
words = ((bs.astype(np.int64) + 31) // 32).sum()
res["model_bytes_compose"] = int(16 * len(bs) + 24 * words + 48 * n)
res["model_bytes_render_read"] = int(32 * (text // 16) + 40 * len(bs))
res["score_sum"] = int(score.astype(np.int64).sum())
res["match_sum"] = int(match.sum())
print("PROF_JSON " + json.dumps(res), flush=True)
cs.close()
e.close()
