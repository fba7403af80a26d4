"""chainAntiRepeat's kernel on C5 (the chains with score < 200000): k_compose
and k_tile<true, true> (whole chains, local score) on the same uploaded set,
for one rocprofv3 --kernel-trace --stats run (scripts/antirepeat_profile.sh).
Prints one "PROF_JSON {...}" line: the set, the traffic models' bytes
 and the calls' wall times.

    python scripts/antirepeat_profile.py <C5 directory of bench.py>"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine, GapCosts  # noqa: E402

d = sys.argv[1]
ch = bench.load_chains_bin(d)
keep = ch["score"] < 200000
nbk = np.diff(ch["off"])
bsel = np.repeat(keep, nbk)
off = np.concatenate([[0], np.cumsum(nbk[keep])]).astype(np.int64)
bt, bq, bs = ch["bt"][bsel], ch["bq"][bsel], ch["bs"][bsel]
n = int(keep.sum())
e = Engine(0)
e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"), soft_mask=True)
e.set_scoring(bench.BLASTZ, GapCosts("loose"))
names = lambda path: [ln.split()[0] for ln in open(path) if ln.strip()]
tmap = np.array([e.seq_index(GAC_T, x) for x in names(os.path.join(d, "t.sizes"))], np.int32)
qmap = np.array([e.seq_index(GAC_Q, x) for x in names(os.path.join(d, "q.sizes"))], np.int32)
cs = e.upload_chain_arrays(tmap[ch["tseq"][keep]], qmap[ch["qseq"][keep]], ch["strand"][keep], off,
                           bt, bq, bs)
d_g, d_l, d_a = e.dev_alloc(8 * n + 8), e.dev_alloc(8 * n + 8), e.dev_alloc(4 * n + 8)
d_c = e.dev_alloc(48 * n + 8)
res = {"chains": n, "of": int(ch["n"]), "blocks": int(len(bs)), "bases": int(bs.sum(dtype=np.int64))}
for name, call in (("score_chains_local", lambda: e.score_chains_device(cs, d_g, d_a, d_l, True)),
                   ("composition", lambda: e.chain_composition_device(cs, d_c, d_c + 32 * n,
                                                                      d_c + 40 * n))):
    for _ in range(2):
        call()
    e.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        call()
    e.synchronize()
    res[name + "_wall_ms"] = (time.perf_counter() - t0) / 5 * 1e3
# traffic model (DESIGN): per block its 16-B record + ceil(size/32) words x
# (8 + 8 + 4 + 4) B; nmask words only for flagged blocks (not counted); 48 B per chain
words = ((bs.astype(np.int64) + 31) // 32).sum()
res["model_bytes_compose"] = int(16 * len(bs) + 24 * words + 48 * n)
res["model_bytes_tile"] = int(12 * len(bs) + 16 * words + 20 * n)
m = np.zeros(4 * n, np.int64)
e.d2h(m, d_c)
res["match_sum"] = int(m.sum())
print("PROF_JSON " + json.dumps(res), flush=True)
cs.close()
e.close()
