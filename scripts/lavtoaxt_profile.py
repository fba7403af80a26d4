"""lavToAxt on the pieces of a gac_synth chain set (scripts/lavtoaxt_profile.sh).

    python scripts/lavtoaxt_profile.py lav <C5 directory> <out.lav>
        the pieces gac_axt_split (-maxGap=100) makes of the set's chains as a
        .lav, one 'a' stanza per piece and an 's' / 'h' pair wherever the
        sequences or the strand change: no outside data is needed
    python scripts/lavtoaxt_profile.py kernels <C5 directory>
        k_axt_pairs beside k_axt_stat on the same pieces in one process (for
        one rocprofv3 --kernel-trace --stats run); prints "PROF_JSON {...}"
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine  # noqa: E402


def load(d):
    ch = bench.load_chains_bin(d)
    rows = lambda path: [ln.split() for ln in open(path) if ln.strip()]  # noqa: E731
    return ch, rows(os.path.join(d, "t.sizes")), rows(os.path.join(d, "q.sizes"))


def write_lav(d, out):
    ch, ts, qs = load(d)
    off, bt, bq, bs = ch["off"].astype(np.int64), ch["bt"], ch["bq"], ch["bs"]
    pieces = Engine.axt_split(ch["tseq"], ch["qseq"], ch["strand"], off, bt, bq, bs, 100)
    last = None
    with open(out, "w") as f:
        f.write("#:lav\n")
        for c, _, _, first, nb in pieces.tolist():
            key = (int(ch["tseq"][c]), int(ch["qseq"][c]), int(ch["strand"][c]))
            if key != last:
                (tn, tz), (qn, qz), rc = ts[key[0]][:2], qs[key[1]][:2], key[2]
                f.write('s {\n  "%s" 1 %s 0 1\n  "%s" 1 %s %d 1\n}\nh {\n  ">%s"\n  ">%s%s"\n}\n' % (
                    tn, tz, qn, qz, rc, tn, qn, " (reverse complement)" if rc else ""))
                last = key
            b0 = int(off[c]) + first
            t, q, z = bt[b0:b0 + nb].tolist(), bq[b0:b0 + nb].tolist(), bs[b0:b0 + nb].tolist()
            f.write("a {\n  s %d\n" % (3000 + c % 1000) +
                    "".join("  l %d %d %d %d 90\n" % (t[i] + 1, q[i] + 1, t[i] + z[i], q[i] + z[i])
                            for i in range(nb)) + "}\n")
    print("%d pieces, %d blocks, %d bytes in %s" % (len(pieces), int(pieces[:, 4].sum()),
                                                    os.path.getsize(out), out))


def kernels(d):
    ch, ts, qs = load(d)
    off, bt, bq, bs = ch["off"].astype(np.int64), ch["bt"], ch["bq"], ch["bs"]
    e = Engine(0)
    e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
    e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"), soft_mask=True)
    tmap = np.array([e.seq_index(GAC_T, r[0]) for r in ts], np.int32)
    qmap = np.array([e.seq_index(GAC_Q, r[0]) for r in qs], np.int32)
    tseq, qseq = tmap[ch["tseq"]], qmap[ch["qseq"]]
    cs = e.upload_chain_arrays(tseq, qseq, ch["strand"], off, bt, bq, bs)
    pieces = e.axt_split(tseq, qseq, ch["strand"], off, bt, bq, bs, 100)
    n = len(pieces)
    res = {"chains": int(ch["n"]), "blocks": int(len(bs)), "bases": int(bs.sum(dtype=np.int64)), "pieces": n}
    d_w = e.dev_alloc(20 * n + 8)
    e.h2d(d_w, np.ascontiguousarray(pieces))
    d_r = e.dev_alloc(17 * 8 * n + 8)
    calls = (("axt_measure", lambda: e.axt_measure_device(cs, d_w, n, d_r, d_r + 8 * n, d_r + 16 * n, d_r + 24 * n)),
             ("axt_pair_counts", lambda: e.axt_pair_counts_device(cs, d_w, n, d_r, d_r + 128 * n)))
    for name, call in calls:
        for _ in range(2):
            call()
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            call()
        e.synchronize()
        res[name + "_wall_ms"] = (time.perf_counter() - t0) / 5 * 1e3
    out = np.zeros(17 * n, np.int64)
    e.d2h(out, d_r)
    ali = e.axt_measure(cs, pieces)[2]
    res["columns_agree"] = bool((out[:16 * n].reshape(n, 16).sum(1) + out[16 * n:] == ali).all())
    print("PROF_JSON " + json.dumps(res), flush=True)
    cs.close()
    e.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "lav":
        write_lav(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 3 and sys.argv[1] == "kernels":
        kernels(sys.argv[2])
    else:
        sys.exit(__doc__)
