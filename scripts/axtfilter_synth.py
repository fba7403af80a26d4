#!/usr/bin/env python3
"""A seeded, lastz-like axt file for timing filterAxtIdentityEntropy.py.

    scripts/axtfilter_synth.py OUT.axt BYTES [SEED]

Entries of 50..5000 columns.  About 30 % are low-complexity hits of the kind
sensitive lastz settings produce in bulk (a short repeat unit, lightly
mutated, or one or two letters), the rest are random sequence; the query is a
copy of the target with 10-40 % substitutions, a few gap runs go into either
row, and some runs of both rows are lower case as soft-masked sequence comes
out of lastz.  A pool of 64 MB of distinct entries is made and written over and
over until BYTES are reached (the headers repeat with it; the filter reads
nothing of them but the third word), so a 4 GB file takes seconds."""
import sys

import numpy as np

POOL = 64 << 20
BASES = np.frombuffer(b"ACGT", np.uint8)


def entry(rng, k):
    L = int(rng.integers(50, 5001))
    if rng.random() < 0.3:
        kind = rng.random()
        if kind < 0.5:   # a microsatellite: a unit of 1-4 bases, 3 % of the columns changed
            unit = BASES[rng.integers(0, 4, int(rng.integers(1, 5)))]
            t = np.tile(unit, L // len(unit) + 1)[:L].copy()
            hit = rng.random(L) < 0.03
            t[hit] = BASES[rng.integers(0, 4, int(hit.sum()))]
        else:            # two letters, one of them rare
            two = BASES[rng.permutation(4)[:2]]
            t = two[(rng.random(L) < 0.1).astype(np.int64)]
    else:
        t = BASES[rng.integers(0, 4, L)]
    q = t.copy()
    sub = rng.random(L) < rng.uniform(0.1, 0.4)
    q[sub] = BASES[rng.integers(0, 4, int(sub.sum()))]
    for row in (t, q):  # gap runs: a base of the other row against '-'
        for _ in range(int(rng.integers(0, 1 + L // 400))):
            a = int(rng.integers(0, L))
            row[a:a + int(rng.integers(1, 30))] = ord("-")
    both = (t == ord("-")) & (q == ord("-"))
    q[both] = BASES[0]
    for _ in range(int(rng.integers(0, 1 + L // 500))):  # soft-masked runs
        a = int(rng.integers(0, L))
        b = a + int(rng.integers(10, 300))
        for row in (t, q):
            seg = row[a:b]
            seg[seg != ord("-")] |= 0x20
    tn, qn = int((t != ord("-")).sum()), int((q != ord("-")).sum())
    ts, qs = int(rng.integers(1, 10 ** 8)), int(rng.integers(1, 10 ** 8))
    head = "%d chr%d %d %d scaffold%d %d %d %s %d\n" % (
        k, 1 + k % 22, ts, ts + tn - 1, k % 997, qs, qs + qn - 1, "+-"[k & 1], int(rng.integers(3000, 10 ** 6)))
    return head.encode() + t.tobytes() + b"\n" + q.tobytes() + b"\n\n"


def main():
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    out, want = sys.argv[1], int(float(sys.argv[2]))
    rng = np.random.default_rng(int(sys.argv[3]) if len(sys.argv) == 4 else 1234)
    parts, size = [], 0
    while size < min(POOL, want):
        parts.append(entry(rng, len(parts)))
        size += len(parts[-1])
    pool = b"".join(parts)
    with open(out, "wb") as f:
        written = 0
        while written + len(pool) <= want:
            f.write(pool)
            written += len(pool)
        for p in parts:  # whole entries up to the size asked for
            if written >= want:
                break
            f.write(p)
            written += len(p)
    print("%s: %d bytes, pool of %d entries" % (out, written, len(parts)))


if __name__ == "__main__":
    main()
