"""The netting's records (gac_net.c): a 64-byte fill with its 32-byte gaps
right behind it in one arena group, the gap's parent found from its index, a
gap's single fill held inline.  None of it may change a net: both nets are compared byte for byte across threads
(GAC_THREADS 1, 3, 8) and arena block sizes (the default, and blocks of a few
records, GAC_NET_ARENA_BLOCK, so that groups roll over at every position and
some exceed a block), and with the reference chainNet where it is built; the
target fills' block windows are checked against chainSubsetOnT's rule.  No
device involved."""
import os
import re
import subprocess

import numpy as np
import pytest

THREADS = (1, 3, 8)
ENV_KEYS = ("GAC_NET_LOOKAHEAD", "GAC_THREADS", "GAC_NET_SPLIT", "GAC_TIMING", "GAC_NET_ARENA_BLOCK")
OPTS = [("ms1", dict(min_score=0.0, min_space=1)),  # -minSpace=1 -minScore=0
        ("default", dict(min_score=2000.0))]
# shapes of the nested set
GAPS_PER_FILL = (0, 1, 2, 3, 13, 19)  # 3: odd, the group is padded; 19: more than a 512-byte block
FILLS_PER_GAP = (0, 1, 2, 16, 20)     # 1: inline; 16: the insertion sort's last size; 20: qsort
SMALL_BLOCK = 512                     # bytes: a fill and at most 14 gaps
TOP_B = 5                             # top-level fills of the second target sequence


def _set_env(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _nets(ca, tsizes, qsizes, env, d, tag, monkeypatch, **kw):
    """Both nets of one gac_net_build under env, as bytes, and the target
    fills (chain, range, window)."""
    from genomealignmenttools_amd._lib import GAC_Q, GAC_T
    from genomealignmenttools_amd.chainnet import Net
    _set_env(monkeypatch, env)
    net = Net(ca, tsizes, qsizes, **kw)
    fills = net.fills(GAC_T)
    out = []
    for side, s in ((GAC_T, "t"), (GAC_Q, "q")):
        p = os.path.join(d, f"{tag}.{s}.net")
        net.write(side, p, meta=ca.meta)
        out.append(open(p, "rb").read())
    net.close()
    return out, fills


def _ref_nets(d, kw):
    """The reference chainNet's nets of d/in.chain, or None where it is not built."""
    from oracle.oracle import have_ref, ref_tool
    if not have_ref():
        return None
    p = lambda x: os.path.join(d, x)
    opts = [f"-minScore={kw['min_score']:g}"]
    if "min_space" in kw:
        opts.append(f"-minSpace={kw['min_space']}")
    r = subprocess.run([ref_tool("chainNet"), p("in.chain"), p("t.sizes"), p("q.sizes"),
                        p("ref.t.net"), p("ref.q.net")] + opts, capture_output=True)
    assert r.returncode == 0, r.stderr
    return [open(p("ref.t.net"), "rb").read(), open(p("ref.q.net"), "rb").read()]


def _through_file(ca, tsizes, qsizes, d):
    """Write the set the way the tools read it; the chains as read back."""
    from genomealignmenttools_amd import chainfile, synth
    synth.write_sizes(tsizes, os.path.join(d, "t.sizes"))
    synth.write_sizes(qsizes, os.path.join(d, "q.sizes"))
    chainfile.write_chains(ca, os.path.join(d, "in.chain"))
    return chainfile.read_chains(os.path.join(d, "in.chain"))


def _subset_windows(ca, chain, s, e):
    """chainSubsetOnT's window (kent/src/lib/chain.c:481-500) of each (chain,
    s, e): chain-local first block with tEnd > s, and the count of blocks from
    there with tStart < e."""
    first, cnt = np.zeros(len(chain), np.int64), np.zeros(len(chain), np.int64)
    for i, (c, a, b) in enumerate(zip(chain, s, e)):
        o0, o1 = ca.blk_off[c], ca.blk_off[c + 1]
        bt, bs = ca.blk_t[o0:o1], ca.blk_size[o0:o1]
        f = int(np.searchsorted(bt + bs, a, side="right"))
        first[i], cnt[i] = f, int(np.searchsorted(bt, b, side="left")) - f
    return first, cnt


def _check_windows(ca, fills, min_partial):
    """Every target fill's window, whole-chain fills included; at least
    min_partial of them cover part of their chain."""
    assert ((fills["flags"] & 1) == 1).sum() >= min_partial
    first, cnt = _subset_windows(ca, fills["chain"], fills["start"], fills["end"])
    assert np.array_equal(fills["first_block"], first)
    assert np.array_equal(fills["n_blocks"], cnt)


def _chain(score, blocks, tname, minus=False):
    """One chain of the nested set: target blocks [(start, end), ...], the
    query the same stretch of the sequence of the same size (reversed for a
    '-' chain)."""
    size = SIZES[tname]
    ts, te = blocks[0][0], blocks[-1][1]
    bt = [b[0] for b in blocks]
    bq = [size - te + (b[0] - ts) for b in blocks] if minus else bt
    return dict(score=score, minus=minus, tname=tname, qname="chrQ" + tname[-1], size=size, ts=ts,
                te=te, qs=bq[0], qe=bq[-1] + blocks[-1][1] - blocks[-1][0], bt=bt, bq=bq,
                bs=[b[1] - b[0] for b in blocks])


SIZES = {"chrA": 1_000_000, "chrB": 500_000}


def _run(s, n_blocks, size, step):
    """n_blocks blocks of size bases, step apart, from s."""
    return [(s + i * step, s + i * step + size) for i in range(n_blocks)]


def _shapes_case():
    """chrA: one top-level chain (its root gap holds one fill) with six gaps,
    holding 0, 1, 2, 20, 16 and 2 fills; among those fills one with 13 gaps
    (every other one filled again), fills with 1, 2, 3 and 19 gaps, and the 20,
    each with one gap that is filled by a fill without gaps.  chrB: TOP_B
    top-level chains of 1 to 4 blocks and the pieces of a chain that crosses
    them (a root gap with many fills, partial fills).  '-'
    chains at every level, so both sides hold some."""
    from genomealignmenttools_amd.chainfile import ChainArrays
    ch = [_chain(100000, [(1000, 2000), (10000, 11000), (20000, 21000), (30000, 31000),
                          (60000, 61000), (70000, 71000), (100000, 101000)], "chrA")]
    # gap (2000, 10000): no fill.  gap (11000, 20000): one fill with 13 gaps
    many = _run(12000, 14, 200, 500)
    ch.append(_chain(50000, many, "chrA", minus=True))
    for i in range(0, 13, 2):
        s = many[i][1] + 50
        ch.append(_chain(9000 - i, [(s, s + 100)], "chrA", minus=i % 4 == 0))
    # gap (21000, 30000): two fills, with one gap and with two
    ch.append(_chain(49000, _run(22000, 2, 300, 600), "chrA"))
    ch.append(_chain(48000, _run(25000, 3, 300, 600), "chrA", minus=True))
    # gap (31000, 60000): 20 fills in shuffled order, each with one gap, filled
    rng = np.random.default_rng(3)
    order = rng.permutation(20)
    for r, j in enumerate(order):
        s = 32000 + int(j) * 1300
        ch.append(_chain(40000 - r, [(s, s + 300), (s + 800, s + 1100)], "chrA", minus=j % 3 == 0))
    for r, j in enumerate(order[::-1]):
        s = 32000 + int(j) * 1300
        ch.append(_chain(8000 - r, [(s + 400, s + 600)], "chrA", minus=j % 2 == 0))
    # gap (61000, 70000): 16 fills without gaps, shuffled
    for r, j in enumerate(rng.permutation(16)):
        s = 61500 + int(j) * 500
        ch.append(_chain(30000 - r, [(s, s + 200)], "chrA", minus=j % 5 == 0))
    # gap (71000, 100000): a fill with 3 gaps and one with 19 (more than a small block)
    ch.append(_chain(47000, _run(72000, 4, 300, 600), "chrA"))
    ch.append(_chain(46000, _run(76000, 20, 300, 600), "chrA", minus=True))
    # chrB: top-level fills only
    for j in range(TOP_B):
        ch.append(_chain(20000 - j, _run(10000 + 50000 * ((j * 3) % TOP_B), 1 + j % 4, 400, 900),
                         "chrB", minus=j == 2))
    # and one chain across them all, cut into partial fills by the first of them
    ch.append(_chain(5000, _run(9800, 30, 500, 1500), "chrB"))
    ch.sort(key=lambda c: -c["score"])
    n = len(ch)
    i32 = lambda k: np.array([c[k] for c in ch], np.int32)
    cat = lambda k: np.concatenate([np.asarray(c[k], np.int32) for c in ch])
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(c["bt"]) for c in ch])
    ca = ChainArrays(score=np.array([c["score"] for c in ch], np.float64),
                     tname=[c["tname"] for c in ch], tsize=i32("size"), tstart=i32("ts"),
                     tend=i32("te"), qname=[c["qname"] for c in ch], qsize=i32("size"),
                     qstrand=np.array([c["minus"] for c in ch], np.uint8), qstart=i32("qs"),
                     qend=i32("qe"), id=np.arange(1, n + 1, dtype=np.int64), blk_off=off,
                     blk_t=cat("bt"), blk_q=cat("bq"), blk_size=cat("bs"))
    return ca, dict(SIZES), {"chrQA": SIZES["chrA"], "chrQB": SIZES["chrB"]}


def _tree_counts(text):
    """From a .net text: the gap counts of its fills, the fill counts of its
    gaps, and the fill counts of its root gaps (per "net" line)."""
    gaps_of_fill, fills_of_gap, roots = [], [], []
    stack = []  # (depth, kind, index into its list)
    for ln in text.splitlines():
        if ln.startswith("#"):
            continue
        if ln.startswith("net "):
            roots.append(0)
            stack = []
            continue
        depth = len(ln) - len(ln.lstrip())
        kind = ln.split()[0]
        while stack and stack[-1][0] >= depth:
            stack.pop()
        if kind == "fill":
            if stack:
                fills_of_gap[stack[-1][2]] += 1
            else:
                roots[-1] += 1
            gaps_of_fill.append(0)
            stack.append((depth, kind, len(gaps_of_fill) - 1))
        else:
            gaps_of_fill[stack[-1][2]] += 1
            fills_of_gap.append(0)
            stack.append((depth, kind, len(fills_of_gap) - 1))
    return gaps_of_fill, fills_of_gap, roots


@pytest.mark.parametrize("tag,kw", OPTS)
def test_fill_and_gap_shapes(tag, kw, tmp_path, monkeypatch):
    d = str(tmp_path)
    ca, ts, qs = _shapes_case()
    ca = _through_file(ca, ts, qs, d)
    base, fills = _nets(ca, ts, qs, {"GAC_THREADS": "1"}, d, "base", monkeypatch, **kw)
    # the set has the shapes it is meant to have (target net)
    gof, fog, roots = _tree_counts(base[0].decode())
    assert set(GAPS_PER_FILL) <= set(gof), sorted(set(gof))
    assert set(FILLS_PER_GAP) <= set(fog), sorted(set(fog))
    assert roots[0] == 1 and roots[1] > TOP_B
    assert b" - " in base[0] and b" - " in base[1]
    _check_windows(ca, fills, 2)
    for block in (None, SMALL_BLOCK):
        for nt in THREADS:
            env = {"GAC_THREADS": str(nt)}
            if block:
                env["GAC_NET_ARENA_BLOCK"] = str(block)
            got, f = _nets(ca, ts, qs, env, d, f"b{block}t{nt}", monkeypatch, **kw)
            assert got[0] == base[0], (tag, block, nt, "target net")
            assert got[1] == base[1], (tag, block, nt, "query net")
            for k in fills:
                assert np.array_equal(f[k], fills[k]), (tag, block, nt, k)
    want = _ref_nets(d, kw)
    if want is not None:
        assert base[0] == want[0], (tag, "target net vs reference")
        assert base[1] == want[1], (tag, "query net vs reference")


@pytest.fixture(scope="module")
def split_case():
    """One target sequence with 30000 chains of up to 3000 blocks: split into
    regions from 2 threads on, whose workers push fills onto shared gaps."""
    from genomealignmenttools_amd import synth
    tg, qg, ca = synth.small_case(seed=21, n_chains=30000, tsize=6_000_000,
                                  qsizes=(3_000_000, 2_000_000, 1_000_000), max_blocks=3000)
    return ca, tg.sizes, qg.sizes


@pytest.mark.parametrize("tag,kw", OPTS)
def test_region_workers_share_gaps(tag, kw, split_case, tmp_path, monkeypatch, capfd):
    """The region path with the default block and with 1 KB blocks: most
    groups of the long chains (up to 64 + 32 x 2999 bytes reserved) take a
    block of their own, the rest roll over every few fills."""
    ca, ts, qs = split_case
    d = str(tmp_path)
    ca = _through_file(ca, ts, qs, d)
    base, fills = _nets(ca, ts, qs, {"GAC_THREADS": "1"}, d, "base", monkeypatch, **kw)
    _check_windows(ca, fills, 1000)
    for block in (None, 1024):
        for nt in THREADS:
            env = {"GAC_THREADS": str(nt), "GAC_TIMING": "1"}
            if block:
                env["GAC_NET_ARENA_BLOCK"] = str(block)
            capfd.readouterr()
            got, f = _nets(ca, ts, qs, env, d, f"b{block}t{nt}", monkeypatch, **kw)
            err = capfd.readouterr().err
            assert got[0] == base[0], (tag, block, nt, "target net")
            assert got[1] == base[1], (tag, block, nt, "query net")
            for k in fills:
                assert np.array_equal(f[k], fills[k]), (tag, block, nt, k)
            m = re.search(r"side 0 seq 0: (\d+) chains, \d+ sequential, (\d+) regions", err)
            if nt == 1:
                assert m is None  # one thread nets every side whole
            else:
                assert m and int(m.group(2)) > 1, err
            # the record sizes the layout promises, and every record counted
            m = re.search(r"fill/gap arenas \d+ MB: (\d+) fills of 64 bytes, (\d+) gaps of 32 bytes", err)
            assert m, err
            assert int(m.group(1)) >= len(fills["chain"])
    want = _ref_nets(d, kw)
    if want is not None:
        assert base[0] == want[0] and base[1] == want[1]
