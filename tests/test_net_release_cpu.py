"""chainNet frees the nets and the chains under its writers (chainNet.c's
release helper, started by the writers' "formatted" signal:
gac_par_output_buf_ex -> gac_net_write_ex -> gac_net_release).  That moves
when memory is released, never what is written: both nets are compared byte
for byte with GAC_EARLY_FREE=0 (everything freed after the writes, as before
the signal existed) and with the reference chainNet where it is built.

oracle/_build/chainNet_cpu is the real tool on the CPU stand-in of the device
ABI (as in test_sparse_upload.py).  Every set is a few KB.  TEST
INFRASTRUCTURE only; no device involved."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "oracle", "_build", "chainNet_cpu")
SIZE = 400_000
THREADS = (1, 3, 8)
# the deepest nest of the "nested" set (levels 0 .. DEPTH - 1)
DEPTH = 6
# fills of the "many" set: the writer cuts a side's nf fills into runs of
# nf / (64 * threads) + 1, so 8 threads make 2-fill runs of them: 350 runs,
# more than one 256-run writev batch
MANY = 700


@pytest.fixture(scope="module")
def tool():
    # one build at a time: pytest-xdist workers may reach this together
    import fcntl
    os.makedirs(os.path.join(ROOT, "oracle", "_build"), exist_ok=True)
    with open(os.path.join(ROOT, "oracle", "_build", ".cpu-chainnet.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "cpu-chainnet"], cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


def _chain(score, blocks, minus=False):
    """Target blocks [(start, end), ...]; the query the same stretch of its
    sequence (mirrored for a '-' chain)."""
    ts, te = blocks[0][0], blocks[-1][1]
    bt = [b[0] for b in blocks]
    bq = [SIZE - te + (b[0] - ts) for b in blocks] if minus else bt
    return dict(score=score, minus=minus, ts=ts, te=te, qs=bq[0],
                qe=bq[-1] + blocks[-1][1] - blocks[-1][0], bt=bt, bq=bq,
                bs=[b[1] - b[0] for b in blocks])


def _sets():
    s = {"empty": [], "one_block": [_chain(5000, [(1000, 1100)])]}
    # whole chains only: fills, but no partial target fill to rescore
    s["no_partial"] = [_chain(9000 - i, [(10_000 * (i + 1), 10_000 * (i + 1) + 300),
                                        (10_000 * (i + 1) + 500, 10_000 * (i + 1) + 900)], minus=i == 1)
                       for i in range(3)]
    # DEPTH levels, each chain inside the one gap of the chain above it; at
    # the bottom fills with 0, 1 and 5 gaps; then chains that overlap what is
    # already filled (partial fills: rescored) at several levels
    nest = [_chain(100_000 - k, [(1000 + 2000 * k, 1500 + 2000 * k),
                                 (SIZE - 1500 - 2000 * k, SIZE - 1000 - 2000 * k)], minus=k % 2 == 1)
            for k in range(DEPTH - 1)]
    lo = 1500 + 2000 * (DEPTH - 2) + 1000
    nest.append(_chain(50_000, [(lo, lo + 400)]))
    nest.append(_chain(49_000, [(lo + 1000, lo + 1400), (lo + 2000, lo + 2400)], minus=True))
    nest.append(_chain(48_000, [(lo + 5000 + 600 * j, lo + 5000 + 600 * j + 300) for j in range(6)]))
    nest.append(_chain(20_000, [(lo + 5350, lo + 5550), (lo + 5950, lo + 6150)]))  # inside two of its gaps
    for k in (0, 2, DEPTH - 2):  # starts on a filled block, runs on into the gap
        a = 1000 + 2000 * k + 300
        nest.append(_chain(10_000 - k, [(a, a + 600), (a + 700, a + 900)], minus=k == 2))
    nest.append(_chain(9000, [(lo + 200, lo + 800), (lo + 1200, lo + 2200)]))
    s["nested"] = nest
    many = [_chain(90_000 - i, [(500 * i + 100, 500 * i + 400)], minus=i % 3 == 0) for i in range(MANY)]
    many += [_chain(1000 - i, [(500 * i + 300, 500 * i + 480)]) for i in range(0, MANY, 2)]
    s["many"] = many
    return s


def _write_set(d, chains):
    from genomealignmenttools_amd import chainfile, synth
    from genomealignmenttools_amd.chainfile import ChainArrays
    ch = sorted(chains, key=lambda c: -c["score"])
    n = len(ch)
    i32 = lambda k: np.array([c[k] for c in ch], np.int32)
    cat = lambda k: (np.concatenate([np.asarray(c[k], np.int32) for c in ch]) if n
                     else np.zeros(0, np.int32))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(c["bt"]) for c in ch])
    ca = ChainArrays(score=np.array([c["score"] for c in ch], np.float64), tname=["chrT"] * n,
                     tsize=np.full(n, SIZE, np.int32), tstart=i32("ts"), tend=i32("te"),
                     qname=["chrQ"] * n, qsize=np.full(n, SIZE, np.int32),
                     qstrand=np.array([c["minus"] for c in ch], np.uint8), qstart=i32("qs"),
                     qend=i32("qe"), id=np.arange(1, n + 1, dtype=np.int64), blk_off=off,
                     blk_t=cat("bt"), blk_q=cat("bq"), blk_size=cat("bs"))
    p = lambda x: os.path.join(d, x)
    os.makedirs(d, exist_ok=True)
    tg = synth.random_genome({"chrT": SIZE}, seed=5)
    qg = synth.random_genome({"chrQ": SIZE}, seed=6)
    synth.write_2bit(tg, p("t.2bit"))
    synth.write_2bit(qg, p("q.2bit"))
    synth.write_sizes({"chrT": SIZE}, p("t.sizes"))
    synth.write_sizes({"chrQ": SIZE}, p("q.sizes"))
    if n:
        chainfile.write_chains(ca, p("in.chain"))
    else:
        open(p("in.chain"), "w").close()


def _run(exe, d, tnet, qnet, env=None, check=True):
    p = lambda x: os.path.join(d, x)
    cmd = [exe, p("in.chain"), p("t.sizes"), p("q.sizes"), tnet, qnet, "-rescore",
           f"-tNibDir={p('t.2bit')}", f"-qNibDir={p('q.2bit')}", "-linearGap=loose"]
    e = {k: v for k, v in os.environ.items() if k not in ("GAC_EARLY_FREE", "GAC_THREADS")}
    r = subprocess.run(cmd, capture_output=True, timeout=120, env=dict(e, **(env or {})))
    if check:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def _nets(exe, d, tag, env=None):
    p = lambda x: os.path.join(d, x)
    _run(exe, d, p(tag + ".t.net"), p(tag + ".q.net"), env)
    return open(p(tag + ".t.net"), "rb").read(), open(p(tag + ".q.net"), "rb").read()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Every set written once, with the reference's nets where it is built."""
    from oracle.oracle import ref_tool
    ref = ref_tool("chainNet")
    out = {}
    for name, chains in _sets().items():
        d = str(tmp_path_factory.mktemp(name))
        _write_set(d, chains)
        out[name] = (d, _nets(ref, d, "ref") if os.path.exists(ref) else None)
    return out


@pytest.mark.parametrize("nt", THREADS)
@pytest.mark.parametrize("name", ["empty", "one_block", "no_partial", "nested", "many"])
def test_nets_identical(tool, cases, name, nt):
    d, ref = cases[name]
    on = _nets(tool, d, f"on{nt}", {"GAC_THREADS": str(nt)})
    off = _nets(tool, d, f"off{nt}", {"GAC_THREADS": str(nt), "GAC_EARLY_FREE": "0"})
    assert on[0] == off[0], "target net"
    assert on[1] == off[1], "query net"
    if ref is not None:
        assert on[0] == ref[0], "target net vs reference"
        assert on[1] == ref[1], "query net vs reference"


def test_the_sets_have_the_shapes_they_claim(tool, cases):
    fills = lambda net: [ln for ln in net.decode().splitlines() if ln.lstrip().startswith("fill")]
    gaps_under = lambda net: _gap_counts(net.decode().splitlines())
    t, q = _nets(tool, cases["empty"][0], "shape")
    assert fills(t) == [] and fills(q) == []
    t, _ = _nets(tool, cases["one_block"][0], "shape")
    assert len(fills(t)) == 1  # a single run
    t, _ = _nets(tool, cases["no_partial"][0], "shape")
    assert len(fills(t)) == 3
    t, _ = _nets(tool, cases["nested"][0], "shape")
    depth = [(len(ln) - len(ln.lstrip()) - 1) // 2 for ln in fills(t)]
    assert max(depth) >= DEPTH - 1 > 2
    assert {0, 1, 5} <= set(gaps_under(t))
    t, q = _nets(tool, cases["many"][0], "shape", {"GAC_THREADS": "8"})
    assert len(fills(t)) >= MANY and len(fills(q)) >= MANY
    # some fill was rescored in the sets that have partial fills: its score is
    # not its chain's
    for name in ("nested", "many"):
        d = cases[name][0]
        scores = {ln.split()[0] for ln in open(os.path.join(d, "in.chain")) if ln.startswith("chain")}
        t, _ = _nets(tool, d, "shape")
        assert any(ln.split()[ln.split().index("score") + 1] not in scores for ln in fills(t)), name


def _gap_counts(lines):
    """Number of gap lines directly under each fill line."""
    out, stack = [], []
    for ln in lines:
        w = ln.split()
        if not w or w[0] not in ("fill", "gap"):
            continue
        ind = len(ln) - len(ln.lstrip())
        while stack and stack[-1][0] >= ind:
            out.append(stack.pop()[1])
        if w[0] == "fill":
            stack.append([ind, 0])
        elif stack and stack[-1][0] == ind - 1:
            stack[-1][1] += 1
    return out + [s[1] for s in stack]


@pytest.mark.parametrize("which", ["t", "q"])
@pytest.mark.parametrize("name", ["empty", "nested"])
def test_one_net_to_stdout(tool, cases, name, which):
    d, ref = cases[name]
    p = lambda x: os.path.join(d, x)
    want = _nets(tool, d, "file", {"GAC_EARLY_FREE": "0"})
    for env in ({}, {"GAC_THREADS": "3"}):
        f = p(f"so.{which}.net")
        r = _run(tool, d, "stdout" if which == "t" else f, f if which == "t" else "stdout", env)
        got = (r.stdout, open(f, "rb").read()) if which == "t" else (open(f, "rb").read(), r.stdout)
        assert got == want
    if ref is not None:
        assert want == ref


@pytest.mark.parametrize("which", ["t", "q"])
@pytest.mark.parametrize("name", ["one_block", "many"])
def test_failed_write_aborts_the_same_way(tool, cases, name, which):
    """A net that cannot be written (/dev/full): the message and the exit
    status the tool had before the release existed (and has with
    GAC_EARLY_FREE=0), whichever net fails and with the other net's signal
    already given; no crash."""
    d, _ = cases[name]
    good = os.path.join(d, f"full.{which}.net")
    for env in ({}, {"GAC_EARLY_FREE": "0"}, {"GAC_THREADS": "8"}):
        r = _run(tool, d, "/dev/full" if which == "t" else good, good if which == "t" else "/dev/full",
                 env, check=False)
        assert r.returncode == 255, (env, r.returncode, r.stderr[-500:])
        assert r.stderr.decode().splitlines()[-1] == "write error on /dev/full", (env, r.stderr[-500:])
