"""chainToPsl on the GPU: the per-chain PSL match counts kernel (exact integers
against the numpy restatement in tests/pslout_ref.py and against the fixtures
made with the reference's tool) and the drop-in tool, byte for byte."""
import gzip
import os
import subprocess

import numpy as np
import pytest
# torch before libgachain (see the note at the top of tests/test_gpu_antirepeat.py)
import torch  # noqa: F401

from conftest import BLASTZ, GOLDEN

import pslout_ref as PS

pytestmark = pytest.mark.gpu

GAC_E_ARG, GAC_E_STATE = -1, -5
USAGE = b"chainToPsl - Convert chain file to psl format\nusage:\n   chainToPsl in.chain tSizes qSizes target.lst query.lst out.psl\n"


def _bin(name):
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, name)


def _engine(tg, qg, t_soft=True):
    """The target with the soft-mask plane, the query without (it needs none)."""
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    e = Engine(0)
    e.add_sequences(GAC_T, tg.seq_records(), mask_runs=tg.mruns if t_soft else None)
    e.add_sequences(GAC_Q, qg.seq_records())
    return e


# ------------------------------------------------------- counts on fixtures
@pytest.mark.parametrize("name", sorted(PS.SETS))
def test_counts_equal_fixture(name):
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    d, chain = PS.SETS[name]
    want = np.load(os.path.join(PS.PSL_DIR, f"{name}.counts.npz"))["counts"]
    ca = read_chains(chain)
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
        e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"))
        cs = e.upload_chains(ca)  # '-' blocks unshifted: flipped with the .2bit size
        got = e.chain_psl_counts(cs)
        assert got.dtype == np.int64 and got.shape == (ca.n, 4)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
        cs.close()
    finally:
        e.close()


# -------------------------------------------------- hand-built edge shapes
def _long_run(runs, need):
    """(start, size) of the first run of at least `need` bases"""
    for a, l in zip(*runs):
        if l >= need:
            return int(a), int(l)
    raise AssertionError("no run of %d bases" % need)


def _edge_case():
    """(tg, qg, ChainArrays): the smallest shapes that reach each path of the
    walk, '+' and '-' each."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.chainfile import ChainArrays
    tg = synth.random_genome({"t1": 200_003, "t2": 4_099}, 31, n_frac=0.01, n_mean=150, mask_frac=0.3)
    qg = synth.random_genome({"q1": 150_013, "q2": 4_001}, 32, n_frac=0.01, n_mean=150, mask_frac=0.3)
    rng = np.random.default_rng(33)
    rec = []

    def chain(tn, qn, minus, t0, q0, sizes, gaps=None):
        sizes = np.asarray(sizes, np.int64)
        nb = len(sizes)
        if gaps is None:
            gaps = np.stack([rng.integers(0, 6, nb - 1), rng.integers(1, 6, nb - 1)], 1)
        gaps = np.asarray(gaps, np.int64).reshape(-1, 2)
        bt = t0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps[:, 0])])
        bq = q0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps[:, 1])])
        assert bt[-1] + sizes[-1] <= tg.sizes[tn] and bq[-1] + sizes[-1] <= qg.sizes[qn]
        rec.append((tn, qn, minus, bt, bq, sizes))

    tn_run = _long_run(tg.nruns[0], 40)    # an N run of t1
    tm_run = _long_run(tg.mruns[0], 100)   # a mask run of t1
    qn_run = _long_run(qg.nruns[0], 40)    # an N run of q1 (forward coordinates)
    for minus in (0, 1):
        chain("t1", "q1", minus, 100, 200, [1] * 5)                      # 1-base blocks
        chain("t1", "q1", minus, 31, 63, [5])                            # starts at bit 31
        chain("t1", "q1", minus, 30, 62, [3])                            # ends at bit 0
        chain("t1", "q2", minus, 64 + 20, 32 + 7, [60])                  # crosses 3 words
        chain("t1", "q1", minus, 1000, 2001, [4095])                     # below the wide record
        chain("t1", "q1", minus, 9001, 7003, [4096])                     # the wide record
        chain("t1", "q1", minus, 120_001, 70_007, [70_000])              # many words per block
        for nb in (1, 63, 64, 65, 300):                                  # lane / tile / workgroup edges
            chain("t1", "q1", minus, int(rng.integers(0, 50_000)), int(rng.integers(0, 50_000)),
                  rng.integers(1, 41, nb))
        for k in range(200):                                             # many chains per tile
            tn, qn = ("t2", "q2") if k % 3 == 0 else ("t1", "q1")
            z = int(rng.integers(1, 70))
            chain(tn, qn, minus, int(rng.integers(0, tg.sizes[tn] - z)),
                  int(rng.integers(0, qg.sizes[qn] - z)), [z])
        chain("t2", "q2", minus, 4_099 - 40, 4_001 - 40, [40])           # the last bases of both
        chain("t1", "q1", minus, tn_run[0] + 2, 40_000, [36])            # inside a target N run
        chain("t1", "q1", minus, tm_run[0] + 3, 41_000, [90])            # inside a target mask run
        q0 = 150_013 - (qn_run[0] + 38) if minus else qn_run[0] + 2      # inside a query N run
        chain("t1", "q1", minus, 42_000, q0, [36])
    off = np.concatenate([[0], np.cumsum([len(r[5]) for r in rec])]).astype(np.int64)
    n = len(rec)
    i32 = lambda x: np.asarray(x, np.int32)
    ca = ChainArrays(
        score=np.full(n, 1000.0), tname=[r[0] for r in rec], tsize=i32([tg.sizes[r[0]] for r in rec]),
        tstart=i32([r[3][0] for r in rec]), tend=i32([r[3][-1] + r[5][-1] for r in rec]),
        qname=[r[1] for r in rec], qsize=i32([qg.sizes[r[1]] for r in rec]),
        qstrand=np.asarray([r[2] for r in rec], np.uint8), qstart=i32([r[4][0] for r in rec]),
        qend=i32([r[4][-1] + r[5][-1] for r in rec]), id=np.arange(1, n + 1, dtype=np.int64),
        blk_off=off, blk_t=i32(np.concatenate([r[3] for r in rec])),
        blk_q=i32(np.concatenate([r[4] for r in rec])), blk_size=i32(np.concatenate([r[5] for r in rec])))
    return tg, qg, ca


@pytest.fixture(scope="module")
def edge():
    tg, qg, ca = _edge_case()
    return tg, qg, ca, PS.counts(tg, qg, ca)


def test_counts_edge_shapes(edge):
    tg, qg, ca, want = edge
    assert (want.sum(0) > 0).all()
    # the planted blocks: all N (target run, query run) and all lower case on both strands
    sizes = np.add.reduceat(ca.blk_size.astype(np.int64), ca.blk_off[:-1])
    assert np.array_equal(want.sum(1), sizes)
    for s in (0, 1):
        k = np.flatnonzero(ca.qstrand == s)[-3:]
        assert want[k[0], 3] == 36 and want[k[2], 3] == 36, want[k]
        assert want[k[1], 0] == 0 and want[k[1], 2] > 0, want[k]
    e = _engine(tg, qg)
    try:
        cs = e.upload_chains(ca)
        got = e.chain_psl_counts(cs)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (bad[:10], got[bad[:3]], want[bad[:3]])
        # the _device variant on the context's stream gives the same
        n = ca.n
        d = e.dev_alloc(n * 4 * 8)
        e.chain_psl_counts_device(cs, d)
        e.synchronize()
        out = np.zeros((n, 4), np.int64)
        e.d2h(out, d)
        e.dev_free(d)
        assert np.array_equal(out, got)
        cs.close()
        # an empty set: success, nothing written
        empty = e.upload_chain_arrays(*([np.zeros(0, np.int32)] * 2), np.zeros(0, np.uint8),
                                      np.zeros(1, np.int64), *([np.zeros(0, np.int32)] * 3))
        assert e.chain_psl_counts(empty).shape == (0, 4)
        e.chain_psl_counts_device(empty, 0)
        empty.close()
    finally:
        e.close()


def test_softmask_state_and_scoring_without_plane():
    """The plane on T alone is enough; without it the call is GAC_E_STATE, and
    on that context scoring still gives the reference's sub-chain scores."""
    from genomealignmenttools_amd._lib import GacError, lib
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine, GapCosts
    d = os.path.join(GOLDEN, "synth11")
    z = np.load(os.path.join(d, "subchain.npz"))
    want = np.load(os.path.join(PS.PSL_DIR, "synth11.counts.npz"))["counts"]
    ca = read_chains(os.path.join(d, "in.chain"))
    for soft in (True, False):
        e = Engine(0)
        try:
            e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=soft)
            e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"))  # the query side never has it here
            e.set_scoring(np.asarray(BLASTZ, np.int32), GapCosts("loose"))
            cs = e.upload_chains(ca)
            if soft:
                assert np.array_equal(e.chain_psl_counts(cs), want)
            else:
                with pytest.raises(GacError) as ei:
                    e.chain_psl_counts(cs)
                assert ei.value.code == GAC_E_STATE
                d_buf = e.dev_alloc(ca.n * 32)
                with pytest.raises(GacError) as ei:
                    e.chain_psl_counts_device(cs, d_buf)
                assert ei.value.code == GAC_E_STATE
                e.dev_free(d_buf)
            g, l, a = e.score_ranges(cs, z["ranges"], want_local=True)
            assert np.array_equal(g, z["glob"]) and np.array_equal(l, z["loc"])
            assert np.array_equal(a, z["ali"])
            buf = np.zeros(8, np.int64)
            assert lib().gac_chain_psl_counts(e.h, None, buf.ctypes.data) == GAC_E_ARG
            cs.close()
        finally:
            e.close()


# ------------------------------------------------------------------- tool
def _run_tool(args, **kw):
    return subprocess.run([_bin("chainToPsl")] + args, capture_output=True, timeout=300, **kw)


def _args(name, chain=None, out="out.psl", tmp=""):
    d, c = PS.SETS[name]
    # tSizes / qSizes: the reference never opens them; neither path exists
    return [chain or c, os.path.join(str(tmp), "no.t.sizes"), os.path.join(str(tmp), "no.q.sizes"),
            os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"), out]


@pytest.mark.parametrize("name", sorted(PS.SETS))
def test_tool_byte_identical(name, tmp_path):
    out = tmp_path / "out.psl"
    a = _args(name, out=str(out), tmp=tmp_path)
    r = _run_tool(a)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == PS.fixture(f"{name}.psl")
    assert ("Scanning %s\nScanning %s\nConverting %s\n" % (a[3], a[4], a[0])).encode() in r.stderr


def test_tool_stdin_stdout_gz_and_ignored_option(tmp_path):
    want = PS.fixture("edge.psl")
    text = open(PS.SETS["edge"][1], "rb").read()
    r = _run_tool(_args("edge", chain="stdin", out="stdout", tmp=tmp_path), input=text)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    gz = tmp_path / "in.chain.gz"
    gz.write_bytes(gzip.compress(text))
    # optionHash: an unknown option is accepted and ignored
    r = _run_tool(_args("edge", chain=str(gz), out=str(tmp_path / "o"), tmp=tmp_path) + ["-x=1"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o").read_bytes() == want


def test_tool_usage_and_aborts(tmp_path):
    a = _args("built", out=str(tmp_path / "o"), tmp=tmp_path)
    r = _run_tool(a[:5])  # argc != 7: usage, exit 255
    assert r.returncode == 255 and r.stderr.startswith(USAGE)
    r = _run_tool(a + ["extra"])
    assert r.returncode == 255 and r.stderr.startswith(USAGE)
    # a non-2bit genome
    r = _run_tool(a[:4] + [a[0]] + a[5:])
    assert r.returncode == 255 and b"2bit" in r.stderr
    tsize, qsize = 60001, 50003  # chrT2, chrQ2 of antirepeat/built
    bad = tmp_path / "bad.chain"

    def run_bad(text):
        bad.write_text(text)
        return _run_tool(_args("built", chain=str(bad), out=str(tmp_path / "o"), tmp=tmp_path))

    # a chain naming a sequence the genome does not hold (hashMustFindVal)
    r = run_bad("chain 9000 chrT2 %d + 100 150 chrNone 50003 + 100 150 7\n50\n\n" % tsize)
    assert r.returncode == 255 and b"hashMustFindVal: 'chrNone' not found" in r.stderr
    r = run_bad("chain 9000 chrNoT 60001 + 100 150 chrQ2 %d + 100 150 7\n50\n\n" % qsize)
    assert r.returncode == 255 and b"hashMustFindVal: 'chrNoT' not found" in r.stderr
    # a block past the end of its .2bit sequence (the header claims a larger size)
    r = run_bad("chain 9000 chrT2 %d + %d %d chrQ2 %d + 100 150 7\n50\n\n"
                % (tsize + 100, tsize - 10, tsize + 40, qsize))
    assert r.returncode == 255 and b"chrT2" in r.stderr
    r = run_bad("chain 9000 chrT2 %d + 100 150 chrQ2 %d + %d %d 7\n50\n\n"
                % (tsize, qsize + 100, qsize - 10, qsize + 40))
    assert r.returncode == 255 and b"chrQ2" in r.stderr
    # '-': the flipped position is checked against the .2bit size
    r = run_bad("chain 9000 chrT2 %d + 100 150 chrQ2 %d - %d %d 7\n50\n\n"
                % (tsize, qsize + 100, qsize - 10, qsize + 40))
    assert r.returncode == 255 and b"chrQ2" in r.stderr
    # the same blocks inside the sequence pass
    r = run_bad("chain 9000 chrT2 %d + 100 150 chrQ2 %d - %d %d 7\n50\n\n"
                % (tsize, qsize + 100, qsize - 50, qsize))
    assert r.returncode == 0, r.stderr
