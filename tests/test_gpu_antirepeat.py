"""chainAntiRepeat on the GPU: the soft-mask plane, the per-chain match
composition kernel (exact integers against the numpy restatement in
tests/antirepeat_ref.py and against the fixtures made with the reference's
tool) and the drop-in tool, byte for byte."""
import gzip
import os
import subprocess

import numpy as np
import pytest
# torch before libgachain: torch ships its own copy of the ROCm runtime, and
# the GPU suite has always loaded it first (test_gpu_bench imports torch and
# used to be the first GPU module).  With libgachain's runtime initialised
# first, the later RCCL / torch / ctypes-HIP tests of the same process find
# no device; this module now sorts first, so it keeps that order itself.
import torch  # noqa: F401

from conftest import BLASTZ, GOLDEN

import antirepeat_ref as AR

pytestmark = pytest.mark.gpu

AR_DIR = os.path.join(GOLDEN, "antirepeat")
SETS = {
    "synth11": (os.path.join(GOLDEN, "synth11"), os.path.join(AR_DIR, "synth11.npz"),
                os.path.join(AR_DIR, "synth11.%s.chain")),
    "synth12": (os.path.join(GOLDEN, "synth12"), os.path.join(AR_DIR, "synth12.npz"),
                os.path.join(AR_DIR, "synth12.%s.chain")),
    "built": (os.path.join(AR_DIR, "built"), os.path.join(AR_DIR, "built", "counts.npz"),
              os.path.join(AR_DIR, "built", "%s.chain")),
}
OPTS = {"default": [], "opts": ["-minScore=1000", "-noCheckScore=20000"]}
GAC_E_ARG, GAC_E_STATE = -1, -5


def _bin(name):
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, name)


def _engine(tg, qg):
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    e = Engine(0)
    e.add_sequences(GAC_T, tg.seq_records(), mask_runs=tg.mruns)
    e.add_sequences(GAC_Q, qg.seq_records(), mask_runs=qg.mruns)
    return e


# ------------------------------------------------------------- decode_case
def _runs(*r):
    return (np.array([a for a, _ in r], np.int32), np.array([b - a for a, b in r], np.int32))


def test_decode_case_mask_edges():
    """Mask runs ending / starting at bits 0, 31 and 32 of a word, a run over
    a whole sequence, the last partial word of a sequence and the first word
    of the next one; N inside and outside runs."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T
    g = synth.random_genome({"a": 100, "b": 45, "c": 70, "d": 33, "e": 64}, 5, n_frac=0.0)
    g.mruns = [_runs((0, 1), (31, 32), (33, 34), (62, 65), (95, 100)),  # bits 0, 31, 1, 30-0, tail
               _runs((0, 45)),                                          # a whole sequence
               _runs((32, 33), (64, 70)),                               # bit 32; the last partial word
               _runs((0, 1), (32, 33)),                                 # first word after a partial one
               _runs()]                                                 # none
    g.nruns = [_runs((30, 34), (97, 99)), _runs((10, 12)), _runs((60, 66)), _runs(), _runs((5, 9))]
    e = _engine(g, g)
    try:
        for side in (GAC_T, GAC_Q):
            for i, n in enumerate(g.names):
                size = len(g.codes[i])
                want = AR.decode_case(g, i, 0, size)
                assert e.decode_case(side, i, 0, size) == want, n
                for a, b in ((0, 1), (31, 33), (size - 1, size), (size // 2, size)):
                    assert e.decode_case(side, i, a, b) == want[a:b], (n, a, b)
                assert e.decode(side, i, 0, size) == want.lower()  # the old decode is unchanged
        assert any(c.islower() for c in AR.decode_case(g, 0, 0, 100))
        assert "n" in AR.decode_case(g, 0, 0, 100) and "N" in AR.decode_case(g, 0, 0, 100)
    finally:
        e.close()


# -------------------------------------------------- composition on fixtures
@pytest.mark.parametrize("name", sorted(SETS))
def test_composition_equals_fixture(name):
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    d, npz, _ = SETS[name]
    z = np.load(npz)
    ca = read_chains(os.path.join(d, "in.chain"))
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=True)
        e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"), soft_mask=True)
        cs = AR.upload(e, ca, AR.read_2bit(os.path.join(d, "q.2bit")).sizes)
        match, rep, total = e.chain_composition(cs)
        assert np.array_equal(total, z["total"])
        assert np.array_equal(rep, z["rep"])
        assert np.array_equal(match, z["match"])
        cs.close()
    finally:
        e.close()


# -------------------------------------------------- hand-built edge shapes
def _edge_case():
    """(tg, qg, ChainArrays): the smallest shapes that reach each path of the
    kernel, '+' and '-' each."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.chainfile import ChainArrays
    tg = synth.random_genome({"t1": 200_003, "t2": 4_099}, 21, n_frac=0.01, n_mean=150, mask_frac=0.3)
    qg = synth.random_genome({"q1": 150_013, "q2": 9_001}, 22, n_frac=0.01, n_mean=150, mask_frac=0.3)
    rng = np.random.default_rng(23)
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
        chain("t2", "q2", minus, 4_099 - 40, 9_001 - 40, [40])           # the last bases of both
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
    return tg, qg, ca, AR.composition(tg, qg, ca)


def test_composition_edge_shapes(edge):
    tg, qg, ca, (wm, wr, wt) = edge
    assert wm.sum() > 0 and wr.sum() > 0 and (wr < wt).any()
    e = _engine(tg, qg)
    try:
        cs = AR.upload(e, ca, qg.sizes)
        match, rep, total = e.chain_composition(cs)
        assert np.array_equal(total, wt)
        bad = np.flatnonzero((rep != wr) | (match != wm).any(1))
        assert bad.size == 0, (bad[:10], match[bad[:3]], wm[bad[:3]], rep[bad[:3]], wr[bad[:3]])
        # the _device variant on the context's stream gives the same
        n = ca.n
        d = e.dev_alloc(n * 6 * 8)
        e.chain_composition_device(cs, d, d + n * 32, d + n * 40)
        e.synchronize()
        out = np.zeros(n * 6, np.int64)
        e.d2h(out, d)
        e.dev_free(d)
        assert np.array_equal(out[:4 * n].reshape(n, 4), match)
        assert np.array_equal(out[4 * n:5 * n], rep) and np.array_equal(out[5 * n:], total)
        cs.close()
        # an empty set: success, nothing written
        empty = e.upload_chain_arrays(*([np.zeros(0, np.int32)] * 2), np.zeros(0, np.uint8),
                                      np.zeros(1, np.int64), *([np.zeros(0, np.int32)] * 3))
        m0, r0, t0 = e.chain_composition(empty)
        assert m0.shape == (0, 4) and r0.size == 0 and t0.size == 0
        empty.close()
    finally:
        e.close()


def test_composition_errors_and_scoring_without_plane():
    """Without the opt-in a side has no plane: composition is GAC_E_STATE, and
    scoring gives the reference's sub-chain scores (subchain.npz) as before --
    as it does with the plane."""
    from genomealignmenttools_amd._lib import GacError, lib
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine, GapCosts
    d = os.path.join(GOLDEN, "synth11")
    z = np.load(os.path.join(d, "subchain.npz"))
    ca = read_chains(os.path.join(d, "in.chain"))
    for soft in (False, True):
        e = Engine(0)
        try:
            e.load_2bit(GAC_T, os.path.join(d, "t.2bit"), soft_mask=soft)
            e.load_2bit(GAC_Q, os.path.join(d, "q.2bit"))  # the query side never has it here
            e.set_scoring(np.asarray(BLASTZ, np.int32), GapCosts("loose"))
            cs = e.upload_chains(ca)
            g, l, a = e.score_ranges(cs, z["ranges"], want_local=True)
            assert np.array_equal(g, z["glob"]) and np.array_equal(l, z["loc"])
            assert np.array_equal(a, z["ali"])
            with pytest.raises(GacError) as ei:
                e.chain_composition(cs)
            assert ei.value.code == GAC_E_STATE
            with pytest.raises(GacError) as ei:
                e.decode_case(GAC_Q, 0, 0, 10)
            assert ei.value.code == GAC_E_STATE
            buf = np.zeros(8, np.int64)
            assert lib().gac_chain_composition(e.h, None, buf.ctypes.data, buf.ctypes.data,
                                               buf.ctypes.data) == GAC_E_ARG
            cs.close()
        finally:
            e.close()


# ------------------------------------------------------------------- tool
def _run_tool(args, **kw):
    return subprocess.run([_bin("chainAntiRepeat")] + args, capture_output=True, timeout=300, **kw)


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("tag", sorted(OPTS))
def test_tool_byte_identical(name, tag, tmp_path):
    d, _, exp = SETS[name]
    out = tmp_path / "out.chain"
    r = _run_tool([os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"), os.path.join(d, "in.chain"),
                   str(out)] + OPTS[tag])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(exp % tag, "rb").read()


def test_tool_stdin_stdout_gz(tmp_path):
    d, _, exp = SETS["built"]
    want = open(exp % "default", "rb").read()
    t2, q2 = os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit")
    text = open(os.path.join(d, "in.chain"), "rb").read()
    r = _run_tool([t2, q2, "stdin", "stdout"], input=text)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    gz = tmp_path / "in.chain.gz"
    gz.write_bytes(gzip.compress(text))
    r = _run_tool([t2, q2, str(gz), str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o").read_bytes() == want


def test_tool_usage_and_aborts(tmp_path):
    d, _, _ = SETS["built"]
    t2, q2 = os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit")
    r = _run_tool([t2, q2, os.path.join(d, "in.chain")])  # argc != 5: usage, exit 255
    assert r.returncode == 255
    assert b"chainAntiRepeat - Get rid of chains" in r.stderr and b"-noCheckScore=N" in r.stderr
    r = _run_tool([t2, q2, os.path.join(d, "in.chain"), str(tmp_path / "o"), "-bogus=1"])
    assert r.returncode == 255
    r = _run_tool([t2, "q.nib", os.path.join(d, "in.chain"), str(tmp_path / "o")])
    assert r.returncode == 255
    # a checked chain whose target span leaves the .2bit sequence (its header
    # claims a larger tSize): twoBitReadSeqFrag's abort
    tsize = AR.read_2bit(t2).sizes["chrT2"]
    bad = tmp_path / "bad.chain"
    bad.write_text("chain 9000 chrT2 %d + %d %d chrQ2 50003 + 100 150 7\n50\n\n"
                   % (tsize + 100, tsize - 10, tsize + 40))
    r = _run_tool([t2, q2, str(bad), str(tmp_path / "o")])
    assert r.returncode == 255
    assert b"twoBitReadSeqFrag in chrT2 end" in r.stderr
    # the same chain at or above -noCheckScore is never fetched: it passes
    r = _run_tool([t2, q2, str(bad), str(tmp_path / "o"), "-noCheckScore=9000"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o").read_text() == bad.read_text()
    # a '-' chain whose shifted query span leaves the sequence
    qsize = AR.read_2bit(q2).sizes["chrQ2"]
    bad.write_text("chain 9000 chrT2 %d + 100 150 chrQ2 %d - 10 60 7\n50\n\n" % (tsize, qsize + 100))
    r = _run_tool([t2, q2, str(bad), str(tmp_path / "o")])
    assert r.returncode == 255
    assert b"twoBitReadSeqFrag in chrQ2 end" in r.stderr
