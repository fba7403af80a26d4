"""chainToAxt on the GPU: the per-piece measure kernel and the rendering
kernel (exact against the numpy restatement in tests/axtout_ref.py, which
tests/test_axtout_cpu.py ties to the reference's output) and the drop-in
tool, byte for byte against the fixtures made with the reference's tool."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest
# torch before libgachain, for the reason written at the top of
# test_gpu_antirepeat.py: this module sorts before it
import torch  # noqa: F401

from conftest import GOLDEN

import antirepeat_ref as AR
import axtout_ref as AX

pytestmark = pytest.mark.gpu

AX_DIR = os.path.join(GOLDEN, "axtout")
SETS = {"built": os.path.join(GOLDEN, "antirepeat", "built"), "synth11": os.path.join(GOLDEN, "synth11"),
        "synth12": os.path.join(GOLDEN, "synth12")}
TOOL_OPTS = {
    "default": [],
    "opts": ["-maxGap=10", "-minId=90", "-minScore=3000"],
    "bed": ["-bed", "-minId=70"],
    "maxchain": ["-maxChain=50"],
}
TOOL_CASES = [("built", t) for t in sorted(TOOL_OPTS)] + [("synth11", "default"), ("synth12", "default")]
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


def _check(e, cs, tt, qt, ca, pieces):
    """measure and render of `pieces` against the restatement, every piece."""
    ws, wm, wa, wy = AX.measure(tt, qt, ca, pieces)
    score, match, ali, sym = e.axt_measure(cs, pieces)
    assert np.array_equal(sym, wy) and np.array_equal(ali, wa)
    bad = np.flatnonzero((score != ws) | (match != wm))
    assert bad.size == 0, (bad[:10], score[bad[:5]], ws[bad[:5]], match[bad[:5]], wm[bad[:5]])
    want, off = AX.render(tt, qt, ca, pieces)
    got = e.axt_render(cs, pieces, sym=sym)  # packed in order, offsets scanned on the device
    assert got.size == want.size
    if not np.array_equal(got, want):
        first = int(np.flatnonzero(got != want)[0])
        p = int(np.searchsorted(off, first, side="right")) - 1
        raise AssertionError((p, pieces[p].tolist(), first - int(off[p]), int(sym[p]),
                              got[first - 8:first + 24].tobytes(), want[first - 8:first + 24].tobytes()))
    return score, match, ali, sym


# ------------------------------------------------------------ the three sets
@pytest.mark.parametrize("name", sorted(SETS))
def test_measure_and_render_equal_restatement(name):
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    d = SETS[name]
    t2, q2 = os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit")
    ca = read_chains(os.path.join(d, "in.chain"))
    tt, qt = AX.Text(AR.read_2bit(t2)), AX.Text(AR.read_2bit(q2))
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, t2, soft_mask=True)
        e.load_2bit(GAC_Q, q2, soft_mask=True)
        cs = AX.upload(e, ca)
        for max_gap in (100, 10):
            pieces = AX.split(ca, max_gap)
            score, match, ali, sym = _check(e, cs, tt, qt, ca, pieces)
        assert (score < 0).any() and (score > 0).any() and (match > 0).any()
        cs.close()
    finally:
        e.close()


# -------------------------------------------------- hand-built edge shapes
def _runs(*r):
    return (np.array([a for a, _ in r], np.int32), np.array([b - a for a, b in r], np.int32))


GAPS = (1, 2, 31, 32, 33, 100, 101)
SIZES = (1, 31, 32, 33, 63, 64, 65)


def _edge_case():
    """(tg, qg, ChainArrays): the smallest shapes that reach each path of the
    two kernels, '+' and '-' each."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.chainfile import ChainArrays
    tg = synth.random_genome({"t1": 400_003, "t2": 4_099, "t3": 1_000}, 31, n_frac=0.01, n_mean=150,
                             mask_frac=0.3)
    qg = synth.random_genome({"q1": 300_013, "q2": 9_001, "q3": 1_000}, 32, n_frac=0.01, n_mean=150,
                             mask_frac=0.3)
    # half of q1 copies t1, so that matches and every matrix entry are common
    qg.codes[0][:150_000] = tg.codes[0][1_000:151_000]
    rng = np.random.default_rng(33)
    sub = rng.random(150_000) < 0.15
    qg.codes[0][:150_000][sub] = rng.integers(0, 4, int(sub.sum()))
    # runs that start and end at bits 0, 31 and 32 of a word, N inside and
    # outside mask runs, N against N
    for g in (tg, qg):
        g.mruns[2] = _runs((0, 1), (31, 32), (33, 34), (62, 65), (95, 128), (160, 161))
        g.nruns[2] = _runs((30, 34), (63, 64), (96, 97), (128, 160), (191, 193))
    rec = []

    def chain(tn, qn, minus, t0, q0, sizes, gaps=None):
        sizes = np.asarray(sizes, np.int64)
        nb = len(sizes)
        if gaps is None:  # one-sided, on either side, some abutting
            g = rng.integers(0, 6, nb - 1)
            side = rng.integers(0, 2, nb - 1)
            gaps = np.stack([g * side, g * (1 - side)], 1)
        gaps = np.asarray(gaps, np.int64).reshape(-1, 2)
        bt = t0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps[:, 0])])
        bq = q0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps[:, 1])])
        assert bt[-1] + sizes[-1] <= tg.sizes[tn] and bq[-1] + sizes[-1] <= qg.sizes[qn]
        rec.append((tn, qn, minus, bt, bq, sizes))

    for minus in (0, 1):
        for z in SIZES:                                                  # one block of each size
            chain("t1", "q1", minus, 5_000 + 97 * z, 3_000 + 89 * z, [z])
        chain("t1", "q1", minus, 20_011, 19_003, SIZES, [(2, 0), (0, 3), (0, 0), (1, 0), (0, 1), (5, 0)])
        for r in range(32):                                              # every start residue, both sides
            chain("t1", "q1", minus, 30_000 + 96 * r + r, 29_000 + 96 * r + (7 * r + 3) % 32, [40, 7],
                  [(r % 3, 0)])
        chain("t1", "q1", minus, 40_000, 39_000, [20] * (2 * len(GAPS) + 1),   # inner gaps, 101 cuts
              [(g, 0) for g in GAPS] + [(0, g) for g in GAPS])
        chain("t1", "q1", minus, 50_000, 49_000, [9, 9, 9, 9], [(3, 5), (0, 0), (0, 4)])  # double-sided, abutting
        chain("t3", "q3", minus, 0, 0, [200])                            # the word-edge runs, whole
        chain("t3", "q3", minus, 29, 27, [5, 30, 40, 60], [(0, 1), (31, 0), (0, 33)])
        chain("t3", "q3", minus, 500, 500, [100], None)
        chain("t2", "q2", minus, 4_099 - 40, 9_001 - 40, [40])           # the last bases of both, then t3 / q3
        chain("t2", "q2", minus, 0, 0, [33, 10], [(0, 2)])               # and the first
        chain("t1", "q1", minus, 60_000, 59_000, rng.integers(1, 41, 200))   # 200 blocks in one piece
        chain("t1", "q1", minus, 200_001, 100_007, [100_000])            # one long block
        for k in range(300):                                             # one-base single-block chains
            chain("t1", "q1", minus, int(rng.integers(0, 150_000)), int(rng.integers(0, 150_000)), [1])
        for nb in (63, 64, 65, 300):                                     # lane / tile / workgroup edges
            chain("t1", "q1", minus, int(rng.integers(0, 100_000)), int(rng.integers(0, 100_000)),
                  rng.integers(1, 80, nb))
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
    tt, qt = AX.Text(tg), AX.Text(qg)
    pieces = AX.split(ca, 100)
    return tg, qg, ca, tt, qt, pieces


def test_edge_shapes(edge):
    tg, qg, ca, tt, qt, pieces = edge
    nblk = pieces[:, 4]
    assert (nblk == 200).any() and (nblk == 1).sum() >= 600 and len(pieces) > ca.n
    e = _engine(tg, qg)
    try:
        cs = AX.upload(e, ca)
        z = np.zeros(ca.n, np.int32)
        assert np.array_equal(e.axt_split(z, z, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q,
                                          ca.blk_size, 100), pieces)
        score, match, ali, sym = _check(e, cs, tt, qt, ca, pieces)
        assert (match == ali).any() and (match == 0).any() and sym.max() >= 100_000
        # windows in another order than the set's, and single blocks that are
        # no pieces of the split
        _check(e, cs, tt, qt, ca, pieces[::-1].copy())
        c = int(np.flatnonzero(np.diff(ca.blk_off) == 200)[0])
        ones = np.array([[c, 0, 0, k, 1] for k in range(0, 200, 7)], np.int32)
        _check(e, cs, tt, qt, ca, ones)
        # the _device variants on the context's stream give the same
        n = len(pieces)
        w = np.ascontiguousarray(pieces, np.int32)
        d_w = e.dev_alloc(n * 20)
        d_r = e.dev_alloc(n * 32)
        e.h2d(d_w, w)
        e.axt_measure_device(cs, d_w, n, d_r, d_r + 8 * n, d_r + 16 * n, d_r + 24 * n)
        e.synchronize()
        out = np.zeros(4 * n, np.int64)
        e.d2h(out, d_r)
        assert np.array_equal(out[:n].view(np.int32)[:n], score)
        assert np.array_equal(out[n:2 * n], match) and np.array_equal(out[2 * n:3 * n], ali)
        assert np.array_equal(out[3 * n:], sym)
        want, _ = AX.render(tt, qt, ca, pieces)
        d_t = e.dev_alloc(want.size + 16)
        e.axt_render_device(cs, d_w, n, 0, d_t + 5, want.size)  # a text buffer that is not aligned
        e.synchronize()
        got = np.zeros(want.size + 16, np.uint8)
        e.d2h(got, d_t)
        assert np.array_equal(got[5:5 + want.size], want)
        for p in (d_w, d_r, d_t):
            e.dev_free(p)
        # no pieces, and an empty set: success, nothing written
        none = np.zeros((0, 5), np.int32)
        assert all(a.size == 0 for a in e.axt_measure(cs, none))
        buf = np.full(64, 0xEE, np.uint8)
        e.axt_render(cs, none, out=buf)
        assert (buf == 0xEE).all()
        cs.close()
        empty = e.upload_chain_arrays(*([np.zeros(0, np.int32)] * 2), np.zeros(0, np.uint8),
                                      np.zeros(1, np.int64), *([np.zeros(0, np.int32)] * 3))
        assert all(a.size == 0 for a in e.axt_measure(empty, none))
        e.axt_render(empty, none, out=buf)
        assert (buf == 0xEE).all()
        empty.close()
    finally:
        e.close()


def test_render_touches_only_its_rows(edge):
    """Rows starting at every residue mod 16 in a buffer of 0xEE: every byte
    outside the rows and their line ends keeps its value (the single-byte
    stores at the head and tail of a run)."""
    tg, qg, ca, tt, qt, pieces = edge
    # short and long pieces, with and without gaps, both strands
    nblk = pieces[:, 4]
    pick = np.concatenate([np.flatnonzero(nblk == 1)[:40], np.flatnonzero(nblk == 1)[-40:],
                           np.flatnonzero(nblk > 1)])
    sel = pieces[pick]
    sym = AX.measure(tt, qt, ca, sel)[3]
    off = np.zeros(len(sel), np.int64)
    cur = 3
    for i in range(len(sel)):
        cur += (i - cur) % 16 + 16 * (i % 3)  # start residue i mod 16, gaps of 0..47 bytes
        off[i] = cur
        cur += 2 * int(sym[i]) + 3
    assert set(off % 16) == set(range(16)) and len(set((off + sym + 1) % 16)) == 16
    size = cur + 37
    want = np.full(size, 0xEE, np.uint8)
    AX.render(tt, qt, ca, sel, off, want)
    e = _engine(tg, qg)
    try:
        cs = AX.upload(e, ca)
        got = e.axt_render(cs, sel, offsets=off, out=np.full(size, 0xEE, np.uint8))
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        cs.close()
    finally:
        e.close()


def test_errors(edge):
    from genomealignmenttools_amd._lib import GacError, lib
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    tg, qg, ca, tt, qt, pieces = edge
    few = pieces[:50]
    sym = AX.measure(tt, qt, ca, few)[3]
    need = int((2 * sym + 3).sum())
    e = _engine(tg, qg)
    try:
        cs = AX.upload(e, ca)
        # rows that pass out_bytes: refused, nothing written
        buf = np.full(need, 0xEE, np.uint8)
        with pytest.raises(GacError) as ei:
            e.axt_render(cs, few, out=buf[:need - 1])
        assert ei.value.code == GAC_E_ARG and (buf == 0xEE).all()
        off = np.concatenate([[0], np.cumsum(2 * sym + 3)[:-1]]).astype(np.int64)
        off[7] = need - 2
        with pytest.raises(GacError) as ei:
            e.axt_render(cs, few, offsets=off, out=buf)
        assert ei.value.code == GAC_E_ARG and (buf == 0xEE).all()
        e.axt_render(cs, few, out=buf)  # exactly enough: fine
        assert np.array_equal(buf, AX.render(tt, qt, ca, few)[0])
        # a window outside its chain, a chain out of range
        for bad in ((0, 0, 0, 0, int(ca.blk_off[1] - ca.blk_off[0]) + 1), (0, 0, 0, -1, 1),
                    (ca.n, 0, 0, 0, 1), (-1, 0, 0, 0, 1)):
            w = np.concatenate([few[:3], np.array([bad], np.int32), few[3:6]])
            for fn in (lambda: e.axt_measure(cs, w), lambda: e.axt_render(cs, w, out=buf.copy())):
                with pytest.raises(GacError) as ei:
                    fn()
                assert ei.value.code == GAC_E_ARG
        # a double-sided gap inside a window: not a piece
        c = int(np.flatnonzero(np.diff(ca.blk_off) == 4)[0])
        with pytest.raises(GacError) as ei:
            e.axt_measure(cs, np.array([[c, 0, 0, 0, 4]], np.int32))
        assert ei.value.code == GAC_E_ARG
        # a NULL set
        p = buf.ctypes.data
        assert lib().gac_axt_measure(e.h, None, p, 1, p, p, p, p) == GAC_E_ARG
        assert lib().gac_axt_render(e.h, None, p, 1, None, p, 8) == GAC_E_ARG
        cs.close()
    finally:
        e.close()
    # without the soft-mask plane on one side: GAC_E_STATE
    e = Engine(0)
    try:
        e.add_sequences(GAC_T, tg.seq_records(), mask_runs=tg.mruns)
        e.add_sequences(GAC_Q, qg.seq_records())
        cs = AX.upload(e, ca)
        with pytest.raises(GacError) as ei:
            e.axt_measure(cs, few)
        assert ei.value.code == GAC_E_STATE
        with pytest.raises(GacError) as ei:
            e.axt_render(cs, few, out=np.zeros(need, np.uint8))
        assert ei.value.code == GAC_E_STATE
        cs.close()
    finally:
        e.close()


# ------------------------------------------------------------------- tool
def _run_tool(args, env=None):
    return subprocess.run([_bin("chainToAxt")] + args, capture_output=True, timeout=300,
                          env=dict(os.environ, **(env or {})))


def _golden(name, tag):
    return gzip.open(os.path.join(AX_DIR, f"{name}.{tag}.gz"), "rb").read()


@pytest.mark.parametrize("name,tag", TOOL_CASES)
def test_tool_byte_identical(name, tag, tmp_path):
    d = SETS[name]
    out = tmp_path / "out.axt"
    r = _run_tool([os.path.join(d, "in.chain"), os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"),
                   str(out)] + TOOL_OPTS[tag])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == _golden(name, tag)


def test_tool_small_batches(tmp_path):
    """GAC_AXT_BUDGET forces the text of `built` through many batches of the
    two alternating render jobs; a budget below the largest piece too."""
    d = SETS["built"]
    args = [os.path.join(d, "in.chain"), os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit")]
    want = _golden("built", "default")
    for budget, least in (("60000", 3), ("100", 1000)):
        out = tmp_path / f"out{budget}.axt"
        r = _run_tool(args + [str(out), "-verbose=2"], env={"GAC_AXT_BUDGET": budget})
        assert r.returncode == 0, r.stderr
        m = re.search(rb"(\d+) pieces in (\d+) batches", r.stderr)
        assert m and int(m.group(1)) == 1594 and int(m.group(2)) >= least, r.stderr
        assert out.read_bytes() == want


def test_tool_usage_and_aborts(tmp_path):
    d = SETS["built"]
    chain, t2, q2 = (os.path.join(d, f) for f in ("in.chain", "t.2bit", "q.2bit"))
    r = _run_tool([chain, t2, q2])  # argc != 5: usage, exit 255
    assert r.returncode == 255
    assert b"chainToAxt - Convert from chain to axt file" in r.stderr
    assert b"default 100\n" in r.stderr and b"default 1073741823\n" in r.stderr
    r = _run_tool([chain, t2, q2, str(tmp_path / "o"), "extra"])
    assert r.returncode == 255
    r = _run_tool([chain, t2, q2, str(tmp_path / "o"), "-bogus=1"])
    assert r.returncode == 255
    r = _run_tool([chain, t2, "q.nib", str(tmp_path / "o")])
    assert r.returncode == 255
    # overlapping blocks (a negative gap): refused with the chain's id
    bad = tmp_path / "bad.chain"
    bad.write_text("chain 9000 chrT2 60001 + 100 170 chrQ2 50003 + 100 165 77\n50\t0\t-5\n20\n\n")
    r = _run_tool([str(bad), t2, q2, str(tmp_path / "o")])
    assert r.returncode == 255 and b"chain 77" in r.stderr
