"""The lav front end on the GPU: the per-piece letter-pair count kernel
(k_axt_pairs, exact against the plain restatement in tests/lav_ref.py over
Engine.decode, and tied to k_axt_stat by two identities) and lavToAxt
-device, byte for byte against the fixtures made with the reference's tool."""
import os
import subprocess

import numpy as np
import pytest
# torch before libgachain, for the reason written at the top of
# test_gpu_antirepeat.py
import torch  # noqa: F401

from conftest import GOLDEN

import lav_ref as LR

pytestmark = pytest.mark.gpu

LAV_DIR = os.path.join(GOLDEN, "lav")
SIZES = (1, 31, 32, 33, 64, 65, 2049)   # 2049: 65 chunks, the chunk loop's second turn
PHASES = (0, 1, 31)
PIECE_BLOCKS = (1, 63, 64, 65, 257)     # a piece inside a wave, across waves, across workgroups


def _runs(*r):
    return (np.array([a for a, _ in r], np.int32), np.array([b - a for a, b in r], np.int32))


def _case():
    """(tg, qg, ChainArrays): a small seeded genome pair and the chains whose
    whole block lists are the pieces under test."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.chainfile import ChainArrays
    tg = synth.random_genome({"t1": 90_001, "t3": 1_000}, 71, n_frac=0.01, n_mean=60, mask_frac=0.2)
    qg = synth.random_genome({"q1": 80_003, "q3": 1_000}, 72, n_frac=0.01, n_mean=60, mask_frac=0.2)
    # part of q1 copies t1 with substitutions, so that every pair is common
    rng = np.random.default_rng(73)
    qg.codes[0][:40_000] = tg.codes[0][512:40_512]
    sub = rng.random(40_000) < 0.25
    qg.codes[0][:40_000][sub] = rng.integers(0, 4, int(sub.sum()))
    # N runs that end at word edges: on one side only, and on both at once
    tg.nruns[1] = _runs((30, 32), (60, 64), (96, 128), (191, 193), (300, 320))
    qg.nruns[1] = _runs((62, 64), (100, 101), (160, 192), (310, 352))
    for g in (tg, qg):
        for a, z in zip(*g.nruns[1]):
            g.codes[1][a:a + z] = 0
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
        k = 0
        for z in SIZES:
            for pt in PHASES:
                for pq in PHASES:   # (on '-' the forward window's phase follows from q1's size)
                    chain("t1", "q1", minus, 832 + 2_240 * (k % 16) + pt, 320 + 2_240 * (k % 16) + pq, [z])
                    k += 1
        chain("t3", "q3", minus, 0, 0, [400])                      # every N run, whole
        chain("t3", "q3", minus, 29, 27, [5, 30, 40, 60], [(0, 1), (31, 0), (0, 33)])
        chain("t3", "q3", minus, 1_000 - 40, 1_000 - 40, [40])     # the last bases of both
        for nb in PIECE_BLOCKS:
            chain("t1", "q1", minus, int(rng.integers(0, 30_000)), int(rng.integers(0, 30_000)),
                  rng.integers(1, 41, nb))
        chain("t1", "q1", minus, 41_000, 41_000, [7, 0, 9, 0, 0, 5],  # zero-length blocks inside
              [(2, 0), (0, 3), (0, 0), (4, 0), (0, 1)])
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


class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx():
    """One engine, one uploaded set, the decoded text and the reference counts
    of every whole-chain piece, shared by the tests below (read only)."""
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    tg, qg, ca = _case()
    e = Engine(0)
    e.add_sequences(GAC_T, tg.seq_records(), mask_runs=tg.mruns)
    e.add_sequences(GAC_Q, qg.seq_records(), mask_runs=qg.mruns)
    c = _Ctx()
    c.e, c.ca = e, ca
    c.tidx = np.array([e.seq_index(GAC_T, n) for n in ca.tname], np.int32)
    c.qidx = np.array([e.seq_index(GAC_Q, n) for n in ca.qname], np.int32)
    c.cs = e.upload_chain_arrays(c.tidx, c.qidx, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q,
                                 ca.blk_size)
    ttxt = {i: e.decode(GAC_T, i, 0, e.seq_size(GAC_T, i)) for i in set(c.tidx.tolist())}
    qtxt = {i: e.decode(GAC_Q, i, 0, e.seq_size(GAC_Q, i)) for i in set(c.qidx.tolist())}
    c.ref = lambda pieces: LR.pair_counts(ttxt.__getitem__, qtxt.__getitem__, c.tidx, c.qidx,
                                          ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q, ca.blk_size,
                                          pieces)
    nb = np.diff(ca.blk_off)
    c.whole = np.stack([np.arange(ca.n), ca.tstart, ca.tend, np.zeros(ca.n, np.int64), nb],
                       1).astype(np.int32)
    c.want = c.ref(c.whole)
    yield c
    c.cs.close()
    e.close()


def _same(got, want, pieces):
    pairs, ncols = got
    wp, wn = want
    bad = np.flatnonzero((pairs != wp).any(1) | (ncols != wn))
    assert bad.size == 0, (bad[:10], pieces[bad[:3]].tolist(), pairs[bad[:3]].tolist(),
                           wp[bad[:3]].tolist(), ncols[bad[:3]], wn[bad[:3]])


def test_pair_counts_equal_restatement(ctx):
    wp, wn = ctx.want
    # the case holds what it is meant to: every pair, N on one side and both,
    # both strands, the block counts and the long block
    assert (wp.sum(0) > 0).all() and (wn > 0).any()
    assert set(PIECE_BLOCKS) <= set(ctx.whole[:, 4].tolist())
    assert (ctx.ca.blk_size == 2049).sum() == 18 and set(ctx.ca.qstrand.tolist()) == {0, 1}
    _same(ctx.e.axt_pair_counts(ctx.cs, ctx.whole), ctx.want, ctx.whole)
    # another order than the set's
    rev = ctx.whole[::-1].copy()
    _same(ctx.e.axt_pair_counts(ctx.cs, rev), (wp[::-1], wn[::-1]), rev)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_one_block_pieces(ctx, n):
    """n pieces of one block each: the last workgroup's slots full, one short
    and one over."""
    for minus in (0, 1):
        c = int(np.flatnonzero((np.diff(ctx.ca.blk_off) == 257) & (ctx.ca.qstrand == minus))[0])
        ones = np.array([[c, 0, 0, k, 1] for k in range(n)], np.int32)
        _same(ctx.e.axt_pair_counts(ctx.cs, ones), ctx.ref(ones), ones)


def test_no_pieces_writes_nothing(ctx):
    import ctypes as C
    from genomealignmenttools_amd._lib import lib
    e = ctx.e
    pairs = np.full(16, -7, np.int64)
    ncols = np.full(1, -7, np.int64)
    w = np.zeros((1, 5), np.int32)
    rc = lib().gac_axt_pair_counts(e.h, ctx.cs.handle, C.c_void_p(w.ctypes.data), 0,
                                   C.c_void_p(pairs.ctypes.data), C.c_void_p(ncols.ctypes.data))
    assert rc == 0 and (pairs == -7).all() and (ncols == -7).all()
    d = e.dev_alloc(17 * 8 + 32)
    e.h2d(d, np.concatenate([pairs, ncols]))
    e.axt_pair_counts_device(ctx.cs, d + 17 * 8, 0, d, d + 16 * 8)
    e.synchronize()
    back = np.zeros(17, np.int64)
    e.d2h(back, d)
    e.dev_free(d)
    assert (back == -7).all()
    p, c = e.axt_pair_counts(ctx.cs, np.zeros((0, 5), np.int32))
    assert p.shape == (0, 16) and c.shape == (0,)


def test_identities_with_measure(ctx):
    """Against k_axt_stat on the same pieces: the pairs and the N columns are
    the columns without a dash, and the default matrix over the pairs minus
    the gap terms is its score."""
    from genomealignmenttools_amd.gachain import read_score_scheme
    ca = ctx.ca
    pairs, ncols = ctx.e.axt_pair_counts(ctx.cs, ctx.whole)
    score, match, ali, sym = ctx.e.axt_measure(ctx.cs, ctx.whole)
    assert np.array_equal(pairs.sum(1) + ncols, ali)
    mat, go, ge, _ = read_score_scheme(None)
    assert (go, ge) == (400, 30)
    letters = pairs @ mat.reshape(16).astype(np.int64)
    gaps = np.array([LR.gap_terms(ca.blk_t, ca.blk_q, ca.blk_size, int(ca.blk_off[c]), int(nb))
                     for c, nb in zip(ctx.whole[:, 0], ctx.whole[:, 4])], np.int64)
    # (k_axt_stat opens a run per block with a gap before it: the same thing
    # wherever no zero-length block lies between two gaps)
    plain = np.array([(ca.blk_size[ca.blk_off[c]:ca.blk_off[c + 1]] > 0).all() for c in ctx.whole[:, 0]])
    assert plain.sum() == len(plain) - 2
    want = (letters - gaps).astype(np.int32)
    assert np.array_equal(score[plain], want[plain])
    # match counts N against N too: equal where no column holds an N
    same = np.diagonal(pairs.reshape(-1, 4, 4), axis1=1, axis2=2).sum(1)
    assert (same <= match).all() and np.array_equal(same[ncols == 0], match[ncols == 0])


def test_device_form_agrees(ctx):
    e = ctx.e
    n = len(ctx.whole)
    d_w = e.dev_alloc(n * 20)
    d_r = e.dev_alloc(n * 17 * 8)
    e.h2d(d_w, ctx.whole)
    e.h2d(d_r, np.full(n * 17, 0x5A5A, np.int64))  # (the call zeroes its results itself)
    e.axt_pair_counts_device(ctx.cs, d_w, n, d_r, d_r + n * 16 * 8)
    e.synchronize()
    out = np.zeros(n * 17, np.int64)
    e.d2h(out, d_r)
    e.dev_free(d_w)
    e.dev_free(d_r)
    _same((out[:n * 16].reshape(n, 16), out[n * 16:]), ctx.want, ctx.whole)


def test_argument_errors(ctx):
    from genomealignmenttools_amd._lib import GacError
    from genomealignmenttools_amd.gachain import GAC_T, Engine
    nb = int(ctx.whole[0, 4])
    with pytest.raises(GacError, match="outside its chain"):
        ctx.e.axt_pair_counts(ctx.cs, np.array([[0, 0, 0, 0, nb + 1]], np.int32))
    with pytest.raises(GacError, match="outside its chain"):
        ctx.e.axt_pair_counts(ctx.cs, np.array([[ctx.ca.n, 0, 0, 0, 1]], np.int32))
    e2 = Engine(0)
    try:
        with pytest.raises(GacError, match="orphaned"):
            e2.axt_pair_counts(ctx.cs, ctx.whole[:1])
    finally:
        e2.close()


# ------------------------------------------------------------------ the tool
def _bin(name):
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, name)


CASES = LR.load_cases()
DEVICE_CASES = sorted(k for k, c in CASES.items() if c["tool"] == "lavToAxt" and
                      not {"-fa", "-tfa"} & set(c["options"]))


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_lavtoaxt_device_equals_reference(case, tmp_path):
    c = CASES[case]
    IN = LR.inputs_dir()
    opts = [o.replace("{dir}", IN) for o in c["options"]]
    out = str(tmp_path / "out.axt")
    r = subprocess.run([_bin("lavToAxt"), "-device"] + opts +
                       [os.path.join(IN, c["lav"]), os.path.join(IN, c["t"]),
                        os.path.join(IN, c["q"]), out], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert LR.read_input(out) == LR.read_input(os.path.join(LAV_DIR, c["output"]))


def test_device_cases_cover_dropself():
    assert {"self_drop", "self_drop_old", "self_drop_new", "both", "qsize", "crea_2bit"} <= set(DEVICE_CASES)


def test_lavtoaxt_device_error_row(tmp_path):
    """the checks in front of the device path are the host path's"""
    e = LR.load_errors()["axt_outside_q"]
    IN = LR.inputs_dir()
    paths = {"{lav}": os.path.join(IN, e["lav"]), "{t}": os.path.join(IN, e["t"]),
             "{q}": os.path.join(IN, e["q"]), "{out}": str(tmp_path / "out")}
    r = subprocess.run([_bin("lavToAxt"), "-device"] + [paths.get(a, a) for a in e["args"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and r.stderr.split("\n")[0] == e["stderr"]


def test_lav_of_chain_pieces_gives_chaintoaxt_rows(tmp_path):
    """A .lav written from the pieces gac_axt_split makes of a synthetic chain
    file renders exactly the rows chainToAxt renders for that file."""
    import antirepeat_ref as AR
    import axtout_ref as AX
    from genomealignmenttools_amd.chainfile import read_chains
    d = os.path.join(GOLDEN, "synth11")
    t2, q2 = os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit")
    ca = read_chains(os.path.join(d, "in.chain"))
    pieces = AX.split(ca, 100)
    pieces = pieces[ca.score[pieces[:, 0]] >= 0]   # chainToAxt's -minScore default drops the others
    assert len(pieces) > ca.n and set(ca.qstrand[pieces[:, 0]].tolist()) == {0, 1}
    lav = str(tmp_path / "pieces.lav")
    with open(lav, "wb") as f:
        f.write(LR.lav_from_pieces(ca, pieces, AR.read_2bit(t2).sizes, AR.read_2bit(q2).sizes))
    got, want = str(tmp_path / "lav.axt"), str(tmp_path / "chain.axt")
    for args in ([_bin("lavToAxt"), "-device", lav, t2, q2, got],
                 [_bin("chainToAxt"), os.path.join(d, "in.chain"), t2, q2, want]):
        r = subprocess.run(args, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
    a, b = LR.read_input(got).split(b"\n"), LR.read_input(want).split(b"\n")
    assert len(a) == len(b) == 4 * len(pieces) + 1
    # header lines but for the score, which is the lav's there; both rows
    assert [ln.rsplit(b" ", 1)[0] for ln in a[0::4]] == [ln.rsplit(b" ", 1)[0] for ln in b[0::4]]
    assert a[1::4] == b[1::4] and a[2::4] == b[2::4]
