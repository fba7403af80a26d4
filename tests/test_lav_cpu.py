"""lavToAxt and lavToPsl without a GPU: the restatement (tests/lav_ref.py)
against the reference's outputs (tests/golden/make_lav_golden.py), the two
tools -- lavToPsl, and lavToAxt on its host path, the -fa / -tfa runs of
kent's own makefile included -- against every golden and every row of the
error table, the host twin of the pair-count kernel against the restatement
on pieces over the golden genomes, and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antirepeat_ref as AR
import lav_ref as LR

CASES = LR.load_cases()
ERRORS = LR.load_errors()
AXT_CASES = sorted(k for k, c in CASES.items() if c["tool"] == "lavToAxt")
PSL_CASES = sorted(k for k, c in CASES.items() if c["tool"] == "lavToPsl")


def tool(name):
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, name)


def path(name):
    """an input file (committed, or made from the committed ones)"""
    return os.path.join(LR.inputs_dir(), name)


def gold(name):
    """what the reference wrote"""
    return os.path.join(LR.LAV_DIR, name)


def options(case, scores=""):
    return [o.replace("{dir}", LR.inputs_dir()).replace("{scores}", scores) for o in CASES[case]["options"]]


def restate(case):
    c = CASES[case]
    opts = options(case)
    data = LR.read_input(path(c["lav"]))
    if c["tool"] == "lavToPsl":
        ts = [o.split("=", 1)[1] for o in opts if o.startswith("-target-strand=")]
        return LR.to_psl(data, path(c["lav"]), ts[-1] if ts else "", "-bed" in opts)
    scheme = [LR.scheme_from_file(o.split("=", 1)[1]) for o in opts if o.startswith("-scoreScheme=")]
    return LR.to_axt(data, path(c["lav"]), LR.Seqs(path(c["t"]), "-tfa" in opts),
                     LR.Seqs(path(c["q"]), "-fa" in opts), "-dropSelf" in opts,
                     scheme[-1] if scheme else None), b""


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_reference(case):
    out, scores = restate(case)
    assert out == LR.read_input(gold(CASES[case]["output"]))
    if "scores" in CASES[case]:
        assert scores == LR.read_input(gold(CASES[case]["scores"]))


def test_goldens_hold_what_they_are_for():
    heads = lambda name: [ln.split() for ln in LR.read_input(gold(CASES[name]["output"])).split(b"\n")  # noqa: E731
                          if ln[:1].isdigit()]
    both = heads("both")
    assert {h[7] for h in both} == {b"+", b"-"} and [int(h[0]) for h in both] == list(range(len(both)))
    assert b"12345" in {h[8] for h in both} and b"2147483647" in {h[8] for h in both}
    text = LR.read_input(gold(CASES["both"]["output"]))
    assert text.startswith(b"##aligner=lastz.v1.03") and b"##matrix=lastz.v1.03 16 91,-114" in text
    assert any(c in text for c in b"acgt") and b"N" in text and b"n" in text
    # -dropSelf: more records than stanzas with blocks left, and new scores
    lav_scores = {b"11", b"12", b"13", b"14", b"15", b"16"}
    drop = heads("self_drop")
    assert len(drop) > 6 and any(h[8] not in lav_scores for h in drop) and any(h[8] == b"11" for h in drop)
    by = {n: heads(n) for n in ("self_drop", "self_drop_old", "self_drop_new")}
    assert [h[:8] for h in by["self_drop"]] == [h[:8] for h in by["self_drop_new"]]
    assert [h[8] for h in by["self_drop"]] != [h[8] for h in by["self_drop_new"]]
    # the lav's qSize flips '-' coordinates: the same blocks read other bases
    assert LR.read_input(gold(CASES["qsize"]["output"])) != b""
    # percentId products that end in .5 round away from zero
    first = [ln for ln in LR.read_input(gold(CASES["psl_both"]["output"])).split(b"\n")
             if ln[:1].isdigit()][0].split(b"\t")
    assert first[0] == b"%d" % (2 + 3 + 1 + 2 + 2)      # 1.5, 2.5, 0.5, 1.5, 1.5
    scores = LR.read_input(gold(CASES["psl_both_plus"]["scores"])).split()
    psl = [ln for ln in LR.read_input(gold(CASES["psl_both_plus"]["output"])).split(b"\n") if ln[:1].isdigit()]
    assert len(scores) == len(psl) + 1 and all(ln.split(b"\t")[8] in (b"++", b"-+") for ln in psl)


@pytest.mark.parametrize("case", PSL_CASES)
def test_lavtopsl_equals_reference(case, tmp_path):
    c = CASES[case]
    out, scores = str(tmp_path / "out"), str(tmp_path / "scores")
    r = subprocess.run([tool("lavToPsl")] + options(case, scores) + [path(c["lav"]), out], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert LR.read_input(out) == LR.read_input(gold(c["output"]))
    if "scores" in c:
        assert LR.read_input(scores) == LR.read_input(gold(c["scores"]))


@pytest.mark.parametrize("case", AXT_CASES)
def test_lavtoaxt_host_equals_reference(case, tmp_path):
    c = CASES[case]
    out = str(tmp_path / "out")
    r = subprocess.run([tool("lavToAxt"), "-host"] + options(case) + [path(c["lav"]), path(c["t"]), path(c["q"]), out],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    assert LR.read_input(out) == LR.read_input(gold(c["output"]))


def test_lavtoaxt_host_threads_and_default_path(tmp_path):
    """One thread and many give the same bytes, and so does the tool without
    -host (the default path needs no GPU)."""
    c = CASES["self_drop_new"]
    args = options("self_drop_new") + [path(c["lav"]), path(c["t"]), path(c["q"])]
    want = LR.read_input(gold(c["output"]))
    for k, (extra, threads) in enumerate(((["-host"], "1"), (["-host"], "7"), ([], "3"))):
        out = str(tmp_path / ("out%d" % k))
        r = subprocess.run([tool("lavToAxt")] + extra + args + [out], capture_output=True,
                           env=dict(os.environ, GAC_THREADS=threads))
        assert r.returncode == 0 and LR.read_input(out) == want, (extra, threads, r.stderr)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_error_rows(name, tmp_path):
    e = ERRORS[name]
    paths = {"{lav}": path(e["lav"]), "{t}": path(e["t"]), "{q}": path(e["q"]), "{out}": str(tmp_path / "out")}
    args = [paths.get(a, a) for a in e["args"]]
    if e["tool"] == "lavToAxt":
        args = ["-host"] + args
    r = subprocess.run([tool(e["tool"])] + args, capture_output=True, text=True)
    assert r.returncode == e["status"] == 255
    first = r.stderr.split("\n")[0]
    for tag, p in paths.items():
        first = first.replace(p, tag)
    assert first == e["stderr"]


@pytest.mark.parametrize("name", ["lavToAxt", "lavToPsl"])
def test_usage_text(name):
    r = subprocess.run([tool(name)], capture_output=True)
    assert r.returncode == 255 and r.stdout == b""
    assert r.stderr == LR.read_input(gold("usage_%s.txt" % name))


# ------------------------------------------------------------ the host twin
def _pieces(seed, tg, qg, n=160):
    """seeded pieces over two genomes, both strands: chains of 1..6 blocks with
    single-sided gaps, sizes from 1 to past two plane words"""
    rng = np.random.default_rng(seed)
    t_seq, q_seq, strand, off, bt, bq, bs = [], [], [], [0], [], [], []
    big = lambda g: [i for i, c in enumerate(g.codes) if len(c) >= 1000]  # noqa: E731
    for _ in range(n):
        ti, qi = int(rng.choice(big(tg))), int(rng.choice(big(qg)))
        nb = int(rng.integers(1, 7))
        sizes = rng.choice([0, 1, 2, 31, 32, 33, 64, 65, 70], nb)
        gaps = rng.integers(0, 5, nb - 1)
        side = rng.integers(0, 2, nb - 1)
        span_t = int(sizes.sum() + (gaps * side).sum()), int(sizes.sum() + (gaps * (1 - side)).sum())
        t0 = int(rng.integers(0, len(tg.codes[ti]) - span_t[0]))
        q0 = int(rng.integers(0, len(qg.codes[qi]) - span_t[1]))
        t = t0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps * side)])
        q = q0 + np.concatenate([[0], np.cumsum(sizes[:-1] + gaps * (1 - side))])
        t_seq.append(ti), q_seq.append(qi), strand.append(int(rng.integers(0, 2)))
        bt += t.tolist()
        bq += q.tolist()
        bs += sizes.tolist()
        off.append(len(bt))
    nbk = np.diff(off)
    pieces = np.stack([np.arange(n), np.zeros(n), np.zeros(n), np.zeros(n), nbk], 1).astype(np.int32)
    # and windows that are no whole chain
    sub = np.array([[c, 0, 0, 1, nbk[c] - 1] for c in range(n) if nbk[c] > 2], np.int32)
    return (np.array(t_seq, np.int32), np.array(q_seq, np.int32), np.array(strand, np.uint8),
            np.array(off, np.int64), np.array(bt, np.int32), np.array(bq, np.int32),
            np.array(bs, np.int32)), np.concatenate([pieces, sub])


@pytest.mark.parametrize("t2,q2", [("hm.2bit", "hm.2bit"), ("hg19.chrM.2bit", "crea.2bit")])
def test_host_twin_equals_restatement(t2, q2):
    from genomealignmenttools_amd.gachain import axt_pair_counts_host
    tg, qg = AR.read_2bit(path(t2)), AR.read_2bit(path(q2))
    arrs, pieces = _pieces(5, tg, qg)
    got = axt_pair_counts_host(path(t2), path(q2), *arrs, pieces)
    want = LR.pair_counts(lambda i: AR.decode_case(tg, i, 0, len(tg.codes[i])),
                          lambda i: AR.decode_case(qg, i, 0, len(qg.codes[i])), *arrs, pieces)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (want[0].sum(0) > 0).all() and (t2 != "hm.2bit" or want[1].sum() > 0)
    # the counts are the columns
    sizes = np.array([arrs[6][arrs[3][p[0]] + p[3]:arrs[3][p[0]] + p[3] + p[4]].sum() for p in pieces])
    assert np.array_equal(got[0].sum(1) + got[1], sizes)


def test_host_twin_argument_errors():
    from genomealignmenttools_amd._lib import GacError
    from genomealignmenttools_amd.gachain import axt_pair_counts_host
    one = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.array([0, 2], np.int64))
    hm = path("hm.2bit")
    ok = one + (np.array([10, 30], np.int32), np.array([10, 20], np.int32), np.array([10, 5], np.int32))
    p, n = axt_pair_counts_host(hm, hm, *ok, np.array([[0, 0, 0, 0, 2]], np.int32))
    assert p.sum() + n.sum() == 15
    with pytest.raises(GacError, match="outside its chain"):
        axt_pair_counts_host(hm, hm, *ok, np.array([[0, 0, 0, 1, 2]], np.int32))
    both = one + (np.array([10, 30], np.int32), np.array([10, 30], np.int32), np.array([10, 5], np.int32))
    with pytest.raises(GacError, match="double-sided"):
        axt_pair_counts_host(hm, hm, *both, np.array([[0, 0, 0, 0, 2]], np.int32))
    far = one + (np.array([10, 3990], np.int32), np.array([10, 20], np.int32), np.array([10, 15], np.int32))
    with pytest.raises(GacError, match="outside its sequences"):
        axt_pair_counts_host(hm, hm, *far, np.array([[0, 0, 0, 0, 2]], np.int32))
    p, n = axt_pair_counts_host(hm, hm, *ok, np.zeros((0, 5), np.int32))
    assert p.shape == (0, 16) and n.shape == (0,)


def test_gap_terms_join_runs_over_a_zero_length_block():
    bt, bq, bs = [0, 24, 24], [0, 20, 26], [20, 0, 20]
    assert LR.gap_terms(bt, bq, bs, 0, 3) == 400 + 30 * 10
    bs[1] = 1
    bq[2] += 1
    bt[2] += 1
    assert LR.gap_terms(bt, bq, bs, 0, 3) == 2 * 400 + 30 * 10


def test_abi_exports():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    assert L.gac_abi_minor() >= 10
    for name in ("gac_axt_pair_counts", "gac_axt_pair_counts_device", "gac_axt_pair_counts_host"):
        assert name in _lib.EXPORTED and isinstance(getattr(L, name), C._CFuncPtr)
    with open(os.path.join(_lib.REPO_DIR, "include", "gachain.h")) as f:
        assert "#define GAC_ABI_MINOR %d\n" % L.gac_abi_minor() in f.read()
