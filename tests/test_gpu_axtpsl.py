"""axtToPsl on the GPU: Engine.axt_psl (gac_axt_psl: a wave walks an entry in
tiles of GAC_AXTPSL_TILE columns, counts and blocks from prefix scans over
the columns' kinds) against the restatement (tests/axtpsl_ref.py) and the
host twin -- entry lengths at every tile edge with patterns that carry state
over the edges, the goldens' entries, the random rows, rows kept apart,
batches and the byte budget -- and bin/axtToPsl -device byte for byte against
the reference's outputs.  Every comparison is exact."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import axtpsl_ref as AR
from test_axtpsl_cpu import assert_equals_restatement

pytestmark = pytest.mark.gpu

CASES = AR.load_cases()
T = 512  # checked against the exported constant below
LENGTHS = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5)


def _host(t_rows, q_rows):
    from genomealignmenttools_amd.gachain import axt_psl_host
    return axt_psl_host(t_rows, q_rows)


def _with_runs(L, kind, r):
    """aligned rows of L columns with a run of `kind` ('q' query-only, 't'
    target-only, 'b' both-gap) across every tile edge (and one in the middle
    of an entry shorter than a tile); the runs' lengths vary"""
    t = [r.choice("ACGT") for _ in range(L)]
    q = list(t)
    edges = list(range(T, L, T)) or [L // 2]
    for e in edges:
        a, b = max(0, e - r.randint(1, 5)), min(L, e + r.randint(1, 5))
        for j in range(a, b):
            if kind in "qb":
                t[j] = "-"
            if kind in "tb":
                q[j] = "-"
    return "".join(t), "".join(q)


def patterns(L, r):
    """{name: (target row, query row)} of L columns"""
    out = {}
    base = "".join(r.choice("ACGT") for _ in range(L))
    out["aligned"] = (base, base)
    # a gap every other column, the sides taking turns: the most blocks a length allows
    out["alternate"] = ("".join(c if j % 2 == 0 or j % 4 == 1 else "-" for j, c in enumerate(base)),
                        "".join(c if j % 2 == 0 or j % 4 == 3 else "-" for j, c in enumerate(base)))
    for kind in "qtb":
        out["runs_" + kind] = _with_runs(L, kind, r)
    # an insert, then a whole tile (and more) of both-gap columns, then an aligned run: the
    # previous column's kind crosses a tile that has nothing
    # (from 2 T + 1 columns on the hole covers whole tiles)
    if L >= 12:
        hole, a = L - 4, 1
        t = list(base)
        q = list(base)
        q[a] = q[a + 1] = "-"                       # a target insert
        for j in range(a + 2, a + 2 + hole):
            t[j] = q[j] = "."
        out["hole_after_t_insert"] = ("".join(t), "".join(q))
        t2, q2 = list(t), list(base)
        t2[a] = t2[a + 1] = "_"                     # a query insert
        for j in range(a + 2, a + 2 + hole):
            q2[j] = "="
        out["hole_after_q_insert"] = ("".join(t2), "".join(q2))
        t3, q3 = list(base), list(base)
        for j in range(a + 2, a + 2 + hole):       # inside an aligned run: one block
            t3[j] = q3[j] = "-"
        out["hole_in_a_block"] = ("".join(t3), "".join(q3))
    # head and tail trims longer than a tile (of what fits), one-sided columns of both
    # kinds with both-gap columns among them
    h = min(T + 3, L // 3)
    t, q = list(base), list(base)
    for j in list(range(h)) + list(range(L - h, L)):
        k = r.choice("qqttb")
        if k in "qb":
            t[j] = "-"
        if k in "tb":
            q[j] = "-"
    out["long_trims"] = ("".join(t), "".join(q))
    t = [r.choice("ACGT-_") for _ in range(L)]
    q = ["-" if c in "ACGT" else r.choice("ACGT=") for c in t]   # never a column without a gap
    out["gaps_only"] = ("".join(t), "".join(q))
    out["both_gaps_only"] = ("-" * L, "." * L)
    t = "".join(r.choice("ACGTacgtNn") for _ in range(L))
    q = "".join(c if r.random() < 0.5 else r.choice("ACGTacgtNn") for c in t)
    out["case_and_n"] = (t, q)
    return out


@pytest.fixture(scope="module")
def edge_rows():
    """every pattern at every length, and the restatement's results, computed once"""
    r = random.Random(512)
    names, t_rows, q_rows = [], [], []
    for L in LENGTHS:
        for name, (t, q) in patterns(L, r).items():
            assert len(t) == len(q) == L, (name, L)
            names.append((L, name))
            t_rows.append(t)
            q_rows.append(q)
    return names, t_rows, q_rows, AR.results(t_rows, q_rows)


@pytest.fixture(scope="module")
def random_expected():
    t_rows, q_rows = AR.random_rows()
    return t_rows, q_rows, AR.results(t_rows, q_rows)


@pytest.fixture
def batch_bytes():
    """the text budget of a batch, for one test"""
    old = os.environ.get("GAC_AXTPSL_BATCH_BYTES")

    def set_(v):
        os.environ["GAC_AXTPSL_BATCH_BYTES"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("GAC_AXTPSL_BATCH_BYTES", None)
    else:
        os.environ["GAC_AXTPSL_BATCH_BYTES"] = old


def test_tile_constant():
    from genomealignmenttools_amd import _lib
    assert _lib.GAC_AXTPSL_TILE == T


def test_patterns_are_what_they_claim(edge_rows):
    names, _t, _q, want = edge_rows
    by = {k: w for k, w in zip(names, want)}
    assert len(by[(3 * T + 5, "alternate")][3]) >= (3 * T + 5) // 2 - 1
    assert by[(2 * T, "long_trims")][1][0] + by[(2 * T, "long_trims")][1][1] > T // 2
    assert by[(T + 1, "gaps_only")][2] == 0 and len(by[(T + 1, "gaps_only")][3]) == 1
    assert len(by[(2 * T + 1, "hole_in_a_block")][3]) == 1
    assert by[(2 * T + 1, "hole_after_t_insert")][0][6] == 1 and len(by[(2 * T + 1, "hole_after_t_insert")][3]) == 2
    assert len(by[(3 * T + 5, "runs_q")][3]) >= 3 and len(by[(3 * T + 5, "runs_b")][3]) == 1


def test_every_length_and_pattern(engine, edge_rows):
    names, t_rows, q_rows, want = edge_rows
    entries, blocks, st = engine.axt_psl(t_rows, q_rows)
    assert st["fell_back"] == 0 and st["batches"] == 1 and st["host_entries"] == 0
    # entry by entry first, so that a failure names its length and pattern
    for i, (counts, trims, cols, blks) in enumerate(want):
        e = entries[i]
        got = ([int(e[f]) for f in ("match", "mis_match", "rep_match", "n_count", "q_num_insert",
                                    "q_base_insert", "t_num_insert", "t_base_insert")],
               tuple(int(e[f]) for f in ("q_head", "t_head", "q_tail", "t_tail")), int(e["cols"]),
               [tuple(b) for b in blocks[int(e["block0"]):int(e["block0"]) + int(e["n_blocks"])].tolist()])
        assert got == (counts, trims, cols, blks), names[i]
    assert_equals_restatement(entries, blocks, want)
    h_entries, h_blocks, _ = _host(t_rows, q_rows)
    assert np.array_equal(entries, h_entries) and np.array_equal(blocks, h_blocks)


def test_goldens_entries(engine):
    t_rows, q_rows = AR.golden_rows()
    entries, blocks, _st = engine.axt_psl(t_rows, q_rows)
    assert_equals_restatement(entries, blocks, AR.results(t_rows, q_rows))


def test_random_rows(engine, random_expected):
    t_rows, q_rows, want = random_expected
    entries, blocks, st = engine.axt_psl(t_rows, q_rows)
    assert_equals_restatement(entries, blocks, want)
    assert st["blocks"] == len(blocks) and st["columns"] == sum(len(t) for t in t_rows)
    h_entries, h_blocks, _ = _host(t_rows, q_rows)
    assert np.array_equal(entries, h_entries) and np.array_equal(blocks, h_blocks)


def test_sides_kept_apart(engine, random_expected):
    """a caller's text with every target row before every query row: two spans"""
    from genomealignmenttools_amd import _lib
    from genomealignmenttools_amd.gachain import _axt_psl_result, _p
    t_rows, q_rows, want = random_expected
    ln = np.array([len(q) for q in q_rows], np.int32)
    off = np.concatenate([[0], np.cumsum(ln.astype(np.int64))[:-1]]).astype(np.int64)
    t_off = off.copy()
    q_off = (int(ln.sum()) + 1000 + off).astype(np.int64)
    text = ("".join(t_rows) + "#" * 1000 + "".join(q_rows)).encode()
    res = C.POINTER(_lib.AxtPslResult)()
    st = _lib.AxtPslStats()
    _lib.check(_lib.lib().gac_axt_psl(engine.h, len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                      C.byref(res), C.byref(st)))
    entries, blocks, stats = _axt_psl_result(res, st)
    assert_equals_restatement(entries, blocks, want)
    assert stats["fell_back"] == 0 and stats["batches"] == 1


def test_batches_and_the_byte_budget(engine, random_expected, batch_bytes):
    t_rows, q_rows, want = random_expected
    batch_bytes(20000)
    entries, blocks, st = engine.axt_psl(t_rows, q_rows)
    assert st["batches"] >= 3 and st["fell_back"] == 0 and st["host_entries"] == 0
    assert_equals_restatement(entries, blocks, want)
    # one entry alone over the budget goes to the host twin, the others stay
    big_t = "ACGT--ACgtNa" * 2000
    big_q = "AC-TTGACGTnA" * 2000
    t2 = t_rows[:200] + [big_t] + t_rows[200:]
    q2 = q_rows[:200] + [big_q] + q_rows[200:]
    entries, blocks, st = engine.axt_psl(t2, q2)
    assert st["fell_back"] == 2 and st["host_entries"] == 1 and st["batches"] >= 3
    assert_equals_restatement(entries, blocks, want[:200] + AR.results([big_t], [big_q]) + want[200:])
    # and when it is the first or the last entry, or the only one
    for t3, q3, w3 in (([big_t] + t_rows[:50], [big_q] + q_rows[:50], AR.results([big_t], [big_q]) + want[:50]),
                       (t_rows[:50] + [big_t], q_rows[:50] + [big_q], want[:50] + AR.results([big_t], [big_q])),
                       ([big_t], [big_q], AR.results([big_t], [big_q]))):
        entries, blocks, st = engine.axt_psl(t3, q3)
        assert st["host_entries"] == 1
        assert_equals_restatement(entries, blocks, w3)


def test_no_entries(engine):
    entries, blocks, st = engine.axt_psl([], [])
    assert entries.shape == (0,) and blocks.shape == (0, 3)
    assert st == dict(blocks=0, columns=0, host_entries=0, batches=0, fell_back=0)


def test_kernel_timing_is_one_lap_per_batch(engine, random_expected):
    from genomealignmenttools_amd._lib import GAC_K_AXTPSL
    t_rows, q_rows, _want = random_expected
    engine.prof_enable(True, kernels=[GAC_K_AXTPSL])
    engine.prof_reset()
    try:
        _e, _b, st = engine.axt_psl(t_rows, q_rows)
        ms, laps = engine.prof_read(GAC_K_AXTPSL)
    finally:
        engine.prof_enable(False)
    assert st["batches"] == 1 and laps == 1 and ms > 0


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "axtToPsl")


def test_tool_device_jobs_equal_reference_on_every_golden(tmp_path):
    """every golden case as one line of a -jobs file: one process, one device"""
    cases = sorted(CASES)
    lines = [" ".join(CASES[c][:3] + (str(tmp_path / (c + ".psl")),)) for c in cases]
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_tool(), "-device", "-verbose=2", "-jobs=" + str(jobs)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("convert (GPU): ") == len(cases) and "on the host" not in r.stderr
    for c in cases:
        assert open(str(tmp_path / (c + ".psl")), "rb").read() == open(CASES[c][3], "rb").read(), c


def test_job_line_chains_equal_the_reference_psl_chains(tmp_path):
    """INTEGRATION.md's patchChain line on bin/ alone: axtToPsl's output piped
    into axtChain -psl gives the chains that the reference's axtToPsl output
    (the committed golden) gives"""
    from genomealignmenttools_amd._lib import BIN_DIR
    axt, ts, qs, psl = CASES["chain_s5"]
    d = os.path.dirname(axt)
    chain = os.path.join(BIN_DIR, "axtChain") + " -psl -linearGap=loose %s " + d + "/t.2bit " + d + "/q.2bit %s"
    piped, golden = str(tmp_path / "piped.chain"), str(tmp_path / "golden.chain")
    line = "set -o pipefail; %s %s %s %s stdout | %s" % (_tool(), axt, ts, qs, chain % ("stdin", piped))
    r = subprocess.run(["bash", "-c", line], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["bash", "-c", chain % (psl, golden)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = open(piped, "rb").read()
    assert got.count(b"chain ") > 10 and got == open(golden, "rb").read()
