"""axtToMaf's scores on the GPU: Engine.axt_score (gac_axt_score: a wave sums
a chunk of GAC_AXTSCORE_CHUNK columns of one entry, four columns a lane from
aligned words, one atomic add a chunk) against the restatement
(tests/axtscore_ref.py) -- every length up to two chunks and one column at every
row alignment, the scoring rules placed on both sides of a chunk edge and at an
entry's first column, neighbours kept apart, the int wrap-around, batches and
the byte budget -- then bin/axtToMaf -device byte for byte against the
reference's outputs, and the route from chains to a MAF.  Every comparison is
exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
# torch before libgachain, for the reason written at the top of
# test_gpu_antirepeat.py
import torch  # noqa: F401

from conftest import GOLDEN

import axtscore_ref as AS
from test_axtmaf_cpu import CASES, MAF_CASES, assert_output, maf_args, path, tool

pytestmark = pytest.mark.gpu

CH = 1024  # checked against the exported constant below


@pytest.fixture
def batch_bytes():
    """the text budget of a batch, for one test"""
    old = os.environ.get("GAC_AXTSCORE_BATCH_BYTES")

    def set_(v):
        os.environ["GAC_AXTSCORE_BATCH_BYTES"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("GAC_AXTSCORE_BATCH_BYTES", None)
    else:
        os.environ["GAC_AXTSCORE_BATCH_BYTES"] = old


def raw_score(engine, text, t_off, q_off, ln):
    """gac_axt_score on a text laid out by the caller"""
    from genomealignmenttools_amd import _lib
    from genomealignmenttools_amd.gachain import _p
    t_off, q_off = np.ascontiguousarray(t_off, np.int64), np.ascontiguousarray(q_off, np.int64)
    ln = np.ascontiguousarray(ln, np.int32)
    score = np.full(len(ln), 12345, np.int32)
    st = _lib.AxtScoreStats()
    _lib.check(_lib.lib().gac_axt_score(engine.h, len(ln), bytes(text), len(text), _p(t_off), _p(q_off), _p(ln),
                                        _p(score), C.byref(st)))
    return score, st


def gappy_row_pair(rng, L):
    """two rows of L columns: letters in both cases, N, runs of dashes in either row"""
    alphabet = np.frombuffer(b"ACGTacgtACGTNn.", np.uint8)
    t = alphabet[rng.integers(0, len(alphabet), L)].copy()
    q = alphabet[rng.integers(0, len(alphabet), L)].copy()
    at = 0
    while at < L:
        at += int(rng.integers(1, 40))
        run = int(rng.integers(1, 9))
        side = int(rng.integers(0, 3))
        if side != 1:
            t[at:at + run] = ord("-")
        if side != 0:
            q[at + run // 2:at + run + run // 2] = ord("-")
        at += run
    return t[:L].tobytes(), q[:L].tobytes()


def test_chunk_constant():
    from genomealignmenttools_amd import _lib
    assert _lib.GAC_AXTSCORE_CHUNK == CH


def test_every_length_and_alignment(engine):
    """lengths 0 .. 2 * chunk + 1; t_off % 16 takes all 16 values, each against four q_off % 16"""
    rng = np.random.default_rng(1024)
    q_res = (1, 6, 11, 12)
    text = bytearray()
    t_off, q_off, ln, want = [], [], [], []

    def place(row, residue):
        text.extend(b"#" * ((residue - len(text)) % 16))
        text.extend(row)
        return len(text) - len(row)

    for L in range(0, 2 * CH + 2):
        t, q = gappy_row_pair(rng, L)
        t_off.append(place(t, L % 16))
        q_off.append(place(q, q_res[(L // 16) % 4]))
        ln.append(L)
        want.append(AS.score(t, q))
    pairs = {(a % 16, b % 16) for a, b in zip(t_off, q_off)}
    assert len(pairs) == 64 and {a for a, _ in pairs} == set(range(16))
    got, st = raw_score(engine, text, t_off, q_off, ln)
    bad = np.flatnonzero(got != np.array(want, np.int32))
    assert bad.size == 0, (bad[:10], got[bad[:5]], [want[k] for k in bad[:5]])
    assert st.host_entries == 0 and st.fell_back == 0 and st.columns == sum(ln)


SNIPPETS = {  # the rules, as (target, query) pieces of a row
    "gap": ("-", "A"),
    "gap_in_target_run": ("----", "ACGT"),
    "gap_in_query_run": ("ACGT", "----"),
    "run_changes_rows": ("GG--", "--AA"),
    "run_changes_rows_twice": ("-G-", "A-A"),
    "both_dash_in_a_run": ("---", "A-A"),
    "both_dash_alone": ("-", "-"),
    "run_ends_new_run_one_later": ("--A-", "ACGT"),
    "dot_ends_a_run": ("-.-", "A.A"),
    "equals_ends_a_run": ("-=-", "A=A"),
    "underscore_ends_a_run": ("-_-", "A_A"),
    "dot_against_dash": (".", "-"),
    "case_and_n": ("aCgTNnxA", "AcGtAnxa"),
    "mismatches": ("AAAACCCCGGGGTTTT", "ACGTACGTACGTACGT"),
}


def test_pattern_rows_at_chunk_edges(engine):
    """every column of every snippet on the last column of a chunk, on the first
    column of the next, and on column 0 of an entry"""
    rng = np.random.default_rng(7)
    L = 2 * CH + 9
    base = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
    names, t_rows, q_rows = [], [], []
    for name, (ts, qs) in SNIPPETS.items():
        assert len(ts) == len(qs)
        for named in (CH - 1, CH, 2 * CH - 1, 2 * CH, 0):
            for anchor in range(len(ts)):
                at = named - anchor
                if at < 0:
                    continue
                t = base[:at] + ts.encode() + base[at + len(ts):]
                q = base[:at] + qs.encode() + base[at + len(ts):]
                names.append((name, named, anchor))
                t_rows.append(t)
                q_rows.append(q)
    # entries of gaps only, of one column, and short ones that end inside a lane's four columns
    for n in (1, 2, 3, 4, 5, CH - 1, CH, CH + 1, L):
        for t, q in ((b"-" * n, base[:n]), (base[:n], b"-" * n), (b"-" * n, b"-" * n),
                     (b"-A" * n, b"A-" * n), (base[:n], base[:n].lower())):
            names.append(("gaps_or_short", n, 0))
            t_rows.append(t[:n])
            q_rows.append(q[:n])
    want = AS.scores(t_rows, q_rows)
    got, st = engine.axt_score(t_rows, q_rows)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(names[k], int(got[k]), int(want[k])) for k in bad[:8]]
    assert st["host_entries"] == 0
    # the snippets do what they are named for
    assert AS.score("GG--", "--AA") == -400 - 4 * 30 and AS.score("--A-", "ACGT") == 2 * -430 - 30 - 31
    assert AS.score("-.-", "A.A") == 2 * -430 and AS.score(".", "-") == -430


@pytest.mark.parametrize("first_len", [4, CH, CH + 3])
def test_neighbours_kept_apart(engine, first_len):
    """the first entry ends in a gap and the second starts with one: the second
    opens a gap of its own; as one entry the run goes on"""
    rng = np.random.default_rng(first_len)
    body = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, first_len + 40)].tobytes()
    t1, q1 = body[:first_len - 1] + b"-", body[:first_len]
    t2, q2 = b"--" + body[first_len + 2:], body[first_len:]
    text = t1 + t2 + q1 + q2   # the rows of the two entries lie end to start
    n1, n2 = len(t1), len(t2)
    got, _st = raw_score(engine, text, [0, n1], [n1 + n2, n1 + n2 + n1], [n1, n2])
    assert got.tolist() == [AS.score(t1, q1), AS.score(t2, q2)]
    one, _st = raw_score(engine, text, [0], [n1 + n2], [n1 + n2])
    assert one.tolist() == [AS.score(t1 + t2, q1 + q2)]
    assert int(one[0]) == int(got[0]) + int(got[1]) + 400


def test_wrap_around(engine):
    n = 21474837  # 100 * n > 2^31 - 1
    row = b"C" * n
    got, st = engine.axt_score([row], [row])
    assert got.tolist() == [100 * n - (1 << 32)] and got[0] < 0
    assert st["host_entries"] == 0 and st["fell_back"] == 0 and st["batches"] == 1 and st["columns"] == n


def test_batches(engine, batch_bytes):
    t_rows, q_rows = AS.random_rows(n=300)
    want = AS.scores(t_rows, q_rows)
    plain, st = engine.axt_score(t_rows, q_rows)
    assert plain.tolist() == want.tolist() and st["batches"] == 1
    batch_bytes(600)    # an entry has at most 600 bytes: about one a batch
    got, st = engine.axt_score(t_rows, q_rows)
    assert got.tolist() == want.tolist() and st["batches"] > 150 and st["fell_back"] == 0
    batch_bytes(20000)  # several batches
    got, st = engine.axt_score(t_rows, q_rows)
    assert got.tolist() == want.tolist() and 2 <= st["batches"] < 20 and st["host_entries"] == 0
    # one entry over the budget, among the others
    rng = np.random.default_rng(5)
    big = gappy_row_pair(rng, 3 * CH + 5)
    t3, q3 = t_rows[:100] + [big[0]] + t_rows[100:], q_rows[:100] + [big[1]] + q_rows[100:]
    batch_bytes(2000)
    got, st = engine.axt_score(t3, q3)
    assert st["fell_back"] == 2 and st["host_entries"] == 1
    assert got.tolist() == want[:100].tolist() + [AS.score(*big)] + want[100:].tolist()


def test_goldens_random_rows_and_none(engine):
    for case in MAF_CASES:
        t_rows, q_rows = AS.rows_of(AS.read_input(path(CASES[case]["input"])))
        got, _st = engine.axt_score(t_rows, q_rows)
        assert got.tolist() == AS.scores(t_rows, q_rows).tolist(), case
    t_rows, q_rows = AS.random_rows()
    got, _st = engine.axt_score(t_rows, q_rows)
    assert got.tolist() == AS.scores(t_rows, q_rows).tolist()
    got, st = engine.axt_score([], [])
    assert len(got) == 0 and st["batches"] == 0 and st["columns"] == 0


def test_profiler_lap_per_batch(engine, batch_bytes):
    from genomealignmenttools_amd._lib import GAC_K_AXTSCORE
    t_rows, q_rows = AS.random_rows(n=100)
    batch_bytes(8000)
    engine.prof_enable(True, kernels=[GAC_K_AXTSCORE])
    try:
        engine.prof_reset()
        _s, st = engine.axt_score(t_rows, q_rows)
        ms, laps = engine.prof_read(GAC_K_AXTSCORE)
    finally:
        engine.prof_enable(False)
    assert laps == st["batches"] > 1 and ms > 0


@pytest.mark.parametrize("case", MAF_CASES)
def test_axttomaf_device_equals_reference(tmp_path, case):
    out = str(tmp_path / "out")
    r = subprocess.run([tool("axtToMaf"), "-device", "-verbose=2"] + maf_args(case, out), capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    scored = bool(set(CASES[case]["options"]) & {"-score", "-scoreZero"})
    assert ("score (GPU)" in r.stderr) == scored
    assert_output(case, out)


def test_axttomaf_device_jobs_in_one_context(tmp_path):
    runs = {"basic_score": None, "crlf_score": None, "nofinal_nl": None, "meta_score": None, "empty": None,
            "basic_dup_sizes": None}
    lines = []
    for k, case in enumerate(runs):
        c = CASES[case]
        assert c["options"] == ["-score"]
        runs[case] = str(tmp_path / ("job%d.maf" % k))
        lines.append(" ".join([path(c["input"]), path(c["t_sizes"]), path(c["q_sizes"]), runs[case]]))
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    r = subprocess.run([tool("axtToMaf"), "-device", "-score", "-verbose=2", "-jobs=" + str(jobs)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "%d jobs in one device context" % len(runs) in r.stderr
    for case, out in runs.items():
        assert_output(case, out)


def test_chains_to_maf_scores_equal_piece_scores(tmp_path):
    """chainToAxt | axtSort | axtToMaf -device -score on the s5 chains: the text
    kernel gives every record the score the bit-plane kernel (gac_axt_measure)
    gave its piece"""
    import axtout_ref as AX
    from genomealignmenttools_amd.chainfile import read_chains
    from genomealignmenttools_amd.gachain import GAC_Q, GAC_T, Engine
    d = os.path.join(GOLDEN, "axtchain", "s5")
    t2, q2, chain = os.path.join(d, "t.2bit"), os.path.join(d, "q.2bit"), os.path.join(d, "loose.chain")
    ca = read_chains(chain)
    e = Engine(0)
    try:
        e.load_2bit(GAC_T, t2, soft_mask=True)
        e.load_2bit(GAC_Q, q2, soft_mask=True)
        cs = AX.upload(e, ca)
        pieces = AX.split(ca, 100)
        piece_score = e.axt_measure(cs, pieces)[0]
        cs.close()
    finally:
        e.close()
    axt, srt, maf = str(tmp_path / "pieces.axt"), str(tmp_path / "sorted.axt"), str(tmp_path / "out.maf")
    # (the sizes of the s5 sequences are the axtToPsl goldens')
    sizes = {side: os.path.join(GOLDEN, "axtpsl", "s5.%s.sizes" % side) for side in "tq"}
    for cmd in ([tool("chainToAxt"), chain, t2, q2, axt], [tool("axtSort"), axt, srt],
                [tool("axtToMaf"), "-device", "-score", srt, sizes["t"], sizes["q"], maf]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stderr)
    # chainToAxt writes every piece of the chains (all at or above -minScore=0), in order,
    # with the measure kernel's scores
    assert (ca.score >= 0).all()
    recs, _tail = AS.read_axt(AS.read_input(axt))
    assert len(recs) == len(pieces) > 100 and [r["score"] for r in recs] == piece_score.tolist()
    by_head = {}
    for r in recs:
        by_head.setdefault((r["t_name"], r["t_start"], r["t_end"], r["q_name"], r["q_start"], r["q_end"],
                            r["strand"]), []).append(r["score"])
    sorted_recs, _tail = AS.read_axt(AS.read_input(srt))
    blocks = [b for b in AS.read_input(maf).split(b"\n\n") if b.startswith(b"a score=") or b"\na score=" in b]
    assert len(blocks) == len(sorted_recs) == len(recs)
    clean = 0
    for r, b in zip(sorted_recs, blocks):
        a = [ln for ln in b.split(b"\n") if ln.startswith(b"a score=")][0]
        got = int(float(a[len(b"a score="):]))
        want = by_head[(r["t_name"], r["t_start"], r["t_end"], r["q_name"], r["q_start"], r["q_end"], r["strand"])]
        assert len(set(want)) == 1
        if b"N" in r["t_sym"].upper() or b"N" in r["q_sym"].upper():
            continue
        clean += 1
        assert got == want[0] == AS.score(r["t_sym"], r["q_sym"])
    assert clean * 10 >= len(recs) * 9
