"""filterAxtIdentityEntropy.py on the GPU: Engine.axt_filter (gac_axt_filter:
packed prefix counts per tile of columns, a lane per window start) against the
host twin and the restatement (tests/axtfilter_ref.py) on every golden, the
random rows, a sweep of the one passing window over every chunk edge, the
packed counters' fields at their largest, the window cap, batches and the
byte budget, and bin/filterAxtIdentityEntropy.py -device byte for byte against
the reference's outputs.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import axtfilter_ref as AR

pytestmark = pytest.mark.gpu

CASES = AR.load_cases()
SMALLEST = 5e-324  # the smallest positive double


def _host(t_rows, q_rows, ident, ent, w):
    from genomealignmenttools_amd.gachain import axt_filter_host
    return axt_filter_host(t_rows, q_rows, ident, ent, w)[0]


@pytest.fixture(scope="module")
def random_expected():
    """the random rows and the restatement's flags per window, computed once"""
    t_rows, q_rows = AR.random_rows(20261021)
    entries = [("", t, q) for t, q in zip(t_rows, q_rows)]
    want = {w: np.array(AR.filter_entries(entries, *AR.RANDOM_THRESHOLDS[w], w), np.uint8)
            for w in AR.WINDOWS}
    return t_rows, q_rows, want


@pytest.fixture
def batch_bytes():
    """the text budget of a batch, for one test"""
    old = os.environ.get("GAC_AXTF_BATCH_BYTES")

    def set_(v):
        os.environ["GAC_AXTF_BATCH_BYTES"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("GAC_AXTF_BATCH_BYTES", None)
    else:
        os.environ["GAC_AXTF_BATCH_BYTES"] = old


@pytest.mark.parametrize("run", sorted(CASES))
def test_goldens(engine, run):
    """(the runs named tie_* hold the thresholds one ulp apart)"""
    src, (ident, ent, w), _want = CASES[run]
    entries = AR.read_entries(AR.read_text(src))
    t_rows, q_rows = [e[1] for e in entries], [e[2] for e in entries]
    want = np.array(AR.filter_entries(entries, float(ident), float(ent), int(w)), np.uint8)
    keep, st = engine.axt_filter(t_rows, q_rows, float(ident), float(ent), int(w))
    assert keep.dtype == np.uint8 and np.array_equal(keep, want)
    assert np.array_equal(keep, _host(t_rows, q_rows, float(ident), float(ent), int(w)))
    assert st["kept"] == int(want.sum())
    assert st["windows"] == sum(max(0, len(q) - int(w) + 1) for q in q_rows)
    if int(w) <= 1024:
        assert st["fell_back"] == 0 and st["host_entries"] == 0
        assert st["batches"] == (1 if st["windows"] else 0)
    else:
        assert st["fell_back"] == 1 and st["host_entries"] == len(entries) and st["batches"] == 0


@pytest.mark.parametrize("w", AR.WINDOWS)
def test_random_rows(engine, random_expected, w):
    t_rows, q_rows, want = random_expected
    ident, ent = AR.RANDOM_THRESHOLDS[w]
    keep, st = engine.axt_filter(t_rows, q_rows, ident, ent, w)
    assert np.array_equal(keep, want[w]) and np.array_equal(keep, _host(t_rows, q_rows, ident, ent, w))
    assert st["fell_back"] == 0 and st["batches"] == 1 and st["kept"] == int(want[w].sum())


_OTHER = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"CGTA"):
    _OTHER[_a] = _b


def _edge_rows(w, ps):
    """Per p: an entry whose only window of w matching columns starts at p, and
    its twin with one more mismatch at column p.  The target is a 64-base
    pattern of 16 each of A, C, G, T (H = 2.0 over any 64) repeated to 3 * 1024
    + w columns; the query is a copy with a mismatch every w columns outwards
    from p - 1 and from p + w, so every other window of w columns holds one."""
    rng = np.random.default_rng(64)
    pat = np.frombuffer(b"ACGT" * 16, np.uint8).copy()
    rng.shuffle(pat)
    L = 3 * 1024 + w
    t = np.tile(pat, L // 64 + 1)[:L]
    t_rows, q_rows = [], []
    for p in ps:
        q = t.copy()
        idx = np.concatenate([np.arange(p - 1, -1, -w), np.arange(p + w, L, w)])
        q[idx] = _OTHER[t[idx]]
        twin = q.copy()
        twin[p] = _OTHER[t[p]]
        t_rows += [t.tobytes()] * 2
        q_rows += [q.tobytes(), twin.tobytes()]
    return t_rows, q_rows, L


@pytest.mark.parametrize("w", (30, 1024))
def test_the_one_passing_window_at_every_chunk_edge(engine, w):
    last = 3 * 1024  # L - w
    if w == 30:
        ps = list(range(last + 1))
    else:
        near = {m + d for m in range(0, last + 1, 64) for d in (-2, -1, 0, 1, 2)}
        ps = sorted(p for p in near | set(range(0, last + 1, 97)) if 0 <= p <= last)
    t_rows, q_rows, L = _edge_rows(w, ps)
    keep, st = engine.axt_filter(t_rows, q_rows, 100.0, 0.0, w)
    want = np.tile(np.array([1, 0], np.uint8), len(ps))
    bad = np.flatnonzero(keep != want)
    assert bad.size == 0, "p = %s" % [ps[i // 2] for i in bad[:8]]
    assert st["fell_back"] == 0 and st["windows"] == 2 * len(ps) * (L - w + 1)
    assert np.array_equal(_host(t_rows, q_rows, 100.0, 0.0, w), want)


def test_counter_fields_at_their_largest(engine):
    """1024 of one base: a carry between the packed fields would give a
    neighbour a count and H > 0"""
    rows = [b * 1024 for b in ("A", "C", "G", "T", "a", "t")]
    keep, _st = engine.axt_filter(rows, rows, 100.0, 0.0, 1024)
    assert keep.tolist() == [1] * 6
    keep, _st = engine.axt_filter(rows, rows, 100.0, SMALLEST, 1024)
    assert keep.tolist() == [0] * 6
    # and the match field: 1024 matches, not one less
    q = ["C" + r[1:] if r[0] in "Aa" else "A" + r[1:] for r in rows]
    keep, _st = engine.axt_filter(rows, q, 100.0, 0.0, 1024)
    assert keep.tolist() == [0] * 6
    keep, _st = engine.axt_filter(rows, q, 100.0 * 1023 / 1024, 0.0, 1024)
    assert keep.tolist() == [1] * 6


def test_window_of_one_and_the_window_cap(engine, random_expected):
    t_rows, q_rows, want = random_expected
    keep, st = engine.axt_filter(t_rows, q_rows, *AR.RANDOM_THRESHOLDS[1], 1)
    assert np.array_equal(keep, want[1]) and st["fell_back"] == 0
    t = "ACGT" * 600
    rows_t, rows_q = [t, t, "A" * 2400, t[:1024]], [t, "ACGA" * 600, "A" * 2400, t[:1024]]
    for w in (1024, 1025):
        keep, st = engine.axt_filter(rows_t, rows_q, 100.0, 1.99, w)
        assert keep.tolist() == [1, 0, 0, int(w == 1024)]
        assert np.array_equal(keep, _host(rows_t, rows_q, 100.0, 1.99, w))
        assert st["fell_back"] == int(w == 1025) and st["host_entries"] == (4 if w == 1025 else 0)
        assert st["batches"] == (0 if w == 1025 else 1)


def test_batches_and_the_byte_budget(engine, random_expected, batch_bytes):
    t_rows, q_rows, want = random_expected
    w = 30
    ident, ent = AR.RANDOM_THRESHOLDS[w]
    batch_bytes(20000)
    keep, st = engine.axt_filter(t_rows, q_rows, ident, ent, w)
    assert st["batches"] >= 3 and st["fell_back"] == 0 and st["host_entries"] == 0
    assert np.array_equal(keep, want[w])
    # one entry alone over the budget goes to the host twin, the others stay
    big = "ACGTTGCA" * 4000
    t2 = t_rows[:200] + [big] + t_rows[200:]
    q2 = q_rows[:200] + [big] + q_rows[200:]
    keep, st = engine.axt_filter(t2, q2, ident, ent, w)
    assert st["fell_back"] == 2 and st["host_entries"] == 1 and st["batches"] >= 3
    assert np.array_equal(keep, np.concatenate([want[w][:200], [1], want[w][200:]]))


def test_sides_kept_apart(engine, random_expected):
    """a caller's text with every target row before every query row"""
    from genomealignmenttools_amd import _lib
    from genomealignmenttools_amd.gachain import _p
    t_rows, q_rows, want = random_expected
    w = 30
    ident, ent = AR.RANDOM_THRESHOLDS[w]
    ln = np.array([len(q) for q in q_rows], np.int32)
    tl = np.array([len(t) for t in t_rows], np.int64)
    t_off = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64)
    q_off = (int(tl.sum()) + 1000 + np.concatenate([[0], np.cumsum(ln.astype(np.int64))[:-1]])).astype(np.int64)
    text = ("".join(t_rows) + "#" * 1000 + "".join(q_rows)).encode()
    keep = np.zeros(len(ln), np.uint8)
    st = _lib.AxtFilterStats()
    _lib.check(_lib.lib().gac_axt_filter(engine.h, len(ln), text, len(text), _p(t_off), _p(q_off), _p(ln),
                                         ident, ent, w, _p(keep), C.byref(st)))
    assert np.array_equal(keep, want[w]) and st.fell_back == 0 and st.batches == 1


def test_no_entries(engine):
    keep, st = engine.axt_filter([], [], 50.0, 1.0, 10)
    assert keep.shape == (0,) and st == dict(kept=0, windows=0, host_entries=0, batches=0, fell_back=0)


def test_kernel_timing_is_one_lap_per_batch(engine, random_expected):
    from genomealignmenttools_amd._lib import GAC_K_AXTFILTER
    t_rows, q_rows, _want = random_expected
    engine.prof_enable(True, kernels=[GAC_K_AXTFILTER])
    engine.prof_reset()
    try:
        _keep, st = engine.axt_filter(t_rows, q_rows, 70.0, 1.2, 30)
        ms, laps = engine.prof_read(GAC_K_AXTFILTER)
    finally:
        engine.prof_enable(False)
    assert st["batches"] == 1 and laps == 1 and ms > 0


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "filterAxtIdentityEntropy.py")


def test_tool_device_equals_reference(tmp_path):
    src, args, want = CASES["rules_w10"]
    out = str(tmp_path / "out.axt")
    r = subprocess.run([_tool(), "-device", "-verbose=2", src] + args + [out], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
    assert "filter (GPU): " in r.stderr and "on the host" not in r.stderr


def test_tool_device_jobs_equal_reference_on_every_golden(tmp_path):
    """every golden run as one line of a -jobs file: one process, one device"""
    runs = sorted(CASES)
    lines = [" ".join([CASES[run][0]] + CASES[run][1] + [str(tmp_path / (run + ".axt"))]) for run in runs]
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("\n".join(lines) + "\n")
    r = subprocess.run([_tool(), "-device", "-verbose=2", "-jobs=" + str(jobs)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stderr.count("filter (GPU): ") == len(runs) and "%d jobs in one device context" % len(runs) in r.stderr
    for run in runs:
        assert open(str(tmp_path / (run + ".axt")), "rb").read() == open(CASES[run][2], "rb").read(), run
