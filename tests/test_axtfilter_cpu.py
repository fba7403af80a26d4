"""filterAxtIdentityEntropy.py without a GPU: the restatement
(tests/axtfilter_ref.py) against the reference's outputs
(tests/golden/make_axtfilter_golden.py), the host twin (gac_axt_filter_host)
against the restatement on every golden and on seeded random rows, the
argument checks, bin/filterAxtIdentityEntropy.py -host byte for byte against
the reference's outputs and its error table, -jobs, and the new symbols.  Every
comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import axtfilter_ref as AR

GAC_E_ARG = -1
CASES = AR.load_cases()
ERRORS = AR.load_errors()


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "filterAxtIdentityEntropy.py")


def _host(t_rows, q_rows, ident, ent, w, **kw):
    from genomealignmenttools_amd.gachain import axt_filter_host
    return axt_filter_host(t_rows, q_rows, ident, ent, w, **kw)


@pytest.fixture(scope="module")
def random_expected():
    """the random rows and the restatement's flags per window, computed once"""
    t_rows, q_rows = AR.random_rows(20261021)
    entries = [("", t, q) for t, q in zip(t_rows, q_rows)]
    want = {w: np.array(AR.filter_entries(entries, *AR.RANDOM_THRESHOLDS[w], w), np.uint8)
            for w in AR.WINDOWS}
    return t_rows, q_rows, want


@pytest.mark.parametrize("run", sorted(CASES))
def test_restatement_equals_reference(run):
    src, (ident, ent, w), want = CASES[run]
    mine = AR.filter_text(AR.read_text(src), float(ident), float(ent), int(w))
    with open(want, newline="") as f:
        assert mine == f.read()


def test_goldens_hold_what_they_are_for():
    def kept(run):
        with open(CASES[run][2]) as f:
            return [int(ln.split()[0]) for ln in f.read().split("\n")[0::4] if ln]
    assert kept("rules_w10") == [0, 2, 3, 6, 8, 9, 10]
    assert kept("rules_w2000") == [] and kept("empty_w10") == [] and kept("comments_only_w10") == []
    assert kept("hash_w12") == kept("crlf_w12") == kept("cr_w12") == [0, 2]
    for tie in ("tie_ident60", "tie_ident33", "tie_ent1111", "tie_ent15_15", "tie_ent10_10_10",
                "tie_ent0123"):
        assert kept(tie + "_at") == [0] and kept(tie + "_above") == [], tie
        at, above = CASES[tie + "_at"][1], CASES[tie + "_above"][1]
        k = 0 if "ident" in tie else 1
        assert float(above[k]) == np.nextafter(float(at[k]), np.inf) and at[2] == above[2]
    # the order of the terms is part of the result: the same counts given to
    # other bases stay below the threshold that (0, 1, 2, 3) reaches
    thr = float(CASES["tie_ent0123_at"][1][1])
    assert thr == AR.entropy(0, 1, 2, 3)
    _h, t, _q = AR.read_entries(AR.read_text(CASES["tie_ent0123_at"][0]))[1]
    counts = [t.count(b) for b in "ACGT"]
    assert sorted(counts) == [0, 1, 2, 3] and AR.entropy(*counts) < thr


@pytest.mark.parametrize("run", sorted(CASES))
def test_host_twin_on_goldens(run):
    src, (ident, ent, w), _want = CASES[run]
    entries = AR.read_entries(AR.read_text(src))
    want = np.array(AR.filter_entries(entries, float(ident), float(ent), int(w)), np.uint8)
    keep, st = _host([e[1] for e in entries], [e[2] for e in entries], float(ident), float(ent), int(w))
    assert keep.dtype == np.uint8 and np.array_equal(keep, want)
    assert st["kept"] == int(want.sum()) and st["host_entries"] == len(entries)
    assert st["windows"] == sum(max(0, len(e[2]) - int(w) + 1) for e in entries)
    assert st["batches"] == 0 and st["fell_back"] == 0


@pytest.mark.parametrize("w", AR.WINDOWS)
def test_host_twin_on_random_rows(random_expected, w):
    t_rows, q_rows, want = random_expected
    ident, ent = AR.RANDOM_THRESHOLDS[w]
    assert 0 < int(want[w].sum()) < len(want[w])
    for nthreads in (1, 3):
        keep, st = _host(t_rows, q_rows, ident, ent, w, nthreads=nthreads)
        assert np.array_equal(keep, want[w]) and st["kept"] == int(want[w].sum())


def test_host_twin_large_windows():
    """windows past the host's term table compute the terms in place"""
    t = "ACGT" * 700
    for w in (2048, 2049, 2800):
        keep, _st = _host([t, t, "A" * 2800], [t, t[:w - 1], "A" * 2800], 100.0, 1.99, w)
        assert keep.tolist() == [1, 0, 0]


def test_argument_checks():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    text = b"ACGTACGT"
    off = np.array([0, 4], np.int64)
    ln = np.array([4, 4], np.int32)
    keep = np.zeros(2, np.uint8)

    def p(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def call(n=2, text=text, text_bytes=len(text), t=off, q=off, ln=ln, w=2, keep=keep):
        return L.gac_axt_filter_host(n, text, text_bytes, p(t), p(q), p(ln), 0.0, 0.0, w, 1, p(keep), None)
    assert call() == 0 and keep.tolist() == [1, 1]
    assert call(w=0) == GAC_E_ARG and call(w=-3) == GAC_E_ARG
    assert call(n=-1) == GAC_E_ARG
    assert call(ln=np.array([4, -1], np.int32)) == GAC_E_ARG
    assert call(ln=np.array([4, 5], np.int32)) == GAC_E_ARG          # a row past the text
    assert call(t=np.array([0, 5], np.int64)) == GAC_E_ARG
    assert call(q=np.array([-1, 4], np.int64)) == GAC_E_ARG
    assert call(text_bytes=7) == GAC_E_ARG
    for missing in ("t", "q", "ln", "keep"):
        assert call(**{missing: None}) == GAC_E_ARG, missing
    assert call(text=None) == GAC_E_ARG
    assert call(n=0, text=None, text_bytes=0, t=None, q=None, ln=None, keep=None) == 0
    assert call(w=0) == GAC_E_ARG and b"window" in L.gac_last_error()
    # the device entry point checks before it looks at its context
    assert L.gac_axt_filter(None, 2, text, len(text), None, None, None, 0.0, 0.0, 2, None, None) == GAC_E_ARG


def test_symbols_and_minor():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    for name in ("gac_axt_filter", "gac_axt_filter_host"):
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 7
    assert _lib.GAC_K_AXTFILTER == 5 and _lib.GAC_AXTF_MAX_WINDOW == 1024


@pytest.mark.parametrize("run", sorted(CASES))
def test_tool_host_equals_reference(tmp_path, run):
    src, args, want = CASES[run]
    out = str(tmp_path / "out.axt")
    r = subprocess.run([_tool(), "-host", src] + args + [out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "" and open(out, "rb").read() == open(want, "rb").read()


def test_tool_default_on_a_small_input(tmp_path):
    """no option: a small input takes the host path, and no device is needed"""
    src, args, want = CASES["rules_w10"]
    out = str(tmp_path / "out.axt")
    r = subprocess.run([_tool(), src] + args + [out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_error_table(tmp_path, case):
    e = ERRORS[case]
    out = str(tmp_path / "out.axt")
    paths = {"{in}": os.path.join(AR.AXTF_DIR, e["input"]), "{out}": out}
    r = subprocess.run([_tool(), "-host"] + [paths.get(a, a) for a in e["args"]], capture_output=True,
                       text=True)
    # the reference dies with status 1; here an abort is any non-zero status
    # with a message, and the usage line (stdout, status 1) is as there
    assert (r.returncode != 0) == (e["status"] != 0), r.stderr
    if len(e["args"]) != 5:
        assert r.returncode == 1 and r.stdout.lower().startswith("usage") and r.stderr == ""
    elif e["status"]:
        assert r.stderr.strip() != "" and r.stdout == ""
    if case == "window0":
        assert not os.path.exists(out)  # refused before anything is read or made


def test_negative_numbers_are_positional(tmp_path):
    src, args, want = CASES["rules_w12_negative"]
    assert args[0].startswith("-") and args[1].startswith("-")
    out = str(tmp_path / "out.axt")
    r = subprocess.run([_tool(), src] + args + [out, "-host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()


def test_jobs_equal_single_runs(tmp_path):
    runs = ["rules_w10_loose", "crlf_w4", "tie_ent0123_at"]
    lines = []
    for k, run in enumerate(runs):
        src, args, _want = CASES[run]
        lines.append(" ".join([src] + args + [str(tmp_path / ("job%d.axt" % k))]))
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("# three runs\n" + lines[0] + "\n\n" + lines[1] + "\n" + lines[2] + "\n")
    r = subprocess.run([_tool(), "-host", "-jobs=" + str(jobs)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for k, run in enumerate(runs):
        single = str(tmp_path / ("single%d.axt" % k))
        src, args, want = CASES[run]
        r = subprocess.run([_tool(), "-host", src] + args + [single], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = open(str(tmp_path / ("job%d.axt" % k)), "rb").read()
        assert got == open(single, "rb").read() == open(want, "rb").read()
    # a line that is not five arguments stops the batch
    jobs.write_text(lines[0] + " extra\n")
    r = subprocess.run([_tool(), "-host", "-jobs=" + str(jobs)], capture_output=True, text=True)
    assert r.returncode != 0 and "five arguments" in r.stderr
