"""axtToPsl without a GPU: the restatement (tests/axtpsl_ref.py) against the
reference's outputs (tests/golden/make_axtpsl_golden.py), the host twin
(gac_axt_psl_host) against the restatement on the goldens' entries and on
seeded random rows, the argument check, bin/axtToPsl -host byte for byte
against the reference's outputs and its error table, -jobs, stdin / stdout,
and the new symbols.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import axtpsl_ref as AR

GAC_E_ARG = -1
CASES = AR.load_cases()
ERRORS = AR.load_errors()
COUNTS = ("match", "mis_match", "rep_match", "n_count", "q_num_insert", "q_base_insert", "t_num_insert",
          "t_base_insert")
TRIMS = ("q_head", "t_head", "q_tail", "t_tail")


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "axtToPsl")


def _host(t_rows, q_rows, **kw):
    from genomealignmenttools_amd.gachain import axt_psl_host
    return axt_psl_host(t_rows, q_rows, **kw)


def assert_equals_restatement(entries, blocks, want):
    """a call's result against [entry_result(...)]; the blocks lie in entry order"""
    assert len(entries) == len(want)
    at = 0
    for i, (counts, trims, cols, blks) in enumerate(want):
        e = entries[i]
        assert [int(e[f]) for f in COUNTS] == counts, i
        assert tuple(int(e[f]) for f in TRIMS) == trims, i
        assert int(e["cols"]) == cols and int(e["n_blocks"]) == len(blks), i
        assert int(e["block0"]) == at, i
        assert [tuple(b) for b in blocks[at:at + len(blks)].tolist()] == blks, i
        at += len(blks)
    assert at == len(blocks)


@pytest.fixture(scope="module")
def random_expected():
    t_rows, q_rows = AR.random_rows()
    return t_rows, q_rows, AR.results(t_rows, q_rows)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_reference(case):
    axt, ts, qs, psl = CASES[case]
    data = [AR.read_input(p) for p in (axt, ts, qs, psl)]
    assert AR.convert(data[0], data[1], data[2]) == data[3]


def test_goldens_hold_what_they_are_for():
    def lines(case):
        with open(CASES[case][3], "rb") as f:
            return [ln.split(b"\t") for ln in f.read().split(b"\n") if ln]
    # the flipped-trim quirk: leading query-only columns on '-' move qEnd's side
    plus, minus = lines("trims")[0], lines("trims")[7]
    assert plus[8] == b"+" and minus[8] == b"-"
    assert (int(plus[11]), int(plus[12])) == (2002, 2008)
    assert (int(minus[11]), int(minus[12])) == (90000 - 2008 + 2, 90000 - 2000)
    assert int(minus[12]) - int(minus[11]) == 6 and minus[19] == b"%d," % (2000 + 0)
    # records that trim to nothing write nothing; ranges left over give a block of 0
    assert len(lines("empty")) == 2 and len(AR.read_axt(AR.read_input(CASES["empty"][0]))) == 18
    assert any(ln[17] == b"1" and ln[18] == b"0," for ln in lines("disagree"))
    assert len(lines("counts")) == 56 and len(lines("chain_s5")) == 610
    assert lines("dup_sizes") == lines("strands")
    assert lines("nofinal") == lines("nofinal_nonl")
    for case in CASES:
        for ln in lines(case):
            assert len(ln) == 21 and ln[18].endswith(b",") and ln[19].endswith(b",") and ln[20].endswith(b",")


def test_count_rule_branches():
    def counts(t, q):
        return AR.entry_result(t, q)[0][:4]
    assert counts(b"n", b"n") == [0, 0, 1, 0] and counts(b"n", b"a") == [0, 1, 0, 0]
    assert counts(b"N", b"n") == [0, 0, 0, 1] and counts(b"a", b"N") == [0, 0, 0, 1]
    assert counts(b"A", b"A") == [1, 0, 0, 0] and counts(b"A", b"a") == [0, 0, 1, 0]
    assert counts(b"A", b"C") == [0, 1, 0, 0] and counts(b"a", b"c") == [0, 1, 0, 0]


def test_host_twin_on_the_goldens():
    t_rows, q_rows = AR.golden_rows()
    assert len(t_rows) > 700
    entries, blocks, st = _host(t_rows, q_rows)
    assert_equals_restatement(entries, blocks, AR.results(t_rows, q_rows))
    assert st["host_entries"] == len(t_rows) and st["blocks"] == len(blocks)
    assert st["columns"] == sum(len(t) for t in t_rows)


@pytest.mark.parametrize("nthreads", [1, 7])
def test_host_twin_on_random_rows(random_expected, nthreads):
    t_rows, q_rows, want = random_expected
    assert len(t_rows) == 2000 and {len(t) for t in t_rows} >= {1, 300}
    entries, blocks, _st = _host(t_rows, q_rows, nthreads=nthreads)
    assert_equals_restatement(entries, blocks, want)


def test_host_twin_empty_call():
    entries, blocks, st = _host([], [])
    assert len(entries) == 0 and blocks.shape == (0, 3) and st["blocks"] == 0


def test_argument_check():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    text = b"ACGTACGT"

    def p(a):
        return C.c_void_p(a.ctypes.data)

    def host(n, text_bytes, t, q, ln, res=True):
        r = C.POINTER(_lib.AxtPslResult)()
        rc = L.gac_axt_psl_host(n, text, text_bytes, p(t), p(q), p(ln), 1, C.byref(r) if res else None, None)
        if rc == 0:
            L.gac_axtpsl_free(r)
        else:
            assert not r
        return rc

    t, q = np.array([0, 4], np.int64), np.array([4, 0], np.int64)
    ln = np.array([4, 4], np.int32)
    assert host(2, 8, t, q, ln) == 0
    assert host(2, 8, t, q, np.array([4, -1], np.int32)) == GAC_E_ARG       # a negative length
    assert host(2, 7, t, q, ln) == GAC_E_ARG                                # a row past text_bytes
    assert host(2, 8, t, np.array([4, 5], np.int64), ln) == GAC_E_ARG
    assert host(2, 8, np.array([0, -4], np.int64), q, ln) == GAC_E_ARG      # a negative offset
    assert host(-1, 8, t, q, ln) == GAC_E_ARG
    assert host(2, 8, t, q, ln, res=False) == GAC_E_ARG                     # nowhere to put the result
    r = C.POINTER(_lib.AxtPslResult)()
    assert L.gac_axt_psl_host(2, text, 8, None, None, None, 1, C.byref(r), None) == GAC_E_ARG   # NULL arrays
    assert b"NULL" in L.gac_last_error()
    assert L.gac_axt_psl_host(2, None, 8, p(t), p(q), p(ln), 1, C.byref(r), None) == GAC_E_ARG
    # the device call checks the same before it touches the context
    assert L.gac_axt_psl(None, 2, text, 8, p(t), p(q), p(ln), C.byref(r), None) == GAC_E_ARG
    L.gac_axtpsl_free(None)


def test_symbols_and_constants():
    from genomealignmenttools_amd import _lib, gachain
    L = _lib.lib()
    for name in ("gac_axt_psl", "gac_axt_psl_host", "gac_axtpsl_free"):
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 8
    assert _lib.GAC_K_AXTPSL == 6 and _lib.GAC_AXTPSL_TILE == 512
    assert _lib.GAC_K_AXTFILTER == 5  # the earlier ids keep their values
    assert C.sizeof(_lib.AxtPslEntry) == 64 and gachain.AXT_PSL_ENTRY.itemsize == 64
    assert "axt_psl_host" in gachain.__all__ and hasattr(gachain.Engine, "axt_psl")
    with open(os.path.join(_lib.REPO_DIR, "include", "gachain.h")) as f:
        header = f.read()
    assert "#define GAC_AXTPSL_TILE %d\n" % _lib.GAC_AXTPSL_TILE in header
    assert "#define GAC_K_AXTPSL %d " % _lib.GAC_K_AXTPSL in header


@pytest.mark.parametrize("case", sorted(CASES))
def test_tool_host_equals_reference(tmp_path, case):
    axt, ts, qs, psl = CASES[case]
    out = str(tmp_path / "out.psl")
    r = subprocess.run([_tool(), "-host", axt, ts, qs, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "" and open(out, "rb").read() == open(psl, "rb").read()


def test_tool_default_and_unknown_options(tmp_path):
    """no path option: a small input needs no device; any option is accepted, as optionHash does"""
    axt, ts, qs, psl = CASES["trims"]
    out = str(tmp_path / "out.psl")
    r = subprocess.run([_tool(), "-foo", axt, ts, "-bar=7", qs, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(psl, "rb").read()


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_error_table(tmp_path, case):
    e = ERRORS[case]
    assert e["status"] == 255
    out = str(tmp_path / "out.psl")
    paths = {"{in}": os.path.join(AR.AXTPSL_DIR, e["input"]), "{t}": os.path.join(AR.AXTPSL_DIR, e["t_sizes"]),
             "{q}": os.path.join(AR.AXTPSL_DIR, e["q_sizes"]), "{out}": out}
    r = subprocess.run([_tool(), "-host"] + [paths.get(a, a) for a in e["args"]], capture_output=True, text=True)
    assert r.returncode == 255 and r.stderr.strip() != "" and r.stdout == ""
    # nothing is written, also where the reference left the earlier records behind
    assert not os.path.exists(out) or os.path.getsize(out) == 0
    if case.startswith("argcount"):
        assert r.stderr.startswith(e["stderr"]) and "axtToPsl in.axt tSizes qSizes out.psl" in r.stderr


def test_jobs_equal_single_runs(tmp_path):
    runs = ["bothgap", "dup_sizes"]
    lines = [" ".join(CASES[c][:3] + (str(tmp_path / ("job%d.psl" % k)),)) for k, c in enumerate(runs)]
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("# two runs\n" + lines[0] + "\n\n" + lines[1] + "\n")
    r = subprocess.run([_tool(), "-host", "-jobs=" + str(jobs)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for k, c in enumerate(runs):
        assert open(str(tmp_path / ("job%d.psl" % k)), "rb").read() == open(CASES[c][3], "rb").read()
    r = subprocess.run([_tool(), "-host", "-jobs=" + str(jobs), "extra"], capture_output=True, text=True)
    assert r.returncode == 255


def test_stdin_and_stdout():
    axt, ts, qs, psl = CASES["strands"]
    assert not axt.endswith(".gz")
    with open(axt, "rb") as f:
        r = subprocess.run([_tool(), "-host", "stdin", ts, qs, "stdout"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(psl, "rb").read()


def test_gzip_input(tmp_path):
    import gzip
    axt, ts, qs, psl = CASES["counts"]
    gz = str(tmp_path / "in.axt.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(axt, "rb").read())
    out = str(tmp_path / "out.psl")
    r = subprocess.run([_tool(), "-host", gz, ts, qs, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(psl, "rb").read()
