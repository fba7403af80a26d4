"""axtToMaf and axtSort without a GPU: the restatement (tests/axtscore_ref.py)
against the reference's outputs (tests/golden/make_axtmaf_golden.py), the host
twin (gac_axt_score_host) against the restatement on the goldens' rows, on the
rules' edge rows and on seeded random rows, and the two tools on the host path
against every golden and every row of the error table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import axtscore_ref as AS

GAC_E_ARG = -1
CASES = AS.load_cases()
ERRORS = AS.load_errors()
MAF_CASES = sorted(k for k, c in CASES.items() if c["tool"] == "axtToMaf")
SORT_CASES = sorted(k for k, c in CASES.items() if c["tool"] == "axtSort")
SCORED = [k for k in MAF_CASES if set(CASES[k]["options"]) & {"-score", "-scoreZero"}]


def tool(name):
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, name)


def path(name):
    return os.path.join(AS.AXTMAF_DIR, name)


def maf_args(case, out):
    c = CASES[case]
    return c["options"] + [path(c["input"]), path(c["t_sizes"]), path(c["q_sizes"]), out]


def assert_output(case, out):
    """what a tool wrote for a case against the reference's committed output"""
    want = CASES[case]["output"]
    if isinstance(want, dict):
        assert sorted(os.listdir(out)) == want["files"]
        for fn in want["files"]:
            assert AS.read_input(os.path.join(out, fn)) == AS.read_input(path(os.path.join(want["dir"], fn))), fn
    else:
        assert AS.read_input(out) == AS.read_input(path(want))


def restate(case):
    c = CASES[case]
    data = AS.read_input(path(c["input"]))
    if c["tool"] == "axtSort":
        return AS.sort_axt(data, by_query="-query" in c["options"], by_score="-byScore" in c["options"])
    kw = {}
    for o in c["options"]:
        if o.startswith("-tPrefix="):
            kw["t_prefix"] = o[9:].encode()
        elif o.startswith("-qPrefix="):
            kw["q_prefix"] = o[9:].encode()
        else:
            kw[{"-tSplit": "t_split", "-score": "rescore", "-scoreZero": "score_zero"}[o]] = True
    return AS.to_maf(data, AS.read_input(path(c["t_sizes"])), AS.read_input(path(c["q_sizes"])), **kw)


def _host(t_rows, q_rows, **kw):
    from genomealignmenttools_amd.gachain import axt_score_host
    return axt_score_host(t_rows, q_rows, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_reference(case):
    want = CASES[case]["output"]
    got = restate(case)
    if isinstance(want, dict):
        assert sorted(got) == [fn.encode() for fn in want["files"]]
        for fn in want["files"]:
            assert got[fn.encode()] == AS.read_input(path(os.path.join(want["dir"], fn)))
    else:
        assert got == AS.read_input(path(want))


def test_goldens_hold_what_they_are_for():
    maf = AS.read_input(path(CASES["basic_score"]["output"])).split(b"\n")
    plain = AS.read_input(path(CASES["basic"]["output"])).split(b"\n")
    zero = AS.read_input(path(CASES["basic_scorezero"]["output"])).split(b"\n")
    a = lambda lines: [ln for ln in lines if ln.startswith(b"a score=")]  # noqa: E731
    assert len(a(maf)) == len(a(plain)) == len(a(zero)) == 10
    # -scoreZero changes exactly the records whose score is 0; -score others too
    changed_zero = [k for k in range(10) if a(zero)[k] != a(plain)[k]]
    assert changed_zero and all(a(plain)[k] == b"a score=0.000000" for k in changed_zero)
    assert all(a(zero)[k] == a(maf)[k] for k in changed_zero)
    assert any(a(maf)[k] != a(plain)[k] for k in range(10) if k not in changed_zero)
    assert any(ln.startswith(b"a score=-") for ln in maf + plain)
    assert any(ln.startswith(b"s defaultName") for ln in plain)
    assert plain[0] == b"##maf version=1 scoring=blastz" and plain[1] == b"# made by hand"
    assert plain[-3:] == [b"# at the end", b"#", b""]
    # axtSort: equal keys come out in the reverse of their input order
    srt = AS.read_input(path(CASES["sort_target"]["output"])).split(b"\n")
    heads = [ln.split() for ln in srt if ln[:1].isdigit()]
    assert [h[1] for h in heads] == sorted(h[1] for h in heads) and heads[0][1] == b"chr10"
    assert [int(h[0]) for h in heads] == list(range(9))
    ties = [(h[1], h[2]) for h in heads]
    assert len(set(ties)) < len(ties)


def test_host_twin_equals_restatement_on_goldens():
    for case in MAF_CASES:
        t_rows, q_rows = AS.rows_of(AS.read_input(path(CASES[case]["input"])))
        got, st = _host(t_rows, q_rows, nthreads=2)
        assert got.dtype == np.int32 and got.tolist() == AS.scores(t_rows, q_rows).tolist(), case
        assert st["columns"] == sum(len(t) for t in t_rows) and st["host_entries"] == len(t_rows)


def test_host_twin_edge_rows():
    t_rows, q_rows = AS.edge_rows()
    want = AS.scores(t_rows, q_rows)
    got, st = _host(t_rows, q_rows)
    assert got.tolist() == want.tolist()
    by = dict(zip(zip(t_rows, q_rows), want.tolist()))
    assert by[("", "")] == 0 and by[("A", "A")] == 91 and by[("-", "A")] == -430 and by[("-", "-")] == -430
    assert by[("AC--GT", "AC-TGT")] == 91 + 100 - 430 - 30 + 100 + 91          # a both-dash column inside a run
    assert by[("AC-TGT", "ACT-GT")] == 91 + 100 - 430 - 30 + 100 + 91          # the run changes rows: one opening
    assert by[("AC-.-GT", "ACT.TGT")] == 91 + 100 - 430 + 0 - 430 + 100 + 91   # '.' ends a run
    assert by[("acgtACGT", "ACGTacgt")] == 2 * (91 + 100 + 100 + 91)
    assert by[("------", "ACGTAC")] == -400 - 6 * 30


def test_host_twin_random_rows_and_threads():
    t_rows, q_rows = AS.random_rows()
    want = AS.scores(t_rows, q_rows).tolist()
    for nt in (1, 3, 0):
        got, _st = _host(t_rows, q_rows, nthreads=nt)
        assert got.tolist() == want


def test_host_twin_wraps_like_an_int():
    n = 21474837  # 100 * n > 2^31 - 1
    row = b"C" * n
    got, _st = _host([row], [row])
    assert got.tolist() == [100 * n - (1 << 32)] and got[0] < 0


def test_bad_arguments():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    text = b"ACGTACGT"
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    t, q, ln = np.array([0], np.int64), np.array([4], np.int64), np.array([4], np.int32)
    sc = np.zeros(1, np.int32)
    assert L.gac_axt_score_host(1, text, 8, p(t), p(q), p(ln), 1, p(sc), None) == 0 and sc[0] == 382
    assert L.gac_axt_score_host(-1, text, 8, p(t), p(q), p(ln), 1, p(sc), None) == GAC_E_ARG
    assert L.gac_axt_score_host(1, text, 7, p(t), p(q), p(ln), 1, p(sc), None) == GAC_E_ARG   # a row past the text
    assert L.gac_axt_score_host(1, text, 8, p(t), p(q), p(np.array([-1], np.int32)), 1, p(sc), None) == GAC_E_ARG
    assert L.gac_axt_score_host(1, text, 8, p(np.array([-1], np.int64)), p(q), p(ln), 1, p(sc), None) == GAC_E_ARG
    assert L.gac_axt_score_host(1, text, 8, None, None, None, 1, p(sc), None) == GAC_E_ARG
    assert L.gac_axt_score_host(1, text, 8, p(t), p(q), p(ln), 1, None, None) == GAC_E_ARG
    assert b"gac_axt_score" in L.gac_last_error()
    assert L.gac_axt_score_host(0, None, 0, None, None, None, 1, None, None) == 0              # n == 0
    assert L.gac_axt_score(None, 1, text, 8, p(t), p(q), p(ln), p(sc), None) == GAC_E_ARG      # no context
    got, st = _host([], [])
    assert len(got) == 0 and st["columns"] == 0
    with pytest.raises(ValueError):
        _host(["ACG"], ["AC"])


def test_abi_exports_and_constants():
    from genomealignmenttools_amd import _lib, gachain
    L = _lib.lib()
    for name in ("gac_axt_score", "gac_axt_score_host"):
        assert hasattr(L, name)
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 9
    assert _lib.GAC_K_AXTSCORE == 7 and _lib.GAC_AXTSCORE_CHUNK == 1024
    assert _lib.GAC_K_AXTPSL == 6 and _lib.GAC_K_AXTFILTER == 5  # the earlier ids keep their values
    assert "axt_score_host" in gachain.__all__ and hasattr(gachain.Engine, "axt_score")
    with open(os.path.join(_lib.REPO_DIR, "include", "gachain.h")) as f:
        header = f.read()
    assert "#define GAC_AXTSCORE_CHUNK %d\n" % _lib.GAC_AXTSCORE_CHUNK in header
    assert "#define GAC_K_AXTSCORE %d " % _lib.GAC_K_AXTSCORE in header
    assert C.sizeof(_lib.AxtScoreStats) == 24


@pytest.mark.parametrize("case", MAF_CASES)
def test_axttomaf_host_equals_reference(tmp_path, case):
    out = str(tmp_path / "out")
    r = subprocess.run([tool("axtToMaf"), "-host"] + maf_args(case, out), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    assert_output(case, out)


@pytest.mark.parametrize("case", SORT_CASES)
def test_axtsort_equals_reference(tmp_path, case):
    c = CASES[case]
    out = str(tmp_path / "out.axt")
    r = subprocess.run([tool("axtSort")] + c["options"] + [path(c["input"]), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ""
    assert_output(case, out)


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_error_table(tmp_path, case):
    e = ERRORS[case]
    assert e["status"] == 255
    out = str(tmp_path / "out")
    paths = {"{in}": path(e["input"]), "{t}": path(e["t_sizes"]), "{q}": path(e["q_sizes"]), "{out}": out}
    cmd = [tool(e["tool"])] + (["-host"] if e["tool"] == "axtToMaf" else []) + [paths.get(a, a) for a in e["args"]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 255 and r.stderr.strip() != "" and r.stdout == ""
    # nothing is written, also where the reference left the earlier records behind
    assert not os.path.exists(out) or (os.path.isfile(out) and os.path.getsize(out) == 0)
    if case.startswith("argcount"):
        usage = "axtToMaf in.axt tSizes qSizes out.maf" if e["tool"] == "axtToMaf" else "axtSort in.axt out.axt"
        assert r.stderr.startswith(e["stderr"]) and usage in r.stderr
    if case == "maf_split_unsorted":
        assert e["stderr"] == "{in} isn't sorted, which is necessary when -tSplit option is used"
        assert r.stderr.split("\n")[0] == e["stderr"].replace("{in}", paths["{in}"])


def test_axttomaf_usage_is_the_references():
    r = subprocess.run([tool("axtToMaf")], capture_output=True, text=True)
    assert r.returncode == 255
    assert "    -tPrefex=YY. - add YY. to start of target sequence name in maf\n" in r.stderr
    assert "    -score       - recalculate score \n    -scoreZero   - recalculate score if zero \n" in r.stderr


def test_jobs_equal_single_runs(tmp_path):
    runs = ["basic_score", "crlf_score", "meta_score"]   # one command line's options for every job
    lines = []
    for k, case in enumerate(runs):
        c = CASES[case]
        lines.append(" ".join([path(c["input"]), path(c["t_sizes"]), path(c["q_sizes"]), str(tmp_path / ("job%d" % k))]))
    jobs = tmp_path / "jobs.txt"
    jobs.write_text("# three runs\n" + lines[0] + "\n\n" + lines[1] + "\n" + lines[2] + "\n")
    r = subprocess.run([tool("axtToMaf"), "-host", "-score", "-jobs=" + str(jobs)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for k, case in enumerate(runs):
        assert_output(case, str(tmp_path / ("job%d" % k)))
    r = subprocess.run([tool("axtToMaf"), "-host", "-jobs=" + str(jobs), "extra"], capture_output=True, text=True)
    assert r.returncode == 255


def test_no_score_option_never_loads_a_device(tmp_path):
    """without -score / -scoreZero there is nothing to score: -device included,
    no device is opened (the run holds up where none can be)"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", GAC_TIMING="1")
    out = str(tmp_path / "out.maf")
    for extra in ([], ["-device"]):
        r = subprocess.run([tool("axtToMaf"), "-verbose=2"] + extra + maf_args("basic", out), capture_output=True,
                           text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert "device open" not in r.stderr and "score (" not in r.stderr
        assert_output("basic", out)
    # and the default path of a small input with -score is the host's
    r = subprocess.run([tool("axtToMaf"), "-verbose=2"] + maf_args("basic_score", out), capture_output=True, text=True,
                       env=env)
    assert r.returncode == 0, r.stderr
    assert "score (host)" in r.stderr and "device open" not in r.stderr
    assert_output("basic_score", out)


def test_stdin_and_stdout():
    c = CASES["basic_score"]
    with open(path(c["input"]), "rb") as f:
        r = subprocess.run([tool("axtToMaf"), "-host", "-score", "stdin", path(c["t_sizes"]), path(c["q_sizes"]),
                            "stdout"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == AS.read_input(path(c["output"]))
    c = CASES["sort_query"]
    with open(path(c["input"]), "rb") as f:
        r = subprocess.run([tool("axtSort"), "-query", "stdin", "stdout"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == AS.read_input(path(c["output"]))


def test_sort_then_maf_pipeline(tmp_path):
    """axtSort | axtToMaf -tSplit: what is unsorted for -tSplit is sorted first"""
    c = CASES["split"]
    srt, out = str(tmp_path / "sorted.axt"), str(tmp_path / "split")
    r = subprocess.run([tool("axtSort"), path("split_unsorted.axt"), srt], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([tool("axtToMaf"), "-tSplit", srt, path(c["t_sizes"]), path(c["q_sizes"]), out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == ["chr10.maf", "chr2.maf", "chrT.maf"]
    want = AS.to_maf(AS.read_input(srt), AS.read_input(path(c["t_sizes"])), AS.read_input(path(c["q_sizes"])),
                     t_split=True)
    for fn, data in want.items():
        assert AS.read_input(os.path.join(out, fn.decode())) == data
