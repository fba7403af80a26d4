"""netSyntenic without a GPU: the coverage count's restatement against a
per-base count (random cases, tied positions, the whole int8 range of deltas
under thresholds up to 2^31 - 1, 31 widths of the sequence id), the host twin
(gac_depth_count_host) against the restatement on every shape of
netsyn_ref.SHAPES (`stride` and `ties` among them, whose positions are too
many or too large for the per-base count) and against the per-base count on
the small inputs, bin/netSyntenic -host byte for byte against the reference's outputs
(tests/golden/make_netsyn_golden.py), the reference's error messages, the new
symbols, and the pipeline netSyntenic | NetFilterNonNested.perl.  Every
comparison is exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import netsyn_ref as NS

GAC_E_ARG = -1


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "netSyntenic")


def _host(*a):
    from genomealignmenttools_amd.gachain import depth_count_host
    return depth_count_host(*a)


SHAPES, BAD_ARGS = NS.SHAPES, NS.BAD_ARGS
shape_ref_test_block, shape_wide = NS.shape_ref_test_block, NS.shape_wide


@pytest.fixture(scope="module")
def expected():
    """the restatement's counts of every shape (threshold 2), computed once"""
    return {k: NS.depth_count(*f(), 2) for k, f in SHAPES.items()}


def test_restatement_equals_brute_force():
    cases = 0
    for seq, start, end, delta in NS.random_small_cases():
        for thr in (1, 2, 3):
            assert np.array_equal(NS.depth_count(seq, start, end, delta, thr),
                                  NS.depth_count_brute(seq, start, end, delta, thr))
        cases += 1
    assert cases == 200
    for a in (shape_ref_test_block(), NS.shape_ties_small()):
        for thr in (1, 2, 3):
            assert np.array_equal(NS.depth_count(*a, thr), NS.depth_count_brute(*a, thr))
    a = NS.shape_delta_range()
    nonzero = {}
    for thr in NS.DELTA_THRESHOLDS:
        want = NS.depth_count_brute(*a, thr)
        assert np.array_equal(NS.depth_count(*a, thr), want)
        nonzero[thr] = int((want != 0).sum())
    assert nonzero[1] > nonzero[255] > 0 and nonzero[1000] == 0
    for k in NS.ID_WIDTHS:
        a = NS.shape_id_width(k)
        want = NS.depth_count_brute(*a, 2)
        assert np.array_equal(NS.depth_count(*a, 2), want)
        # without bit k, sequence 2^k falls on sequence 0 and the counts change
        assert not np.array_equal(NS.depth_count(np.asarray(a[0]) & ~(1 << k), *a[1:], 2), want)
    assert NS.depth_count(*shape_wide(), 2).tolist() == [2**31 - 1] * 8
    assert NS.depth_count(*shape_wide(), 3).tolist() == [0] * 8


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_host_twin_equals_restatement(expected, shape):
    a = SHAPES[shape]()
    assert np.array_equal(_host(*a, 2), expected[shape])
    if shape == "ref_test":
        for thr in (1, 3):
            assert np.array_equal(_host(*a, thr), NS.depth_count_brute(*a, thr))
    if shape == "dense":
        assert expected[shape].max() > 0 and (expected[shape] == 0).sum() > 7000
    if shape == "stride":
        assert len(a[0]) == 2048 * 256 + 77 and expected[shape][-77:].any()
    if shape == "ties":  # (positions too large for the per-base count)
        assert (a[1] == a[2]).sum() > 300 and expected[shape].max() == 2**31 - 1
        assert len(np.unique(expected[shape])) > 5
    if shape == "ties_small":
        assert np.array_equal(expected[shape], NS.depth_count_brute(*a, 2))


def test_host_twin_edges_equal_per_base_count():
    """the device tests' small inputs through the host twin: the whole int8
    range of deltas under every threshold, the 31 key widths, the 200 random
    cases"""
    a = NS.shape_delta_range()
    for thr in NS.DELTA_THRESHOLDS:
        assert np.array_equal(_host(*a, thr), NS.depth_count_brute(*a, thr)), thr
    for k in NS.ID_WIDTHS:
        a = NS.shape_id_width(k)
        assert np.array_equal(_host(*a, 2), NS.depth_count_brute(*a, 2)), k
    for a in NS.random_small_cases():
        for thr in (1, 2, 3):
            assert np.array_equal(_host(*a, thr), NS.depth_count_brute(*a, thr))
    # the tied positions at the depths their stretches lie under, where the counts change
    small, large, seen = NS.shape_ties_small(), NS.shape_ties(), set()
    for thr in NS.ties_thresholds():
        want = NS.depth_count_brute(*small, thr)
        assert np.array_equal(NS.depth_count(*small, thr), want)
        assert np.array_equal(_host(*small, thr), want), thr
        assert np.array_equal(_host(*large, thr), NS.depth_count(*large, thr)), thr
        seen.add(want.tobytes())
    assert len(seen) > 4


def test_host_twin_small_and_bad_arguments():
    from genomealignmenttools_amd._lib import GacError, lib
    assert _host([], [], [], [], 2).shape == (0,)
    assert _host([7], [3], [9], [1], 1).tolist() == [6]
    assert _host([7], [3], [9], [1], 2).tolist() == [0]
    for name, a in BAD_ARGS.items():
        with pytest.raises(GacError) as e:
            _host(*a)
        assert e.value.code == GAC_E_ARG, name
    # 2n > INT32_MAX is refused before a buffer is read
    one = (C.c_int32 * 1)()
    p = C.cast(one, C.c_void_p)
    assert lib().gac_depth_count_host(2**30, p, p, p, p, 2, p) == GAC_E_ARG


def test_symbols_and_minor():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    for name in ("gac_depth_count", "gac_depth_count_host"):
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 5
    one = (C.c_int32 * 1)()
    p = C.cast(one, C.c_void_p)
    assert L.gac_depth_count(None, 1, p, p, p, p, 2, p) == GAC_E_ARG  # NULL context


@pytest.mark.parametrize("case", sorted(NS.CASES))
def test_tool_host_equals_reference(tmp_path, case):
    src, want = NS.CASES[case]
    out = str(tmp_path / "out.net")
    r = subprocess.run([_tool(), "-host", src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()


def test_tool_host_stdin_stdout():
    src, want = NS.CASES["synth11"]
    with open(src, "rb") as f:
        r = subprocess.run([_tool(), "-host", "stdin", "stdout"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(want, "rb").read()


def test_fixtures_hold_every_type():
    """what the goldens pin: all four types, non-zero qDup, a far and a
    touching fill, a dropped child list"""
    text = open(NS.CASES["edge"][1]).read()
    for t in ("type top", "type syn", "type inv", "type nonSyn", "qOver 0 qFar 0", "qOver 0 qFar 10",
              "score 1235 ", " gap 100 200 chrA + 200 200 qDup 3 tR 5\n"):
        assert t in text, t
    assert "bogus" not in text and "foo" not in text
    assert text.startswith("##matrix=16 91 -114\n# a comment between nets\nnet chr1 10000\n")
    ind = open(NS.CASES["indent"][1]).read()
    assert " id 2 " not in ind and "indented comment" not in ind and ind.startswith("#trailing meta\n")
    syn = open(NS.CASES["synth11"][1]).read()
    assert sum(" qDup 0 " not in s for s in syn.split("\n") if " fill " in s) == 274


with open(os.path.join(NS.NETSYN_DIR, "errors.json")) as _f:
    ERRORS = json.load(_f)


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_error_table(tmp_path, case):
    e = ERRORS[case]
    src = os.path.join(NS.NETSYN_DIR, e["input"]) if e["input"] else ""
    out = str(tmp_path / "out.net")
    args = [a.replace("{in}", src).replace("{out}", out) for a in e["args"]]
    r = subprocess.run([_tool(), "-host"] + args, capture_output=True, text=True)
    assert r.returncode == e["status"], r.stderr
    if e["status"]:
        assert r.stderr.split("\n")[0] == e["stderr"].replace("{in}", src)
    else:
        assert r.stderr == ""
    if e["output_empty"]:
        assert not os.path.exists(out) or os.path.getsize(out) == 0


def test_field_name_without_value_aborts(tmp_path):
    """(the reference reads past the line's words here)"""
    src = tmp_path / "in.net"
    src.write_text("net chr1 100\n fill 0 10 chrA + 0 10 id 1 ali\n")
    r = subprocess.run([_tool(), "-host", str(src), str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 255
    assert r.stderr == f"Field ali without a value line 2 of {src}\n"


with open(os.path.join(NS.NETFILTER_DIR, "typed_cases.json")) as _f:
    TYPED = json.load(_f)


@pytest.mark.parametrize("net", ["synth11", "cleaner", "big"])
@pytest.mark.parametrize("case", sorted(TYPED))
def test_pipeline_into_netfilter(net, case):
    """netSyntenic stdin stdout | NetFilterNonNested.perl, as the reference's
    FilterChains_Net_FilterNets.perl chains them"""
    from genomealignmenttools_amd._lib import BIN_DIR
    typed = subprocess.run([_tool(), "-host", NS.CASES[net][0], "stdout"], capture_output=True)
    assert typed.returncode == 0, typed.stderr
    r = subprocess.run([os.path.join(BIN_DIR, "NetFilterNonNested.perl"), "/dev/stdin"] + TYPED[case],
                       input=typed.stdout, capture_output=True)
    assert r.returncode == 0, r.stderr
    want = os.path.join(NS.NETFILTER_DIR, f"{net}.syn.{case}.out")
    assert r.stdout == open(want, "rb").read()
