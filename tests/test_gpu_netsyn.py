"""netSyntenic on the GPU: Engine.depth_count (gac_depth_count: events, sort,
depth scan, covered-length scan) against the numpy restatement
(tests/netsyn_ref.py) on the shapes of tests/test_netsyn_cpu.py, its argument
checks, and the default (device) tool byte for byte against the reference's
outputs and against the reference binary run here.  Every comparison is
exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import netsyn_ref as NS

pytestmark = pytest.mark.gpu

GAC_E_ARG = -1


@pytest.fixture(scope="module")
def expected():
    """the restatement's counts of every shape (threshold 2), computed once"""
    return {k: NS.depth_count(*f(), 2) for k, f in NS.SHAPES.items()}


@pytest.mark.parametrize("thr", [1, 2, 3])
def test_reference_test_block(engine, thr):
    a = NS.shape_ref_test_block()
    got = engine.depth_count(*a, thr)
    assert np.array_equal(got, NS.depth_count(*a, thr))
    assert np.array_equal(got, NS.depth_count_brute(*a, thr))


def test_empty_and_single(engine):
    assert engine.depth_count([], [], [], [], 2).shape == (0,)
    assert engine.depth_count([7], [3], [9], [1], 1).tolist() == [6]
    assert engine.depth_count([7], [3], [9], [1], 2).tolist() == [0]
    assert engine.depth_count([7], [3], [3], [1], 1).tolist() == [0]


@pytest.mark.parametrize("shape", ["dense", "sparse", "wide"])
def test_shapes(engine, expected, shape):
    got = engine.depth_count(*NS.SHAPES[shape](), 2)
    assert got.dtype == np.int32
    assert np.array_equal(got, expected[shape])
    if shape == "wide":  # the covered lengths sum to 4 * (2^31 - 1) > 2^32
        assert got.tolist() == [2**31 - 1] * 8


@pytest.mark.parametrize("case", sorted(NS.BAD_ARGS))
def test_bad_arguments(engine, case):
    from genomealignmenttools_amd._lib import GacError
    with pytest.raises(GacError) as e:
        engine.depth_count(*NS.BAD_ARGS[case])
    assert e.value.code == GAC_E_ARG


def test_too_many_ranges(engine):
    """2n > INT32_MAX is refused before a buffer is read"""
    from genomealignmenttools_amd._lib import lib
    one = (C.c_int32 * 1)()
    p = C.cast(one, C.c_void_p)
    assert lib().gac_depth_count(engine.h, 2**30, p, p, p, p, 2, p) == GAC_E_ARG


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "netSyntenic")


@pytest.mark.parametrize("case", sorted(NS.CASES))
def test_tool_device_equals_reference(tmp_path, case):
    src, want = NS.CASES[case]
    out = str(tmp_path / "out.net")
    r = subprocess.run([_tool(), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()


def test_tool_device_equals_reference_binary(tmp_path):
    from oracle.oracle import ref_tool
    ref = ref_tool("netSyntenic")
    if not os.path.exists(ref):
        pytest.fail(f"reference tool {ref} not built (make ref)")
    src = NS.CASES["synth11"][0]
    ours, theirs = str(tmp_path / "ours.net"), str(tmp_path / "ref.net")
    r = subprocess.run([_tool(), src, ours], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([ref, src, theirs], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(ours, "rb").read() == open(theirs, "rb").read()
