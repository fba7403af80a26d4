"""chainPreNet on the GPU: Engine.prenet_keep (gac_prenet_keep: per-base first
cover by atomicMin, rounds of two passes) against the numpy restatement
(tests/prenet_ref.py) on the shapes of tests/test_prenet_cpu.py with the
rounds, passes and groups it must take, the fallbacks, the argument checks,
and the default (device) tool byte for byte against the reference's outputs.
Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import prenet_ref as PR

pytestmark = pytest.mark.gpu

GAC_E_ARG = -1
ON_DEVICE, FELL_ROUNDS, FELL_MEMORY = 0, 1, 2


@pytest.fixture(scope="module")
def expected():
    """the restatement's flags of every shape, computed once"""
    out = {}
    for k, f in PR.SHAPES.items():
        arrays, pad = f()
        out[k] = PR.prenet_keep(*arrays, pad=pad)
    return out


@pytest.fixture
def fc_bytes():
    """the per-base words' budget, for one test"""
    old = os.environ.get("GAC_PRENET_FC_BYTES")

    def set_(v):
        os.environ["GAC_PRENET_FC_BYTES"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("GAC_PRENET_FC_BYTES", None)
    else:
        os.environ["GAC_PRENET_FC_BYTES"] = old


@pytest.mark.parametrize("shape", sorted(PR.SHAPES))
def test_shapes(engine, expected, shape):
    arrays, pad = PR.SHAPES[shape]()
    keep, st = engine.prenet_keep(*arrays, pad=pad)
    assert keep.dtype == np.uint8 and np.array_equal(keep, expected[shape])
    n = len(expected[shape])
    if n == 0:
        assert st["rounds"] == 0 and st["passes"] == 0
        return
    assert st["fell_back"] == ON_DEVICE and st["kept"] == int(expected[shape].sum())
    assert st["passes"] == 2 * st["rounds"] and 1 <= st["rounds"] <= n
    used = (arrays[1] >= 0) & (arrays[2] >= 0)
    assert st["groups"] == (int(used.any()), int(used.any()))  # everything fits one group a side
    if pad == 0:
        assert st["rounds"] == 1
    if shape == "domino":
        assert st["rounds"] == 21 and st["kept"] == 21
    if shape == "all_dropped_but_first":
        assert st["rounds"] == 1


def test_max_rounds_falls_back(engine, expected):
    arrays, pad = PR.SHAPES["domino"]()
    keep, st = engine.prenet_keep(*arrays, pad=pad, max_rounds=3)
    assert np.array_equal(keep, expected["domino"])
    assert st["fell_back"] == FELL_ROUNDS and st["rounds"] == 3 and st["passes"] == 6
    assert st["kept"] == 21
    keep, st = engine.prenet_keep(*arrays, pad=pad, max_rounds=21)
    assert np.array_equal(keep, expected["domino"]) and st["fell_back"] == ON_DEVICE


def test_sequence_groups(engine, expected, fc_bytes):
    arrays, pad = PR.SHAPES["groups"]()
    fc_bytes(PR.GROUPS_FC_BYTES)
    keep, st = engine.prenet_keep(*arrays, pad=pad)
    assert st["groups"] == (3, 3) and st["fell_back"] == ON_DEVICE
    assert np.array_equal(keep, expected["groups"])
    arrays, pad = PR.SHAPES["domino"]()
    keep, st = engine.prenet_keep(*arrays, pad=pad)  # and many rounds over a buffer used again
    assert np.array_equal(keep, expected["domino"]) and st["rounds"] == 21


def test_sequence_over_the_budget_falls_back(engine, expected, fc_bytes):
    arrays, pad = PR.SHAPES["groups"]()
    fc_bytes(PR.GROUPS_FC_BYTES - 4)  # the largest sequence no longer fits
    keep, st = engine.prenet_keep(*arrays, pad=pad)
    assert st["fell_back"] == FELL_MEMORY and st["rounds"] == 0
    assert np.array_equal(keep, expected["groups"]) and st["kept"] == int(expected["groups"].sum())


@pytest.mark.parametrize("case", sorted(PR.BAD_ARGS))
def test_bad_arguments(engine, case):
    from genomealignmenttools_amd._lib import GacError
    arrays, pad = PR.BAD_ARGS[case]
    with pytest.raises(GacError) as e:
        engine.prenet_keep(*arrays, pad=pad)
    assert e.value.code == GAC_E_ARG


def test_kernel_timing_is_one_lap_per_call(engine):
    from genomealignmenttools_amd._lib import GAC_K_PRENET
    arrays, pad = PR.SHAPES["clip_pad1"]()
    engine.prof_enable(True, kernels=[GAC_K_PRENET])
    engine.prof_reset()
    try:
        engine.prenet_keep(*arrays, pad=pad)
        ms, laps = engine.prof_read(GAC_K_PRENET)
    finally:
        engine.prof_enable(False)
    assert laps == 1 and ms > 0


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "chainPreNet")


@pytest.mark.parametrize("case", sorted(PR.CASES))
def test_tool_device_equals_reference(tmp_path, case):
    src, ts, qs, opts, want = PR.CASES[case]
    out = str(tmp_path / "out.chain")
    r = subprocess.run([_tool(), "-verbose=2"] + opts + [src, ts, qs, out], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(want, "rb").read()
    assert "keep (GPU): " in r.stderr and "on the host" not in r.stderr
