"""chainPreNet without a GPU: the restatement (tests/prenet_ref.py) against the
reference's outputs (tests/golden/make_prenet_golden.py), the host twin
(gac_prenet_keep_host) against the restatement on every shape, bin/chainPreNet
-host byte for byte against the reference's outputs and its error table, and
the new symbols.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import prenet_ref as PR

GAC_E_ARG = -1


def _tool():
    from genomealignmenttools_amd._lib import BIN_DIR
    return os.path.join(BIN_DIR, "chainPreNet")


def _host(arrays, pad):
    from genomealignmenttools_amd.gachain import prenet_keep_host
    return prenet_keep_host(*arrays, pad=pad)


@pytest.fixture(scope="module")
def expected():
    """the restatement's flags of every shape, computed once"""
    out = {}
    for k, f in PR.SHAPES.items():
        arrays, pad = f()
        out[k] = PR.prenet_keep(*arrays, pad=pad)
    return out


@pytest.mark.parametrize("case", sorted(PR.CASES))
def test_restatement_equals_reference(case):
    src, ts, qs, opts, want = PR.CASES[case]
    text = open(src).read()
    pad, hap = PR.case_options(opts)
    mine = PR.file_keep(text, PR.read_sizes(ts), PR.read_sizes(qs), pad, hap)
    assert np.array_equal(mine, PR.kept_mask(text, open(want).read()))


def test_shapes_hold_what_they_are_for(expected):
    """the domino's 21 of 41 (a rule that lets dropped chains cover keeps 1),
    a pad that decides, clipping at both ends, blocks of no bases"""
    assert int(expected["domino"].sum()) == 21 and expected["domino"][:5].tolist() == [1, 0, 1, 0, 1]
    assert expected["clip_pad1"].tolist() != expected["clip_pad5"].tolist()
    assert expected["zero_blocks"].tolist() != expected["zero_blocks_pad0"].tolist()
    assert expected["all_dropped_but_first"].tolist() == [1] + [0] * 60
    assert expected["same_id_both_sides"].tolist() == [1, 1, 0, 0]
    assert expected["skipped_between"].tolist() == [1, 0, 1, 0, 0, 1]
    assert expected["pad_over_own_gap"].tolist() == [1, 0, 0, 1]
    for k in ("straddle", "many_blocks", "groups", "random_pad0", "random_pad1", "random_pad3"):
        assert 0 < int(expected[k].sum()) < len(expected[k]), k


@pytest.mark.parametrize("shape", sorted(PR.SHAPES))
def test_host_twin_equals_restatement(expected, shape):
    arrays, pad = PR.SHAPES[shape]()
    keep, st = _host(arrays, pad)
    assert keep.dtype == np.uint8 and np.array_equal(keep, expected[shape])
    assert st["kept"] == int(expected[shape].sum()) and st["rounds"] == 0 and st["fell_back"] == 0


@pytest.mark.parametrize("case", sorted(PR.BAD_ARGS))
def test_host_twin_bad_arguments(case):
    from genomealignmenttools_amd._lib import GacError
    arrays, pad = PR.BAD_ARGS[case]
    with pytest.raises(GacError) as e:
        _host(arrays, pad)
    assert e.value.code == GAC_E_ARG


def test_symbols_and_minor():
    from genomealignmenttools_amd import _lib
    L = _lib.lib()
    for name in ("gac_prenet_keep", "gac_prenet_keep_host"):
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 6
    one = (C.c_int64 * 2)()
    p = C.cast(one, C.c_void_p)
    # a NULL context, and more chains than a call takes, before a buffer is read
    assert L.gac_prenet_keep(None, 1, p, p, p, 0, p, p, p, 1, p, 1, p, 1, 0, p, None) == GAC_E_ARG
    assert L.gac_prenet_keep_host(2**31 - 2, p, p, p, 0, p, p, p, 1, p, 1, p, 1, p, None) == GAC_E_ARG
    assert L.gac_prenet_keep_host(1, p, p, p, 2**31 - 2, p, p, p, 1, p, 1, p, 1, p, None) == GAC_E_ARG
    assert L.gac_prenet_keep_host(0, None, None, None, 0, None, None, None, 0, None, 0, None, 1, None,
                                  None) == 0


@pytest.mark.parametrize("case", sorted(PR.CASES))
def test_tool_host_equals_reference(tmp_path, case):
    src, ts, qs, opts, want = PR.CASES[case]
    out = str(tmp_path / "out.chain")
    r = subprocess.run([_tool(), "-host"] + opts + [src, ts, qs, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "" and open(out, "rb").read() == open(want, "rb").read()


def test_tool_host_stdin_stdout_and_dots():
    src, ts, qs, _opts, want = PR.CASES["built"]
    with open(src, "rb") as f:
        r = subprocess.run([_tool(), "-host", "stdin", ts, qs, "stdout"], stdin=f, capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == open(want, "rb").read()
    # 49 chains, a dot at the first and then at every 10th
    r = subprocess.run([_tool(), "-host", "-dots=10", src, ts, qs, "/dev/null"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"....."


with open(os.path.join(PR.PRENET_DIR, "errors.json")) as _f:
    ERRORS = json.load(_f)


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_error_table(tmp_path, case):
    e = ERRORS[case]
    out = str(tmp_path / "out.chain")
    paths = {"{in}": os.path.join(PR.PRENET_DIR, e["input"]), "{t}": os.path.join(PR.PRENET_DIR, e["t_sizes"]),
             "{q}": os.path.join(PR.PRENET_DIR, e["q_sizes"]), "{out}": out}
    r = subprocess.run([_tool(), "-host"] + [paths.get(a, a) for a in e["args"]], capture_output=True,
                       text=True)
    assert r.returncode == e["status"], r.stderr
    if e["status"]:
        want = e["stderr"]
        for tag, p in paths.items():
            want = want.replace(tag, p)
        assert r.stderr.split("\n")[0] == want
    else:
        assert r.stderr == ""
    if e["output_empty"]:
        assert not os.path.exists(out) or os.path.getsize(out) == 0


def test_block_outside_the_sizes_file_is_refused(tmp_path):
    """(the reference writes outside its bitmap here)"""
    src, _ts, qs, _opts, _want = PR.CASES["built"]
    small = tmp_path / "t.sizes"
    small.write_text("chrT1\t4000\nchrT2\t3000\nchrS\t2000\n")
    r = subprocess.run([_tool(), "-host", src, str(small), qs, str(tmp_path / "o")], capture_output=True,
                       text=True)
    assert r.returncode == 255 and "outside sequences" in r.stderr
