"""chainToPsl / chainToPslBasic without a GPU: the numpy restatement
(tests/pslout_ref.py) against the fixtures made with the reference's tools
(tests/golden/make_psl_golden.py), deliberately wrong restatements that the
fixtures must catch, the new entry points of the C ABI, and the host-only
bin/chainToPslBasic byte for byte."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import pslout_ref as PS

GAC_E_ARG = -1
# the bases of each set by class (pslout_ref.CLASSES): '-' chains, matches on
# an upper-case target, matches on a lower-case target (repMatch), mismatches
# on a lower-case target, N on the target only, N on the query only, N
# positions on a lower-case target
TABLE = {
    "built": (135, None, 20544, 3784, 437, 270, 358),
    "synth11": (213, None, 10815, 3295, 655, 435, 77),
    "synth12": (125, None, 8075, 1706, 739, 217, 235),
}
N_CHAINS = {"built": 271, "synth11": 400, "synth12": 250, "edge": 8}
_cache = {}


def load(name):
    if name not in _cache:
        _cache[name] = PS.load(name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(PS.SETS))
def test_restatement_reproduces_reference(name):
    tg, qg, ca = load(name)
    assert ca.n == N_CHAINS[name]
    z = np.load(os.path.join(PS.PSL_DIR, f"{name}.counts.npz"))
    cnt = PS.counts(tg, qg, ca)
    assert np.array_equal(cnt, z["counts"])
    assert np.array_equal(PS.inserts(ca), z["inserts"])
    want = PS.fixture(f"{name}.psl")
    assert PS.tool_output(tg, qg, ca) == want
    assert PS.basic_output(ca) == PS.fixture(f"{name}.basic.psl")
    # the .npz holds the reference's own first four columns
    cols = np.array([[int(v) for v in line.split(b"\t")[:4]] for line in want.splitlines()], np.int64)
    assert np.array_equal(cols, z["counts"])
    assert np.array_equal(z["counts"].sum(1), [ca.blocks(c)[2].sum() for c in range(ca.n)])


@pytest.mark.parametrize("wrong", PS.WRONG)
def test_wrong_restatements_are_caught(wrong):
    """Each deliberate mistake changes the output of at least one set, so the
    fixtures tell it from the reference's behaviour."""
    differs = [name for name in sorted(PS.SETS)
               if PS.tool_output(*load(name), wrong={wrong}) != PS.fixture(f"{name}.psl")]
    assert differs, wrong


@pytest.mark.parametrize("name", sorted(TABLE))
def test_fixture_classes(name):
    """What the sets must hold for the other tests to mean anything."""
    cls = PS.classes(*load(name))
    got = tuple(cls[k] for k in PS.CLASSES)
    assert np.array_equal(np.load(os.path.join(PS.PSL_DIR, f"{name}.counts.npz"))["classes"], got)
    assert got[1] >= 38000
    assert [g for g, w in zip(got, TABLE[name]) if w is not None] == \
        [w for w in TABLE[name] if w is not None]


def test_edge_chain_holds_its_cases():
    tg, qg, ca = load("edge")
    text = open(PS.SETS["edge"][1]).read()
    lines = text.split("\n")
    assert lines[0].startswith("#") and lines[-2].startswith("#") and text.count("\n#") >= 5
    assert sum(len(l.split()) == 12 for l in lines if l.startswith("chain ")) == 1  # id-less
    cnt = PS.counts(tg, qg, ca)
    sizes = [ca.blocks(c)[2] for c in range(ca.n)]
    assert any(len(s) == 1 and s[0] == 1 for s in sizes)                         # one base
    assert any(cnt[c, 3] == sizes[c].sum() and cnt[c, 3] > 1 for c in range(ca.n))  # all N
    assert any(cnt[c, 0] == 0 and cnt[c, 2] > 0 for c in range(ca.n))            # target all lower
    qs = qg.sizes
    assert sum(bool(ca.qstrand[c]) and ca.qsize[c] != qs[ca.qname[c]] for c in range(ca.n)) == 2


def test_symbols_and_null_arguments():
    from genomealignmenttools_amd._lib import lib
    L = lib()
    for name in ("gac_chain_psl_counts", "gac_chain_psl_counts_device"):
        assert isinstance(getattr(L, name), C._CFuncPtr), name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 3
    buf = np.zeros(8, np.int64)
    assert L.gac_chain_psl_counts(None, None, buf.ctypes.data) == GAC_E_ARG
    assert L.gac_chain_psl_counts_device(None, None, buf.ctypes.data, None) == GAC_E_ARG
    from genomealignmenttools_amd.gachain import Engine
    assert callable(Engine.chain_psl_counts) and callable(Engine.chain_psl_counts_device)


# ------------------------------------------------------- bin/chainToPslBasic
USAGE = b"chainToPslBasic - Basic conversion chain file to psl format\nusage:\n   chainToPsl in.chain out.psl\n"


def _basic(args, **kw):
    from genomealignmenttools_amd._lib import BIN_DIR
    return subprocess.run([os.path.join(BIN_DIR, "chainToPslBasic")] + args, capture_output=True,
                          timeout=120, **kw)


@pytest.mark.parametrize("name", sorted(PS.SETS))
def test_basic_tool_byte_identical(name, tmp_path):
    out = tmp_path / "out.psl"
    r = _basic([PS.SETS[name][1], str(out)])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == PS.fixture(f"{name}.basic.psl")


def test_basic_tool_stdin_stdout_gz(tmp_path):
    want = PS.fixture("edge.basic.psl")  # (edge.chain has an id-less header and '#' lines)
    text = open(PS.SETS["edge"][1], "rb").read()
    r = _basic(["stdin", "stdout"], input=text)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    gz = tmp_path / "in.chain.gz"
    gz.write_bytes(gzip.compress(text))
    r = _basic([str(gz), str(tmp_path / "o"), "-verbose=0"])
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o").read_bytes() == want


def test_basic_tool_usage_and_unknown_option(tmp_path):
    r = _basic([PS.SETS["edge"][1]])  # argc != 3
    assert r.returncode == 255 and r.stderr.startswith(USAGE)
    r = _basic([PS.SETS["edge"][1], str(tmp_path / "o"), "extra"])
    assert r.returncode == 255 and r.stderr.startswith(USAGE)
    r = _basic([PS.SETS["edge"][1], str(tmp_path / "o"), "-bogus=1"])  # optionInit, empty spec
    assert r.returncode == 255 and b"bogus" in r.stderr
    assert not (tmp_path / "o").exists() or (tmp_path / "o").read_bytes() == b""
