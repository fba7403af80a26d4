"""chainToAxt without a GPU: the numpy restatement (tests/axtout_ref.py)
against the fixtures made with the reference's tool, gac_axt_split against the
restatement's pieces, and deliberately wrong restatements that the fixtures
must catch."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN

import antirepeat_ref as AR
import axtout_ref as AX

AX_DIR = os.path.join(GOLDEN, "axtout")
SETS = {"built": os.path.join(GOLDEN, "antirepeat", "built"), "synth11": os.path.join(GOLDEN, "synth11"),
        "synth12": os.path.join(GOLDEN, "synth12")}
KW = {
    "default": {},
    "opts": dict(max_gap=10, min_id=90, min_score=3000),
    "bed": dict(bed=True, min_id=70),
    "maxchain": dict(max_chain=50),
}
CASES = [("built", t) for t in sorted(KW)] + [("synth11", "default"), ("synth12", "default")]
GAC_E_ARG, GAC_E_FORMAT = -1, -4
_cache = {}


def golden(name, tag):
    return gzip.open(os.path.join(AX_DIR, f"{name}.{tag}.gz"), "rb").read()


def load(name):
    """(Text of t, Text of q, ChainArrays) of a set, read once."""
    if name not in _cache:
        from genomealignmenttools_amd.chainfile import read_chains
        d = SETS[name]
        _cache[name] = (AX.Text(AR.read_2bit(os.path.join(d, "t.2bit"))),
                        AX.Text(AR.read_2bit(os.path.join(d, "q.2bit"))),
                        read_chains(os.path.join(d, "in.chain")))
    return _cache[name]


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_reproduces_reference(name, tag):
    tt, qt, ca = load(name)
    assert AX.tool_output(tt, qt, ca, **KW[tag]) == golden(name, tag)


def test_fixture_categories():
    """What the default output on `built` must hold for the other tests to
    mean anything; -maxChain changed nothing in the reference."""
    text = golden("built", "default")
    assert golden("built", "maxchain") == text
    lines = text.split(b"\n")
    heads, trow, qrow = lines[0:-1:4], lines[1:-1:4], lines[2:-1:4]
    assert len(heads) == 1594
    assert sum(h.split()[7] == b"-" for h in heads) == 831
    assert sum(int(h.split()[8]) < 0 for h in heads) == 181
    assert sum(b"-" in t for t in trow) == 41 and sum(b"-" in q for q in qrow) == 52
    assert sum(b"N" in t or b"N" in q for t, q in zip(trow, qrow)) > 0
    assert sum(b"n" in t or b"n" in q for t, q in zip(trow, qrow)) == 28


@pytest.mark.parametrize("wrong", AX.WRONG)
def test_wrong_restatements_are_caught(wrong):
    """Each deliberate mistake changes the output for at least one option set
    of `built`, so the fixtures tell it from the reference's behaviour."""
    tt, qt, ca = load("built")
    differs = [tag for tag in sorted(KW)
               if AX.tool_output(tt, qt, ca, wrong={wrong}, **KW[tag]) != golden("built", tag)]
    assert differs, wrong


def _split(ca, max_gap):
    from genomealignmenttools_amd.gachain import Engine
    z = np.zeros(ca.n, np.int32)
    return Engine.axt_split(z, z, ca.qstrand, ca.blk_off, ca.blk_t, ca.blk_q, ca.blk_size, max_gap)


@pytest.mark.parametrize("name", sorted(SETS))
def test_split_equals_restatement(name):
    _, _, ca = load(name)
    for max_gap in (100, 10, 1, 0):
        want = AX.split(ca, max_gap)
        got = _split(ca, max_gap)
        assert got.shape == want.shape and np.array_equal(got, want), max_gap
    assert len(AX.split(ca, 10)) > len(AX.split(ca, 100)) >= ca.n


def test_split_negative_gap_and_edges():
    from genomealignmenttools_amd._lib import GacError, lib
    from genomealignmenttools_amd.gachain import Engine
    z2 = np.zeros(2, np.int32)
    off = np.array([0, 2, 4], np.int64)
    # chain 1: the second block starts inside the first on the query
    bt = np.array([0, 10, 100, 120], np.int32)
    bq = np.array([0, 10, 50, 55], np.int32)
    bs = np.array([10, 5, 10, 10], np.int32)
    with pytest.raises(GacError) as ei:
        Engine.axt_split(z2, z2, np.zeros(2, np.uint8), off, bt, bq, bs)
    assert ei.value.code == GAC_E_FORMAT and "chain 1" in str(ei.value)
    # abutting blocks stay together; an empty chain gives no piece; no chains, no pieces
    bq[3] = 60
    got = Engine.axt_split(z2, z2, np.zeros(2, np.uint8), off, bt, bq, bs)
    assert got.tolist() == [[0, 0, 15, 0, 2], [1, 100, 130, 0, 2]]
    got = Engine.axt_split(z2, z2, np.zeros(2, np.uint8), np.array([0, 0, 4], np.int64), bt, bq, bs)
    assert got[:, 0].tolist() == [1, 1] and got[:, 3].tolist() == [0, 2]  # double-sided cuts
    e = np.zeros(0, np.int32)
    assert Engine.axt_split(e, e, np.zeros(0, np.uint8), np.zeros(1, np.int64), e, e, e).shape == (0, 5)
    assert lib().gac_axt_split(None, 100, None, None) == GAC_E_ARG


def test_symbols_exported():
    from genomealignmenttools_amd._lib import lib
    L = lib()
    for name in ("gac_axt_split", "gac_axt_free", "gac_axt_measure", "gac_axt_measure_device",
                 "gac_axt_render", "gac_axt_render_device", "gac_axt_job_open", "gac_axt_job_submit",
                 "gac_axt_job_wait", "gac_axt_job_close", "gac_abi_minor"):
        assert isinstance(getattr(L, name), C._CFuncPtr), name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 1
    buf = np.zeros(8, np.int64)
    p = buf.ctypes.data
    # no context: an error, not a crash
    assert L.gac_axt_measure(None, None, p, 1, p, p, p, p) == GAC_E_ARG
    assert L.gac_axt_render(None, None, p, 1, None, p, 8) == GAC_E_ARG
