"""netToAxt without a GPU: the restatement (tests/netaxt_ref.py) against the
fixtures made with the reference's tool (tests/golden/make_netaxt_golden.py),
the record categories the GPU tests rely on, deliberately wrong restatements
that the fixtures must catch, and the new symbols of the library."""
import ctypes as C

import pytest

import netaxt_ref as NX

CASES = sorted(NX.CASES)


@pytest.fixture(scope="module")
def outputs():
    """the restatement's (axt, gapOut, counts) of every case, computed once"""
    out = {}
    for name, tag in CASES:
        kw = NX.CASES[(name, tag)][1]
        out[(name, tag)] = NX.tool_output(*NX.case_inputs(name, bool(kw.get("q_chain"))), **kw)
    return out


@pytest.mark.parametrize("name,tag", CASES)
def test_restatement_reproduces_fixture(outputs, name, tag):
    assert outputs[(name, tag)][0] == NX.golden(name, tag)


def test_gapout_fixture(outputs):
    assert outputs[("synth11", "default")][1] == NX.golden("synth11", "gapout")
    assert NX.golden("synth11", "gapout").count(b"\n") > 100


def test_categories(outputs):
    total = dict.fromkeys(NX.CATEGORIES, 0)
    for (name, tag), (text, _, cnt) in outputs.items():
        for k in ("head_cut", "tail_cut", "one_block_both", "insert_split", "meta_between"):
            total[k] += cnt[k]
        for k, v in NX.row_categories(NX.golden(name, tag)).items():
            total[k] += v
        total["multi_net"] += cnt["nets"] > 1
    assert all(v > 0 for v in total.values()), total
    # the counts the issue's feasibility check found in the T nets
    t11, t12 = outputs[("synth11", "nosplit")][2], outputs[("synth12", "default")][2]
    assert (t11["ranges"], t11["head_cut"], t11["tail_cut"], t11["one_block_both"]) == (319, 24, 23, 1)
    assert (t12["head_cut"], t12["tail_cut"], t12["one_block_both"]) == (14, 9, 1)
    # -maxGap=100000 is what pins splitting at inserts
    assert outputs[("synth11", "maxgap100000")][2]["records"] == 754
    assert outputs[("synth11", "maxgap100000_nosplit")][2]["records"] == 717
    assert NX.golden("synth11", "qchain").count(b" - ") == 505
    # a '#' line between two nets comes out before the first net's records
    text = NX.golden("built", "default")
    assert text.index(b"# between the first two nets") < text.index(b"\n0 chrT")
    assert text.startswith(b"# nets of antirepeat/built, t side\n")
    last = text.rindex(b"# after the last net\n")
    # (read with the last net: after the first net's records, before the last net's)
    assert text.index(b" chrT1 ") < last < text.index(b" chrT2 ")


@pytest.mark.parametrize("wrong", NX.WRONG)
def test_wrong_restatement_is_caught(wrong):
    caught = []
    for name, tag in CASES:
        kw = NX.CASES[(name, tag)][1]
        if wrong.startswith("swap") and not kw.get("q_chain"):
            continue
        try:
            got = NX.tool_output(*NX.case_inputs(name, bool(kw.get("q_chain"))), wrong=(wrong,), **kw)[0]
        except (ValueError, AssertionError, IndexError):
            got = None  # (the mistake left a range without blocks or a bad gap)
        if got != NX.golden(name, tag):
            caught.append((name, tag))
    assert caught, wrong


def test_symbols_and_null_context():
    from genomealignmenttools_amd._lib import lib
    L = lib()
    for name in ("gac_axt_cut", "gac_axt_measure_clip", "gac_axt_measure_clip_device",
                 "gac_axt_render_clip", "gac_axt_render_clip_device", "gac_axt_job_submit_clip"):
        assert hasattr(L, name), name
    assert L.gac_abi_version() == 1 and L.gac_abi_minor() >= 2
    GAC_E_ARG = -1
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    pieces, first, n = C.c_void_p(1), C.c_void_p(1), C.c_int64(7)
    assert L.gac_axt_cut(None, None, p, 1, 100, C.byref(pieces), C.byref(first), C.byref(n)) == GAC_E_ARG
    assert pieces.value is None and first.value is None and n.value == 0
    assert L.gac_axt_measure_clip(None, None, p, 1, p, p, p, p) == GAC_E_ARG
    assert L.gac_axt_measure_clip_device(None, None, p, 1, p, p, p, p, None) == GAC_E_ARG
    assert L.gac_axt_render_clip(None, None, p, 1, None, p, 8) == GAC_E_ARG
    assert L.gac_axt_render_clip_device(None, None, p, 1, None, p, 8, None) == GAC_E_ARG
    assert L.gac_axt_job_submit_clip(None, None, p, 1, p, 8) == GAC_E_ARG
