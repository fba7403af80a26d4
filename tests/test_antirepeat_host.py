"""chainAntiRepeat, host side (no GPU): the decision function reproduces which
chains the reference kept from the fixture counts, the .2bit reader keeps the
soft-mask runs, and the library exports the new ABI.

Fixtures: tests/golden/antirepeat (made by tests/golden/make_antirepeat_golden.py
with the reference's chainAntiRepeat)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

import antirepeat_ref as AR

AR_DIR = os.path.join(GOLDEN, "antirepeat")
SETS = {
    "synth11": (os.path.join(GOLDEN, "synth11"), os.path.join(AR_DIR, "synth11.npz")),
    "synth12": (os.path.join(GOLDEN, "synth12"), os.path.join(AR_DIR, "synth12.npz")),
    "built": (os.path.join(AR_DIR, "built"), os.path.join(AR_DIR, "built", "counts.npz")),
}
OPTIONS = {"default": (5000, 200000), "opts": (1000, 20000)}

NEW_SYMBOLS = ["gac_genome_want_softmask", "gac_genome_add_seq_masked", "gac_genome_decode_case",
               "gac_twobit_mask_runs", "gac_chain_composition", "gac_chain_composition_device",
               "gac_antirepeat_pass"]


@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("tag", sorted(OPTIONS))
def test_pass_equals_reference(name, tag):
    from genomealignmenttools_amd.gachain import antirepeat_pass
    z = np.load(SETS[name][1])
    min_score, no_check = OPTIONS[tag]
    kept = z[f"kept_{tag}"]
    checked = 0
    for c in range(len(kept)):
        if z["score"][c] < no_check:
            got = antirepeat_pass(z["score"][c], z["match"][c], z["rep"][c], z["total"][c], min_score)
            checked += 1
        else:
            got = True  # passes untouched (chainAntiRepeat.c:138)
        assert got == bool(kept[c]), (name, tag, c)
    assert checked > 0 and 0 < kept.sum() < len(kept)


def test_pass_branches():
    """Each branch by hand, with the reference's constants: no match at all
    (0/0 = NaN) is dropped; overOk <= 0 skips the adjustment; the adjusted
    score and the repeat score are compared with >=."""
    from genomealignmenttools_amd.gachain import antirepeat_pass
    assert not antirepeat_pass(1e9, [0, 0, 0, 0], 0, 100, 0)          # NaN: dropped even at minScore 0
    assert antirepeat_pass(5000, [25, 25, 25, 25], 50, 100, 5000)     # 5000 * 2 * 50 / 100 == 5000
    assert not antirepeat_pass(4999, [25, 25, 25, 25], 50, 100, 5000)
    assert antirepeat_pass(2500, [40, 40, 10, 10], 0, 100, 5000)      # best2 exactly 0.80: no adjustment
    assert not antirepeat_pass(100000, [50, 50, 0, 0], 0, 100, 5000)  # factor 0.01 -> 1000
    assert antirepeat_pass(600000, [50, 50, 0, 0], 0, 100, 5000)      # 6000.000000000005 >= 5000
    assert antirepeat_pass(10000, [45, 45, 5, 5], 0, 100, 5000)       # factor 0.51 -> 5100
    assert not antirepeat_pass(10000, [45, 45, 5, 5], 80, 100, 5000)  # then the repeat filter: 4000
    assert not antirepeat_pass(10000, [25, 25, 25, 25], 0, 0, 5000)   # total 0: NaN


@pytest.mark.parametrize("name", sorted(SETS))
def test_reader_keeps_mask_runs(name):
    from genomealignmenttools_amd.gachain import twobit_mask_runs
    n_runs = 0
    for f in ("t.2bit", "q.2bit"):
        path = os.path.join(SETS[name][0], f)
        g = AR.read_2bit(path)
        for i, nm in enumerate(g.names):
            st, sz = twobit_mask_runs(path, nm)
            assert np.array_equal(st, g.mruns[i][0]) and np.array_equal(sz, g.mruns[i][1]), (f, nm)
            n_runs += len(st)
    assert n_runs > 10


def test_reader_mask_runs_equal_synth_genome(tmp_path):
    """The runs the reader returns are synth.Genome's own (the genomes of
    tests/golden/synth11, regenerated from its seed, and a file written here)."""
    from genomealignmenttools_amd import synth
    from genomealignmenttools_amd.gachain import twobit_mask_runs
    tg, qg, _ = synth.small_case(seed=11, n_chains=400, max_blocks=400, n_frac=0.01)
    for g, f in ((tg, "t.2bit"), (qg, "q.2bit")):
        mine = str(tmp_path / f)
        synth.write_2bit(g, mine)
        for path in (mine, os.path.join(GOLDEN, "synth11", f)):
            for i, nm in enumerate(g.names):
                st, sz = twobit_mask_runs(path, nm)
                assert len(st) > 0
                assert np.array_equal(st, g.mruns[i][0]) and np.array_equal(sz, g.mruns[i][1])
    from genomealignmenttools_amd._lib import GacError
    with pytest.raises(GacError):
        twobit_mask_runs(os.path.join(GOLDEN, "synth11", "t.2bit"), "no_such_sequence")


def test_abi_exports_new_symbols():
    from genomealignmenttools_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
        assert s in _lib.EXPORTED, s
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "gachain.h")).read()
    for s in NEW_SYMBOLS:
        assert s + "(" in hdr, s
