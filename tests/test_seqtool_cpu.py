"""tools/lib/gac_seqtool.c on the CPU: the axt batch planner and the chain
subset builder that chainAntiRepeat, chainToAxt and netToAxt share.

tests/seqtool_driver.c is compiled here against tools/lib/*.c and libgachain
and run as a child process; the device is never opened.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

LIBSRC = os.path.join(REPO, "genomealignmenttools_amd", "csrc", "tools", "lib")
BUILT = os.path.join(GOLDEN, "antirepeat", "built", "in.chain")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    from genomealignmenttools_amd._lib import LIB_DIR
    exe = tmp_path_factory.mktemp("seqtool") / "drv"
    r = subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-I", os.path.join(REPO, "include"),
                        "-I", os.path.join(REPO, "genomealignmenttools_amd", "csrc"), "-I", LIBSRC,
                        os.path.join(REPO, "tests", "seqtool_driver.c")]
                       + sorted(glob.glob(os.path.join(LIBSRC, "*.c")))
                       + ["-o", str(exe), "-L", LIB_DIR, "-lgachain", f"-Wl,-rpath,{LIB_DIR}",
                          "-lz", "-lm", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _fields(stdout):
    out = {}
    for ln in stdout.splitlines():
        tag, *vals = ln.split()
        out[tag] = [int(v) for v in vals]
    return out


# ---------------------------------------------------------------- planner
def plan_rules(sym, budget):
    """The rules of gac_seqtool.h, restated."""
    size = [2 * s + 3 for s in sym]
    lo, nbytes, off = [], [], []
    for p, sz in enumerate(size):
        if not lo or nbytes[-1] + sz > budget:  # no batch yet, or it does not fit: a new one
            lo.append(p)
            nbytes.append(0)
        off.append(nbytes[-1])
        nbytes[-1] += sz
    cap = max([budget] + size)
    jobs = [0, 0] if not lo else [cap if len(lo) > 1 or cap > budget else nbytes[0],
                                  cap if len(lo) > 1 else 0]
    return dict(nbatch=[len(lo)], cap=[cap], jobs=jobs, lo=lo + [len(sym)], bytes=nbytes, off=off)


PLAN_CASES = {
    "no piece": ([], 100),
    "one piece": ([10], 100),                      # 23 bytes
    "one piece over the budget": ([100], 100),     # 203 bytes
    "exactly the budget": ([10, 10, 11], 71),      # 23 + 23 + 25 = 71: one batch, job 0 = 71
    "exact fit at the boundary": ([10, 10, 11, 4], 71),
    "one byte over at the boundary": ([10, 10, 12, 4], 72),  # 23 + 23 + 27 = 73 > 72
    "a large piece among small ones": ([1, 2, 200, 3, 1], 50),
    "1000 pieces": (list(np.random.default_rng(5).integers(0, 51, 1000)), 100),
}


@pytest.mark.parametrize("case", list(PLAN_CASES))
def test_plan(driver, case):
    sym, budget = PLAN_CASES[case]
    r = subprocess.run([driver, "plan", str(budget)], input=" ".join(str(int(s)) for s in sym),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got, want = _fields(r.stdout), plan_rules([int(s) for s in sym], budget)
    assert got == want
    lo, n = got["lo"], len(sym)
    assert lo[0] == 0 and lo[-1] == n and all(a < b for a, b in zip(lo, lo[1:]))  # tiles [0, n)
    for k in range(got["nbatch"][0]):
        assert got["off"][lo[k]] == 0
        assert got["bytes"][k] <= budget or lo[k + 1] - lo[k] == 1
    # what each case is there for
    if case == "no piece":
        assert got["nbatch"] == [0] and got["jobs"] == [0, 0]
    elif case == "one piece":
        assert got["jobs"] == [23, 0]
    elif case == "one piece over the budget":
        assert got["cap"] == [203] and got["jobs"] == [203, 0]
    elif case == "exactly the budget":
        assert got["nbatch"] == [1] and got["jobs"] == [71, 0]
    elif case == "exact fit at the boundary":
        assert lo == [0, 3, 4] and got["bytes"] == [71, 11] and got["jobs"] == [71, 71]
    elif case == "one byte over at the boundary":
        assert lo == [0, 2, 4] and got["bytes"] == [46, 38]
    elif case == "a large piece among small ones":
        assert got["cap"] == [403] and got["jobs"] == [403, 403] and lo == [0, 2, 3, 5]
    else:
        assert got["nbatch"][0] > 16


# --------------------------------------------------------- subset builder
@pytest.fixture(scope="module")
def built():
    from genomealignmenttools_amd.chainfile import read_chains
    return read_chains(BUILT)


def _index(names):
    """index of each name in order of first appearance (the file's name table)"""
    tab = {}
    return np.array([tab.setdefault(n, len(tab)) for n in names], np.int64)


@pytest.mark.parametrize("min_score,kind", [(0, "all"), (1e12, "none"), (20000, "some")])
def test_subset(driver, built, min_score, kind):
    ca = built
    assert ca.score.size == 271
    sel = np.flatnonzero(ca.score >= min_score)
    assert {"all": sel.size == 271, "none": sel.size == 0, "some": 0 < sel.size < 271}[kind]
    r = subprocess.run([driver, "subset", BUILT, repr(float(min_score)), "1"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = _fields(r.stdout)
    blocks = np.concatenate([np.arange(ca.blk_off[i], ca.blk_off[i + 1]) for i in sel]
                            + [np.zeros(0, np.int64)]).astype(np.int64)
    n_blk = ca.blk_off[sel + 1] - ca.blk_off[sel]
    assert got["desc"] == [1]
    assert got["sel"] == sel.tolist()
    assert got["boff"] == np.concatenate([[0], np.cumsum(n_blk)]).tolist()
    assert got["tseq"] == _index(ca.tname)[sel].tolist()
    assert got["qseq"] == _index(ca.qname)[sel].tolist()
    assert got["strand"] == ca.qstrand[sel].tolist()
    assert got["bt"] == ca.blk_t[blocks].tolist()
    assert got["bq"] == ca.blk_q[blocks].tolist()
    assert got["bs"] == ca.blk_size[blocks].tolist()


GOOD = "chain 5000 chrT1 60001 + 10 40 chrQ1 50003 + 10 40 {id}\n10\t5\t5\n15\n\n"
# overlapping blocks (a negative gap), as in the tools' usage-and-abort tests
BAD = "chain 9000 chrT2 60001 + 100 170 chrQ2 50003 + 100 165 {id}\n50\t0\t-5\n20\n\n"


def test_subset_negative_gap(driver, tmp_path):
    f = tmp_path / "two.chain"
    f.write_text(GOOD.format(id=76) + BAD.format(id=77))
    r = subprocess.run([driver, "subset", str(f), "0", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255
    assert "chain 77: blocks overlap (negative gap before block 1)" in r.stderr
    r = subprocess.run([driver, "subset", str(f), "0", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = _fields(r.stdout)
    assert got["sel"] == [0, 1] and got["boff"] == [0, 2, 4]
    assert got["bt"] == [10, 25, 100, 150] and got["bq"] == [10, 25, 100, 145]
    assert got["bs"] == [10, 15, 50, 20]
    # a chain that is not kept is not checked
    r = subprocess.run([driver, "subset", str(f), "9500", "1"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0 and _fields(r.stdout)["sel"] == []


def test_subset_abort_order(driver, tmp_path):
    """Of a file's defects the first in file order wins: a chain's own checks
    (here a target name the map lacks) run before its blocks are looked at,
    and after the blocks of every chain before it."""
    f = tmp_path / "overlap_first.chain"
    f.write_text(BAD.format(id=77) + GOOD.format(id=76))
    r = subprocess.run([driver, "subset", str(f), "0", "1", "chrT1"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 255
    assert "chain 77: blocks overlap" in r.stderr and "is not in" not in r.stderr
    f = tmp_path / "name_first.chain"
    f.write_text(GOOD.format(id=76) + BAD.format(id=77))
    r = subprocess.run([driver, "subset", str(f), "0", "1", "chrT1"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 255
    assert "chrT1 is not in t.2bit" in r.stderr and "blocks overlap" not in r.stderr
