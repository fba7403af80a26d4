"""bin/chainNet -rescore on the GPU with the nets released under the writers
(the default) and after them (GAC_EARLY_FREE=0): the same nets, and the
reference's (tests/golden/synth*, made with the reference chainNet).  The
CPU side of the same check, with the shapes that can go wrong, is
test_net_release_cpu.py; the full-size C5 nets are checked by sha256 in
test_gpu_configs.py."""
import os
import subprocess

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _nets(d, out, env):
    from genomealignmenttools_amd._lib import BIN_DIR
    p = lambda x: os.path.join(d, x)
    e = {k: v for k, v in os.environ.items() if k != "GAC_EARLY_FREE"}
    r = subprocess.run([os.path.join(BIN_DIR, "chainNet"), p("in.chain"), p("t.sizes"), p("q.sizes"),
                        out + ".t.net", out + ".q.net", "-rescore", f"-tNibDir={p('t.2bit')}",
                        f"-qNibDir={p('q.2bit')}", "-linearGap=loose"],
                       capture_output=True, text=True, timeout=600, env=dict(e, **env))
    assert r.returncode == 0, r.stderr
    return open(out + ".t.net", "rb").read(), open(out + ".q.net", "rb").read()


@pytest.mark.parametrize("seed", [11, 12])
def test_release_under_the_writers_keeps_the_nets(seed, tmp_path):
    d = os.path.join(GOLDEN, f"synth{seed}")
    want = tuple(open(os.path.join(d, f"rescore.{s}.net"), "rb").read() for s in "tq")
    on = _nets(d, str(tmp_path / "on"), {})
    off = _nets(d, str(tmp_path / "off"), {"GAC_EARLY_FREE": "0"})
    assert on == off
    assert on[0] == want[0], "target net vs the reference's"
    assert on[1] == want[1], "query net vs the reference's"
