"""chainToAxt and netToAxt when nothing is rendered: no kept chain, no piece, no
batch, no render job opened (tools/lib/gac_seqtool*.c).  The other paths of the
shared front end are covered by the tools' own byte-identity, small-batch and
abort tests."""
import os
import subprocess

import pytest
# torch before libgachain, for the reason written at the top of
# test_gpu_antirepeat.py
import torch  # noqa: F401

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BUILT = os.path.join(GOLDEN, "antirepeat", "built")


def _run(tool, args):
    from genomealignmenttools_amd._lib import BIN_DIR
    return subprocess.run([os.path.join(BIN_DIR, tool)] + args, capture_output=True, timeout=120)


def _built():
    return [os.path.join(BUILT, f) for f in ("in.chain", "t.2bit", "q.2bit")]


@pytest.mark.parametrize("bed", [False, True])
def test_chaintoaxt_no_chain_kept(bed, tmp_path):
    """-minScore above every chain of `built` (the highest scores 200000): an
    empty set is uploaded, nothing is rendered, the output is empty."""
    out = tmp_path / "out"
    r = _run("chainToAxt", _built() + [str(out), "-minScore=1e12", "-verbose=2"] + ["-bed"] * bed)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b""
    if not bed:
        assert b"0 pieces in 0 batches of at most 67108864 text bytes\n" in r.stderr


def test_nettoaxt_net_without_fill(tmp_path):
    """A net file whose only net has no fill.  The tool before the shared front
    end exited 0 with an empty output, printing "0 ranges, 0 pieces in 0
    batches of at most 67108864 text bytes" under -verbose=2 (an empty chain set
    is uploaded and cut; no render job is opened): that is what is asserted."""
    chain, t2, q2 = _built()
    with open(chain) as f:
        head = next(ln for ln in f if ln.startswith("chain ")).split()
    net = tmp_path / "empty.net"
    net.write_text(f"net {head[2]} {head[3]}\n")  # the first chain's target and its size
    out = tmp_path / "out.axt"
    r = _run("netToAxt", [str(net), chain, t2, q2, str(out), "-verbose=2"])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b""
    assert b"0 ranges, 0 pieces in 0 batches of at most 67108864 text bytes\n" in r.stderr
