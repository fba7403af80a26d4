"""gac_par_output's direct path: for a regular file the workers write their
own groups of runs at file offsets (pwrite) instead of handing every run to
one in-order writer.  That changes how the bytes reach the file, never the
bytes: every case below runs with the direct path on and off
(GAC_OUT_DIRECT=0), with 1, 3 and 8 threads, with the release hook on and off
(GAC_EARLY_FREE=0), and is compared byte for byte with the goldens and with
the other path.  GAC_OUT_GROUP_BYTES=1 makes every run a group of its own, so
the offsets are resolved across as many groups as there are runs.

oracle/_build/chainNet_cpu is the real tool on the CPU stand-in of the device
ABI (as in test_net_release_cpu.py); bin/chainSort writes through the FILE*
form of the callback.  Inputs: tests/golden/synth11.  TEST INFRASTRUCTURE
only; no device involved."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "oracle", "_build", "chainNet_cpu")
D11 = os.path.join(ROOT, "tests", "golden", "synth11")
THREADS = (1, 3, 8)
HOOK = ({}, {"GAC_EARLY_FREE": "0"})
PATHS = {"direct": {}, "ordered": {"GAC_OUT_DIRECT": "0"}}
KNOBS = ("GAC_EARLY_FREE", "GAC_THREADS", "GAC_OUT_DIRECT", "GAC_OUT_GROUP_BYTES", "GAC_OUT_WRITERS",
         "GAC_OUTPUT_MMAP_MIN", "GAC_TIMING", "OMP_NUM_THREADS")
DIRECT_LINE = re.compile(r"\[gac_par_output\] direct: (\d+) runs in (\d+) groups \((\d+) kept for a later "
                         r"turn\), (\d+) bytes at offset (\d+)")


@pytest.fixture(scope="module")
def tool():
    # one build at a time: pytest-xdist workers may reach this together
    import fcntl
    os.makedirs(os.path.join(ROOT, "oracle", "_build"), exist_ok=True)
    with open(os.path.join(ROOT, "oracle", "_build", ".cpu-chainnet.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "cpu-chainnet"], cwd=ROOT, capture_output=True,
                           text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return TOOL


@pytest.fixture(scope="module")
def golden():
    return (open(os.path.join(D11, "plain.t.net"), "rb").read(),
            open(os.path.join(D11, "plain.q.net"), "rb").read())


def _env(nt, *more):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(GAC_THREADS=str(nt), GAC_OUT_GROUP_BYTES="1", GAC_TIMING="1")
    for m in more:
        e.update(m)
    return e


def _cmd(tnet, qnet, chain=None):
    return [TOOL, chain or os.path.join(D11, "in.chain"), os.path.join(D11, "t.sizes"),
            os.path.join(D11, "q.sizes"), str(tnet), str(qnet)]


def _run(cmd, env, check=True, **kw):
    r = subprocess.run(cmd, stderr=subprocess.PIPE, timeout=120, env=env, **kw)
    if check:
        assert r.returncode == 0, r.stderr[-2000:]
    return r


def _direct_lines(r):
    return [tuple(map(int, m.groups())) for m in DIRECT_LINE.finditer(r.stderr.decode())]


def _read(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.mark.parametrize("hook", HOOK, ids=["hook", "nohook"])
@pytest.mark.parametrize("nt", THREADS)
def test_file_new_and_over_a_longer_one(tool, golden, tmp_path, nt, hook):
    """A new file, and a file that exists and is longer than the new text: it
    ends at exactly the new length.  The direct path is really taken, with
    one group per run, and the ordered one really is not."""
    for path, knob in PATHS.items():
        env = _env(nt, hook, knob)
        t, q = tmp_path / f"{path}.t.net", tmp_path / f"{path}.q.net"
        for rnd in ("new", "over"):
            if rnd == "over":
                t.write_bytes(golden[0] + b"x" * 100_000)
                q.write_bytes(b"y" * (len(golden[1]) + 1))
            r = _run(_cmd(t, q), env, stdout=subprocess.PIPE)
            assert (_read(t), _read(q)) == golden, (path, rnd)
            lines = _direct_lines(r)
            if path == "ordered":
                assert lines == []
                continue
            assert len(lines) == 2  # both nets
            for runs, groups, _kept, nbytes, at in lines:
                assert groups == runs >= 1
                assert at > 0  # the '#' lines went out first
                assert at + nbytes in (len(golden[0]), len(golden[1]))
            if nt == 8:
                assert max(x[0] for x in lines) > 256  # more runs than an ordered batch holds


@pytest.mark.parametrize("nt", THREADS)
def test_group_targets_give_the_same_bytes(tool, golden, tmp_path, nt):
    """Groups of several runs (the default target, and one that a few runs
    fill) and the group count the estimate leads to."""
    for target in ("3000", "20000", None):
        env = _env(nt)
        if target:
            env["GAC_OUT_GROUP_BYTES"] = target
        else:
            del env["GAC_OUT_GROUP_BYTES"]
        t, q = tmp_path / "g.t.net", tmp_path / "g.q.net"
        r = _run(_cmd(t, q), env, stdout=subprocess.PIPE)
        assert (_read(t), _read(q)) == golden, target
        lines = _direct_lines(r)
        assert len(lines) == 2
        for runs, groups, _kept, _nbytes, _at in lines:
            assert 1 <= groups <= runs
        if nt == 8 and target == "20000":
            assert all(groups < runs for runs, groups, *_ in lines)


@pytest.mark.parametrize("hook", HOOK, ids=["hook", "nohook"])
@pytest.mark.parametrize("which", ["t", "q"])
@pytest.mark.parametrize("nt", THREADS)
def test_stdout_pipe_append_and_positioned_file(tool, golden, tmp_path, nt, which, hook):
    """One net to stdout: into a pipe (ordered path whatever the knob says),
    appended by the shell's >> onto a file with content (O_APPEND: ordered
    path, the old content kept), and into a regular file whose descriptor
    stands past existing content without O_APPEND (direct path from that
    position)."""
    k = 0 if which == "t" else 1
    old = b"# what was there before\n" * 500
    for path, knob in PATHS.items():
        env = _env(nt, hook, knob)
        other = tmp_path / f"{path}.other.net"
        cmd = _cmd("stdout" if which == "t" else other, other if which == "t" else "stdout")
        r = _run(cmd, env, stdout=subprocess.PIPE)
        assert r.stdout == golden[k], path
        assert _read(other) == golden[1 - k], path
        assert len(_direct_lines(r)) == (1 if path == "direct" else 0)  # the other net only

        app = tmp_path / f"{path}.append.net"
        app.write_bytes(old)
        r = _run(" ".join(shlex.quote(str(c)) for c in cmd) + " >> " + shlex.quote(str(app)), env,
                 shell=True)
        assert _read(app) == old + golden[k], path
        assert _read(other) == golden[1 - k], path
        assert len(_direct_lines(r)) == (1 if path == "direct" else 0)

        pos = tmp_path / f"{path}.pos.net"
        pos.write_bytes(old + b"z" * (len(golden[k]) + 77))
        with open(pos, "r+b") as f:
            f.seek(len(old))
            r = _run(cmd, env, stdout=f)
        # (stdout is not cut by the tool: the text lies at the position, the rest stays)
        got = _read(pos)
        assert got[:len(old)] == old and got[len(old):len(old) + len(golden[k])] == golden[k], path
        assert got[len(old) + len(golden[k]):] == b"z" * 77, path
        lines = _direct_lines(r)
        assert len(lines) == (2 if path == "direct" else 0)
        if lines:
            assert len(old) + len(golden[k]) in [at + n for _r, _g, _k, n, at in lines]


@pytest.mark.parametrize("which", ["t", "q"])
@pytest.mark.parametrize("nt", THREADS)
def test_dev_full_fails_the_same_way(tool, tmp_path, nt, which):
    """/dev/full as either net (a device: ordered path): the same last stderr
    line and exit status with the knob on and off, hook on and off."""
    good = tmp_path / "good.net"
    seen = set()
    for knob in PATHS.values():
        for hook in HOOK:
            env = _env(nt, hook, knob)
            del env["GAC_TIMING"]
            r = _run(_cmd("/dev/full" if which == "t" else good, good if which == "t" else "/dev/full"),
                     env, check=False, stdout=subprocess.PIPE)
            seen.add((r.returncode, r.stderr.decode().splitlines()[-1]))
    assert seen == {(255, "write error on /dev/full")}


def _first_chain(n):
    """The first n chain records of synth11's in.chain (its '#' lines kept)."""
    out, seen = [], 0
    for ln in open(os.path.join(D11, "in.chain")):
        if ln.startswith("chain"):
            seen += 1
            if seen > n:
                break
        out.append(ln)
    return "".join(out)


@pytest.mark.parametrize("hook", HOOK, ids=["hook", "nohook"])
@pytest.mark.parametrize("nt", THREADS)
def test_zero_runs_and_one_run(tool, tmp_path, nt, hook):
    """No chain that nets (no run at all: nothing but '#' lines, an earlier
    longer file cut to them) and a single chain (one run, one group)."""
    want = {}
    for name, text in (("none", ""), ("one", _first_chain(1))):
        chain = tmp_path / f"{name}.chain"
        chain.write_text(text)
        for path, knob in PATHS.items():
            env = _env(nt, hook, knob)
            t, q = tmp_path / f"{name}.{path}.t.net", tmp_path / f"{name}.{path}.q.net"
            t.write_bytes(b"x" * 50_000)
            r = _run(_cmd(t, q, chain), env, stdout=subprocess.PIPE)
            got = (_read(t), _read(q))
            assert want.setdefault(name, got) == got, (name, path)
            lines = _direct_lines(r)
            if name == "none":
                assert lines == [] and b"fill" not in got[0] + got[1]
            elif path == "direct":
                assert [x[:2] for x in lines] == [(1, 1), (1, 1)]
                assert got[0].count(b"fill") == 1 and got[1].count(b"fill") == 1
    # the same single-chain nets whatever the thread count (against 1 thread, ordered)
    env = _env(1, {"GAC_OUT_DIRECT": "0"})
    t, q = tmp_path / "ref.t.net", tmp_path / "ref.q.net"
    _run(_cmd(t, q, tmp_path / "one.chain"), env, stdout=subprocess.PIPE)
    assert (_read(t), _read(q)) == want["one"]


@pytest.mark.parametrize("nt", THREADS)
def test_file_callback_form_chainsort(tmp_path, nt):
    """bin/chainSort writes through gac_par_output's FILE* form (each run
    formatted into a memory stream and copied into the group's buffer on the
    direct path): a file, an existing longer file and a pipe, both paths."""
    from genomealignmenttools_amd._lib import BIN_DIR
    exe = os.path.join(BIN_DIR, "chainSort")
    src = os.path.join(D11, "in.chain")
    want = None
    for path, knob in PATHS.items():
        env = _env(nt, knob)
        out = tmp_path / f"{path}.chain"
        for rnd in ("new", "over"):
            if rnd == "over":
                out.write_bytes(b"x" * (os.path.getsize(out) + 4096))
            r = _run([exe, src, str(out), "-target"], env, stdout=subprocess.PIPE)
            got = _read(out)
            want = want if want is not None else got
            assert got == want, (path, rnd)
            lines = _direct_lines(r)
            assert len(lines) == (1 if path == "direct" else 0)
            if lines:
                assert lines[0][0] == lines[0][1] > 1 and lines[0][3] + lines[0][4] == len(want)
        r = _run([exe, src, "stdout", "-target"], env, stdout=subprocess.PIPE)
        assert r.stdout == want and _direct_lines(r) == []
    assert want.count(b"chain ") == _read(src).count(b"chain ") > 100
