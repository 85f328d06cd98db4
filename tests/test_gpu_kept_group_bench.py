"""tools/kept_group_bench.py once, end to end, at the smallest arguments at which both kernel shapes, groups below, at and above a
chunk of 64 sources, several handles and the tool's own byte comparisons still run: the file it writes carries the tree's stamp,
one "median (min .. max)" row per measured thing per shape, and one gate line per gated shape and kernel shape (whether a gate is
met is the run's to say, not this test's).  The tool runs in a fresh child process (its step limit ends the process), as
tests/test_gpu_kept_gather_bench.py runs its tool; after a child that was killed, aborted or timed out nothing more is started here."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROW, SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ended = []                                                              # (status,) of a child that must be the last
GATED = ["256 names -> 64 groups of 4 x 1 handle", "256 names -> 4 groups of 64 x 1 handle", "128 names -> 2 groups of 64 x 3 handles"]
REPORTED = ["256 names -> ONE group x 1 handle", "256 names -> 8 groups of Zipf sizes "]


@pytest.mark.gpu
def test_tool_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: an earlier child ended with {ended[0]}"
    out = tmp_path / "profiles" / "kept_group.txt"
    assert SMALL[:4] == ["--names", "256", "--pairs", "2e5"]             # what the shapes above are named after
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_group_bench.py")] + SMALL + [
        "--sizes", "4,64", "--zipf-groups", "8", "--host-reps", "1", "--fleet-names", "128", "--fleet-handles", "3", "--fleet-size", "64",
        "--fleet-pairs", "1e5", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append("the subprocess timeout")
        raise
    if r.returncode in FATAL:
        ended.append(r.returncode)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    for what in GATED + REPORTED:                                       # a row per measured thing per shape: the call, the old route
        for start in (f"lh_kept_group_device (wall), {what}", f"  the route there was (wall), {what}"):
            rows = [ln for ln in lines if ln.startswith(start) and ROW.search(ln)]
            assert len(rows) == 2 and sum(" wave per row" in ln for ln in rows) == 1, (start, rows)
    for what in GATED:                                                  # it says whether each gate is met, per kernel shape
        gates = [ln for ln in lines if ln.startswith(f"#   gate, lh_kept_group_device, {what}, a ")]
        assert len(gates) == 2 and all(": met: median " in ln or ": NOT met: median " in ln for ln in gates), (what, gates)
    for what in REPORTED:                                               # the others carry their numbers without a verdict
        told = [ln for ln in lines if ln.startswith(f"#   reported, lh_kept_group_device, {what}")]
        assert len(told) == 2 and not any(" met" in ln for ln in told), (what, told)
    assert sum(ln.startswith("#   gate, ") for ln in lines) == 2 * len(GATED)
