"""tools/kept_gather_bench.py once, end to end, at the smallest arguments at which both kernel shapes, every route and the tool's own
comparisons still run: the file it writes carries the tree's stamp, one "median (min .. max)" row per measured thing per shape, and
the gate lines.  The tool runs in a fresh child process (its step limit ends the process), as tests/test_gpu_bench_tools.py runs
the others; after a child that was killed, aborted or timed out nothing more is started here."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROW, SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ended = []                                                              # (status,) of a child that must be the last
ONE, FEW, FLEET = "1 handle x 256 rows", "3 handles x 256 rows", "4 handles x 128 rows"
MEASURED = [f"lh_kept_gather_device (wall), {ONE}, the direct route, a ", f"lh_kept_gather_device (wall), {ONE}, the tile route, a ",
            f"lh_kept_gather_device (wall), {ONE}, the tile route, map transposed, a ", f"  the route there was (wall), {ONE}:"]
for _what in (FEW, FLEET):
    MEASURED += [f"lh_kept_gather_device (wall), {_what}, the tile route, a ", f"lh_kept_gather_device (wall), {_what}, the tile route, map transposed, a ",
                 f"  the route there was (wall), {_what}:"]


@pytest.mark.gpu
def test_tool_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: an earlier child ended with {ended[0]}"
    out = tmp_path / "profiles" / "kept_gather.txt"
    assert SMALL[:4] == ["--names", "256", "--pairs", "2e5"]             # what ONE and FEW above are named after
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_gather_bench.py")] + SMALL + [
        "--k", "3", "--host-reps", "1", "--fleet-names", "128", "--fleet-handles", "4", "--fleet-pairs", "1e5", "--out", str(out)]
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
    for what in MEASURED:                                               # a row per measured thing per shape
        rows = [ln for ln in lines if ln.startswith(what) and ROW.search(ln)]
        assert len(rows) == 2, (what, rows)
    for what, routes in ((ONE, 3), (FEW, 2), (FLEET, 2)):               # it says whether each gate is met, per route and shape
        assert sum(ln.startswith(f"#   gate, lh_kept_gather_device, {what}") for ln in lines) == 2 * routes, what
        assert sum(ln.startswith(f"#   transposing the staged map on the device, {what}") for ln in lines) == 1, what
