"""tools/kept_top_series_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(both kernel shapes, the three measured forms, each one's per-window route, its passes and the tool's own byte comparisons still
run): the file it writes carries the tree's stamp and a row in the kit's "median (min .. max)" format for each thing the tool
measures, per shape.  The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_top_series_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_top_series_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_top_series_bench.py")] + SMALL + ["--k", "3", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_top_series_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_top_series_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for what, n in (("lh_kept_top_series_device,", 2), ("lh_kept_movers_series_device,", 1)):
        for shape in ("wave", "workgroup"):
            assert sum(ln.startswith(what) and f"a {shape} per entry" in ln for ln in rows) == n, (what, shape, lines)
    for route, n in (("lh_kept_top_device", 4), ("lh_kept_movers_device", 2)):
        assert sum(ln.startswith("  the route:") and f" x {route} over" in ln for ln in rows) == n, (route, lines)
    for which in ("score", "select"):
        assert sum(ln.startswith(f"  its {which} pass (") for ln in rows) == 6, (which, lines)
    assert sum(ln.startswith("#   gate, ") for ln in lines) == 4
    assert sum(ln.startswith("#   gate, ") and "a note" in ln for ln in lines) == 2
    assert sum(ln.startswith("#   lh_kept_top_series_device, ") and "the route's min .. max" in ln for ln in lines) == 2
