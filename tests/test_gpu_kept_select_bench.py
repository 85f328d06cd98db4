"""tools/kept_select_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(both kernel shapes of the score passes, the per-name route, the import route and the tool's own comparisons still run): the
file it writes carries the tree's stamp and a row in the kit's "median (min .. max)" format for each thing the tool measures.
The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_select_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_select_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_select_bench.py")] + SMALL + ["--k", "4", "--host-reps", "1", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_select_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_select_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for by in ("count", "sum", "percentile", "count_above"):
        assert sum(ln.startswith(f"lh_kept_top by {by}: score pass") for ln in rows) == 2, (by, lines)      # both shapes
        assert sum(ln.startswith(f"lh_kept_top by {by}: select pass") for ln in rows) == 2, (by, lines)
    for by in ("ks", "w1", "shift", "percentile"):
        assert sum(ln.startswith(f"lh_kept_movers by {by}: score pass") for ln in rows) == 2, (by, lines)
    for what in ("(b) lh_kept_across_device alone", "(b) lh_kept_compare_device alone", "(b) per-name route", "(a) import route"):
        assert sum(ln.startswith(what) for ln in rows) >= (1 if "alone" in what else 2), (what, lines)
