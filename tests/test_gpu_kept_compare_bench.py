"""tools/kept_compare_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(both kernel shapes, the old route and the tool's own comparisons still run): the file it writes carries the tree's stamp and
rows in the kit's "median (min .. max)" format.  The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_compare_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_compare_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_compare_bench.py")] + SMALL + ["--k", "1,3", "--host-reps", "1", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_compare_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_compare_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    assert any(ROW.search(ln) for ln in lines), lines
