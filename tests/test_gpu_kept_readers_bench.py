"""tools/kept_readers_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(both kernel shapes, the ids forms, the import route and the tool's own comparisons still run): the file it writes carries the
tree's stamp and a row in the kit's "median (min .. max)" format for each thing the tool measures.  The tool runs in a fresh
child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_readers_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_readers_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_readers_bench.py")] + SMALL + ["--k", "3", "--host-reps", "1", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_readers_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_readers_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for what in ("lh_kept_count_le_device,", "lh_kept_spread_device,", "lh_kept_count_le_ids_device,", "lh_kept_spread_ids_device,",
                 "(b) lh_kept_across_device,", "(a) import route", "lh_count_le_device on", "lh_spread_device on"):
        shapes = 2 if what.startswith(("lh_kept", "(b)")) else 1
        assert sum(ln.startswith(what) for ln in rows) >= shapes, (what, lines)
