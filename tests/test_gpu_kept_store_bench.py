"""tools/kept_store_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(the three saves, the three loads, both old routes, the check's two kernels and k_keep_count alone, and the tool's own byte
comparisons still run): the file it writes carries the tree's stamp and a row in the kit's "median (min .. max)" format for
each thing the tool measures.  The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_store_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_store_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_store_bench.py")] + SMALL + ["--host-reps", "1", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_store_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_store_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for what in ("k_keep_count alone", "k_kept_check alone", "k_kept_check_samples alone", "lh_kept_save, pageable", "lh_kept_save, pinned",
                 "lh_kept_save_device", "lh_kept_load, pageable", "lh_kept_load, pinned", "lh_kept_load_device",
                 "old route (wall): lh_kept_arrays", "old route (wall): add_buckets_csr"):
        assert sum(ln.startswith(what) for ln in rows) == 1, (what, lines)
    assert any("k_kept_check / k_keep_count" in ln for ln in lines)
