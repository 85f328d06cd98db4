"""tools/kept_slide_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(the slide and the merge it replaces in both shapes, the slide's two passes alone, and the tool's own byte comparisons still
run): the file it writes carries the tree's stamp and a row in the kit's "median (min .. max)" format for each thing the tool
measures.  The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_slide_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_slide_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_slide_bench.py")] + SMALL + ["--k", "3", "--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_slide_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_slide_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for what in ("lh_kept_slide (wall)", "lh_kept_merge (wall)", "k_slide_count alone", "k_slide_fill alone"):
        for shape in ("a wave per row", "a workgroup per row"):
            assert sum(ln.startswith(what) and shape in ln for ln in rows) == 1, (what, shape, lines)
    assert any("lh_kept_merge of the 3 / lh_kept_slide" in ln for ln in lines)
