"""tools/kept_slo_bench.py once, end to end, at the smallest arguments at which both kernel shapes and the tool's own comparisons
still run: the file it writes carries the tree's stamp and one "median (min .. max)" row per measured thing per shape.  The tool
runs in a fresh child process (its step limit ends the process), as tests/test_gpu_bench_tools.py runs the others; after a child
that was killed, aborted or timed out nothing more is started here."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROW, SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ended = []                                                              # (status,) of a child that must be the last
MEASURED = ("lh_kept_slo_ids_device,", "  the route: 20 x lh_kept_heat_ids_device", "lh_kept_burn_ids_device,", "lh_kept_slo_device,",
            "  beside it: lh_kept_heat_device", "lh_kept_burn_device,", "  the route: lh_kept_heat_device")


@pytest.mark.gpu
def test_tool_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: an earlier child ended with {ended[0]}"
    out = tmp_path / "profiles" / "kept_slo.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_slo_bench.py")] + SMALL + ["--k", "3", "--out", str(out)]
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
    assert sum(ln.startswith("#   gate, lh_kept_slo_ids_device") for ln in lines) == 2   # it says whether the gate is met
