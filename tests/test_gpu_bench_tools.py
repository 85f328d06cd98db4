"""Every reader bench tool under tools/ once, end to end, at the smallest arguments at which both kernel shapes and the tool's
own comparisons still run: the file it writes carries the tree's stamp and at least one "median (min .. max)" row, and a
tool that keeps the head of its file keeps it.  Each tool runs in a fresh child process (its step limit ends the process);
after a child that was killed, aborted or timed out no further child is started."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SMALL = ["--names", "256", "--pairs", "2e5", "--reps", "2", "--warmup", "1"]
TOOLS = {
    "across_bench": SMALL + ["--k", "3", "--host-reps", "1"],
    "compare_bench": SMALL,
    "count_le_bench": SMALL + ["--host-reps", "1"],
    # ids_bench.py asserts names >= 2048 (it draws 1 024 ids and reads 1 024 contiguous rows beside them)
    "ids_bench": ["--names", "2048"] + SMALL[2:] + ["--host-reps", "1"],
    "import_bench": SMALL + ["--host-reps", "1"],
    "kept_bench": SMALL + ["--k", "3", "--host-reps", "1"],              # one (names, pairs) size pair
    "kept_merge_bench": SMALL + ["--k", "3", "--host-reps", "1"],
    "lines_bench": SMALL,
    "movers_bench": SMALL + ["--k", "3"],
    "spread_bench": SMALL + ["--host-reps", "1"],
    "top_bench": SMALL + ["--k", "3"],
}
MARKED = {"across_bench", "ids_bench", "movers_bench"}                   # keep what stands above their MARK line
HEAD = ["# compile-time resource table", "kernel_a  vgpr 64  sgpr 32  lds 0", ""]
ROW = re.compile(r" us +[0-9.]+ \([0-9.]+ \.\. [0-9.]+\)")
ROW_MS = re.compile(r" ms +[0-9.]+ \([0-9.]+ \.\. [0-9.]+\)")              # import_bench.py's rows are in ms and always were
FATAL = (124, 134, 137, 139, -6, -9, -11)
ended = []                                                              # (tool, status) of the first child that must be the last


@pytest.mark.gpu
@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_runs_and_writes_its_file(tool, torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / f"{tool}.txt"
    if tool in MARKED:
        out.parent.mkdir()
        out.write_text("\n".join(HEAD + [f"# ==== measured: tools/{tool}.py", "an older run's row"]) + "\n")
    cmd = [sys.executable, os.path.join(ROOT, "tools", f"{tool}.py")] + TOOLS[tool] + ["--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append((tool, "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append((tool, r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    assert out.exists()
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    assert any((ROW_MS if tool == "import_bench" else ROW).search(ln) for ln in lines), lines
    if tool in MARKED:
        assert lines[:len(HEAD) + 1] == HEAD + [f"# ==== measured: tools/{tool}.py"]
        assert "an older run's row" not in lines
