"""tools/kept_encode_bench.py once, end to end, at the size tests/test_gpu_bench_tools.py runs the other reader bench tools at
(the sizes, the two encodes and two decodes beside the verbatim routes, each kernel alone, and the tool's own byte comparisons
still run): the file it writes carries the tree's stamp and a row in the kit's "median (min .. max)" format for each thing the
tool measures.  The tool runs in a fresh child process (its step limit ends the process)."""
import os
import subprocess
import sys

import pytest

from tests.test_gpu_bench_tools import FATAL, ROOT, ROW, SMALL, ended


@pytest.mark.gpu
def test_kept_encode_bench_runs_and_writes_its_file(torch_cuda, tmp_path):
    import bench
    assert not ended, f"not started: {ended[0][0]} ended with {ended[0][1]}"
    out = tmp_path / "profiles" / "kept_encode_bench.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kept_encode_bench.py")] + SMALL + ["--out", str(out)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        ended.append(("kept_encode_bench", "the subprocess timeout"))
        raise
    if r.returncode in FATAL:
        ended.append(("kept_encode_bench", r.returncode))
    assert r.returncode == 0, r.stdout[-3000:]
    lines = out.read_text().splitlines()
    assert f"# tree_stamp: {bench.tree_stamp()}" in lines
    rows = [ln for ln in lines if ROW.search(ln)]
    for what in ("k_enc_size alone", "k_keep_scan of S alone", "k_enc_fill alone", "k_dec_dir alone", "k_keep_scan twice",
                 "k_dec_fill alone", "k_kept_check_samples behind it", "lh_kept_save_device", "lh_kept_encode_device",
                 "lh_kept_save, pinned", "lh_kept_encode, pinned", "lh_kept_load_device", "lh_kept_decode_device",
                 "lh_kept_load, pinned", "lh_kept_decode, pinned"):
        assert sum(ln.startswith(what) for ln in rows) == 1, (what, lines)
    assert any("x smaller" in ln and "B a cell" in ln for ln in lines)
    assert any("pinned encode against pinned save" in ln for ln in lines)
