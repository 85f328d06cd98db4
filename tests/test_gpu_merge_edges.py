"""lh_snapshot_merge's width decisions at their exact boundaries (tests/_merge_edges_driver.py: crafted rows, N engines
on the one GPU as N ranks, tests/cpp/rccl_stub.cc adding the uint32 wire words as RCCL does).

The streams of tests/_stub_merge_driver.py never bring a merged cell to nranks x (the largest per-rank cell), so
`bound <= 0xff` could read `<= 0x100` and every one of them would still pass.  Here the merged cell IS the bound:
  A  nranks x c = 255 | 256, 258 | 65 532, 65 535 | 65 536, 65 538 with the hot cell in every field of its wire word;
  B  merged windows of 1 .. 1 027 cells at every class, every lo % 4, below and above the 2 048 rows where a wave takes over
     from a workgroup, and the same rows on the uint64 wire;
  C  4 x (2^30 - 1) samples (uint32 words, a merged cell of 2^32 - 4) against 4 x 2^30 (uint64 words, a cell of exactly 2^32).
Every case runs in a subprocess: the RCCL library of a process is chosen once, and the cell width when the engine is made."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def drive(case, plan, cell_bits):
    env = dict(os.environ)
    env["LH_TEST_CELL_BITS"] = str(cell_bits)
    env.pop("LH_TEST_WIDEN_AT", None)      # (a suite-wide "widen in the middle" run: these engines keep the cells they were made with)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_merge_edges_driver.py"), case, plan],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["ok"] and res["cell_bits"] == str(cell_bits)
    return res["merges"]


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("plan", ["allreduce", "reduce_scatter"])
def test_class_boundaries_with_the_sum_at_the_bound(native_lib, torch_cuda, plan, cell_bits):
    """Case A: 3 ranks of 85 | 86 and 21 845 | 21 846, 4 ranks of 63 | 64 and 16 383 | 16 384 in one cell."""
    three, four = drive("A", plan, cell_bits)
    for m in (three, four):
        # of 16 boundary rows: 4 at 8 bits, 8 at 16, 4 at 32; the two one-rank rows at 16; the row one rank lacks at 8
        assert (m["rows_8bit"], m["rows_16bit"], m["cell_bytes"]) == (5, 10, 4), m


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("plan", ["allreduce", "reduce_scatter"])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_window_geometry_at_every_class(native_lib, torch_cuda, shape, plan, cell_bits):
    """Case B: 18 widths x {8, 16, 32 bits} in one merge, then the same rows in uint64 words."""
    narrow, wide = drive("B_" + shape, plan, cell_bits)
    assert narrow["rows"] == wide["rows"] == (56 if shape == "small" else 2050)
    assert (narrow["rows_8bit"], narrow["rows_16bit"], narrow["cell_bytes"]) == (18, 18, 4), narrow
    assert (wide["rows_8bit"], wide["rows_16bit"], wide["cell_bytes"]) == (0, 0, 8), wide
    assert wide["packed_words"] == wide["packed_cells"] == narrow["packed_cells"] > narrow["packed_words"]


@pytest.mark.parametrize("sub,plan,cell_bits", [
    ("C1", "allreduce", 64), ("C1", "reduce_scatter", 32),
    ("C2", "reduce_scatter", 64), ("C2", "allreduce", 32),
    ("C3", "allreduce", 64), ("C3", "reduce_scatter", 32),
])
def test_wire_word_boundary(native_lib, torch_cuda, sub, plan, cell_bits):
    """Case C: 4 ranks; 2^30 - 1 pairs each (uint32 words), 2^30 each (uint64), 2^30 on the last rank alone (uint64)."""
    (m,) = drive(sub, plan, cell_bits)
    assert m["cell_bytes"] == (4 if sub == "C1" else 8), m
    print(f"{sub} {plan} {cell_bits}-bit cells: feed {m['feed_s']} s, merge {m['merge_s']} s, driver {m['total_s']} s")
