"""lh_snapshot_merge followed past the merge (tests/_after_merge_driver.py: N engines on the one GPU as N ranks,
tests/cpp/rccl_stub.cc as RCCL; its scenarios are checked without a GPU by tests/test_after_merge_rows.py).

tests/test_gpu_merge_edges.py and tests/test_gpu_merge.py stop when the merge returns: one interval per engine, the owned
rows read through buckets_all and extract.  Here ONE engine per rank lives through five merges on two epoch buffers, so that
  * the unpack's cells are held to the dirty-span contract on the raw store (tests/_span_contract.py), the rows of other
    owners and the rows beyond nrows included;
  * every reader family reads merged cells (extract, spread, count_le, top, keep + Kept.across, serialize), from a narrow
    store too;
  * every release behind a merge is judged by the buffer's next interval: nothing left of cells the rank only RECEIVED;
  * the plan arrays (prefixes, owner blocks, class bytes) of one merge meet the next one: fewer rows, other classes, the
    other wire word;
  * k_unpack_rows runs a wave per row with first_row != 0 and kblock != 0 (rs_wave: owned blocks of 2 100 rows).
Rows of other owners under reduce-scatter: include/loghisto_gpu.h names the [first, last) rows "holding merged data on this
rank" and says nothing of the others.  They are UNSPECIFIED here as well: the driver asserts the span contract of them and
that no cell of theirs exceeds the merged row's, nothing else.
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_after_merge_driver.py"), case, plan],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["ok"] and res["cell_bits"] == str(cell_bits) and res["case"] == case and res["plan"] == plan
    return res


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("plan", ["allreduce", "reduce_scatter"])
def test_five_merges_on_one_engine_per_rank(native_lib, torch_cuda, plan, cell_bits):
    """life: I1 (uint32 wire, 72 rows) | I2 (40 of 72 rows, other classes) | I3 (nobody submits) | I4 (uint64 wire, 2^32 + 5)
    | I5 (uint32 wire again), buffers 0 1 0 1 1."""
    res = drive("life", plan, cell_bits)
    assert res["merges_per_rank"] == [5, 5, 5]
    iv = {x["name"]: x for x in res["intervals"]}
    assert list(iv) == ["I1", "I2", "I3", "I4", "spare", "I5", "end0", "end1"]
    assert [res["buffer_of"][k] for k in ("I1", "I2", "I3", "I4", "I5")] == [0, 1, 0, 1, 1]
    # (f): the store is narrow exactly on an engine of 32-bit cells behind a uint32 wire
    narrow = 4 if cell_bits == 32 else 8
    assert [iv[k]["wire_bytes"] for k in ("I1", "I2", "I3", "I4", "I5")] == [4, 4, 4, 8, 4]
    for k, want in (("I1", narrow), ("I2", narrow), ("I3", narrow), ("I4", 8), ("I5", narrow)):
        assert [x["cell_bytes"] for x in iv[k]["ranks"]] == [want] * 3, (k, iv[k])
        assert [x["violations"] for x in iv[k]["ranks"]] == [0, 0, 0], (k, iv[k])
    assert iv["I3"]["clean_before"] == [0, 1, 2] and iv["I3"]["clean_after"] and [x["nonzero_cells"] for x in iv["I3"]["ranks"]] == [0, 0, 0]
    assert iv["I4"]["clean_before"] == [1]
    assert all(iv[k]["clean_before"] == [0, 1, 2] and not iv[k]["merged"] for k in ("spare", "end0", "end1"))
    assert iv["I2"]["nrows"] == 40 and iv["I2"]["occupied_rows"] == 40 and iv["I1"]["occupied_rows"] == 70
    assert iv["I4"]["rows_8bit"] == iv["I4"]["rows_16bit"] == 0 and iv["I4"]["packed_words"] == iv["I4"]["packed_cells"]
    print(f"life {plan} {cell_bits}-bit cells: driver {res['total_s']} s, per interval {[x['s'] for x in res['intervals']]}")


@pytest.mark.parametrize("cell_bits", [64, 32])
def test_reduce_scatter_blocks_at_the_wave_shape(native_lib, torch_cuda, cell_bits):
    """rs_wave: 2 ranks x 4 200 rows, owned blocks of 2 100 rows each; then the same rows by all-reduce on the same engines."""
    res = drive("rs_wave", "reduce_scatter", cell_bits)
    rs, ar = res["merges"]
    assert (rs["plan"], ar["plan"]) == ("reduce_scatter", "allreduce")
    assert rs["owned"] == [[0, 2100], [2100, 4200]] and min(rs["owned_rows"]) >= 2048, rs
    assert ar["owned"] == [[0, 4200], [0, 4200]] and rs["packed_words"] == ar["packed_words"]
    for m in (rs, ar):
        assert [x["violations"] for x in m["ranks"]] == [0, 0]
        assert [x["cell_bytes"] for x in m["ranks"]] == [4 if cell_bits == 32 else 8] * 2
    print(f"rs_wave {cell_bits}-bit cells: driver {res['total_s']} s, merges {[m['s'] for m in res['merges']]}")
