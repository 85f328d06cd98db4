"""The judge of tests/_span_contract.py on planted stores (no GPU): each kind of violation must be reported with its row and bin,
and clean stores -- cells at bins 0 and 65 535 of a full span included -- must pass.  The one reduction runs on numpy arrays and
on torch tensors; both are held to the same plants, at both cell widths."""
import numpy as np
import pytest

from tests import _span_contract as sc

NKEYS = sc.NKEYS
STRIDE = NKEYS + 32
M = 7
#            row 0          1                2 (empty)   3 (full)        4             5 (one bin)       6 (empty)
RANGES = [(100, 200), (40000, 40010), sc.EMPTY, (0, NKEYS - 1), (65000, NKEYS - 1), (0, 0), sc.EMPTY]


def clean_store(dtype):
    s = np.zeros((M, STRIDE), dtype=dtype)
    s[0, 100], s[0, 150], s[0, 200] = 1, 2, 3                 # both ends of the span are occupied
    s[1, 40005] = np.iinfo(dtype).max                         # (the largest cell: nothing is read as signed)
    s[3, 0], s[3, NKEYS - 1] = 5, 6                           # bins 0 and 65 535 inside a full span, next to the padding
    s[4, NKEYS - 1] = 7
    s[5, 0] = 8
    return s


def judge(backend, store, ranges):
    ranges = np.asarray(ranges, dtype=np.int64)
    if backend == "numpy":
        return sc.check_planted(store, ranges)
    import torch
    signed = torch.from_numpy(store.view(np.int32 if store.dtype.itemsize == 4 else np.int64).copy())
    cols = torch.arange(STRIDE, dtype=torch.int64)[None, :]
    return sc.check_arrays(torch, lambda first, n: signed[first:first + n], ranges, store.dtype.itemsize, STRIDE, cols)


BACKENDS = ["numpy", "torch"]
WIDTHS = [np.uint32, np.uint64]


@pytest.mark.parametrize("dtype", WIDTHS, ids=["cells32", "cells64"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_clean_store_passes_and_is_measured(backend, dtype):
    s = clean_store(dtype)
    rec = judge(backend, s, RANGES)
    assert rec.violations == [] and rec.cell_bytes == s.dtype.itemsize and rec.stride == STRIDE
    sc.assert_contract(rec)
    assert rec.minbin.tolist() == [100, 40005, STRIDE, 0, NKEYS - 1, 0, STRIDE]
    assert rec.maxbin.tolist() == [200, 40005, -1, NKEYS - 1, NKEYS - 1, 0, -1]
    assert rec.nnz.tolist() == [3, 1, 0, 2, 1, 1, 0]
    assert rec.total.dtype == np.uint64 and rec.total.tolist() == [6, int(np.iinfo(dtype).max), 0, 11, 7, 8, 0]
    assert np.array_equal(rec.ranges, np.asarray(RANGES))
    with pytest.raises(AssertionError, match="nonzero cells in 5 rows"):
        sc.assert_clean(rec)


@pytest.mark.parametrize("dtype", WIDTHS, ids=["cells32", "cells64"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_released_store(backend, dtype):
    s = np.zeros((M, STRIDE), dtype=dtype)
    sc.assert_clean(judge(backend, s, [sc.EMPTY] * M))
    with pytest.raises(AssertionError, match=r"row 4: \(65000, 65535\)"):           # all zero, but a range was not reset
        sc.assert_clean(judge(backend, s, [sc.EMPTY] * 4 + [(65000, NKEYS - 1)] + [sc.EMPTY] * 2))


def plants(stride):
    """(what, (row, column, value), the violation it must be reported as) over clean_store / RANGES, for rows `stride` cells long."""
    return [
        ("one bin below lo", (0, 99, 1), ("S", 0, 99, 1)),
        ("one bin above hi", (0, 201, 4), ("S", 0, 201, 4)),
        ("in an empty row", (2, 31000, 9), ("S", 2, 31000, 9)),
        ("bin 65 535 of a row whose span ends below it", (1, NKEYS - 1, 2), ("S", 1, NKEYS - 1, 2)),
        ("bin 0 of a row whose span starts above it", (4, 0, 3), ("S", 4, 0, 3)),
        ("first padding cell", (3, NKEYS, 1), ("P", 3, NKEYS, 1)),
        ("last padding cell", (3, stride - 1, 1), ("P", 3, stride - 1, 1)),
        ("last padding cell of the last row", (M - 1, stride - 1, 77), ("P", M - 1, stride - 1, 77)),
    ]


PLANTS = plants(STRIDE)


@pytest.mark.parametrize("dtype", WIDTHS, ids=["cells32", "cells64"])
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("what,plant,want", PLANTS, ids=[p[0].replace(" ", "_") for p in PLANTS])
def test_a_stray_cell_is_reported_with_its_row_and_bin(backend, dtype, what, plant, want):
    s = clean_store(dtype)
    r, c, val = plant
    s[r, c] = val
    rec = judge(backend, s, RANGES)
    assert rec.violations == [want], what
    assert int(rec.npad.sum()) + int(rec.nstray.sum()) == 1
    with pytest.raises(AssertionError, match=f"row {want[1]} bin {want[2]} = {want[3]}"):
        sc.assert_contract(rec)


@pytest.mark.parametrize("dtype", WIDTHS, ids=["cells32", "cells64"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_all_strays_at_once(backend, dtype):
    s = clean_store(dtype)
    for _, (r, c, val), _ in PLANTS:
        s[r, c] = val
    rec = judge(backend, s, RANGES)
    assert sorted(rec.violations) == sorted(p[2] for p in PLANTS)
    assert int(rec.npad.sum()) == 3 and int(rec.nstray.sum()) == 5


@pytest.mark.parametrize("bad,row", [((NKEYS, 1), 2), ((NKEYS - 1, 0), 2), ((300, 100), 6), ((0xffffffff, 0), 6),
                                     ((100, NKEYS), 0), ((0, 0xffffffff), 5)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_a_bad_range_is_reported(backend, bad, row):
    """Empty but not exactly (65 536, 0), or a hi that reaches past bin 65 535 -- over a store that is clean under it."""
    ranges = list(RANGES)
    ranges[row] = bad
    rec = judge(backend, clean_store(np.uint64), ranges)
    assert rec.violations == [("E", row, bad[0], bad[1])]
    with pytest.raises(AssertionError, match=rf"row {row} range \({bad[0]}, {bad[1]}\)"):
        sc.assert_contract(rec)


def test_more_rows_than_one_pass_takes():
    """The passes are at most 1 024 rows long; a stray in a later pass keeps its row number."""
    assert sc.CHUNK_ROWS <= 1024
    rows = sc.CHUNK_ROWS + 3
    s = np.zeros((rows, NKEYS + 4), dtype=np.uint32)
    ranges = np.tile(np.array(sc.EMPTY), (rows, 1))
    ranges[rows - 1] = (10, 20)
    s[rows - 1, 15], s[rows - 1, 21], s[rows - 2, NKEYS + 3] = 1, 2, 3
    rec = sc.check_planted(s, ranges)
    assert rec.violations == [("P", rows - 2, NKEYS + 3, 3), ("S", rows - 1, 21, 2)]
    assert int(rec.total.sum()) == 6 and int(rec.nnz.sum()) == 3
