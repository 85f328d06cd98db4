"""The dirty-span contract of an epoch buffer, judged on the raw store (tests/test_gpu_span_contract.py drives the engine
through it; tests/test_span_contract.py holds the judge itself to planted stores, without a GPU).

Every row m of an epoch buffer carries a dirty span ranges[m] = (lo, hi) (loghisto_amd/csrc/lh_kernels.h):

  * outside [lo, hi] the row's cells are zero -- the LH_ROW_SKEW_CELLS padding cells between bin 65 535 and the next row
    included (k_extract_wave reads whole 4-bin groups past bin 65 535 and relies on that);
  * an empty row's range is exactly (LH_NKEYS, 0), and no hi reaches LH_NKEYS;
  * after a release the whole store is zero and every range is (LH_NKEYS, 0).

K2 extract, both clear kernels, k_widen_rows, the merge pack, lh_keep and every reader walk only the span, and Snapshot.dense_row
/ buckets_all are rebuilt through it: a cell counted outside its span, or left inside one by a clear, is invisible to them.
check_store reads ALL M x row_stride cells of the store a snapshot reports AT THAT MOMENT (lh_snapshot_cells: 4- or 8-byte
cells as they are; lh_snapshot_rows would move a narrow snapshot to its wide store first) and the M x 2 ranges.  No pointer is
kept from one call to the next: a narrow store can be freed between intervals."""
import types

import numpy as np

NKEYS = 65536
CHUNK_ROWS = 512                    # rows per pass (at most 1 024): one int64 temporary is 0.27 GB at that
EMPTY = (NKEYS, 0)
MAX_NAMED = 64                      # violations named cell by cell (the counts are complete whatever this is)


def reduce_rows(xp, cells, lo, hi, cols):
    """The reduction, once for numpy (xp = numpy) and torch (xp = torch): cells int64[R, stride] (non-negative counts, or
    the bits of uint64 ones: only `!= 0` and a wrapping sum are taken), lo / hi int64[R], cols int64[1, stride] = 0 .. stride - 1.
    Per row: the smallest and largest column that holds a nonzero cell (stride / -1 when there is none), how many cells are
    nonzero, their sum, and how many nonzero cells lie in the padding columns (P) and at a bin outside [lo, hi] (S; with
    lo > hi every nonzero bin)."""
    stride = cells.shape[1]
    nz = cells != 0
    pad = nz & (cols >= NKEYS)
    stray = nz & (cols < NKEYS) & ~((cols >= lo[:, None]) & (cols <= hi[:, None]))
    return dict(minbin=xp.amin(xp.where(nz, cols, stride), axis=1), maxbin=xp.amax(xp.where(nz, cols, -1), axis=1),
                nnz=nz.sum(axis=1), total=cells.sum(axis=1), npad=pad.sum(axis=1), nstray=stray.sum(axis=1))


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _as_int64(xp, a, cell_bytes):
    """uint32 / uint64 cells, however the array library spells them, as int64 of the same counts (uint64: the same bits)."""
    if xp is np:
        return a.astype(np.int64) if cell_bytes == 4 else a.view(np.int64)
    return (a.to(xp.int64) & 0xffffffff) if cell_bytes == 4 else a


def check_arrays(xp, chunks, ranges, cell_bytes, stride, cols):
    """chunks: callable(first, n) -> the integer array [n, stride] of rows [first, first + n) as the store holds them (numpy
    uint32 / uint64, torch int32 / int64 views).  ranges: host int64[M, 2].  Returns the record (see check_store)."""
    M = ranges.shape[0]
    per = {k: np.zeros(M, dtype=np.int64) for k in ("minbin", "maxbin", "nnz", "total", "npad", "nstray")}
    violations = []
    for first in range(0, M, CHUNK_ROWS):
        n = min(CHUNK_ROWS, M - first)
        raw = chunks(first, n)
        cells = _as_int64(xp, raw, cell_bytes)
        lo = ranges[first:first + n, 0]
        hi = ranges[first:first + n, 1]
        if xp is not np:
            lo, hi = xp.from_numpy(np.ascontiguousarray(lo)).to(cells.device), xp.from_numpy(np.ascontiguousarray(hi)).to(cells.device)
        got = reduce_rows(xp, cells, lo, hi, cols)
        for k in per:
            per[k][first:first + n] = _host(got[k])
        for r in np.nonzero((per["npad"][first:first + n] != 0) | (per["nstray"][first:first + n] != 0))[0]:
            if len(violations) >= MAX_NAMED:
                break
            row = _host(_as_int64(xp, raw[int(r):int(r) + 1], cell_bytes))[0].view(np.uint64)
            m = first + int(r)
            for b in np.nonzero(row)[0]:
                if b >= NKEYS:
                    violations.append(("P", m, int(b), int(row[b])))
                elif not (ranges[m, 0] <= b <= ranges[m, 1]):
                    violations.append(("S", m, int(b), int(row[b])))
        del raw, cells, got
    for m in np.nonzero(((ranges[:, 0] > ranges[:, 1]) & ((ranges[:, 0] != EMPTY[0]) | (ranges[:, 1] != EMPTY[1])))
                        | (ranges[:, 1] >= NKEYS))[0][:MAX_NAMED]:
        violations.append(("E", int(m), int(ranges[m, 0]), int(ranges[m, 1])))
    return types.SimpleNamespace(minbin=per["minbin"], maxbin=per["maxbin"], nnz=per["nnz"], total=per["total"].view(np.uint64),
                                 npad=per["npad"], nstray=per["nstray"], ranges=ranges, violations=violations,
                                 cell_bytes=cell_bytes, stride=stride)


def check_planted(store, ranges):
    """The judge on a host store: numpy uint32 / uint64 [M, stride], ranges [M, 2]."""
    store = np.asarray(store)
    stride = store.shape[1]
    cols = np.arange(stride, dtype=np.int64)[None, :]
    return check_arrays(np, lambda first, n: store[first:first + n], np.asarray(ranges).astype(np.int64), store.dtype.itemsize,
                        stride, cols)


def _wait_for_snapshot_stream(snap, torch):
    """The ingest streams are chained into the snapshot's stream at the flip, and a release enqueues its clear there: torch's
    stream waits for it, so that a read sees every add and every clear enqueued so far."""
    torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(snap.stream()))


def store_view(snap, M, torch):
    """(cells [M, stride] int32 / int64 view of the store the open snapshot reports now, ranges [M, 2] int32 view, cell_bytes)."""
    from loghisto_amd import merge
    ptr, nrows, cb = snap.device_cells()
    assert nrows >= M and cb in (4, 8), (nrows, cb)
    stride = snap.row_stride()
    cells = torch.as_tensor(merge._DeviceArray(ptr, (M, stride), "<i4" if cb == 4 else "<i8"), device="cuda")
    ranges = torch.as_tensor(merge._DeviceArray(snap.device_ranges(), (M, 2), "<i4"), device="cuda")
    return cells, ranges, cb


def check_store(snap, M, torch):
    """All M x row_stride cells of the open snapshot's store, as they are, against its ranges.  Returns a record:
      minbin, maxbin, nnz, total   per row: smallest / largest nonzero column (row_stride / -1: none), nonzero cells, sum (uint64)
      ranges                       int64[M, 2]
      violations                   [("P", row, column, value)]  nonzero cell in the padding columns [65 536, row_stride)
                                   [("S", row, bin, value)]     nonzero cell at a bin outside the row's [lo, hi]
                                   [("E", row, lo, hi)]         empty range that is not (65 536, 0), or hi >= 65 536
      npad, nstray                 per row: how many P and S cells (complete; `violations` names the first MAX_NAMED)"""
    _wait_for_snapshot_stream(snap, torch)
    cells, d_ranges, cb = store_view(snap, M, torch)
    ranges = d_ranges.cpu().numpy().view(np.uint32).astype(np.int64)
    stride = cells.shape[1]
    cols = torch.arange(stride, dtype=torch.int64, device="cuda")[None, :]
    rec = check_arrays(torch, lambda first, n: cells[first:first + n], ranges, cb, stride, cols)
    torch.cuda.synchronize()
    return rec


def describe(violations, limit=6):
    what = {"P": "padding cell", "S": "cell outside the span", "E": "range"}
    return "; ".join(f"{k} {what[k]}: row {m} " + (f"range ({a}, {b})" if k == "E" else f"bin {a} = {b}")
                     for k, m, a, b in violations[:limit])


def assert_contract(rec):
    if rec.violations or int(rec.npad.sum()) or int(rec.nstray.sum()):
        raise AssertionError(f"{int(rec.npad.sum())} padding cells, {int(rec.nstray.sum())} cells outside their spans, "
                             f"{sum(v[0] == 'E' for v in rec.violations)} bad ranges: " + describe(rec.violations))


def assert_clean(rec):
    """After a release: no nonzero cell at all, every range (LH_NKEYS, 0)."""
    dirty = np.nonzero(rec.nnz)[0]
    assert dirty.size == 0, (f"{int(rec.nnz.sum())} nonzero cells in {dirty.size} rows of a released buffer, e.g. row {int(dirty[0])} "
                             f"columns {int(rec.minbin[dirty[0]])} .. {int(rec.maxbin[dirty[0]])}")
    bad = np.nonzero((rec.ranges[:, 0] != EMPTY[0]) | (rec.ranges[:, 1] != EMPTY[1]))[0]
    assert bad.size == 0, (f"{bad.size} ranges of a released buffer are not ({EMPTY[0]}, {EMPTY[1]}), e.g. row {int(bad[0])}: "
                           f"({int(rec.ranges[bad[0], 0])}, {int(rec.ranges[bad[0], 1])})")


def raw_rows(snap, rows, torch):
    """uint64[len(rows), 65 536]: the chosen rows' cells straight from the store the open snapshot reports now."""
    _wait_for_snapshot_stream(snap, torch)
    cells, _, cb = store_view(snap, max(int(r) for r in rows) + 1, torch)
    idx = torch.as_tensor([int(r) for r in rows], dtype=torch.int64, device="cuda")
    got = cells[idx][:, :NKEYS].cpu().numpy()
    return got.view(np.uint32).astype(np.uint64) if cb == 4 else got.view(np.uint64)
