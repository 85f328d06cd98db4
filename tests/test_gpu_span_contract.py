"""Every epoch buffer held to its dirty-span contract, cell by cell (the judge: tests/_span_contract.py).

The other GPU parity tests read an interval THROUGH the span (dense_row, buckets_all, extract), one interval per buffer: a cell
counted outside its span is only a missing count there, is never cleared, and turns up as a phantom sample in some later
interval of that buffer; a clear that leaves cells behind shows only if the same buffer is used a third time.  Here every ingest
route, both clear kernels, the widening and the import go through sequences that come back to the same buffer, and after every
interval ALL M x row_stride cells of the store and the M x 2 ranges are read raw:

  interval   submitted                 buffer
  A          wide                      X          +-10^U(-3, 20) plus 0.0, -0.0, +-5e-324, +-MaxFloat64, +-Inf, NaN and the
  B          narrow lognormal          Y          values of keys -32768 and 32767: bins 0 and 65 535, next to the padding
  C          narrow, somewhere else    X again    a stretch of A's own pairs: wholly inside A's span of every row
  D          nothing                   Y
  E          nothing                   X

A, B, C: the contract; the route's samples_* counters moved by exactly the call's size; the store's sum is the interval's sample
count; raw rows equal the oracle's; extract's counts equal the raw row sums.  D, E: no nonzero cell, every range (65 536, 0).
Every assertion is an equality or an exact zero.  Reference semantics: Histogram(name, v) = histogramCache[name][compress(v)] += 1
(metrics.go:273-295, 316-322); a sample belongs to exactly one interval (metrics.go:460-463)."""
import functools
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests import _adversarial_values as av
from tests import _span_contract as sc
from tests.test_gpu_compare import _write_narrow
from tests.test_gpu_import import add_coo, add_csr
from tests.test_gpu_part3 import PCTS, _ids, _values, oracle_cells
from tests.test_gpu_routes_adversarial import _dev, _moved
from tests.test_span_contract import RANGES, clean_store, plants

pytestmark = pytest.mark.gpu
NKEYS = N.NKEYS
U64 = np.uint64
N0 = 150_001                       # >= 2^17 (the lowered minimum of every partitioned generation) and >= 65 536 (the small kernel); odd


def _engine(M, opts=None, cell_bits=64):
    import loghisto_amd
    e = loghisto_amd.Engine(max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16, cell_bits=cell_bits)
    for k, val in (opts or {}).items():
        e.set_option(k, val)
    return e


# ---- the three streams -------------------------------------------------------------------------------------------------

def by_values(ids, v, M):
    ids, v = np.ascontiguousarray(ids, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.float64)
    for a in (ids, v):
        a.setflags(write=False)
    return types.SimpleNamespace(ids=ids, v=v, n=int(v.size), per_row=np.bincount(ids, minlength=M).astype(U64),
                                 want=lambda m: oracle.histogram_dense(v[ids == m]))


@functools.lru_cache(maxsize=None)
def _special():
    """What interval A adds to its decades, all from tests/_adversarial_values.py: first the values the contract's edges need (the
    two ends of the key space, zeros, the smallest and the largest doubles, infinities, a NaN), then the rest of its specials and
    of the doubles where 1 + |v| rounds."""
    sp, rd = av.values()["specials"], av.values()["rounding"]
    keys = av.expected(sp)
    must = [sp[keys == 32767][0], sp[keys == -32768][0]]
    for want in (0.0, -0.0, np.inf, -np.inf, 1.7976931348623157e308, -1.7976931348623157e308):
        must.append(sp[sp.view(U64) == np.float64(want).view(U64)][0])
    for want in (5e-324, -5e-324):
        must.append(rd[rd.view(U64) == np.float64(want).view(U64)][0])
    must.append(sp[np.isnan(sp)][0])
    out = np.concatenate([np.array(must), sp, rd])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def streams(M, n, order=None):
    """(A, B, C) for an engine of M names, n pairs each; read-only, built once per shape.  order (single-name streams):
    "sorted_by_key" -- every K1 tile is narrow -- or None, as drawn: every tile spans the key space."""
    rng = np.random.default_rng(1000 * M + n)
    ids = _ids(rng, M, n, 1.0)
    v = _values(rng, "signed_wide", ids, n)
    hot = int(np.bincount(ids, minlength=M).argmax())
    rows = sorted({0, M - 1, hot})
    s = _special()[:max(13, min(_special().size, n // (4 * len(rows))))]
    for k, m in enumerate(rows):                                   # the first, the last and the most frequent name get them all
        at = slice(k * s.size, (k + 1) * s.size)
        ids[at], v[at] = m, s
    if order == "sorted_by_key":
        v = av.sorted_by_key(v)
    bins = oracle.key_to_bin(av.expected(v))
    for m in rows:
        assert {0, NKEYS - 1} <= set(bins[ids == m].tolist()), m    # next to the padding on both sides
    a = by_values(ids, v, M)
    ids_b = _ids(rng, M, n, 1.0)
    b = by_values(ids_b, _values(rng, "lognormal", ids_b, n), M)
    # C: A's own pairs between -1e8 and -1e6 (460 of A's 9 211 bins, far from B's), repeated up to n pairs: every (name, bin) of C
    # is one of A's, so C lies inside A's span of every row
    sel = np.nonzero((v > -1e8) & (v < -1e6))[0]
    assert sel.size
    take = np.tile(sel, -(-n // sel.size))[:n]
    if order == "sorted_by_key":
        take = np.sort(take)
    c = by_values(ids[take], v[take], M)
    for m in (0, hot):
        ba, bc = bins[ids == m], oracle.key_to_bin(av.expected(c.v[c.ids == m]))
        assert bc.size == 0 or (ba.min() <= bc.min() and bc.max() <= ba.max() and bc.max() - bc.min() < 500)
    return a, b, c


# ---- the assertions ----------------------------------------------------------------------------------------------------

def sample_rows(per_row, M, seed):
    """The first, the last, the most frequent, the least frequent and three random rows."""
    rng = np.random.default_rng(seed)
    return sorted({0, M - 1, int(per_row.argmax()), int(per_row.argmin())} | {int(x) for x in rng.integers(0, M, 3)})


def check_interval(torch, snap, M, iv, what):
    rec = sc.check_store(snap, M, torch)
    sc.assert_contract(rec)
    assert int(rec.total.sum(dtype=U64)) == iv.n, (what, int(rec.total.sum(dtype=U64)), iv.n)
    rows = sample_rows(iv.per_row, M, iv.n)
    raw = sc.raw_rows(snap, rows, torch)
    for got, m in zip(raw, rows):
        want = iv.want(m)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"interval {what}, row {m}: {bad.size} cells differ, e.g. " + ", ".join(
                f"bin {int(b)}: {int(got[b])} != {int(want[b])}" for b in bad[:6]))
    assert np.array_equal(rec.total, iv.per_row), (what, np.nonzero(rec.total != iv.per_row)[0][:8])
    counts = snap.extract(PCTS, M)["count"]
    assert np.array_equal(counts.astype(U64), rec.total), (what, np.nonzero(counts.astype(U64) != rec.total)[0][:8])
    return rec


def check_released(torch, snap, M):
    sc.assert_clean(sc.check_store(snap, M, torch))


def run_sequence(torch, e, M, intervals, moved=None, submit=None, fill=None, before_each=None):
    """A .. E on an engine of two buffers.  submit(iv): enqueue the interval's samples; fill(snap, iv): add them to the open
    snapshot instead (the import).  moved: the samples_* counters that must move by the call's size, and no other.  The buffer
    under a snapshot is the store it reports right after the flip (an import may move a narrow snapshot to its wide store)."""
    ptrs = []
    for what, iv in zip("ABC", intervals):
        if before_each:
            before_each()
        before = e.counters()
        if submit:
            submit(iv)
        e.sync()
        if moved is not None:
            assert _moved(before, e.counters()) == {k: iv.n for k in moved}, (what, _moved(before, e.counters()))
        with e.flip() as snap:
            ptrs.append(snap.device_cells()[0])
            keep = fill(snap, iv) if fill else None
            check_interval(torch, snap, M, iv, what)
            del keep
    for what in "DE":
        with e.flip() as snap:
            ptrs.append(snap.device_cells()[0])
            check_released(torch, snap, M)
    x, y = ptrs[0], ptrs[1]
    assert x != y and ptrs == [x, y, x, y, x], ptrs


# ---- K1 ----------------------------------------------------------------------------------------------------------------

K1 = [
    pytest.param("sorted_by_key", N0, "device", id="sorted-narrow-tiles"),
    pytest.param(None, N0, "device", id="shuffled-wide-floating-windows-global-row"),
    pytest.param(None, 8191, "device", id="remainder-loop-8191"),
    pytest.param(None, N0, "host", id="through-lh_submit"),
]


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("order,n,form", K1)
def test_single_name_routes(native_lib, torch_cuda, order, n, form, cell_bits):
    ivs = streams(1, n, order)
    dev = {id(iv): _dev(torch_cuda, iv.v) for iv in ivs} if form == "device" else {}
    with _engine(1, cell_bits=cell_bits) as e:
        go = (lambda iv: e.submit_device(0, dev[id(iv)])) if form == "device" else (lambda iv: e.submit(0, iv.v))
        run_sequence(torch_cuda, e, 1, ivs, moved=("samples_single",), submit=go)


# ---- mixed routes ------------------------------------------------------------------------------------------------------

GEN1 = {N.OPT_PART_MIN_PAIRS: 1 << 17, N.OPT_PART_V2: 0, N.OPT_PART_V3: 0}
GEN2 = ("samples_partitioned", "samples_partitioned_v2")
GEN3 = ("samples_partitioned", "samples_partitioned_v3")
ROUTES = [
    # names (the smallest at which the route's counter still moves by the whole call), pairs, options, counters, form
    # the small kernel switches itself off after an interval whose samples mostly miss its windows (A): armed again every interval
    pytest.param(20, N0, {N.OPT_SMALL_PATH: 1}, ("samples_small",), "u32", id="small-20"),
    pytest.param(5, N0, {N.OPT_SMALL_PATH: 1}, ("samples_small",), "u32", id="small-5"),
    pytest.param(700, N0, {}, ("samples_direct",), "u32", id="direct-cell-table-uint32"),
    pytest.param(700, N0, {}, ("samples_direct",), "u16", id="direct-cell-table-uint16"),
    pytest.param(700, 999, {}, ("samples_direct",), "u32", id="direct-kp_add-999"),
    pytest.param(700, N0, {}, ("samples_direct",), "submit_pairs", id="direct-host-submit_pairs"),
    pytest.param(700, N0, {}, ("samples_direct",), "reserve_commit", id="direct-host-reserve_commit"),
    pytest.param(1000, N0, GEN1, ("samples_partitioned",), "u32", id="gen1-one-level"),
    pytest.param(2049, N0, {**GEN1, N.OPT_TWO_LEVEL_ABOVE: 0}, ("samples_partitioned",), "u32", id="gen1-two-levels"),
    # the first generation's hot windows need 2 tiles of 4 096 pairs per workgroup, two workgroups per CU
    pytest.param(300, 2_200_000, {**GEN1, N.OPT_HOT_MIN_TILES: 1, N.OPT_HOT_WINDOWS: 1}, ("samples_partitioned",), "u32",
                 id="gen1-hot-windows-2200000-pairs-fill-every-CU-with-tiles"),
] + [
    pytest.param(64, N0, {N.OPT_PART_V2_MIN_PAIRS: 1 << 17, N.OPT_PART_V2_SHAPE: s}, GEN2, "u32", id=f"gen2-shape{s}") for s in range(4)
] + [
    pytest.param(8193, N0, {N.OPT_PART_V3_MIN_PAIRS: 1 << 17, N.OPT_PART_V3_DIRECT_MAX_PAIRS: 1}, GEN3, "u32", id="gen3-windowed-reduce"),
    pytest.param(8193, N0, {N.OPT_PART_V3_MIN_PAIRS: 1 << 17}, GEN3, "u32", id="gen3-window-free-reduce"),
]


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("M,n,opts,moved,form", ROUTES)
def test_mixed_routes(native_lib, torch_cuda, M, n, opts, moved, form, cell_bits):
    ivs = streams(M, n)
    dev = {}
    if form in ("u32", "u16"):
        dev = {id(iv): (_dev(torch_cuda, iv.ids.astype(np.uint16) if form == "u16" else iv.ids), _dev(torch_cuda, iv.v)) for iv in ivs}
    with _engine(M, cell_bits=cell_bits) as e:
        def options():
            for k, val in opts.items():
                e.set_option(k, val)

        def go(iv):
            if form in ("u32", "u16"):
                e.submit_pairs_device(*dev[id(iv)])
            elif form == "submit_pairs":
                e.submit_pairs(iv.ids, iv.v)
            else:
                e.submit_pairs_in_place(iv.ids, iv.v)
        run_sequence(torch_cuda, e, M, ivs, moved=moved, submit=go, before_each=options)


# ---- the import --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("shape", ["coo", "csr"])
def test_the_four_import_forms(native_lib, torch_cuda, shape, form, cell_bits):
    """The cells of A, B and C (A's with keys -32768 and 32767 in the first and the last name) added to EMPTY snapshots: the
    import widens the ranges itself, and the release clears what it added."""
    M = 40
    ivs = streams(M, 20_000)

    def fill(snap, iv):
        cells, counts = oracle_cells(iv.ids, iv.v)
        ids, keys = (cells >> U64(16)).astype(np.uint32), oracle.bin_to_key(cells & U64(0xffff))
        counts = counts.astype(U64)
        if shape == "coo":
            return add_coo(torch_cuda, snap, form, ids, keys, counts)
        offsets = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=M))]).astype(U64)
        return add_csr(torch_cuda, snap, form, offsets, keys, counts)
    with _engine(M, cell_bits=cell_bits) as e:
        run_sequence(torch_cuda, e, M, ivs, fill=fill)


# ---- both clear kernels on crafted spans ---------------------------------------------------------------------------------

SEG = 8192                         # k_clear_spans: 8 workgroups a row, 8 192 bins each
SPANS = [
    # (cells lo, cells hi, marked lo, marked hi); None: the cells' own span
    (0, NKEYS - 1, None), (SEG - 1, SEG, None), (0, 0, None), (NKEYS - 1, NKEYS - 1, None), (3 * SEG - 1, 4 * SEG, None),
    (SEG - 1, SEG - 1, None), (SEG, SEG, None), (30000, 30010, (29000, 31000)),           # ... marked wider than its cells
    (500, 500, None), (40000, 40062, None), (40001, 40064, None), (39999, 40063, None),   # 1, 63, 64 and 65 bins
    (None, None, (20000, 20100)),                                                         # marked, but only zeros
]


def crafted(M):
    """{row: (cells {bin: value}, marked span)}: rows 0 and 3 (the first workgroup of k_clear_rows_wave), 4, the last row of a
    full workgroup and the last row of all lead; every bin of every span holds (row << 16 | bin) + 1."""
    rows = [0, 3, 4, (M - 2) | 3 if ((M - 2) | 3) < M - 1 else M - 2, M - 1, 1, 2, 5, 6, M // 2, M - 5, M - 4, M - 3]
    assert len(set(rows)) == len(SPANS) and max(rows) == M - 1
    out = {}
    for m, (lo, hi, marked) in zip(rows, SPANS):
        cells = {} if lo is None else {b: (m << 16 | b) + 1 for b in range(lo, hi + 1)}
        out[m] = (cells, marked if marked else (lo, hi))
    return out


@pytest.mark.parametrize("cell_bits", [64, 32])
@pytest.mark.parametrize("M", [2047, 2049], ids=["k_clear_spans-2047", "k_clear_rows_wave-2049"])
def test_both_clear_kernels_on_crafted_spans(native_lib, torch_cuda, M, cell_bits):
    torch = torch_cuda
    plan = crafted(M)
    if M == 2049:
        assert {0, 3, 4, 2047, 2048} <= set(plan)
    per_row = np.zeros(M, dtype=U64)
    for m, (cells, _) in plan.items():
        per_row[m] = sum(cells.values())

    def want(m):
        row = np.zeros(NKEYS, dtype=U64)
        for b, c in plan.get(m, ({}, None))[0].items():
            row[b] = c
        return row
    iv = types.SimpleNamespace(n=int(per_row.sum()), per_row=per_row, want=want)
    narrow = streams(M, N0)[1]
    with _engine(M, cell_bits=cell_bits) as e:
        with e.flip() as snap:
            x = snap.device_cells()[0]
            if cell_bits == 64:
                ids = np.concatenate([np.full(len(c), m, dtype=np.uint32) for m, (c, _) in plan.items()])
                bins = np.concatenate([np.fromiter(c.keys(), dtype=np.int64, count=len(c)) for c, _ in plan.values()])
                vals = np.concatenate([np.fromiter(c.values(), dtype=U64, count=len(c)) for c, _ in plan.values()])
                snap.add_buckets(ids, oracle.bin_to_key(bins), vals)
                for m, (_, span) in plan.items():
                    snap.mark_dirty(m, 1, span[0], span[1])
            else:
                _write_narrow(torch, snap, [plan.get(m, ({}, None))[0] for m in range(M)], [plan.get(m, ({}, None))[1] for m in range(M)])
            rec = check_interval(torch, snap, M, iv, "crafted")
            assert snap.device_cells()[0] == x                      # (neither way of writing moved the store)
            for m, (_, span) in plan.items():
                assert tuple(rec.ranges[m]) == span, m
        # the other buffer comes and goes, X is handed out again: clean, cell by cell
        with e.flip() as snap:
            y = snap.device_cells()[0]
            check_released(torch, snap, M)
        with e.flip() as snap:
            assert snap.device_cells()[0] == x
            check_released(torch, snap, M)
        with e.flip() as snap:
            assert snap.device_cells()[0] == y
        # ... and an ingest into it: a range that was not reset, or a cell left behind, shows in the narrow interval
        before = e.counters()
        e.submit_pairs_device(_dev(torch, narrow.ids), _dev(torch, narrow.v))
        e.sync()
        assert _moved(before, e.counters()) == {"samples_direct": narrow.n}
        with e.flip() as snap:
            assert snap.device_cells()[0] == x
            check_interval(torch, snap, M, narrow, "narrow, after the clear")


# ---- across a widening ---------------------------------------------------------------------------------------------------

def test_across_a_widening(native_lib, torch_cuda):
    """A 32-bit engine whose bound falls inside the interval: the buffer moves to its uint64 store between two calls
    (k_widen_rows copies every span and zeroes the narrow store behind it).  The two stores of a buffer have different addresses,
    so the buffer is identified by the ORDER of the flips (two buffers alternate), not by device_cells()[0]; every check reads
    only the store the open snapshot reports."""
    torch = torch_cuda
    M = 300
    a, b, c = streams(M, N0)
    dev = {id(iv): (_dev(torch, iv.ids), _dev(torch, iv.v)) for iv in (a, b, c)}
    h = N0 // 2 & ~1
    with _engine(M, cell_bits=32) as e:
        def interval(iv, widen_at, what):
            e.set_option(N.OPT_WIDEN_AT_SAMPLES, widen_at)
            before = e.counters()
            d_ids, d_v = dev[id(iv)]
            e.submit_pairs_device(d_ids[:h], d_v[:h])
            e.submit_pairs_device(d_ids[h:], d_v[h:])               # (the second call finds the bound passed: the move)
            e.sync()
            after = e.counters()
            with e.flip() as snap:
                assert after["widenings"] - before["widenings"] == (1 if widen_at < iv.n else 0), what
                assert snap.device_cells()[2] == (8 if widen_at < iv.n else 4), what
                check_interval(torch, snap, M, iv, what)

        def empty(cell_bytes):
            with e.flip() as snap:
                assert snap.device_cells()[2] == cell_bytes
                check_released(torch, snap, M)
        interval(a, N0 // 3 * 2, "X: wide stream, widened")         # X's wide store
        empty(4)                                                    # Y
        interval(c, 0xffffffff, "X: narrow again")                  # X's narrow store: k_widen_rows left it clean
        empty(4)                                                    # Y
        interval(a, N0 // 3 * 2, "X: widened again")                # X's wide store, reused: the release cleared it
        empty(4)                                                    # Y
        empty(4)                                                    # X, back on its narrow store
        interval(b, 0xffffffff, "Y: first data")
        assert e.counters()["widenings"] == 2


# ---- release -> flip -> submit, no host synchronisation in between ---------------------------------------------------------

def test_the_clear_is_ordered_before_the_next_ingest(native_lib, torch_cuda):
    """Every row of X marked (0, 65535): the release has a gigabyte to zero (k_clear_spans).  The flip and a submit into the same
    rows follow at once; the ingest stream waits for the buffer's `cleared` event, or the clear wipes what it counted."""
    torch = torch_cuda
    M = 2047
    rows = (0, 1023, 2046)
    rng = np.random.default_rng(4096)
    ids = np.array(rows, dtype=np.uint32)[rng.integers(0, 3, 4096)]
    iv = by_values(ids, _values(rng, "signed_wide", ids, 4096), M)
    d_ids, d_v = _dev(torch, iv.ids), _dev(torch, iv.v)
    with _engine(M, cell_bits=64) as e:
        snap = e.flip()
        x = snap.device_cells()[0]
        cells, _, cb = sc.store_view(snap, M, torch)
        assert cb == 8
        pattern = torch.arange(1, NKEYS + 1, dtype=torch.int64, device="cuda")
        for m in rows:
            cells[m, :NKEYS] = pattern * (m + 1)
        torch.cuda.synchronize()
        snap.mark_dirty(0, M, 0, NKEYS - 1)
        del cells
        before = e.counters()
        snap.release()
        other = e.flip()
        e.submit_pairs_device(d_ids, d_v)                           # into X, behind its clear
        e.sync()
        assert _moved(before, e.counters()) == {"samples_direct": iv.n}
        with other:
            assert other.device_cells()[0] != x
            check_released(torch, other, M)
        with e.flip() as snap:
            assert snap.device_cells()[0] == x
            check_interval(torch, snap, M, iv, "X, behind the clear")


# ---- the judge sees what it is there for -------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_bits", [64, 32])
def test_the_judge_sees_planted_strays_in_a_real_store(native_lib, torch_cuda, cell_bits):
    """The plants of tests/test_span_contract.py written with torch into an open snapshot's store, on an engine of its own; no
    kernel of the project reads them, and they are zeroed again before the release."""
    torch = torch_cuda
    M = len(RANGES)
    with _engine(M, cell_bits=cell_bits) as e:
        with e.flip() as snap:
            cells, _, cb = sc.store_view(snap, M, torch)
            assert cb == cell_bits // 8
            host = clean_store(np.uint32 if cb == 4 else np.uint64)
            signed = host.view(np.int32 if cb == 4 else np.int64)
            for m, (lo, hi) in enumerate(RANGES):
                if lo <= hi:
                    cells[m, lo:hi + 1] = torch.from_numpy(signed[m, lo:hi + 1].copy()).cuda()
            torch.cuda.synchronize()
            for m, (lo, hi) in enumerate(RANGES):
                if lo <= hi:
                    snap.mark_dirty(m, 1, lo, hi)
            rec = sc.check_store(snap, M, torch)
            sc.assert_contract(rec)
            assert np.array_equal(rec.ranges, np.asarray(RANGES)) and rec.total.tolist() == host.sum(axis=1, dtype=U64).tolist()
            todo = plants(snap.row_stride())
            for _, (r, col, val), _ in todo:
                cells[r, col] = val
            torch.cuda.synchronize()
            rec = sc.check_store(snap, M, torch)
            assert sorted(rec.violations) == sorted(p[2] for p in todo)
            assert int(rec.npad.sum()) == 3 and int(rec.nstray.sum()) == 5
            with pytest.raises(AssertionError, match="3 padding cells, 5 cells outside their spans"):
                sc.assert_contract(rec)
            for _, (r, col, val), _ in todo:
                cells[r, col] = 0
            torch.cuda.synchronize()
            sc.assert_contract(sc.check_store(snap, M, torch))
            del cells
        with e.flip() as snap:
            check_released(torch, snap, M)
        with e.flip() as snap:
            check_released(torch, snap, M)
