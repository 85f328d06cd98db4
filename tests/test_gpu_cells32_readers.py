"""Every reader of a snapshot of 32-bit cells (ABI 7: the default store above 8 192 names), on CRAFTED rows.

The other tests reach k_extract<uint32_t>, k_extract_wave<uint32_t>, k_count_cells / k_compact_cells<uint32_t>, the narrow
paths of lh_count.hip, k_widen_rows and the uint32 clear kernels only with ingested streams -- dense, contiguous windows of
small counts -- and tests/test_gpu_extract_thresholds.py writes its rows through lh_snapshot_rows, which moves the snapshot
to uint64 cells before a cell is written.  Here the rows of tests/_cells32_rows.py (every lo % 4, cells either side of
2^22, the largest total the uint32 prefix scan may see, spans around 1 024 bins, the ends of the key space, totals beyond
2^32, sums in every branch of uint64(float64); tests/test_cells32_rows.py keeps that list honest) go straight into the
narrow store through lh_snapshot_cells, and every result is compared with oracle.process_dense on the same row."""
import ctypes as C
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests import _cells32_rows as R
from tests.test_gpu_count_le import device_form, take_of
from tests.test_gpu_extract_thresholds import P_A

pytestmark = pytest.mark.gpu

M = 2400                       # extract(P, M): a wave per metric (>= 2 048 names); extract(P, 1500, first=100): a block per metric
SUB_FIRST, SUB_N = 100, 1500
P_DEFAULT = list(oracle.DEFAULT_PERCENTILES.values())
PSETS = {"P_A": P_A, "default": P_DEFAULT}
FIELDS = ("count", "sum", "avg", "agg_sum_add", "nbuckets", "present", "pvals", "pkeys", "pvalid")
U64 = np.uint64


def _same(a, b, what):
    """Bit for bit, every field; two NaNs (avg of an empty row: 0 / 0) are the same result."""
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        if x.dtype.kind == "f":
            nan = np.isnan(x) & np.isnan(y)
            x, y = np.where(nan, 0.0, x).view(U64), np.where(nan, 0.0, y).view(U64)
        assert np.array_equal(x, y), (what, k)


def _engine(M):
    import loghisto_amd
    return loghisto_amd.Engine(max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16, cell_bits=32)


def _row_view(torch, ptr, m, stride):
    from loghisto_amd import merge
    return torch.as_tensor(merge._DeviceArray(ptr + m * stride * 4, (N.NKEYS,), "<i4"), device="cuda")


def write_rows(torch, e, rows):
    """Row 0 is ingested; rows 1 .. are written into the snapshot's uint32 cells as they are and marked with their spans."""
    e.submit(0, R.ROW0_SAMPLES)
    snap = e.flip()
    e.sync()
    ptr, nrows, cb = snap.device_cells()
    assert cb == 4 and nrows == len(rows)
    stride = snap.row_stride()
    todo = [(m, r) for m, r in enumerate(rows) if m and r.bins.size]
    windows = [r.window() for _, r in todo]
    flat = torch.from_numpy(np.concatenate(windows).view(np.int32)).cuda()          # one upload of the occupied windows
    at = 0
    for (m, r), w in zip(todo, windows):
        lo, hi = r.span
        _row_view(torch, ptr, m, stride)[lo:hi + 1] = flat[at:at + w.size]
        at += w.size
    torch.cuda.synchronize()
    for m, r in enumerate(rows):
        if m and r.span is not None:                                                # (a span of zeros is marked too)
            snap.mark_dirty(m, 1, r.span[0], r.span[1])
    return snap


_REF = {}


def reference(rows, pname):
    """oracle.process_dense of every row, computed once per percentile set (a dense row at a time)."""
    if pname not in _REF:
        _REF[pname] = [oracle.process_dense(r.dense(), PSETS[pname]) for r in rows]
    return _REF[pname]


@pytest.fixture(scope="module")
def crafted(native_lib, torch_cuda):
    rows = R.make_rows(M)
    with _engine(M) as e:
        snap = write_rows(torch_cuda, e, rows)
        c = types.SimpleNamespace(e=e, snap=snap, rows=rows, torch=torch_cuda, cells=snap.device_cells(),
                                  widenings=e.counters()["widenings"], D=oracle.decompress_table())
        yield c
        snap.release()


def still_narrow(c):
    """Reading moves nothing: the same store, 4-byte cells, no widening."""
    assert c.snap.device_cells() == c.cells and c.cells[2] == 4
    assert c.e.counters()["widenings"] == c.widenings


def check_against_oracle(rows, got, ref, D):
    for m, (r, want) in enumerate(zip(rows, ref)):
        what = (m, r.kind)
        assert int(got["count"][m]) == want["count"] == r.total(), what
        assert int(got["nbuckets"][m]) == want["nbuckets"] == r.bins.size, what
        assert np.array_equal(got["pvalid"][m], want["pvalid"]), what
        assert np.array_equal(got["pkeys"][m], want["pkeys"]), (what, got["pkeys"][m], want["pkeys"])
        assert np.array_equal(got["pvals"][m].view(U64), want["pvals"].view(U64)), what
        s = np.float64(got["sum"][m])
        assert abs(float(s) - want["sum"]) <= 1e-12 * r.magnitude(D), (what, float(s), want["sum"])
        with np.errstate(invalid="ignore", divide="ignore"):
            avg = s / np.float64(int(got["count"][m]))
        if r.total():
            assert np.array_equal(np.array([avg]).view(U64), np.array([got["avg"][m]]).view(U64)), (what, avg, got["avg"][m])
        else:
            assert avg != avg and got["avg"][m] != got["avg"][m], what
        assert int(got["agg_sum_add"][m]) == oracle.f64_to_u64_amd64(float(s)), (what, float(s))
        assert int(got["present"][m]) == (1 if r.total() else 0), what
        if r.total() == 0:                                 # never marked, or marked over nothing but zeros
            assert int(got["count"][m]) == 0 and int(got["nbuckets"][m]) == 0 and not got["pvalid"][m].any(), what


@pytest.mark.parametrize("pname", list(PSETS))
def test_extract_on_narrow_cells_against_the_oracle(crafted, pname):
    c, P = crafted, PSETS[pname]
    got = c.snap.extract(P, M)                             # k_extract_wave<uint32_t>
    sub = c.snap.extract(P, SUB_N, first=SUB_FIRST)        # k_extract<uint32_t>
    _same({k: got[k][SUB_FIRST:SUB_FIRST + SUB_N] for k in FIELDS}, sub, "wave per metric / block per metric")
    check_against_oracle(c.rows, got, reference(c.rows, pname), c.D)
    # every branch of the conversion was reached by what the kernels summed
    seen = {R.conversion_branch(float(s)) for s in got["sum"]}
    assert seen >= {"0_to_2_63", "2_63_to_2_64", "ge_2_64", "le_minus_2_63", "negative"}, seen
    still_narrow(c)


@pytest.mark.parametrize("pname", list(PSETS))
def test_compact_and_view_forms_equal_extract(crafted, pname):
    c, P = crafted, PSETS[pname]
    for first, n in ((0, M), (SUB_FIRST, SUB_N)):          # both kernels
        got = c.snap.extract(P, n, first=first)
        view = c.snap.extract_view(P, n, first=first)
        _same(got, {k: np.array(view[k]) for k in FIELDS}, ("extract_view", first))
        # lh_expand_compact derives avg, uint64(sum) and present on the HOST: its own copy of the conversion
        _same(got, c.snap.expand_compact(c.snap.extract_compact(P, n, first=first)), ("expand_compact", first))
    still_narrow(c)


def test_bucket_listings_are_the_nonzero_cells(crafted):
    c = crafted
    off, keys, counts = c.snap.buckets_all(M)              # k_count_cells / k_compact_cells<uint32_t>
    want_off = np.zeros(M + 1, dtype=U64)
    np.cumsum([r.bins.size for r in c.rows], dtype=U64, out=want_off[1:])
    assert np.array_equal(off, want_off)
    assert np.array_equal(keys, np.concatenate([oracle.bin_to_key(r.bins) for r in c.rows]))
    assert np.array_equal(counts, np.concatenate([r.counts for r in c.rows]))
    f, n = 700, 900                                        # a sub-range
    o2, k2, c2 = c.snap.buckets_all(n, first=f)
    a, b = int(off[f]), int(off[f + n])
    assert np.array_equal(o2, off[f:f + n + 1] - off[f]) and np.array_equal(k2, keys[a:b]) and np.array_equal(c2, counts[a:b])
    boundary = [m for m, r in enumerate(c.rows) if r.kind in ("only_bin_0", "only_bin_65535", "both_ends", "full_range_small",
                                                              "full_range_large", "never_marked", "marked_zero_wide")
                or r.kind.startswith(f"one_cell_{R.U32}/") or r.kind.startswith("five_cells_of_2^32-1/")]
    assert len(boundary) == 15
    for m in boundary + [0]:
        k1, c1 = c.snap.buckets(m)
        assert np.array_equal(k1, oracle.bin_to_key(c.rows[m].bins)) and np.array_equal(c1, c.rows[m].counts), (m, c.rows[m].kind)
    still_narrow(c)


def _prefix_counts(rows, bounds):
    """(cum[M, nb], total[M]): the crafted rows' prefix sums at the bounds' bins."""
    E = take_of(bounds)
    cum = np.zeros((len(rows), E.size), dtype=U64)
    total = np.zeros(len(rows), dtype=U64)
    for m, r in enumerate(rows):
        pre = np.zeros(r.bins.size + 1, dtype=U64)
        np.cumsum(r.counts, dtype=U64, out=pre[1:])
        cum[m] = pre[np.searchsorted(r.bins, E, side="left")]                       # cells with bin < E
        total[m] = pre[-1]
    return cum, total


@pytest.mark.parametrize("shape,wave_from", [("wave_per_row", 1), ("workgroup_per_row", 1 << 30)])
def test_count_le_on_narrow_cells(crafted, shape, wave_from):
    c = crafted
    D = c.D
    rng = np.random.default_rng(7)
    fixed = np.array([-np.inf, D[0], D[1], D[255], D[256], D[257], D[32768], D[65535], np.inf])
    occupied = np.concatenate([r.bins[[0, -1]] for r in c.rows[R.FIRST_SPECIAL:R.FIRST_SPECIAL + 160] if r.bins.size])
    sets = [np.sort(np.concatenate([fixed, D[rng.integers(0, 65536, 35)], D[rng.choice(occupied, 20)]])),      # 64 bounds
            np.sort(D[rng.choice(occupied, 9)]), np.array([D[32768]]), fixed]
    prev = C.c_uint32(0)
    try:
        assert N.lib().lh_tool_count_le_switch(wave_from, C.byref(prev)) == 0
        for b in sets:
            want_cum, want_total = _prefix_counts(c.rows, b)
            host = c.snap.count_le(b, M)                                                # k_count_le_*<uint32_t>
            bad = np.argwhere(host["cum"] != want_cum)
            assert bad.size == 0, (shape, len(bad), bad[0], c.rows[bad[0][0]].kind, host["cum"][tuple(bad[0])], want_cum[tuple(bad[0])])
            assert np.array_equal(host["total"], want_total)
            dcum, dtotal = device_form(c.torch, c.snap, b, M)
            assert np.array_equal(dcum, want_cum) and np.array_equal(dtotal, want_total)
            f, n = 3, M - 5                                                             # a sub-range, host form
            part = c.snap.count_le(b, n, f)
            assert np.array_equal(part["cum"], want_cum[f:f + n]) and np.array_equal(part["total"], want_total[f:f + n])
    finally:
        assert N.lib().lh_tool_count_le_switch(0, C.byref(prev)) == 0
    still_narrow(c)


def test_widening_moves_every_crafted_cell_and_nothing_else(native_lib, torch_cuda):
    """lh_snapshot_rows on the crafted snapshot: k_widen_rows copies every span into the uint64 store.  The two stores
    hold the same rows, and k_extract_wave / k_extract<uint64_t> read them to the same bits as the uint32 instantiations."""
    torch = torch_cuda
    from loghisto_amd import merge
    rows = R.make_rows(M)
    with _engine(M) as e:
        with write_rows(torch, e, rows) as snap:
            before = snap.extract(P_A, M), snap.extract(P_A, SUB_N, first=SUB_FIRST)
            assert snap.device_cells()[2] == 4 and e.counters()["widenings"] == 0
            wide, _ = merge.snapshot_tensors(snap, M)
            assert snap.device_cells()[2] == 8 and e.counters()["widenings"] == 1
            todo = [(m, r) for m, r in enumerate(rows) if r.bins.size]
            flat = torch.from_numpy(np.concatenate([r.window().astype(U64) for _, r in todo]).view(np.int64)).cuda()
            bad = torch.zeros((), dtype=torch.int64, device="cuda")
            at = 0
            for m, r in todo:                                                            # window by window, on the device
                lo, hi = r.span
                w = hi - lo + 1
                bad += (wide[m, lo:hi + 1] != flat[at:at + w]).sum()
                at += w
            assert int(bad.item()) == 0
            # ... and nothing outside the windows: every row's sum and number of occupied cells over all 65 536 bins
            sums = wide.sum(dim=1).cpu().numpy().view(U64)
            cells = (wide != 0).sum(dim=1).cpu().numpy()
            assert np.array_equal(sums, np.array([r.total() for r in rows], dtype=U64))
            assert np.array_equal(cells, np.array([r.bins.size for r in rows]))
            after = snap.extract(P_A, M), snap.extract(P_A, SUB_N, first=SUB_FIRST)
            _same(before[0], after[0], "wave per metric, uint32 / uint64 cells")
            _same(before[1], after[1], "block per metric, uint32 / uint64 cells")


TINY = [(5, np.array([3.0, 3.0, 1e6])), (7, np.array([42.0, -1.0]))]


@pytest.mark.parametrize("widen", [False, True], ids=["never_widened", "widened"])
@pytest.mark.parametrize("nrows", [2400, 600], ids=["k_clear_rows_wave", "k_clear_spans"])
def test_release_leaves_the_narrow_store_clean(native_lib, torch_cuda, nrows, widen):
    """launch_clear (lh_kernels.hip) takes k_clear_rows_wave from 2 048 rows on and k_clear_spans + k_init_ranges below:
    2 400 rows the former, 600 the latter, <uint32_t> when the snapshot is released narrow.  A snapshot that widened is
    cleared on its uint64 store (<uint64_t>); its narrow store is the one k_widen_rows zeroed behind its copy.  Either
    way the buffer's next interval finds nothing but its own samples, the padding behind bin 65 535 included."""
    torch = torch_cuda
    from loghisto_amd import merge
    rows = R.make_rows(nrows)
    with _engine(nrows) as e:
        with write_rows(torch, e, rows) as snap:
            ptr0 = snap.device_cells()[0]
            got = snap.extract(P_DEFAULT, nrows)
            assert np.array_equal(got["count"], np.array([r.total() for r in rows], dtype=U64))
            if widen:
                merge.snapshot_tensors(snap, nrows)
                assert snap.device_cells()[2] == 8
        for mid, v in TINY[:1]:                            # the other buffer's interval
            e.submit(mid, v)
        e.flip().release()
        want = {}
        for mid, v in TINY:                                # the crafted snapshot's buffer comes round again
            e.submit(mid, v)
            h = oracle.histogram_dense(v)
            want.update({(mid, int(b)): int(h[b]) for b in np.nonzero(h)[0]})
        with e.flip() as snap:
            e.sync()
            ptr, n, cb = snap.device_cells()
            assert (ptr, n, cb) == (ptr0, nrows, 4)            # the same narrow store
            stride = snap.row_stride()
            store = torch.as_tensor(merge._DeviceArray(ptr, (nrows * stride,), "<i4"), device="cuda")   # padding included
            at = store.nonzero().flatten()
            assert int(at.numel()) == len(want)
            got = {(int(i) // stride, int(i) % stride): int(c) for i, c in zip(at.cpu().numpy(), store[at].cpu().numpy())}
            assert got == want
            if widen:                                          # the wide store behind its clear: this interval's cells, no others
                wide, _ = merge.snapshot_tensors(snap, nrows)
                assert snap.device_cells()[2] == 8
                assert int((wide != 0).sum().item()) == len(want) and int(wide.sum().item()) == sum(want.values())
