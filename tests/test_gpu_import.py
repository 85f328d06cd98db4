"""lh_snapshot_add_buckets* (Snapshot.add_buckets / add_buckets_csr / add_raw): cells back INTO a snapshot, the inverse of
lh_buckets_all -- RawMetricSet.Histograms (metrics.go:54-60) of another process, an older interval or a checkpoint added per
cell (cells are a commutative integer sum, metrics.go:278, 292).  The checker is oracle/ throughout: counts, nbuckets, pkeys
and pvals bit for bit, sum within 1e-12 * sum|terms| (the order of summation is unpinned).

Engines are created with the default cell_bits=None, so that the suite's runs on 32-bit cells (LH_TEST_CELL_BITS=32) and on
engines that widen in the middle of a test (LH_TEST_WIDEN_AT) cover the import too."""
import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N

pytestmark = pytest.mark.gpu

PCTS = list(oracle.DEFAULT_PERCENTILES.values())
U64 = np.uint64


# ---- the oracle side: an interval as sorted packed cells (name << 16 | bin) and their uint64 counts -------------------
def oracle_cells(ids, v):
    bins = oracle.key_to_bin(oracle.compress_many(v)).astype(U64)
    cells, counts = np.unique((np.asarray(ids).astype(U64) << U64(16)) | bins, return_counts=True)
    return cells, counts.astype(U64)


def add_cells(*intervals):
    """Sum of intervals given as (cells, counts); counts wrap mod 2^64 as atomic.AddUint64 does."""
    cells = np.concatenate([c for c, _ in intervals])
    counts = np.concatenate([n for _, n in intervals]).astype(U64)
    uniq, inv = np.unique(cells, return_inverse=True)
    out = np.zeros(uniq.size, dtype=U64)
    np.add.at(out, inv, counts)
    return uniq, out


def coo_of(cells, counts):
    return (cells >> U64(16)).astype(np.uint32), oracle.bin_to_key(cells & U64(0xFFFF)), counts.astype(U64)


def dense_row(cells, counts, m):
    lo, hi = np.searchsorted(cells, [U64(m) << U64(16), U64(m + 1) << U64(16)])
    row = np.zeros(oracle.NKEYS, dtype=U64)
    row[(cells[lo:hi] & U64(0xFFFF)).astype(np.int64)] = counts[lo:hi]
    return row


def snapshot_cells(snap, M):
    off, keys, counts = snap.buckets_all(M)
    rows = np.repeat(np.arange(M, dtype=U64), np.diff(off.astype(np.int64)))
    return (rows << U64(16)) | oracle.key_to_bin(keys).astype(U64), counts


def check(snap, want, M, every=1):
    """The snapshot holds exactly `want` = (cells, counts with no zero among them): buckets_all, and extract against
    oracle.process_dense (count / nbuckets / present of every row; percentiles and sum of every `every`-th row)."""
    cells, counts = want
    got_cells, got_counts = snapshot_cells(snap, M)
    if not (np.array_equal(got_cells, cells) and np.array_equal(got_counts, counts)):
        a = dict(zip(got_cells.tolist(), got_counts.tolist()))
        b = dict(zip(cells.tolist(), counts.tolist()))
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        raise AssertionError(f"{len(bad)} cells differ, e.g. " + ", ".join(
            f"name {k >> 16} bin {k & 0xffff}: {a.get(k)} != {b.get(k)}" for k in bad[:6]))
    got = snap.extract(PCTS, M)
    rows = (cells >> U64(16)).astype(np.int64)
    total = np.zeros(M, dtype=U64)
    np.add.at(total, rows, counts)
    assert np.array_equal(got["count"], total)
    assert np.array_equal(got["nbuckets"], np.bincount(rows, minlength=M))
    assert np.array_equal(got["present"], (total != 0).astype(np.uint32))
    d = oracle.decompress_table()
    for m in range(0, M, every):
        row = dense_row(cells, counts, m)
        ref = oracle.process_dense(row, PCTS)
        assert int(got["count"][m]) == ref["count"] and int(got["nbuckets"][m]) == ref["nbuckets"], m
        assert np.array_equal(got["pvalid"][m], ref["pvalid"]), m
        assert np.array_equal(got["pkeys"][m], ref["pkeys"]), m
        assert np.array_equal(got["pvals"][m].view(U64), ref["pvals"].view(U64)), m
        if ref["count"]:
            assert abs(got["sum"][m] - ref["sum"]) <= 1e-12 * float(np.sum(np.abs(d) * row.astype(np.float64))), m
    return got


def stream(seed, M, n):
    """Seeded and shaped like tests/test_gpu_buckets.py: signed values over twelve decades; name 2 stays empty."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, M, n).astype(np.uint32)
    if M > 2:
        ids[ids == 2] = 0
    return ids, rng.normal(0, 1e3, n) * 10.0 ** rng.integers(0, 12, n)


def dev(torch, a):
    """numpy -> device tensor of the same bits (torch has no uint32 / uint64 arithmetic: the signed views)."""
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
    return torch.from_numpy(a).cuda()


def add_coo(torch, snap, form, ids, keys, counts):
    if form == "host":
        snap.add_buckets(ids, keys, counts)
        return None
    t = (dev(torch, ids), dev(torch, keys), dev(torch, counts))
    torch.cuda.synchronize()               # the producer of the arrays is complete
    snap.add_buckets(*t)
    return t                               # the caller keeps them until the snapshot's stream has passed the add


def add_csr(torch, snap, form, offsets, keys, counts, first=0):
    if form == "host":
        snap.add_buckets_csr(offsets, keys, counts, first)
        return None
    t = (dev(torch, offsets), dev(torch, keys), dev(torch, counts))
    torch.cuda.synchronize()
    snap.add_buckets_csr(*t, first=first)
    return t


def engine(M, **kw):
    import loghisto_amd
    kw.setdefault("num_buffers", 2)
    kw.setdefault("num_lanes", 1)
    kw.setdefault("lane_samples", 1 << 16)
    return loghisto_amd.Engine(max_metrics=M, **kw)


# ---- 1. round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("M,n", [(1, 300_000), (40, 300_000), (1024, 300_000), (20000, 2_000_000)])
def test_round_trip_through_buckets_all(native_lib, torch_cuda, M, n, form):
    """stream -> engine A -> buckets_all -> add_buckets_csr into an EMPTY snapshot of engine B: B's cells and extract equal
    the oracle's (and therefore A's).  20 000 names: an engine of 32-bit cells by default -- the snapshot widens first."""
    ids, v = stream(M * 31 + 7, M, n)
    want = oracle_cells(ids, v)
    with engine(M) as a:
        a.submit_pairs(ids, v)
        with a.flip() as snap:
            offsets, keys, counts = snap.buckets_all(M)
            assert np.array_equal(snapshot_cells(snap, M)[0], want[0])
    assert offsets[-1] == keys.size == counts.size == want[0].size
    with engine(M) as b:
        with b.flip() as snap:
            assert snap.buckets_all(M)[1].size == 0
            keep = add_csr(torch_cuda, snap, form, offsets, keys, counts)
            check(snap, want, M, every=1 if M <= 1024 else 61)
            off2, keys2, counts2 = snap.buckets_all(M)
            del keep
    assert np.array_equal(off2, offsets) and np.array_equal(keys2, keys) and np.array_equal(counts2, counts)


# ---- 2. merge into a live interval -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_coo_import_merges_into_an_ingested_interval(native_lib, torch_cuda, form):
    """X ingested normally; Y's oracle cells imported as COO in shuffled order, ~10 % of them split into 2 - 5 duplicate
    entries, count == 0 entries sprinkled in (some on cells nothing else touches): equals the oracle over X ++ Y."""
    M, n = 40, 300_000
    xi, xv = stream(101, M, n)
    yi, yv = stream(202, M, n)
    yv *= 3.7                                                            # other cells than X's, overlapping ones too
    rng = np.random.default_rng(303)
    ids, keys, counts = coo_of(*oracle_cells(yi, yv))
    split = np.nonzero((rng.random(ids.size) < 0.1) & (counts >= 5))[0]
    parts = [(ids, keys, counts.copy())]
    for j in split:
        k = int(rng.integers(2, 6))
        cut = rng.multinomial(int(counts[j]) - k, np.ones(k) / k) + 1       # k positive pieces of counts[j]
        parts[0][2][j] = cut[0]
        parts.append((np.full(k - 1, ids[j], dtype=np.uint32), np.full(k - 1, keys[j], dtype=np.int16), cut[1:].astype(U64)))
    nz = 5000                                                            # zero counts: on imported cells, on empty ones, on name 2
    parts.append((rng.integers(0, M, nz).astype(np.uint32), rng.integers(-32768, 32768, nz).astype(np.int16), np.zeros(nz, dtype=U64)))
    parts.append((np.full(7, 2, dtype=np.uint32), np.arange(7, dtype=np.int16), np.zeros(7, dtype=U64)))
    ids, keys, counts = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = rng.permutation(ids.size)
    ids, keys, counts = ids[order], keys[order], counts[order]
    assert split.size > 100 and int(counts.sum()) == n
    want = oracle_cells(np.concatenate([xi, yi]), np.concatenate([xv, yv]))
    with engine(M) as e:
        e.submit_pairs(xi, xv)
        with e.flip() as snap:
            keep = add_coo(torch_cuda, snap, form, ids, keys, counts)
            got = check(snap, want, M)
            del keep
    assert int(got["count"].sum()) == 2 * n and got["present"][2] == 0 and got["nbuckets"][2] == 0


# ---- 3. big counts ---------------------------------------------------------------------------------------------------
def test_counts_beyond_32_bits_and_the_wrap_on_32_bit_cells(native_lib, torch_cuda):
    """Engine(cell_bits=32): one cell += 2^32 + 5, one += 2^63, the same again += 2^63 (wraps to where it started)."""
    M, n = 64, 300_000
    ids, v = stream(404, M, n)
    base = oracle_cells(ids, v)
    k5 = int(oracle.bin_to_key(base[0][np.searchsorted(base[0], U64(5) << U64(16))] & U64(0xFFFF)))   # an occupied cell of name 5
    k7 = int(oracle.bin_to_key(base[0][np.searchsorted(base[0], U64(7) << U64(16))] & U64(0xFFFF)))
    big = (np.array([5], dtype=np.uint32), np.array([k5], dtype=np.int16), np.array([(1 << 32) + 5], dtype=U64))
    half = (np.array([7, 9], dtype=np.uint32), np.array([k7, 12345], dtype=np.int16), np.array([1 << 63, 1 << 63], dtype=U64))
    as_cells = lambda t: ((t[0].astype(U64) << U64(16)) | oracle.key_to_bin(t[1]).astype(U64), t[2])
    with engine(M, cell_bits=32) as e:
        assert N.lib().lh_cell_bytes(e._h) == 4
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            assert snap.device_cells()[2] == 4
            snap.add_buckets(*big)
            snap.add_buckets(*half)
            assert snap.device_cells()[2] == 8                          # the import moved the snapshot to its wide store
            want = add_cells(base, as_cells(big), as_cells(half))
            got = check(snap, want, M)                                   # percentiles against oracle.process_dense: no wrap yet
            start = int(dense_row(base[0], base[1], 7)[int(oracle.key_to_bin(k7))])
            keys, counts = snap.buckets(7)
            assert int(counts[keys.tolist().index(k7)]) == start + (1 << 63)
            assert int(got["count"][5]) == int(np.sum(ids == 5)) + (1 << 32) + 5
            snap.add_buckets(*half)                                      # 2^63 + 2^63: both cells wrap to where they started
            keys, counts = snap.buckets(7)
            assert int(counts[keys.tolist().index(k7)]) == start
            wrapped = add_cells(base, as_cells(big))
            got_cells, got_counts = snapshot_cells(snap, M)
            assert np.array_equal(got_cells, wrapped[0]) and np.array_equal(got_counts, wrapped[1])   # name 9's cell is 0 again
            assert snap.buckets(9)[0].size == np.count_nonzero(wrapped[0] >> U64(16) == U64(9))


# ---- 4. extreme keys, previously empty rows, and the clear -----------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_extreme_keys_into_empty_rows_and_the_clear_covers_them(native_lib, torch_cuda, form):
    M = 8
    ids = np.array([1, 1, 1, 1, 3, 6, 6], dtype=np.uint32)
    keys = np.array([32767, -32768, 0, -1, -32768, 32767, 32767], dtype=np.int16)
    counts = np.array([3, 1, 4, 1, 5, 9, 2], dtype=U64)
    want = add_cells(((ids.astype(U64) << U64(16)) | oracle.key_to_bin(keys).astype(U64), counts))
    with engine(M, num_buffers=2) as e:
        with e.flip() as snap:
            keep = add_coo(torch_cuda, snap, form, ids, keys, counts)
            got = check(snap, want, M)
            assert list(got["present"]) == [0, 1, 0, 1, 0, 0, 1, 0] and list(got["nbuckets"]) == [0, 4, 0, 1, 0, 0, 1, 0]
            k, c = snap.buckets(1)
            assert list(k) == [-32768, -1, 0, 32767] and list(c) == [1, 1, 4, 3]
            assert [list(x) for x in snap.buckets(6)] == [[32767], [11]]
            del keep
        # the release cleared what the import added (it clears the rows' dirty spans): nothing was submitted since, the
        # other buffer comes and goes, and the first one is handed out again
        with e.flip() as other:
            assert other.buckets_all(M)[1].size == 0
        with e.flip() as again:
            off, k, c = again.buckets_all(M)
            assert not off.any() and k.size == 0 and c.size == 0
            assert not again.extract(PCTS, M)["count"].any()
            from loghisto_amd import merge                               # and cell by cell, not only inside the spans
            view, _ = merge.snapshot_tensors(again, M)
            torch_cuda.cuda.ExternalStream(again.stream()).synchronize()
            assert int((view != 0).sum()) == 0


# ---- 5. tight ranges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("shape", ["coo", "csr"])
def test_dirty_spans_stay_tight(native_lib, torch_cuda, form, shape):
    """One cell into row 3 of 40: rows 2 and 4 stay empty (lo = 65536, hi = 0), row 3 reads lo == hi == bin; then a second
    import widens row 3 to the union and gives row 10 the span of its own cells, nothing more."""
    from loghisto_amd import merge
    torch = torch_cuda
    M = 40

    def spans(snap):
        torch.cuda.ExternalStream(snap.stream()).synchronize()
        return merge.snapshot_ranges(snap, M).cpu().numpy().view(np.uint32).reshape(M, 2)

    def put(snap, ids, keys, counts):
        ids, keys, counts = np.array(ids, dtype=np.uint32), np.array(keys, dtype=np.int16), np.array(counts, dtype=U64)
        if shape == "coo":
            return add_coo(torch, snap, form, ids, keys, counts)
        order = np.argsort(ids, kind="stable")
        offsets = np.searchsorted(ids[order], np.arange(M + 1)).astype(U64)
        return add_csr(torch, snap, form, offsets, keys[order], counts[order])

    with engine(M) as e:
        with e.flip() as snap:
            keep = [put(snap, [3], [100], [7])]
            b = int(oracle.key_to_bin(100))
            r = spans(snap)
            assert r[3].tolist() == [b, b]
            assert all(r[m].tolist() == [65536, 0] for m in range(M) if m != 3)
            keep.append(put(snap, [10, 3, 10, 10, 3, 4], [5, -200, 900, -7, 150, 33], [1, 1, 1, 1, 0, 0]))
            r = spans(snap)
            assert r[3].tolist() == [int(oracle.key_to_bin(-200)), b]                 # key 150 came with count 0: not there
            assert r[10].tolist() == [int(oracle.key_to_bin(-7)), int(oracle.key_to_bin(900))]
            assert all(r[m].tolist() == [65536, 0] for m in range(M) if m not in (3, 10))   # row 4 only got a zero count
            assert snap.extract(PCTS, M)["nbuckets"].tolist() == [2 if m == 3 else 3 if m == 10 else 0 for m in range(M)]
            del keep


# ---- 6. all or nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_a_bad_batch_adds_nothing(native_lib, torch_cuda, form):
    import loghisto_amd
    M, n = 40, 300_000
    ids, v = stream(606, M, n)
    want = oracle_cells(ids, v)
    y = coo_of(*oracle_cells(*stream(607, M, 50_000)))
    with engine(M) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            # COO: the LAST id is max_metrics
            bad_ids = y[0].copy()
            bad_ids[-1] = M
            with pytest.raises(loghisto_amd.LhError) as ei:
                add_coo(torch_cuda, snap, form, bad_ids, y[1], y[2])
            assert ei.value.code == N.ERANGE
            # ... also when that entry's count is 0
            zero_last = y[2].copy()
            zero_last[-1] = 0
            with pytest.raises(loghisto_amd.LhError) as ei:
                add_coo(torch_cuda, snap, form, bad_ids, y[1], zero_last)
            assert ei.value.code == N.ERANGE
            # CSR: a range past max_metrics
            order = np.argsort(y[0], kind="stable")
            offsets = np.searchsorted(y[0][order], np.arange(M + 1)).astype(U64)
            with pytest.raises(loghisto_amd.LhError) as ei:
                add_csr(torch_cuda, snap, form, offsets, y[1][order], y[2][order], first=1)
            assert ei.value.code == N.ERANGE
            # CSR: offsets that decrease (in the middle; and at the very end)
            for at in (M // 2, M):
                dec = offsets.copy()
                dec[at] = dec[at - 1] - U64(1)
                with pytest.raises(loghisto_amd.LhError) as ei:
                    add_csr(torch_cuda, snap, form, dec, y[1][order], y[2][order])
                assert ei.value.code == N.EINVAL, at
            # n = 0, an all-empty CSR, nothing but zero counts: fine, and nothing happens
            add_coo(torch_cuda, snap, form, y[0][:0], y[1][:0], y[2][:0])
            add_csr(torch_cuda, snap, form, np.zeros(M + 1, dtype=U64), y[1][:0], y[2][:0])
            add_coo(torch_cuda, snap, form, y[0][:100], y[1][:100], np.zeros(100, dtype=U64))
            check(snap, want, M)                                        # unchanged by all of the above
            # and the good batch still goes in afterwards
            keep = add_csr(torch_cuda, snap, form, offsets, y[1][order], y[2][order])
            check(snap, add_cells(want, oracle_cells(*stream(607, M, 50_000))), M)
            del keep


# ---- 7. roll-up ------------------------------------------------------------------------------------------------------
def test_roll_up_of_five_intervals_with_lifetime(native_lib, torch_cuda):
    """Five intervals exported (buckets_all), the first four added into the fifth's snapshot BEFORE accumulate: extract and
    the lifetime stores are the oracle's over the concatenated stream."""
    M, n = 40, 300_000
    parts = [stream(700 + i, M, n // 5) for i in range(5)]
    exported = []
    with engine(M, num_buffers=3) as e:
        for i, (ids, v) in enumerate(parts):
            e.submit_pairs(ids, v * (1.0 + i))
            snap = e.flip()
            if i < 4:
                exported.append(snap.buckets_all(M))
                snap.release()                                          # (never accumulated: the roll-up carries them)
        with snap:
            for offsets, keys, counts in exported:
                snap.add_buckets_csr(offsets, keys, counts)
            snap.accumulate()
            want = oracle_cells(np.concatenate([p[0] for p in parts]),
                                np.concatenate([p[1] * (1.0 + i) for i, p in enumerate(parts)]))
            got = check(snap, want, M)
            life_c, life_s = e.lifetime(M)
    assert int(got["count"].sum()) == n // 5 * 5
    assert np.array_equal(life_c, got["count"])
    assert np.array_equal(life_s, got["agg_sum_add"])
    for m in range(M):
        if got["count"][m]:
            assert int(got["agg_sum_add"][m]) == oracle.f64_to_u64_amd64(float(got["sum"][m]))


# ---- 8. wire text ----------------------------------------------------------------------------------------------------
def test_serialize_after_add_raw_is_the_oracles_text(native_lib, torch_cuda):
    M, n = 24, 300_000
    names = [f"svc_{i}.rpc_latency" for i in range(M)]
    xi, xv = stream(808, M, n)
    yi, yv = stream(809, M, n)
    ycells = oracle_cells(yi, yv)
    raw = {}
    for m in reversed(range(M)):                                         # names arrive in another order than they were interned in
        lo, hi = np.searchsorted(ycells[0], [U64(m) << U64(16), U64(m + 1) << U64(16)])
        if hi > lo:
            raw[names[m]] = (oracle.bin_to_key(ycells[0][lo:hi] & U64(0xFFFF)), ycells[1][lo:hi])
    raw["late.arrival"] = (np.array([100, 200], dtype=np.int16), np.array([2, 3], dtype=U64))   # a name only the peer has
    names.append("late.arrival")
    wire = dict(prefix="put ", sep=" 1411104988 ", suffix=" host=box-1_a\n", underscore_to_dot=False)
    pct = oracle.DEFAULT_PERCENTILES
    with engine(M + 8) as e:
        for nm in names[:M]:
            e.intern(nm)
        e.submit_pairs(xi, xv)
        with e.flip() as snap:
            snap.add_raw(raw)
            assert e.num_metrics() == M + 1 and e.lookup("late.arrival") == M
            text = snap.serialize(pct, **wire)
            stats = snap.extract(PCTS, M + 1)
    late = ((U64(M) << U64(16)) | oracle.key_to_bin(np.array([100, 200])).astype(U64), np.array([2, 3], dtype=U64))
    want = add_cells(oracle_cells(xi, xv), ycells, late)
    rows = [dense_row(want[0], want[1], m) for m in range(M + 1)]
    lines = oracle.wire_lines(names, rows, pct, sums=stats["sum"], **wire)
    assert text.decode() == "".join(lines)
    assert len(lines) == 12 * sum(1 for r in rows if r.any()) and b"put late.arrival_count 1411104988 5.000000 host" in text
    d = oracle.decompress_table()
    for m in range(M + 1):                                               # the sums the text carries are the oracle's within 1e-12
        ref = oracle.process_dense(rows[m], [])
        if ref["count"]:
            assert abs(stats["sum"][m] - ref["sum"]) <= 1e-12 * float(np.sum(np.abs(d) * rows[m].astype(np.float64)))


# ---- 9. extract before and after -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_extract_before_and_after_the_import(native_lib, torch_cuda, form):
    M, n = 40, 300_000
    xi, xv = stream(909, M, n)
    yi, yv = stream(910, M, n)
    x, y = oracle_cells(xi, xv), oracle_cells(yi, yv * 0.01)
    with engine(M) as e:
        e.submit_pairs(xi, xv)
        with e.flip() as snap:
            before = check(snap, x, M)
            keep = add_coo(torch_cuda, snap, form, *coo_of(*y))
            after = check(snap, add_cells(x, y), M)                      # no stale result
            del keep
    assert int(after["count"].sum()) == 2 * int(before["count"].sum()) == 2 * n
    assert not np.array_equal(after["pkeys"], before["pkeys"])
