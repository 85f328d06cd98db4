"""The packed (name, bin) key at its edges.  Several LDS tables of the mixed ingest key a cell as name << 16 | bin in 32 bits
and mark an empty slot with 0xffffffff (OV_EMPTY, lh_windows.h): the cell table of the direct path and of the clustered finish
(k_scatter_clustered, lh_kernels_part2.h) and the overflow tables of the partitioned paths (ov_add).

 1. The marker is a real key: name 65 535 of a 65 536-name engine at key +32767 (bin 65 535, values around 2.0196e142) packs to
    exactly 0xffffffff.  A table that absorbs it counts the sample in a slot that still reads as empty: the sample is lost from
    its cell and the count is credited to whichever key claims the slot next.
 2. An engine of more than 65 536 names takes the direct path for every mixed call; (id << 16) | bin drops the id's high bits,
    so the samples of name 65 536 + i would be counted in row i.

Every test compares every occupied cell of every row, and each row's count, with the oracle (check, tests/test_gpu_part3.py):
a lost sample, a sample in the wrong cell and a sample in the wrong row all show.  histogramCache[name][compress(v)] += 1,
metrics.go:273-295, exact in every cell."""
import functools

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_part3 import PCTS, _dev, _ids, _values, check

gpu = pytest.mark.gpu

M16 = 65536                                      # config 4's name count: the last name is 65 535
MBIG = 65536 + 512                               # 16.1 GiB per epoch buffer at 32-bit cells; names 65 536 .. 66 047 alias 0 .. 511
BIG = 2.0196e142                                 # key +32767 = bin 65 535
WRAP = 3e142                                     # beyond the int16 key domain: amd64 wrap
BASE = 1 << 18                                   # pairs of the edge stream; a call of another size repeats or cuts it
RUNS = ((1500, 1), (5000, 7), (20000, 3000))     # (start, length) of the runs of the marker cell, all below 2^16
# the three configurations of the cell table on its own (launch_cells_t): 1 024-pair tiles + 4 096 slots below 2^17 pairs,
# 1 024-pair tiles + 16 384 slots up to 2 * CUs tiles of 8 192, 8 192-pair tiles above -> (pairs, tile)
TABLE_SIZES = ((70_000, 1024), ((1 << 17) + 1025, 1024), ((1 << 22) + 8191 + 1024, 8192))
N_SORTED = (3 << 20) + 4099                      # third generation, four level-1 tiles per workgroup


def _below_marker():
    """A value in the bin just below the marker's (key +32766)."""
    return oracle.decompress(32766)


@functools.lru_cache(maxsize=None)
def edge_base(values="lognormal"):
    """The edge stream, BASE pairs over 65 536 names: a Zipf x lognormal background (or few-valued: `constant`) and, INTERLEAVED
    with it (appended they would all sit behind the last whole tile, which never sees a table), the marker cell (65 535, bin
    65 535) in runs of 1, 7 and 3 000 and scattered singly, the same name at key -32767, in the neighbouring bin and at ordinary
    values, name 65 534 at key +32767 (0xfffeffff), name 0 at key +32767 and at the wrap value."""
    rng = np.random.default_rng(65535)
    ids = _ids(rng, M16, BASE, 1.0)
    v = _values(rng, values, ids, BASE)
    for start, length in RUNS:
        ids[start:start + length] = M16 - 1
        v[start:start + length] = BIG
    kinds = [(M16 - 1, BIG), (M16 - 1, -BIG), (M16 - 1, _below_marker()), (M16 - 1, 12345.0), (M16 - 2, BIG), (0, BIG), (0, WRAP),
             (M16 - 1, BIG), (M16 - 1, 1e5), (M16 - 2, 77.0)]
    pos = np.arange(37, BASE, 257)               # 1 020 places, every 257th pair: in every tile of 1 024
    pos = pos[~np.isin(pos, np.concatenate([np.arange(s, s + k) for s, k in RUNS]))]
    for j, (name, val) in enumerate(kinds):
        ids[pos[j::len(kinds)]] = name
        v[pos[j::len(kinds)]] = val
    ids.setflags(write=False)
    v.setflags(write=False)
    return ids, v


@functools.lru_cache(maxsize=None)
def edge_stream(n, values="lognormal"):
    ids, v = edge_base(values)
    return np.resize(ids, n), np.resize(v, n)


@functools.lru_cache(maxsize=None)
def plain_stream(n):
    """The background alone (no name at key +-32767): the interval after the edge stream's."""
    rng = np.random.default_rng(7)
    ids = _ids(rng, M16, BASE, 1.0)
    return np.resize(ids, n), np.resize(_values(rng, "lognormal", ids, BASE), n)


@functools.lru_cache(maxsize=None)
def sorted_stream():
    """The edge stream over a few-valued background, sorted by name (stable): name 0 first, names 65 534 and 65 535 last."""
    ids, v = edge_stream(N_SORTED, "constant")
    order = np.argsort(ids, kind="stable")
    return ids[order], v[order]


def _marker(ids, v):
    return (ids == M16 - 1) & (v == BIG)


def test_the_edge_stream_holds_the_marker_cell_inside_whole_tiles():
    """Runs without a GPU: the streams of this file really hold (65 535, bin 65 535) and its neighbours, in front of the last
    whole tile of every call size used below."""
    assert oracle.compress(BIG) == 32767 and int(oracle.key_to_bin(np.int16(32767))) == 65535
    assert ((M16 - 1) << 16 | int(oracle.key_to_bin(np.int16(32767)))) == 0xffffffff
    assert oracle.compress(-BIG) == -32767 and oracle.compress(_below_marker()) == 32766
    assert int(oracle.key_to_bin(np.int16(32766))) == 65534
    ids, v = edge_base()
    bins = oracle.key_to_bin(oracle.compress_many(v)).astype(np.uint64)
    cells = set(((ids.astype(np.uint64) << np.uint64(16)) | bins).tolist())
    for want in (0xffffffff, 0xfffffffe, 0xfffeffff, 0x0000ffff, (M16 - 1) << 16 | int(oracle.key_to_bin(np.int16(-32767))),
                 int(oracle.key_to_bin(np.int16(oracle.compress(WRAP))))):
        assert want in cells, hex(want)
    for n, tile in TABLE_SIZES:
        sid, sv = edge_stream(n)
        whole = n // tile * tile
        assert 0 < whole < n                                     # a ragged tail behind the tiles
        assert np.count_nonzero(_marker(sid, sv)[:whole]) > 3000, n
        assert np.count_nonzero(_marker(sid[2:], sv[2:])[:(n - 2) // tile * tile]) > 3000, n   # ... of the second launch too
        for start, length in RUNS:                               # the runs are runs, in the call's first tiles
            assert _marker(sid, sv)[start:start + length].all() and not _marker(sid, sv)[start - 1], (n, start)
    # sorted by name: the marker samples are the stream's end -- behind the tiles level 1 keeps (the first half: two of every
    # workgroup's four), most of them in front of the last whole tile
    sid, sv = sorted_stream()
    at = np.nonzero(_marker(sid, sv))[0]
    whole = N_SORTED // 8192 * 8192
    assert at.min() > N_SORTED // 2 + 8192 and np.count_nonzero(at < whole) > 3000
    assert sid[0] == 0 and sid[-1] == M16 - 1 and np.all(np.diff(sid.astype(np.int64)) >= 0)
    # the large engine's stream reaches both halves of every aliased pair of rows
    bid, _ = big_stream(70_000)
    assert np.count_nonzero(bid >= M16) > 20_000 and np.count_nonzero(bid < 512) > 20_000 and bid.max() == MBIG - 1


# ---- 1. the marker cell through the cell table on its own ------------------------------------------------------------------

def _fresh(e):
    """An engine shared by several tests starts each of them on an empty interval, whatever the test before it left."""
    import loghisto_amd
    for step in (e.sync, lambda: e.flip().release()):
        try:
            step()
        except loghisto_amd.LhError as err:      # the sticky id error of a test that submitted bad ids, nothing else
            if err.code != N.ERANGE:
                raise
    return e.counters()


@pytest.fixture(scope="module")
def table_engine(native_lib, torch_cuda):
    import loghisto_amd
    with loghisto_amd.Engine(max_metrics=M16, num_buffers=2, num_lanes=1, lane_samples=1 << 16) as e:
        e.set_option(N.OPT_PART_MIN_PAIRS, 1 << 30)        # every call: the direct path (tests/test_gpu_cells.py)
        yield e


@gpu
@pytest.mark.parametrize("n", [n for n, _ in TABLE_SIZES])
@pytest.mark.parametrize("id16", [False, True])
def test_cell_table_counts_the_marker_cell(table_engine, torch_cuda, n, id16):
    """k_scatter_clustered on its own (launch_ingest_pairs_cells), one call size in each of its three configurations, both id
    widths.  Two launches into one interval; then an interval without any name at key +-32767, in which a count left behind in
    a slot that read as empty would show."""
    e = table_engine
    ids, v = edge_stream(n)
    d_ids = _dev(torch_cuda, ids.astype(np.uint16) if id16 else ids)
    d_v = _dev(torch_cuda, v)
    c0 = _fresh(e)
    e.submit_pairs_device(d_ids, d_v)
    e.submit_pairs_device(d_ids[2:], d_v[2:])              # a second launch into the same interval (cells add up)
    e.sync()
    c = e.counters()
    assert c["samples_direct"] - c0["samples_direct"] == 2 * n - 2 and c["samples_partitioned"] == 0, sorted(c.items())
    with e.flip() as snap:
        check(snap, np.concatenate([ids, ids[2:]]), np.concatenate([v, v[2:]]), M16, snap.extract(PCTS, M16))
    pid, pv = plain_stream(n)
    d_pid, d_pv = _dev(torch_cuda, pid.astype(np.uint16) if id16 else pid), _dev(torch_cuda, pv)
    e.submit_pairs_device(d_pid, d_pv)
    e.sync()
    with e.flip() as snap:
        check(snap, pid, pv, M16, snap.extract(PCTS, M16))
    c = e.counters()
    assert c["samples_direct"] - c0["samples_direct"] == 3 * n - 2 and c["samples_partitioned"] == 0, sorted(c.items())


# ---- ... behind the scatter kernels (g_resume) -----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("id16", [False, True])
def test_clustered_finish_counts_the_marker_cell(native_lib, torch_cuda, id16):
    """The stream shape of test_a_clustered_call_is_finished_by_the_cell_table (tests/test_gpu_part3.py) at 65 536 names: sorted
    by name, just above 3 * 2^20 pairs = 384 level-1 tiles, four per workgroup (96 workgroups).  At this size the first half of
    the stream is the 200 most frequent names, which level 1 would count in its hot windows without touching a region (the
    existing test needs 25 M pairs to put names that are NOT hot a few to a tile); the hot windows are therefore off here.
    Every workgroup's first two tiles (the first half of the stream) then hold a handful of names, i.e. of partitions, overflow
    their regions by far more than an eighth, and the workgroup leaves its other two tiles to k_scatter_clustered: the second
    half, which ends in names 65 534 and 65 535.  Name 0's edge values go through level 1's overflow path.  The background is
    few-valued (one cell per name), so that the table meets fewer than a quarter as many cells as samples and reports nothing as
    overflow itself: region_overflows is what level 1 overflowed, at most the two tiles each workgroup kept."""
    import loghisto_amd
    ids, v = sorted_stream()
    n = N_SORTED
    d_ids = _dev(torch_cuda, ids.astype(np.uint16) if id16 else ids)
    d_v = _dev(torch_cuda, v)
    with loghisto_amd.Engine(max_metrics=M16, num_buffers=2, num_lanes=1, lane_samples=1 << 16) as e:
        e.set_option(N.OPT_HOT_WINDOWS, 0)
        e.submit_pairs_device(d_ids, d_v)
        e.sync()
        c = e.counters()
        print("clustered finish:", {k: c[k] for k in ("samples_partitioned_v3", "region_overflows", "regions_disabled")})
        assert c["samples_partitioned_v3"] >= n - 8192, sorted(c.items())
        with e.flip() as snap:
            check(snap, ids, v, M16, snap.extract(PCTS, M16))
        c = e.counters()                                         # (the launch's self-metrics arrive with the flip)
        print("clustered finish:", {k: c[k] for k in ("samples_partitioned_v3", "region_overflows", "regions_disabled")})
        # (the marker cell cannot be stored in the table: one global add per sample, so the few workgroups whose tiles are
        # mostly that cell may report their two tiles as overflow too)
        workgroups = (n // 8192 + 3) // 4
        marker_tiles = np.count_nonzero(_marker(ids, v)) // 8192 + 2
        assert 8192 < c["region_overflows"] <= (workgroups + marker_tiles) * 2 * 8192, sorted(c.items())


# ---- ... through ov_add with a global name (third generation) ---------------------------------------------------------------

@gpu
def test_overflow_tables_of_the_third_generation_with_the_last_name_frequent(native_lib, torch_cuda):
    """ov_add is keyed by the GLOBAL name in the third generation's two scatter levels: level 1 (k_scatter4: samples that miss
    their hot window and find the miss queue full, and the queue itself; flushed in the tile loop and at the kernel's end) and
    level 2 (k_split_records and k_split_waves: records of names counted in place that miss their window).  The reduce pass and
    the first generation key it by a name local to the partition (< 256), the second generation and the small kernel hold fewer
    than 65 535 names: they cannot form the marker.  Here name 65 535 is the most frequent name, its values span far more than a
    1 024-bin window (log_w pinned to 10) and a tenth of them sit at key +32767, so its samples leave their windows at both
    levels.  From outside one cannot prove that a marker sample itself went through ov_add -- a miss queue with room, or a free
    region, takes it elsewhere -- only that the launch used the overflow paths and that every cell is exact."""
    import loghisto_amd
    n = 1_500_000
    with loghisto_amd.Engine(max_metrics=M16, num_buffers=2, num_lanes=1, lane_samples=1 << 16) as e:
        e.set_option(N.OPT_PART_V3_MIN_PAIRS, 1 << 17)
        e.set_option(N.OPT_PART_V3_DIRECT_MAX_PAIRS, 1)    # launches this small keep the windowed reduce pass under test
        e.set_option(N.OPT_PART_V3_LOG_W, 10)
        for kind, skew in (("huge", 1.5), ("loguniform", 1.0)):
            rng = np.random.default_rng(len(kind))
            ids = (M16 - 1 - _ids(rng, M16, n, skew, permute=False)).astype(np.uint32)   # id = 65 535 - rank
            v = _values(rng, kind, ids, n)
            last = np.nonzero(ids == M16 - 1)[0]
            assert last.size > n // 20
            v[last[::10]] = BIG
            v[last[5::50]] = -BIG
            v[np.nonzero(ids == M16 - 2)[0][::7]] = BIG
            d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
            for rep in range(2):                 # rep 1 runs on rep 0's survey
                c0 = e.counters()
                e.submit_pairs_device(d_ids, d_v)
                e.sync()
                with e.flip() as snap:
                    check(snap, ids, v, M16, snap.extract(PCTS, M16))
                c = e.counters()                 # after the flip: this launch's self-metrics have all arrived, the next has not run
                assert c["samples_partitioned_v3"] - c0["samples_partitioned_v3"] == n, sorted(c.items())
                off = {k: c[k] - c0[k] for k in ("region_overflows", "level2_overflows", "reduce_window_misses")}
                print("overflow paths:", kind, rep, off)
                assert sum(off.values()) > 0, sorted(c.items())


# ---- 2. names past 65 536 ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def big_stream(n):
    """MBIG names: two fifths of the pairs on names 65 536 .. 66 047 with the constants 1000 + id % 5, two fifths on names
    0 .. 511 with lognormal values around 1e5 (bins 460 away), the rest Zipf over all names.  A sample of name 65 536 + i counted
    in row i lands in a cell that row does not otherwise have."""
    rng = np.random.default_rng(66048)
    m = min(n, BASE)
    ids = _ids(rng, MBIG, m, 1.0)
    which = rng.random(m)
    ids[which < 0.4] = (M16 + rng.integers(0, 512, m))[which < 0.4]
    ids[which > 0.6] = rng.integers(0, 512, m)[which > 0.6]
    ids[m // 2] = MBIG - 1
    ids = ids.astype(np.uint32)
    v = np.where(ids >= M16, 1000.0 + (ids % 5), _values(rng, "lognormal", ids, m))
    return np.resize(ids, n), np.resize(v, n)


@pytest.fixture(scope="module")
def big_engine(native_lib, torch_cuda):
    import loghisto_amd
    with loghisto_amd.Engine(max_metrics=MBIG, num_buffers=2, num_lanes=1, lane_samples=1 << 16) as e:
        yield e


@gpu
@pytest.mark.parametrize("n", [999] + [n for n, _ in TABLE_SIZES])
def test_device_pairs_past_65536_names(big_engine, torch_cuda, n):
    """Device-resident uint32 pairs on the default path of an engine of 66 048 names (lh_dispatch: DIRECT whatever the size), at
    the call sizes of the cell table's three configurations and one below a tile.  The table cannot key these names: the whole
    call takes one global atomic per sample (launch_ingest_pairs_cells)."""
    e = big_engine
    ids, v = big_stream(n)
    d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
    c0 = _fresh(e)
    e.submit_pairs_device(d_ids, d_v)
    e.sync()
    c = e.counters()
    assert c["samples_direct"] - c0["samples_direct"] == n and c["samples_partitioned"] == 0, sorted(c.items())
    with e.flip() as snap:
        check(snap, ids, v, MBIG, snap.extract(PCTS, MBIG))


@gpu
@pytest.mark.parametrize("form", ["submit_pairs", "reserve_commit", "submit", "add_buckets"])
def test_host_fed_forms_past_65536_names(big_engine, torch_cuda, form):
    """lh_submit_pairs, lh_reserve_pairs / lh_commit_pairs (a lane's half-buffer of 5 000 pairs: four whole tiles of the cell
    table and a rest), lh_submit and lh_snapshot_add_buckets with ids >= 65 536."""
    e = big_engine
    ids, v = big_stream(5000)
    _fresh(e)
    if form == "submit_pairs":
        e.submit_pairs(ids, v)
    elif form == "reserve_commit":
        e.submit_pairs_in_place(ids, v)
    elif form == "submit":
        ids = np.full(5000, M16 + 3, np.uint32)
        e.submit(M16 + 3, v)
    else:
        e.submit_pairs_device(_dev(torch_cuda, ids[:999]), _dev(torch_cuda, v[:999]))
    e.sync()
    with e.flip() as snap:
        if form == "add_buckets":
            cells, counts = np.unique((ids.astype(np.uint64) << np.uint64(16)) |
                                      oracle.compress_many(v).astype(np.uint16).astype(np.uint64), return_counts=True)
            snap.add_buckets((cells >> np.uint64(16)).astype(np.uint32), (cells & np.uint64(0xffff)).astype(np.uint16).view(np.int16),
                             counts.astype(np.uint64))
            ids, v = np.concatenate([ids[:999], ids]), np.concatenate([v[:999], v])
        check(snap, ids, v, MBIG, snap.extract(PCTS, MBIG))


@gpu
@pytest.mark.parametrize("where", ["device", "host"])
def test_uint16_ids_on_an_engine_past_65536_names(big_engine, torch_cuda, where):
    """uint16 ids are valid for any engine of at least 65 536 names (lh_submit_pairs16) and reach rows 0 .. 65 535 only: the edge
    stream, marker cell included, lands in exactly those rows of the 66 048."""
    e = big_engine
    n = 70_000
    ids, v = edge_stream(n)
    _fresh(e)
    if where == "device":
        e.submit_pairs_device(_dev(torch_cuda, ids.astype(np.uint16)), _dev(torch_cuda, v))
    else:
        e.submit_pairs(ids.astype(np.uint16), v)
    e.sync()
    with e.flip() as snap:
        got = snap.extract(PCTS, MBIG)
        check(snap, ids, v, MBIG, got)
        assert not got["count"][M16:].any()


@gpu
def test_an_id_equal_to_max_metrics_is_still_reported(big_engine, torch_cuda):
    import loghisto_amd
    e = big_engine
    ids, v = big_stream(70_000)
    bad = ids.copy()
    where = [5, 40_000, 69_999]
    bad[where] = [MBIG, MBIG + 7, MBIG]
    keep = np.ones(ids.size, bool)
    keep[where] = False
    _fresh(e)
    with pytest.raises(loghisto_amd.LhError) as ei:
        e.submit_pairs(bad[:100], v[:100])                 # the host form checks before it copies
    assert ei.value.code == N.ERANGE
    with pytest.raises(loghisto_amd.LhError) as ei:
        e.submit(MBIG, v[:100])
    assert ei.value.code == N.ERANGE
    d_bad, d_v = _dev(torch_cuda, bad), _dev(torch_cuda, v)
    e.submit_pairs_device(d_bad, d_v)
    with pytest.raises(loghisto_amd.LhError) as ei:
        e.sync()
    assert ei.value.code == 6                              # ids out of range were seen (and skipped)
    with e.flip() as snap:
        try:
            got = snap.extract(PCTS, MBIG)
        except loghisto_amd.LhError as err:      # (the sticky id error once more, nothing else)
            if err.code != N.ERANGE:
                raise
            got = snap.extract(PCTS, MBIG)
        check(snap, ids[keep], v[keep], MBIG, got)


@gpu
def test_readers_on_rows_past_65536(big_engine, torch_cuda):
    """One call per reader family on the rows from 65 536 on: extract, buckets_all, count_le and top with first = 65 536."""
    e = big_engine
    n, hi = 70_000, MBIG - M16
    ids, v = big_stream(n)
    _fresh(e)
    e.submit_pairs_device(_dev(torch_cuda, ids), _dev(torch_cuda, v))
    e.sync()
    per_name = np.bincount(ids, minlength=MBIG)
    keys = oracle.compress_many(v)
    with e.flip() as snap:
        full = snap.extract(PCTS, MBIG)
        check(snap, ids, v, MBIG, full)
        part = snap.extract(PCTS, hi, first=M16)
        assert np.array_equal(part["count"].astype(np.int64), per_name[M16:])
        for k in ("sum", "pvals"):
            assert np.array_equal(part[k].view(np.uint64), full[k][M16:].view(np.uint64)), k
        assert np.array_equal(part["pkeys"], full["pkeys"][M16:])
        off, bkeys, bcounts = snap.buckets_all(hi, first=M16)
        want_cells, want_counts = np.unique((ids[ids >= M16].astype(np.int64) - M16) << 16 |
                                            oracle.key_to_bin(keys[ids >= M16]).astype(np.int64), return_counts=True)
        rows = np.repeat(np.arange(hi, dtype=np.int64), np.diff(off.astype(np.int64)))
        assert np.array_equal(rows << 16 | oracle.key_to_bin(bkeys).astype(np.int64), want_cells)
        assert np.array_equal(bcounts.astype(np.int64), want_counts)
        bounds = [1000.0, 1002.0, 1e9]
        le = snap.count_le(bounds, nmetrics=hi, first=M16)
        assert np.array_equal(le["total"].astype(np.int64), per_name[M16:])
        for j, b in enumerate(bounds):
            sel = (ids >= M16) & (keys <= oracle.compress(b))
            assert np.array_equal(le["cum"][:, j].astype(np.int64), np.bincount(ids[sel] - M16, minlength=hi)), b
        top = snap.top(5, by="count", nmetrics=hi, first=M16)
        order = sorted(range(M16, MBIG), key=lambda m: (-int(per_name[m]), m))[:5]
        assert top["id"].tolist() == order and top["count"].tolist() == [int(per_name[m]) for m in order]
