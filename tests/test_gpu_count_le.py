"""lh_count_le / lh_count_le_device (Snapshot.count_le): samples at or below given values, per name -- the running count of
percentile()'s bucket walk (metrics.go:389-418) read at a value, at bucket resolution.

Every comparison is INTEGER-EXACT against oracle/: the rows are oracle.histogram_pairs' (up to 1 024 names; at 20 000
names, where the dense matrix would be 10 GB, the same cells as sorted (name, bin) pairs from oracle.compress_many, which
the 1 024-name case checks against the dense rows), a bound's bin comes from oracle.kext_many / oracle.compress_many, and
the expected count is numpy.cumsum over the bins.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N

pytestmark = pytest.mark.gpu

PCTS = list(oracle.DEFAULT_PERCENTILES.values())
U64 = np.uint64
INF = np.inf


# ---- the oracle side ---------------------------------------------------------------------------------------------------
def take_of(b):
    """How many leading bins a bound takes in (0 .. 65 536): bin(compress(b)) + 1; 0 / 65 536 for -Inf / +Inf and for
    finite bounds whose extended key exceeds 32 767."""
    b = np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    safe = np.where(fin, b, 0.0)
    kext = oracle.kext_many(1.0 + np.abs(safe).ravel()).reshape(b.shape).astype(np.int64)
    sat = ~fin | (kext > 32767)
    key = np.where(safe < 0, -kext, kext)
    ok = ~sat
    assert np.array_equal(oracle.compress_many(safe[ok]).astype(np.int64), key[ok])    # the two oracle routes agree
    return np.where(sat, np.where(b > 0, 65536, 0), oracle.key_to_bin(np.where(sat, 0, key)) + 1).astype(np.int64)


class Ref:
    """Expected counts of a stream (optionally plus extra (name, key, count) cells)."""

    def __init__(self, ids, v, M, extra=None, dense=None):
        self.M = M
        self.dense = (M <= 1024) if dense is None else dense
        if self.dense:
            rows = oracle.histogram_pairs(ids, v, M)
            if extra is not None:
                np.add.at(rows, (extra[0].astype(np.int64), oracle.key_to_bin(extra[1])), extra[2].astype(U64))
            self.rows = rows
            self.P = np.zeros((M, oracle.NKEYS + 1), dtype=U64)
            np.cumsum(rows, axis=1, dtype=U64, out=self.P[:, 1:])
        else:
            assert extra is None
            bins = oracle.key_to_bin(oracle.compress_many(v)).astype(U64)
            self.cells, counts = np.unique((np.asarray(ids).astype(U64) << U64(16)) | bins, return_counts=True)
            self.G = np.concatenate([[0], np.cumsum(counts)]).astype(U64)

    def count(self, bounds, first=0, nmetrics=None):
        """(cum[nmetrics, nb], total[nmetrics])"""
        nmetrics = self.M - first if nmetrics is None else nmetrics
        E = take_of(bounds)
        if E.ndim == 1:
            E = np.broadcast_to(E, (nmetrics, E.size))
        m = np.arange(first, first + nmetrics, dtype=np.int64)
        if self.dense:
            return self.P[m[:, None], E], self.P[m, oracle.NKEYS]
        start = np.searchsorted(self.cells, (m << 16).astype(U64))
        at = np.searchsorted(self.cells, ((m[:, None] << 16) + E).astype(U64))       # cells of rows < m, and of row m below E
        return self.G[at] - self.G[start][:, None], self.G[np.searchsorted(self.cells, ((m + 1) << 16).astype(U64))] - self.G[start]


def stream(seed, M, n):
    """Half lognormal latencies, half +-10^U(-3, 20) (spans of several thousand bins); names 2 and M - 1 stay empty."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, M, n).astype(np.uint32)
    if M > 3:
        ids[(ids == 2) | (ids == M - 1)] = 0
    v = rng.lognormal(3.0, 1.5, n)
    wide = rng.random(n) < 0.5
    v[wide] = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 20, n))[wide]
    return ids, v


def bound_pool(rng, v):
    """Candidates: -Inf, saturating and ordinary negatives, both zeros, decompress(k) of occupied and unoccupied keys,
    nextafter on both sides of oracle thresholds (both signs), below every lo, above every hi, +-1e150, +Inf."""
    keys = np.unique(oracle.compress_many(v))
    occupied = [oracle.decompress(int(k)) for k in rng.choice(keys, 12)]
    free = [oracle.decompress(int(k)) for k in rng.integers(-32767, 32768, 12)]
    tx = oracle.thresholds()
    edges = []
    for j in rng.choice(np.arange(1, 30000), 6):
        b = float(tx[j]) - 1.0                       # 1 + |b| at threshold j (up to the rounding of the subtraction)
        for s in (1.0, -1.0):
            edges += [s * b, s * np.nextafter(b, INF), s * np.nextafter(b, -INF), s * np.nextafter(np.nextafter(b, INF), INF),
                      s * np.nextafter(np.nextafter(b, -INF), -INF)]
    fixed = [-INF, -1e150, -1e25, -3.5, -1e-9, -0.0, 0.0, 1e-9, 0.25, 250.0, 1e25, 1e150, INF,
             float(v.min()), float(v.max()), float(np.nextafter(v.min(), -INF)), float(np.median(v))]
    return np.array(fixed + occupied + free + edges, dtype=np.float64)


def pick(rng, pool, nb, rows=None):
    """nb bounds (or [rows, nb]) drawn WITH replacement -- equal neighbours occur -- and sorted."""
    shape = (nb,) if rows is None else (rows, nb)
    return np.sort(rng.choice(pool, shape), axis=-1)


def engine(M, **kw):
    import loghisto_amd
    kw.setdefault("num_buffers", 2)
    kw.setdefault("num_lanes", 1)
    kw.setdefault("lane_samples", 1 << 16)
    return loghisto_amd.Engine(max_metrics=M, **kw)


def feed(torch, e, how, ids, v):
    if how == "submit":
        for m in np.unique(ids):
            e.submit(int(m), v[ids == m])
        return None
    if how == "submit_pairs":
        e.submit_pairs(ids, v)
        return None
    t = (torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(v).cuda())
    torch.cuda.synchronize()
    e.submit_pairs_device(*t)
    e.sync()
    return t


def device_form(torch, snap, bounds, nmetrics, first=0, want_cum=True, want_total=True):
    nb = np.asarray(bounds).shape[-1]
    cum = torch.full((nmetrics, nb), -1, dtype=torch.int64, device="cuda") if want_cum else None
    total = torch.full((nmetrics,), -1, dtype=torch.int64, device="cuda") if want_total else None
    torch.cuda.synchronize()
    out = snap.count_le(bounds, nmetrics, first, out=(cum, total))
    torch.cuda.ExternalStream(snap.stream()).synchronize()
    assert out["cum"] is cum and out["total"] is total
    return (cum.cpu().numpy().view(U64) if want_cum else None), (total.cpu().numpy().view(U64) if want_total else None)


def check_both_forms(torch, snap, ref, bounds, first=0, nmetrics=None):
    nmetrics = ref.M - first if nmetrics is None else nmetrics
    want_cum, want_total = ref.count(bounds, first, nmetrics)
    host = snap.count_le(bounds, nmetrics, first)
    assert host["cum"].dtype == U64 and host["cum"].shape == want_cum.shape and host["total"].shape == (nmetrics,)
    bad = np.argwhere(host["cum"] != want_cum)
    assert bad.size == 0, (f"{len(bad)} counts differ, e.g. metric {first + bad[0][0]} bound {np.asarray(bounds)[..., bad[0][1]]}: "
                           f"{host['cum'][tuple(bad[0])]} != {want_cum[tuple(bad[0])]}")
    assert np.array_equal(host["total"], want_total)
    dcum, dtotal = device_form(torch, snap, bounds, nmetrics, first)
    assert np.array_equal(dcum, host["cum"]) and np.array_equal(dtotal, host["total"])          # host form == device form
    assert np.all(np.diff(host["cum"].astype(np.int64), axis=1) >= 0)                           # non-decreasing in j
    assert np.all(host["cum"][:, -1] <= host["total"])
    return host


# ---- 1. every engine size, every way in, every kind of bound ----------------------------------------------------------
@pytest.mark.parametrize("M,n,how", [(1, 200_000, "submit"), (20, 300_000, "submit_pairs"), (1024, 400_000, "submit_pairs_device"),
                                     (20000, 1_500_000, "submit_pairs"), (20, 300_000, "submit"), (20000, 1_500_000, "submit_pairs_device")])
def test_counts_equal_the_oracles_prefix_sums(native_lib, torch_cuda, M, n, how):
    ids, v = stream(1000 + M + len(how), M, n)
    ref = Ref(ids, v, M)
    if M == 1024:                                                         # the sparse reference of the 20 000-name cases
        sparse = Ref(ids, v, M, dense=False)
        b = pick(np.random.default_rng(5), bound_pool(np.random.default_rng(6), v), 64)
        for first, k in ((0, M), (100, 37)):
            assert all(np.array_equal(x, y) for x, y in zip(ref.count(b, first, k), sparse.count(b, first, k)))
    rng = np.random.default_rng(M)
    pool = bound_pool(rng, v)
    with engine(M) as e:
        keep = feed(torch_cuda, e, how, ids, v)
        with e.flip() as snap:
            count = snap.extract([0.5], M)["count"]
            for nb in (1, 9, 64):
                got = check_both_forms(torch_cuda, snap, ref, pick(rng, pool, nb))
                assert np.array_equal(got["total"], count)                               # total == lh_stats.count
            check_both_forms(torch_cuda, snap, ref, pool[np.argsort(pool, kind="stable")][:64])
            check_both_forms(torch_cuda, snap, ref, np.sort(pool)[-64:])
            check_both_forms(torch_cuda, snap, ref, np.array([-INF, -0.0, 0.0, 0.0, INF]))
            for nb in (2, 9):                                                            # a row of bounds per metric
                check_both_forms(torch_cuda, snap, ref, pick(rng, pool, nb, M))
            if M > 3:                                                                    # sub-ranges
                f, k = M // 3, M - M // 3 - 1
                check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 9), f, k)
                check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 5, k), f, k)
                check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 3), M - 1, 1)    # the last row alone: empty
                got = snap.count_le([-INF, 0.0, INF], 3, 1)
                assert not got["cum"][1].any() and got["total"][1] == 0                  # name 2 received nothing
            # either output alone
            b = pick(rng, pool, 9)
            want = ref.count(b)
            c, t = device_form(torch_cuda, snap, b, M, want_total=False)
            assert t is None and np.array_equal(c, want[0])
            c, t = device_form(torch_cuda, snap, b, M, want_cum=False)
            assert c is None and np.array_equal(t, want[1])
        del keep


# ---- 2. both kernel shapes on the same rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(20, 300_000), (1024, 400_000), (3000, 600_000)])
def test_wave_per_row_and_workgroup_per_row_agree_with_the_oracle(native_lib, torch_cuda, M, n):
    """The switch between the shapes depends on the number of rows only; lh_tool_count_le_switch puts every engine size
    through both (spans of thousands of bins through the wave's step loop, thousands of rows through the workgroups)."""
    ids, v = stream(77 + M, M, n)
    ref = Ref(ids, v, M, dense=M <= 1024)
    rng = np.random.default_rng(M + 1)
    pool = bound_pool(rng, v)
    prev = C.c_uint32(0)
    with engine(M, cell_bits=32 if M == 1024 else None) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            try:
                for wave_from in (1, 1 << 30):
                    assert N.lib().lh_tool_count_le_switch(wave_from, C.byref(prev)) == 0
                    for nb in (1, 64):
                        check_both_forms(torch_cuda, snap, ref, pick(rng, pool, nb))
                    check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 7, M))
                    check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 17, M - 5), 3, M - 5)
            finally:
                assert N.lib().lh_tool_count_le_switch(0, C.byref(prev)) == 0
                assert N.lib().lh_tool_count_le_switch(0, C.byref(prev)) == 0 and prev.value == 1024


# ---- 3. the tie to the percentiles -------------------------------------------------------------------------------------
def test_counts_at_the_percentile_keys_reach_the_percentiles(native_lib, torch_cuda):
    """percentile() returns the first bucket whose running count reaches p (float64(sofar) / float64(total) >= p,
    metrics.go:413): the count at decompress(pkey) reaches it and the count at the previous occupied key does not."""
    M, n = 20, 300_000
    ids, v = stream(31, M, n)
    with engine(M) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            got = snap.extract(PCTS, M)
            off, keys, _ = snap.buckets_all(M)
            at = np.full((M, len(PCTS)), 0.0)
            before = np.full((M, len(PCTS)), -INF)
            has_prev = np.zeros((M, len(PCTS)), dtype=bool)
            for m in range(M):
                ks = keys[int(off[m]):int(off[m + 1])]
                for i in range(len(PCTS)):
                    if got["pvalid"][m, i]:
                        k = int(got["pkeys"][m, i])
                        at[m, i] = oracle.decompress(k)
                        j = int(np.searchsorted(ks, k))
                        assert ks[j] == k
                        if j:
                            before[m, i], has_prev[m, i] = oracle.decompress(int(ks[j - 1])), True
            a, b = snap.count_le(at), snap.count_le(before)
    assert np.array_equal(a["total"], got["count"]) and int(got["pvalid"].sum()) == (M - 2) * len(PCTS)
    checked = 0
    for m in range(M):
        tot = float(a["total"][m])
        for i, p in enumerate(PCTS):
            if got["pvalid"][m, i]:
                assert float(a["cum"][m, i]) / tot >= p, (m, i)
                if has_prev[m, i]:
                    assert not float(b["cum"][m, i]) / tot >= p, (m, i)
                    assert b["cum"][m, i] < a["cum"][m, i]
                    checked += 1
                else:
                    assert b["cum"][m, i] == 0
    assert checked > M * 5


# ---- 4. read-only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(40, 300_000), (20000, 1_000_000)])
def test_the_snapshot_is_untouched(native_lib, torch_cuda, M, n):
    from loghisto_amd import merge
    torch = torch_cuda
    ids, v = stream(41 + M, M, n)
    rng = np.random.default_rng(42)
    pool = bound_pool(rng, v)

    def state(snap):
        torch.cuda.ExternalStream(snap.stream()).synchronize()
        ex = snap.extract(PCTS, M)
        return ([ex[k].copy() for k in sorted(ex)], [x.copy() for x in snap.buckets_all(M)],
                merge.snapshot_ranges(snap, M).cpu().numpy().copy(), snap.device_cells())

    with engine(M, cell_bits=32 if M > 8192 else None) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            cells0 = snap.device_cells()
            assert M <= 8192 or cells0[2] == 4
            widenings = e.counters()["widenings"]
            s0 = state(snap)
            snap.count_le(pick(rng, pool, 64))
            snap.count_le(pick(rng, pool, 3, M))
            device_form(torch, snap, pick(rng, pool, 9), M - 1, 1)
            s1 = state(snap)
            assert snap.device_cells() == cells0 and s1[3] == s0[3]                      # same store, same cell width
            assert e.counters()["widenings"] == widenings                                # a narrow snapshot stays narrow
    for x, y in zip(s0[0] + s0[1], s1[0] + s1[1]):
        assert np.array_equal(x.view(np.uint8) if x.dtype.kind == "f" else x, y.view(np.uint8) if y.dtype.kind == "f" else y)
    assert np.array_equal(s0[2], s1[2])


# ---- 5. a snapshot that widened ----------------------------------------------------------------------------------------
def test_exact_after_an_import_widened_the_snapshot(native_lib, torch_cuda):
    M, n = 64, 300_000
    ids, v = stream(51, M, n)
    rng = np.random.default_rng(52)
    pool = bound_pool(rng, v)
    k5 = int(np.sort(oracle.compress_many(v[ids == 5]))[n // M // 2])                    # an occupied cell of name 5
    big = (np.array([5], dtype=np.uint32), np.array([k5], dtype=np.int16), np.array([1 << 33], dtype=U64))
    with engine(M, cell_bits=32) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            assert snap.device_cells()[2] == 4
            check_both_forms(torch_cuda, snap, Ref(ids, v, M), pick(rng, pool, 64))
            snap.add_buckets(*big)
            assert snap.device_cells()[2] == 8
            ref = Ref(ids, v, M, extra=big)
            got = check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 64))
            assert int(got["total"][5]) == int(np.sum(ids == 5)) + (1 << 33)
            at = snap.count_le([oracle.decompress(k5 - 1), oracle.decompress(k5)], 1, 5)     # the cell itself
            assert int(at["cum"][0, 1]) - int(at["cum"][0, 0]) == int(ref.rows[5, int(oracle.key_to_bin(k5))]) > 1 << 33
            check_both_forms(torch_cuda, snap, ref, pick(rng, pool, 4, M))


# ---- 6. one row over the whole key range ------------------------------------------------------------------------------
def test_a_row_filled_over_the_full_key_range(native_lib, torch_cuda):
    """All 65 536 cells of the one name occupied (imported: a sample stream cannot reach every key; 64-bit cells, counts
    beyond 2^32): 256 chunks through the workgroup-per-row kernel, then 256 steps through the wave's loop."""
    rng = np.random.default_rng(60)
    keys = np.arange(-32768, 32768, dtype=np.int16)
    counts = rng.integers(1, 1 << 40, keys.size).astype(U64)
    counts[rng.random(keys.size) < 0.3] = 1
    none = (np.zeros(0, dtype=np.uint32), np.zeros(0))
    ref = Ref(*none, 1, extra=(np.zeros(keys.size, dtype=np.uint32), keys, counts))
    d = oracle.decompress_table()
    pool = np.concatenate([d[rng.integers(1, 65536, 80)], [-INF, -1e150, -0.0, 0.0, 1e150, INF, d[1], d[65535], d[32768], d[255], d[256], d[257]]])
    prev = C.c_uint32(0)
    with engine(1) as e:
        with e.flip() as snap:
            snap.add_buckets(np.zeros(keys.size, dtype=np.uint32), keys, counts)
            try:
                for wave_from in (0, 1):
                    assert N.lib().lh_tool_count_le_switch(wave_from, C.byref(prev)) == 0
                    for nb in (1, 9, 64):
                        got = check_both_forms(torch_cuda, snap, ref, pick(rng, pool, nb))
                    assert int(got["total"][0]) == int(counts.sum(dtype=U64))
                    full = check_both_forms(torch_cuda, snap, ref, np.sort(d[np.arange(1, 65536, 1024)]))
                    assert np.all(np.diff(full["cum"][0].astype(np.int64)) > 0)
            finally:
                assert N.lib().lh_tool_count_le_switch(0, C.byref(prev)) == 0


# ---- 7. the checks that need the snapshot ------------------------------------------------------------------------------
def test_range_errors_and_the_empty_call(native_lib, torch_cuda):
    import loghisto_amd
    M = 8
    with engine(M) as e:
        e.submit(1, np.array([1.0, 2.0, 300.0]))
        with e.flip() as snap:
            for first, k in ((0, M + 1), (M, 1), (M + 1, 0), (7, 2)):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    snap.count_le([1.0], k, first)
                assert ei.value.code == N.ERANGE, (first, k)
            cum = np.full(4, 7, dtype=U64)
            b = np.array([1.0])
            for first, k in ((1, (1 << 32) - 1), (M, (1 << 32) - M), (0xffffffff, 1), (1, (1 << 64) - 1)):   # sums that wrap
                assert N.lib().lh_count_le(snap._h, first, k, b.ctypes.data, 1, 0, cum.ctypes.data, cum.ctypes.data) == N.ERANGE
            for first in (0, M):                                         # nmetrics == 0: LH_OK, nothing written
                assert N.lib().lh_count_le(snap._h, first, 0, b.ctypes.data, 1, 0, cum.ctypes.data, cum.ctypes.data) == 0
            assert np.all(cum == 7)
            with pytest.raises(loghisto_amd.LhError) as ei:
                snap.count_le([2.0, 1.0], M)
            assert ei.value.code == N.EINVAL
            got = snap.count_le([0.5, 1.0, 2.0, 299.0, 301.0], M)
            assert got["cum"][1].tolist() == [0, 1, 2, 2, 3] and got["total"].tolist() == [0, 3, 0, 0, 0, 0, 0, 0]
            # plain (pageable) numpy arrays take the library's pinned block
            cum, total = np.zeros((M, 2), dtype=U64), np.zeros(M, dtype=U64)
            b = np.array([1.5, INF])
            assert N.lib().lh_count_le(snap._h, 0, M, b.ctypes.data, 2, 0, cum.ctypes.data, total.ctypes.data) == 0
            assert cum[1].tolist() == [1, 3] and total[1] == 3 and int(cum.sum()) == 4


# ---- 8. snapshots of two engines on one device ------------------------------------------------------------------------
def test_per_metric_bounds_of_one_engine_survive_calls_on_another(native_lib, torch_cuda):
    """The unit's bounds blocks are one set per device while every engine has a stream of its own: a device-form call with
    per-metric bounds on engine A, then a host-form call with shared bounds on engine B (which waits for B's stream only),
    then per-metric calls on B that rewrite the blocks.  A's counts are those of A's bounds."""
    torch = torch_cuda
    M, n = 20000, 1_000_000
    ia, va = stream(81, M, n)
    ib, vb = stream(82, M, n)
    ra, rb = Ref(ia, va, M), Ref(ib, vb, M)
    rng = np.random.default_rng(83)
    pool = bound_pool(rng, va)
    with engine(M) as a, engine(M) as b:
        a.submit_pairs(ia, va)
        b.submit_pairs(ib, vb)
        with a.flip() as sa, b.flip() as sb:
            for _ in range(4):
                ba, bb = pick(rng, pool, 9, M), pick(rng, pool, 9, M)
                cum = torch.full((M, 9), -1, dtype=torch.int64, device="cuda")
                total = torch.full((M,), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                sa.count_le(ba, M, out=(cum, total))                                     # enqueued on A's stream
                got_b = sb.count_le(pick(rng, pool, 3), M)                               # shared bounds, B's stream
                got_bb = sb.count_le(bb, M)                                              # rewrites the blocks
                torch.cuda.ExternalStream(sa.stream()).synchronize()
                want = ra.count(ba)
                assert np.array_equal(cum.cpu().numpy().view(U64), want[0]) and np.array_equal(total.cpu().numpy().view(U64), want[1])
                assert np.array_equal(got_bb["cum"], rb.count(bb)[0]) and np.array_equal(got_b["total"], rb.count(bb)[1])


# ---- 9. the host form's two ways back ----------------------------------------------------------------------------------
def small_stream():
    """5 names, 301 samples: name 2 stays empty, name 3 receives a single sample."""
    rng = np.random.default_rng(91)
    ids = np.append(rng.choice(np.array([0, 1, 4], dtype=np.uint32), 300), np.uint32(3))
    v = np.append(rng.lognormal(3.0, 1.5, 300), 42.0)
    return ids, v


def host_arrays(torch, pinned, shape, dtype):
    """An output array filled with a pattern no result has: pinned (the copy engine writes it) or plain pageable numpy."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True).numpy() if pinned else np.empty(nbytes, dtype=np.uint8)
    raw[:] = 0x77
    return raw.view(dtype).reshape(shape)


@pytest.mark.parametrize("per_metric", [False, True])
def test_pinned_and_pageable_outputs_receive_the_same_counts(native_lib, torch_cuda, per_metric):
    """lh_count_le through ctypes, cum and total both asked for: into pinned arrays (one copy per array, straight in) and
    into pageable ones (through the unit's pinned block) -- the same bits, and the oracle's."""
    M = 5
    ids, v = small_stream()
    ref = Ref(ids, v, M)
    assert ref.rows[2].sum() == 0 and ref.rows[3].sum() == 1
    b = np.array([-INF, 1.0, 42.0, 100.0, INF])
    if per_metric:
        b = np.sort(np.random.default_rng(92).choice(bound_pool(np.random.default_rng(93), v), (M, 5)), axis=1)
    want_cum, want_total = ref.count(b)
    got = []
    with engine(M) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            for pinned in (True, False, True):
                cum, total = host_arrays(torch_cuda, pinned, (M, 5), U64), host_arrays(torch_cuda, pinned, (M,), U64)
                flags = N.LE_PER_METRIC if per_metric else 0
                assert N.lib().lh_count_le(snap._h, 0, M, b.ctypes.data, 5, flags, cum.ctypes.data, total.ctypes.data) == 0
                got.append((cum.copy(), total.copy()))
    for cum, total in got:
        assert np.array_equal(cum, want_cum) and np.array_equal(total, want_total)
        assert cum.tobytes() == got[0][0].tobytes() and total.tobytes() == got[0][1].tobytes()
