"""lh_keep / lh_kept_across* (Snapshot.keep, Kept): an interval's occupied cells kept in compact form on the device after
its snapshot is gone, and lh_across' outputs over a list of up to 64 such handles.

The model is the one of tests/test_gpu_across.py -- Python integers over Snapshot.buckets_all of each interval (recorded
before the snapshot was released): count, nbuckets, present_bits, keys and valid exact, |sum - exact| <= 1e-12 x sum of
|D[b] C[b]| with exact a fractions.Fraction (the project's _sum parity).  Every reader case runs under both kernel shapes
(lh_tool_kept_switch), on engines of 64- and of 32-bit cells; the tile's width comes from lh_tool_kept_tile.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_across import P_MAIN, check, model
from tests.test_gpu_compare import _import, _write_narrow, rows_of
from tests.test_gpu_count_le import engine

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
U32MAX = (1 << 32) - 1
SHAPES = {"wave": 1, "block": 1 << 30}
FIELDS = dict(count=U64, sum=np.float64, nbuckets=np.uint32, present_bits=U64, pkeys=np.int16, pvalid=np.uint8)
PER_P = ("pkeys", "pvalid")
K = 6            # handles of the crafted fixture
BIG = 3          # the one whose snapshot takes the cells of 2^32 and more (an import: it widens a narrow snapshot)


@contextlib.contextmanager
def shape(name):
    """Put every call through one kernel shape, whatever the number of rows; the previous value comes back afterwards."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    assert N.lib().lh_tool_kept_switch(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_kept_switch(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


def tile():
    t = C.c_uint32(0)
    assert N.lib().lh_tool_kept_tile(C.byref(t)) == 0 and 256 <= t.value <= 8192
    return int(t.value)


def check64(got, want, P, what=""):
    """test_gpu_across.check, whose present_bits are 32 bits wide, on the low half; then all 64 bits."""
    assert got["present_bits"].dtype == U64 and got["present_bits"].shape == (len(want),)
    low = dict(got, present_bits=(got["present_bits"] & U64(U32MAX)).astype(np.uint32))
    check(low, [dict(w, present=w["present"] & U32MAX) for w in want], P, what)
    for m, w in enumerate(want):
        if not w["wrapped"]:
            assert int(got["present_bits"][m]) == w["present"], (what, m, hex(int(got["present_bits"][m])), hex(w["present"]))


def host(t):
    """a torch device tensor of 8-, 2-byte integers as the numpy array of what it holds"""
    a = t.cpu().numpy()
    return a.view(U64) if a.dtype == np.int64 else a


def arrays_of(k):
    return [host(t) for t in k.arrays()]


def same_listing(k, rec, what=""):
    """Kept.arrays() == what buckets_all returned for the same rows, and row_count / info to match."""
    off, keys, counts, row_count = arrays_of(k)
    assert off.dtype == U64 and keys.dtype == np.int16 and counts.dtype == U64 and row_count.dtype == U64
    assert np.array_equal(off, rec[0]) and np.array_equal(keys, rec[1]) and np.array_equal(counts, rec[2]), what
    nrows = len(rec[0]) - 1
    sums = [sum(int(c) for c in rec[2][int(rec[0][m]):int(rec[0][m + 1])]) for m in range(nrows)]
    assert [int(x) for x in row_count] == [s % (1 << 64) for s in sums], what
    assert k.info["nrows"] == nrows and k.info["cells"] == len(rec[1]) and k.info["samples"] == sum(sums) % (1 << 64), what
    assert k.info["bytes"] == 8 * (nrows + 1) + 2 * len(rec[1]) + 8 * len(rec[2]) + 8 * nrows, what


# ---- crafted names: per name {handle index: cells or (cells, span)}; a handle not named never marks the row ----------------
def crafted_names(T):
    names = []

    def add(kind, per):
        names.append((kind, {i: (v if isinstance(v, tuple) else (v, "tight")) for i, v in per.items()}))

    add("plain", {0: {100: 3, 200: 5}, 1: {150: 2}, 2: {100: 1, 300: 7}, 5: {90: 1}})
    add("never", {})
    add("marked_zero", {0: ({}, (700, 1200)), 1: ({}, (30000, 30001))})
    add("only_in_4", {4: {777: 5, 901: 1}})
    # a cell either side of every edge of the first tiles, each in another handle: total 21, prefix 1 3 6 10 15 21
    add("edges", {0: {0: 1}, 1: {T - 1: 2}, 2: {T: 3}, 3: {2 * T - 1: 4}, 4: {2 * T: 5}, 5: {NK - 1: 6}})
    add("edges_in_one", {2: {0: 1, T - 1: 2, T: 3, 2 * T - 1: 4, 2 * T: 5, NK - 1: 6}})
    add("bins_0_65535", {0: {0: 5}, 1: {0: 1, NK - 1: 1}, 4: {NK - 1: 7}})
    add("one_bin", {0: {5000: 2}, 2: {5000: 3}, 5: {5000: 1}})
    add("one_bin_65535", {1: {NK - 1: 3}})
    add("dense300", {1: {b: 1 + b % 3 for b in range(20002, 20302)}, 4: {b: 2 for b in range(20100, 20200)}})
    add("dense_over_an_edge", {0: {b: 1 for b in range(30000 + T - 150, 30000 + T + 150)}, 5: {30000: 2}})
    add("loose", {0: ({40001: 2, 40100: 1}, (39000, 42000)), 1: ({40050: 3}, (0, NK - 1)), 2: ({40002: 1}, (40001, 40003))})
    add("eight_tiles", {i: {b: 1 + i for b in range(1000 + 97 * i, 1000 + 8 * T, 97 * K)} for i in range(K)})
    add("far_apart", {0: {10001: 1}, 1: {40001: 1}})
    # the same cell at 2^32 - 1 in two handles: 0x1fffffffe, and p = 0.5 picks bin 500 only because of it
    add("two_cells_of_2^32-1", {0: {500: U32MAX}, 1: {500: U32MAX}, 2: {600: U32MAX}})
    add("cell_of_2^33", {BIG: {700: 1 << 33, 650: 5}, 0: {640: 9}})
    add("total_2^64-1", {BIG: {100: (1 << 63) - 1, 200: 1 << 63}})
    add("half_of_2^64", {BIG: {100: 1 << 63, 300: 7}})                           # listed twice: the total wraps to 14
    rng = np.random.default_rng(5)
    while len(names) < 70:                                                       # more rows than one workgroup has waves
        per = {}
        for i in rng.choice(K, rng.integers(1, K + 1), replace=False):
            bins = np.unique(rng.normal(33000, 60, rng.integers(1, 400)).astype(np.int64))
            per[int(i)] = {int(b): int(c) for b, c in zip(bins, rng.integers(1, 1000, bins.size))}
        add(f"random{len(names)}", per)
    return names


LISTS = [[0], [BIG], [0, 0], [0, 1], [1, 0], [0, 1, 2], [BIG, BIG], list(range(K)), list(range(K - 1, -1, -1)),
         (list(range(K)) * 11)[:64]]
_WANT = {}


@pytest.fixture(scope="module", params=["wide64", "narrow32"])
def crafted(request, native_lib, torch_cuda):
    """K handles taken from K successive snapshots of ONE two-buffer engine, each snapshot released right after the keep;
    on the engine of 32-bit cells the rows are written into the narrow store, and the cells of 2^32 and more of handle BIG are
    then imported (which widens that one snapshot)."""
    wide = request.param == "wide64"
    T = tile()
    names = crafted_names(T)
    M = len(names)
    at = {k: m for m, (k, _) in enumerate(names)}
    rows = [[dict(per.get(i, ({}, None))[0]) for _, per in names] for i in range(K)]
    spans = [[per.get(i, ({}, None))[1] for _, per in names] for i in range(K)]
    spans = [[None if (s == "tight" and not r) else s for r, s in zip(rs, ss)] for rs, ss in zip(rows, spans)]
    assert all(c <= U32MAX for i in range(K) if i != BIG for r in rows[i] for c in r.values())
    kept, recs, extra = [], [], {}
    with engine(M, cell_bits=64 if wide else 32, num_buffers=2) as e:
        for i in range(K):
            with e.flip() as s:
                if wide:
                    _import(s, rows[i], spans[i])
                else:
                    small = [{b: c for b, c in r.items() if c <= U32MAX} for r in rows[i]]
                    _write_narrow(torch_cuda, s, small, [None if (sp == "tight" and not r) else sp for r, sp in zip(small, spans[i])])
                    big = [(m, b, c) for m, r in enumerate(rows[i]) for b, c in r.items() if c > U32MAX]
                    if big:
                        s.add_buckets(np.array([m for m, _, _ in big], dtype=np.uint32),
                                      oracle.bin_to_key(np.array([b for _, b, _ in big])).astype(np.int16),
                                      np.array([c for _, _, c in big], dtype=U64))
                assert s.device_cells()[2] == (8 if wide or i == BIG else 4)
                assert rows_of(s, M) == rows[i]
                recs.append([x.copy() for x in s.buckets_all(M)])
                kept.append(s.keep(M))
                if i == 0:                                                      # sub-blocks, and one without a cell
                    extra["sub"] = (s.keep(5, 3), [x.copy() for x in s.buckets_all(5, 3)])
                    extra["last"] = (s.keep(1, M - 1), [x.copy() for x in s.buckets_all(1, M - 1)])
                    extra["empty"] = (s.keep(2, at["never"]), [x.copy() for x in s.buckets_all(2, at["never"])])
                assert s.device_cells()[2] == (8 if wide or i == BIG else 4)    # a narrow snapshot stays narrow
        e.flip().release()                                                      # (both buffers have been cleared since)
        e.flip().release()

        def want(lst, P=P_MAIN, first=0, n=M):
            key = (request.param, tuple(lst), tuple(repr(p) for p in P))
            if key not in _WANT:
                _WANT[key] = [model([rows[i][m] for i in lst], P) for m in range(M)]
            return _WANT[key][first:first + n]

        yield types.SimpleNamespace(e=e, kept=kept, recs=recs, extra=extra, rows=rows, names=names, at=at, M=M, T=T, wide=wide,
                                    want=want, torch=torch_cuda)
    # the engine is gone; every handle still holds, byte for byte, what it was made from -- after every reader case
    for k, rec in zip(kept, recs):
        same_listing(k, rec, "at teardown")
    for k, _ in extra.values():
        k.close()
    for k in kept:
        k.close()
        k.close()                                                               # (closing twice is harmless)


def call(c, lst, P=P_MAIN, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].across([c.kept[i] for i in lst[:-1]], P, c.M - first if nmetrics is None else nmetrics, first, **kw)


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------
def test_a_handle_lists_what_buckets_all_listed(crafted):
    c = crafted
    for i, (k, rec) in enumerate(zip(c.kept, c.recs)):
        same_listing(k, rec, i)
        assert k.info["first"] == 0 and k.info["device"] == 0
        assert rows_of(types.SimpleNamespace(buckets_all=lambda M, first, a=arrays_of(k): a[:3]), c.M) == c.rows[i]
    sub, rec = c.extra["sub"]
    same_listing(sub, rec, "first = 3")
    assert sub.info["first"] == 3 and sub.info["nrows"] == 5
    last, rec = c.extra["last"]
    same_listing(last, rec, "the last row")
    empty, rec = c.extra["empty"]
    same_listing(empty, rec, "no cell")
    assert empty.info["cells"] == 0 and empty.info["samples"] == 0 and empty.info["bytes"] == 8 * 3 + 8 * 2
    assert [int(x) for x in arrays_of(empty)[0]] == [0, 0, 0]
    # what the crafted rows were made for
    off, keys, counts, row_count = arrays_of(c.kept[2])
    m = c.at["edges_in_one"]
    bins = (keys[int(off[m]):int(off[m + 1])].astype(np.int64) & 0xffff) ^ 0x8000
    assert list(bins) == [0, c.T - 1, c.T, 2 * c.T - 1, 2 * c.T, NK - 1] and int(row_count[m]) == 21
    off, keys, counts, row_count = arrays_of(c.kept[1])
    m = c.at["dense300"]
    assert int(off[m + 1]) - int(off[m]) == 300
    off, keys, counts, row_count = arrays_of(c.kept[BIG])
    m = c.at["cell_of_2^33"]
    assert [int(x) for x in counts[int(off[m]):int(off[m + 1])]] == [5, 1 << 33]
    assert int(row_count[c.at["total_2^64-1"]]) == (1 << 64) - 1
    assert int(off[c.at["never"] + 1]) == int(off[c.at["never"]])


@pytest.mark.parametrize("bits", (64, 32))
def test_keep_leaves_the_snapshot_untouched_and_add_to_restores_it(native_lib, torch_cuda, bits):
    from loghisto_amd import merge
    M, n = 40, 100_000
    rng = np.random.default_rng(11)
    ids = rng.integers(0, M - 2, n).astype(np.uint32)                            # the last two names stay empty
    v = rng.lognormal(3.0, 1.0, n)
    v[rng.random(n) < 0.02] *= -1.0

    def state(snap):
        torch_cuda.cuda.ExternalStream(snap.stream()).synchronize()
        return ([x.copy() for x in snap.buckets_all(M)], merge.snapshot_ranges(snap, M).cpu().numpy().copy(), snap.device_cells())

    with engine(M, cell_bits=bits) as e, engine(M, cell_bits=bits) as e2:
        e.submit_pairs(ids, v)
        with e.flip() as snap, e2.flip() as spare:
            widenings = e.counters()["widenings"]
            s0 = state(snap)
            assert s0[2][2] == bits // 8
            with snap.keep(M) as k, snap.keep(7, 30) as part:
                s1 = state(snap)
                assert all(np.array_equal(x, y) for x, y in zip(s0[0], s1[0])) and np.array_equal(s0[1], s1[1])
                assert s1[2] == s0[2] and e.counters()["widenings"] == widenings
                assert k.info["nrows"] == M and k.info["samples"] == n and part.info["first"] == 30
                same_listing(k, [x.copy() for x in snap.buckets_all(M)])
                same_listing(part, [x.copy() for x in snap.buckets_all(7, 30)])
                k.add_to(spare)                                                  # the device CSR import, with the handle's arrays
                part.add_to(spare)                                               # rows 30 .. 36 once more
                torch_cuda.cuda.ExternalStream(spare.stream()).synchronize()
            a, b = rows_of(snap, M), rows_of(spare, M)
            for m in range(M):
                twice = 2 if 30 <= m < 37 else 1
                assert b[m] == {j: twice * x for j, x in a[m].items()}, m
        import loghisto_amd
        with e.flip() as snap:
            for first, n_ in ((0, M + 1), (M, 1), (5, M - 4)):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    snap.keep(n_, first)
                assert ei.value.code == N.ERANGE, (first, n_)


# ---- 2. a handle outlives its source -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_64_handles_outlive_their_snapshots_and_the_engine(native_lib, torch_cuda, bits):
    M, n, k = 40, 3000, 64
    rng = np.random.default_rng(64 + bits)
    w = 1.0 / np.arange(1, M + 1)
    kept, recs, rows = [], [], []
    e = engine(M, cell_bits=bits, num_buffers=2)
    try:
        for i in range(k):
            ids = rng.choice(M, n, p=w / w.sum()).astype(np.uint32)
            e.submit_pairs(ids[ids != i % M], rng.lognormal(3.0 + 0.01 * i, 1.0, n)[ids != i % M])   # a name missing from each
            with e.flip() as s:
                recs.append([x.copy() for x in s.buckets_all(M)])
                rows.append(rows_of(s, M))
                kept.append(s.keep(M))
        P = [0.0, .5, .9, .99, .999, 1.0]
        want = [model([r[m] for r in rows], P) for m in range(M)]
        assert sum(x["count"] for x in want) > 0.9 * k * n
        for kk, rec in zip(kept, recs):
            same_listing(kk, rec)
        res = {}
        for kind in SHAPES:
            with shape(kind):
                res[kind] = kept[-1].across(kept[:-1], P, M)
            check64(res[kind], want, P, kind)
        for f in FIELDS:
            assert res["wave"][f].tobytes() == res["block"][f].tobytes(), f
        assert int(res["wave"]["present_bits"][5]) == ((1 << 64) - 1) & ~(1 << 5) & ~(1 << 45)   # intervals 5 and 45 leave it out
    finally:
        e.close()
    for kind in SHAPES:                                                          # the engine is gone
        with shape(kind):
            again = kept[-1].across(kept[:-1], P, M)
        for f in FIELDS:
            assert again[f].tobytes() == res[kind][f].tobytes(), (kind, f)
    for kk, rec in zip(kept, recs):
        same_listing(kk, rec)
        kk.close()


# ---- 3. equals the dense route -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_equals_across_over_live_snapshots_and_the_import_route(native_lib, torch_cuda, bits):
    M, n, k = 40, 20_000, 16
    rng = np.random.default_rng(300 + bits)
    w = 1.0 / np.arange(1, M + 1)
    P = [0.0, .5, .75, .9, .99, .999, 1.0]
    with engine(M, cell_bits=bits, num_buffers=k) as e, engine(M, cell_bits=bits, num_buffers=2) as e2, \
            engine(M, cell_bits=64, num_buffers=2) as spare_engine, contextlib.ExitStack() as stack:
        snaps = []
        for i in range(k):                                                       # (an engine keeps at most 15 snapshots alive)
            eng = e if i < k - 1 else e2
            ids = rng.choice(M, n, p=w / w.sum()).astype(np.uint32)
            v = rng.lognormal(3.0 + 0.1 * i, 1.0, n)
            v[rng.random(n) < 0.02] *= -1.0
            eng.submit_pairs(ids[ids != 7 + i], v[ids != 7 + i])
            snaps.append(stack.enter_context(eng.flip()))
        kept = [stack.enter_context(s.keep(M)) for s in snaps]
        rows = [rows_of(s, M) for s in snaps]
        for K_ in (1, 2, 16):
            want = [model([r[m] for r in rows[:K_]], P) for m in range(M)]
            dense = snaps[K_ - 1].across(snaps[:K_ - 1], P, M)
            with spare_engine.flip() as spare:
                for kk in kept[:K_]:
                    kk.add_to(spare)
                ex = spare.extract(P, M)
            for kind in SHAPES:
                with shape(kind):
                    got = kept[K_ - 1].across(kept[:K_ - 1], P, M)
                check64(got, want, P, (kind, K_))
                for f in ("count", "nbuckets", "pkeys", "pvalid"):
                    assert np.array_equal(got[f], dense[f]), (kind, K_, f)
                    assert np.array_equal(got[f], ex[f]), (kind, K_, f, "import route")
                ok = got["pvalid"] != 0
                assert np.array_equal(got["pvals"][ok], dense["pvals"][ok]) and np.array_equal(got["pvals"][ok], ex["pvals"][ok])
                assert np.array_equal(got["present_bits"] & U64(0xffff), dense["present_bits"].astype(U64)), (kind, K_)
            check(dense, want, P, ("dense", K_))                                 # both sums within the bound of the model


# ---- 4 .. 7: the crafted rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
def test_crafted_lists(crafted, kind):
    c = crafted
    got = {}
    with shape(kind):
        for lst in LISTS:
            got[tuple(lst)] = call(c, lst)
    for lst in LISTS:
        check64(got[tuple(lst)], c.want(lst), P_MAIN, (kind, lst[:8], len(lst)))
    half, p1 = P_MAIN.index(0.5), P_MAIN.index(1.0)

    def bin_of(g, name, i=half):
        return int(oracle.key_to_bin(int(g["pkeys"][c.at[name], i])))

    # 5. 64-bit sums; a handle listed twice counts twice; a total past 2^64 wraps and the call returned LH_OK
    m = c.at["two_cells_of_2^32-1"]
    assert int(got[(0, 1)]["count"][m]) == 0x1fffffffe and int(got[(0, 1, 2)]["count"][m]) == 3 * U32MAX
    assert bin_of(got[(0, 1, 2)], "two_cells_of_2^32-1") == 500
    one, two = got[(0,)], got[(0, 0)]
    assert np.array_equal(two["count"], 2 * one["count"]) and np.array_equal(two["nbuckets"], one["nbuckets"])
    assert np.array_equal(two["pkeys"], one["pkeys"]) and np.array_equal(two["present_bits"], 3 * one["present_bits"])
    assert int(got[(BIG,)]["count"][c.at["total_2^64-1"]]) == (1 << 64) - 1
    assert int(got[(BIG,)]["count"][c.at["half_of_2^64"]]) == (1 << 63) + 7
    assert int(got[(BIG, BIG)]["count"][c.at["half_of_2^64"]]) == 14 and c.want([BIG, BIG])[c.at["half_of_2^64"]]["wrapped"]
    assert int(got[(BIG,)]["count"][c.at["cell_of_2^33"]]) == (1 << 33) + 5
    # the order of the list moves present_bits only -- integer cell sums, one fixed walk: the same bits in sum too
    a, b = got[tuple(range(K))], got[tuple(range(K - 1, -1, -1))]
    for f in ("count", "sum", "nbuckets", "pkeys", "pvalid"):
        assert a[f].tobytes() == b[f].tobytes(), f
    many = got[tuple(LISTS[-1])]
    assert int(many["present_bits"][c.at["only_in_4"]]) == sum(1 << j for j in range(64) if j % K == 4)
    assert int(a["present_bits"][c.at["never"]]) == 0 and int(a["present_bits"][c.at["marked_zero"]]) == 0
    assert bin_of(got[(0, 1)], "far_apart") == 10001 and bin_of(got[(0, 1)], "far_apart", p1) == 40001
    assert int(a["nbuckets"][c.at["one_bin"]]) == 1 and bin_of(a, "one_bin") == 5000 and int(a["count"][c.at["one_bin"]]) == 6
    assert bin_of(a, "one_bin_65535") == NK - 1


@pytest.mark.parametrize("kind", list(SHAPES))
def test_thresholds_at_the_edges_of_a_tile(crafted, kind):
    """Cells at bins 0, T - 1, T, 2T - 1, 2T and 65 535 with counts 1 .. 6 (prefix 1 3 6 10 15 21), one per handle or all in
    one: p = s / 21 has the threshold s exactly."""
    c, T = crafted, crafted.T
    P = [3 / 21, 4 / 21, 0.0, 1.0, 10 / 21, 11 / 21, 1 / 21, 2 / 21, 15 / 21, 16 / 21, 6 / 21, 7 / 21]
    bins = [T - 1, T, 0, NK - 1, 2 * T - 1, 2 * T, 0, T - 1, 2 * T, NK - 1, T, 2 * T - 1]
    with shape(kind):
        for lst, name in ((list(range(K)), "edges"), ([5, 3, 1, 0, 2, 4], "edges"), ([2], "edges_in_one"), ([2, 0], "edges_in_one")):
            m = c.at[name]
            got = call(c, lst, P, 1, m)
            check64(got, c.want(lst, P, m, 1), P, (kind, lst, name))
            if name == "edges" or lst == [2]:
                assert int(got["count"][0]) == 21 and int(got["nbuckets"][0]) == 6
                assert [int(oracle.key_to_bin(int(k))) for k in got["pkeys"][0]] == bins and got["pvalid"].all()
        # without the handle that holds bin T - 1 the same p fall elsewhere: the carry across the tiles is the prefix
        got = call(c, [0, 2, 3, 4, 5], P, 1, c.at["edges"])
        check64(got, c.want([0, 2, 3, 4, 5], P, c.at["edges"], 1), P, (kind, "no T - 1"))
        full = call(c, list(range(K)), P)
        check64(full, c.want(list(range(K)), P), P, (kind, "all rows"))


@pytest.mark.parametrize("kind", list(SHAPES))
def test_percentile_counts_and_ranges(crafted, kind):
    """np = 0 and np = 32; first > 0 with few rows; a block that some handle does not hold is LH_ERANGE."""
    import loghisto_amd
    c, lst = crafted, [0, 1, 2]
    p32 = [((7 * i) % 32) / 31.0 for i in range(32)]
    with shape(kind):
        full = call(c, lst)
        none = call(c, lst, [])
        many = call(c, lst, p32)
        assert set(none) == {"count", "sum", "avg", "nbuckets", "present_bits", "pkeys", "pvalid", "pvals"}
        assert none["pkeys"].shape == (c.M, 0) and none["pvals"].shape == (c.M, 0)
        check64(none, c.want(lst, []), [], (kind, "np=0"))
        check64(many, c.want(lst, p32), p32, (kind, "np=32"))
        for f in ("count", "sum", "nbuckets", "present_bits"):
            assert none[f].tobytes() == full[f].tobytes() == many[f].tobytes(), f
        for first, n in ((1, 1), (2, 3), (3, 4), (c.M - 5, 5), (0, 5), (7, 1)):
            part = call(c, lst, nmetrics=n, first=first)
            for f in FIELDS:
                assert part[f].tobytes() == full[f][first:first + n].tobytes(), (first, n, f)
        # np == 0 through ctypes: the per-percentile outputs are ignored, whatever they point to
        L = N.lib()
        hs = (C.c_void_p * 3)(*[c.kept[i]._h.value for i in lst])
        guard = np.full(c.M, 7, dtype=U64)
        assert L.lh_kept_across(hs, 3, 0, c.M, None, 0, 0, None, guard.ctypes.data, 0, 0, 0, 1, 1) == 0
        assert guard.tobytes() == full["count"].tobytes()
        # rows [3, 8) of the sub-block handle: inside it fine, outside LH_ERANGE, for the list as a whole
        sub = c.extra["sub"][0]
        both = sub.across([c.kept[0]], P_MAIN, 5, 3)
        ref = call(c, [0, 0], nmetrics=5, first=3)
        for f in FIELDS:
            assert both[f].tobytes() == ref[f].tobytes(), f
        assert sub.across([], P_MAIN, first=3)["count"].shape == (5,)          # nmetrics=None: up to the end of its block
        for first, n in ((2, 2), (3, 6), (8, 1), (0, c.M), (7, 2)):
            for earlier in ([], [c.kept[0]], [c.kept[1], c.kept[2]]):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    sub.across(earlier, P_MAIN, n, first)
                assert ei.value.code == N.ERANGE, (first, n)
        for first, n in ((0, c.M + 1), (c.M, 1), (1, c.M)):
            with pytest.raises(loghisto_amd.LhError) as ei:
                call(c, lst, nmetrics=n, first=first)
            assert ei.value.code == N.ERANGE, (first, n)


# ---- 6. the id forms ---------------------------------------------------------------------------------------------------------
def _device_out(torch, n, P, names=tuple(FIELDS)):
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int64, pkeys=torch.int16,
                 pvalid=torch.uint8)
    return {k: torch.full((n, len(P)) if k in PER_P else (n,), 77, dtype=kinds[k], device="cuda") for k in names}


def _back(out):
    return {k: v.cpu().numpy().view(FIELDS[k]) for k, v in out.items()}


@pytest.mark.parametrize("kind", list(SHAPES))
def test_id_forms(crafted, kind):
    import loghisto_amd
    c, torch, lst = crafted, crafted.torch, [0, 1, 2, BIG]
    ids = [c.at["edges"], 0, c.M - 1, c.at["dense300"], 0, c.at["eight_tiles"], 5, 4, 3, c.at["edges"], c.at["never"]]
    with shape(kind):
        full = call(c, lst)
        got = call(c, lst, ids=ids)                                              # a host list: unsorted, repeated
        check64(got, [c.want(lst)[i] for i in ids], P_MAIN, (kind, "ids"))
        # (the shape is chosen by the number of entries: here both calls are pinned to one shape, so the bits agree)
        for f in FIELDS:
            assert got[f].tobytes() == full[f][ids].tobytes(), f
        # device ids on a caller's stream; ids at or beyond the block give the all-zero entry, the others are unaffected
        st = torch.cuda.Stream()
        bad = {2: c.M, 6: c.M + 1000, 9: 0xffffffff}
        dids = [bad.get(j, i) for j, i in enumerate(ids)]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(dids, dtype=torch.int64, device="cuda").to(torch.int32)
            out = _device_out(torch, len(ids), P_MAIN)
        st.synchronize()
        assert call(c, lst, ids=d_ids, out=out, stream=st)["count"] is out["count"]
        st.synchronize()
        dev = _back(out)
        for j in range(len(ids)):
            for f in FIELDS:
                want = np.zeros_like(got[f][j]) if j in bad else got[f][j]
                assert dev[f][j].tobytes() == want.tobytes(), (j, f)
        # ... and so does an id that ONE handle of the list does not hold (the sub-block handle has rows 3 .. 7)
        sub = c.extra["sub"][0]
        with torch.cuda.stream(st):
            d_ids = torch.tensor([3, 2, 7, 8, 5], dtype=torch.int32, device="cuda")
            out = _device_out(torch, 5, P_MAIN)
        st.synchronize()
        sub.across([c.kept[0]], P_MAIN, ids=d_ids, out=out, stream=st)
        st.synchronize()
        dev, ref = _back(out), call(c, [0, 0])
        for j, i in enumerate([3, 2, 7, 8, 5]):
            for f in FIELDS:
                want = ref[f][i] if 3 <= i < 8 else np.zeros_like(ref[f][i])
                assert dev[f][j].tobytes() == want.tobytes(), (j, f)
        # a host id that some handle does not hold: LH_ERANGE, nothing enqueued, nothing written
        for earlier, kk, bad_ids in (([c.kept[i] for i in lst[:-1]], c.kept[lst[-1]], [0, c.M, 1]), ([c.kept[0]], sub, [3, 4, 2]),
                                     ([c.kept[0]], sub, [8]), ([sub], c.kept[0], [7, 0xffffffff])):
            out = {k: np.full((len(bad_ids), len(P_MAIN)) if k in PER_P else (len(bad_ids),), 7, dtype=t) for k, t in FIELDS.items()}
            with pytest.raises(loghisto_amd.LhError) as ei:
                kk.across(earlier, P_MAIN, ids=bad_ids, out=out)
            assert ei.value.code == N.ERANGE
            assert all(np.all(v == 7) for v in out.values())
        assert call(c, lst, ids=[])["count"].shape == (0,)                       # n == 0


# ---- 9. device forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
def test_device_forms(crafted, kind):
    """Device form == host form byte for byte on a caller's stream, outputs left out, pageable == pinned."""
    c, torch, M = crafted, crafted.torch, crafted.M
    st = torch.cuda.Stream()
    with shape(kind):
        for lst in ([0, 1, 2], [BIG, 0, 1], list(range(K)), LISTS[-1]):
            hostf = call(c, lst)
            out = _device_out(torch, M, P_MAIN)
            torch.cuda.synchronize()
            back = call(c, lst, out=out, stream=st)
            st.synchronize()
            assert all(back[k] is out[k] for k in FIELDS)
            dev = _back(out)
            for f in FIELDS:
                assert dev[f].tobytes() == hostf[f].tobytes(), (lst[:8], f)
        lst = [BIG, 0, 1]
        hostf = call(c, lst)
        f0, n = 2, M - 5
        out = _device_out(torch, n, P_MAIN)
        torch.cuda.synchronize()
        call(c, lst, nmetrics=n, first=f0, out=out, stream=st)
        st.synchronize()
        for f, v in _back(out).items():
            assert v.tobytes() == hostf[f][f0:f0 + n].tobytes(), f
        for names in (("count",), ("pkeys",), ("pvalid", "present_bits"), ("sum", "nbuckets"), tuple(k for k in FIELDS if k != "count")):
            out = _device_out(torch, M, P_MAIN, names)
            torch.cuda.synchronize()
            call(c, lst, out=out)                                                # the null stream
            torch.cuda.synchronize()
            pageable = {k: np.full((M, len(P_MAIN)) if k in PER_P else (M,), 7, dtype=FIELDS[k]) for k in names}
            got = call(c, lst, out=pageable)
            assert set(got) - {"avg", "pvals"} == set(names)
            for k, v in _back(out).items():
                assert v.tobytes() == hostf[k].tobytes() == pageable[k].tobytes(), (names, k)


@pytest.mark.parametrize("bits", (64, 32))
def test_release_right_after_a_device_form_call_waits_for_it(native_lib, torch_cuda, bits):
    torch = torch_cuda
    M, n = 70, 50_000
    rng = np.random.default_rng(9)
    P = [0.5, 0.99]
    sets = [(rng.integers(0, M, n).astype(np.uint32), rng.lognormal(2.0 + i, 1.5, n)) for i in range(3)]

    def three(e):
        kept = []
        for ids, v in sets:
            e.submit_pairs(ids, v)
            with e.flip() as s:
                kept.append(s.keep(M))
        return kept

    with engine(M, cell_bits=bits) as e:
        ref = three(e)
        for kind in SHAPES:
            with shape(kind):
                want = ref[2].across(ref[:2], P, M)
                fresh = three(e)                                                 # the same cells in handles to be closed at once
                st = torch.cuda.Stream()
                out, junk = _device_out(torch, M, P), _device_out(torch, M, P)
                torch.cuda.synchronize()
                for _ in range(20):                                              # work ahead of the call on the same stream
                    fresh[2].across(fresh[:2], P, M, out=junk, stream=st)
                fresh[2].across(fresh[:2], P, M, out=out, stream=st)
                for k_ in fresh:
                    k_.close()                                                   # waits for the enqueued kernels
                st.synchronize()
                for f, v in _back(out).items():
                    assert v.tobytes() == want[f].tobytes(), (kind, f)
        for k_ in ref:
            k_.close()


@pytest.mark.parametrize("bits", (64, 32))
def test_release_waits_for_device_form_calls_on_two_streams(native_lib, torch_cuda, bits):
    """The same handles read by device-form calls on TWO caller streams, with work ahead on the first: each call's event is
    chained behind the handle's earlier one, so close() right afterwards waits for both streams' readers."""
    torch = torch_cuda
    M, n = 70, 50_000
    rng = np.random.default_rng(19)
    P = [0.5, 0.99]
    sets = [(rng.integers(0, M, n).astype(np.uint32), rng.lognormal(2.0 + i, 1.5, n)) for i in range(3)]

    def three(e):
        kept = []
        for ids, v in sets:
            e.submit_pairs(ids, v)
            with e.flip() as s:
                kept.append(s.keep(M))
        return kept

    with engine(M, cell_bits=bits) as e:
        ref = three(e)
        for kind in SHAPES:
            with shape(kind):
                want_a = ref[2].across(ref[:2], P, M)
                want_b = ref[0].across([ref[1]], P, M - 3, 3)
                fresh = three(e)
                a, b = torch.cuda.Stream(), torch.cuda.Stream()
                out_a, out_b, junk = _device_out(torch, M, P), _device_out(torch, M - 3, P), _device_out(torch, M, P)
                torch.cuda.synchronize()
                for _ in range(20):                                              # work ahead on the first stream
                    fresh[2].across(fresh[:2], P, M, out=junk, stream=a)
                fresh[2].across(fresh[:2], P, M, out=out_a, stream=a)
                fresh[0].across([fresh[1]], P, M - 3, 3, out=out_b, stream=b)    # two of the three again, on the second
                for k_ in fresh:
                    k_.close()                                                   # waits for the readers on both streams
                a.synchronize()
                b.synchronize()
                for f, v in _back(out_a).items():
                    assert v.tobytes() == want_a[f].tobytes(), (kind, "first stream", f)
                for f, v in _back(out_b).items():
                    assert v.tobytes() == want_b[f].tobytes(), (kind, "second stream", f)
        for k_ in ref:
            k_.close()


@pytest.mark.parametrize("bits", (64, 32))
def test_close_right_after_add_to_waits_for_the_import(native_lib, torch_cuda, bits):
    M, n = 70, 50_000
    rng = np.random.default_rng(23)
    with engine(M, cell_bits=bits) as e, engine(M, cell_bits=bits) as e2:
        e.submit_pairs(rng.integers(0, M, n).astype(np.uint32), rng.lognormal(3.0, 1.0, n))
        with e.flip() as snap, e2.flip() as spare:
            want = rows_of(snap, M)
            k = snap.keep(M)
            for _ in range(3):
                k.add_to(spare)
            k.close()                                                            # (lh_kept_hold: the imports still read it)
            torch_cuda.cuda.ExternalStream(spare.stream()).synchronize()
            got = rows_of(spare, M)
            assert got == [{b: 3 * c for b, c in r.items()} for r in want]
