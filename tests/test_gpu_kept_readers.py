"""lh_kept_count_le* and lh_kept_spread* (Kept.count_le, Kept.spread): lh_count_le's and lh_spread's outputs over a list of
kept intervals, with no dense buffer alive.

On the crafted fixture of tests/test_gpu_kept.py (70 names x 6 handles, engines of 64- and of 32-bit cells), under both kernel
shapes (lh_tool_kept_switch).  The model is Python integers and fractions.Fraction over the recorded rows: C[b] = the sum over
the list of the name's cell b modulo 2^64 (a sum that wraps to 0 is no cell).
  count_le   cum and total EXACT modulo 2^64, whatever wraps
  spread     count exact modulo 2^64; for a name whose total stays below 2^64 (beyond it the other outputs are unspecified) pkeys,
             pvalid and count_le exact, sum and sum_le within 1e-12 x the sum of |D[b] C[b]| over the bins taken in, m2 within
             1e-12 M2 + 2 (1e-12 A)^2 / count: tests/test_gpu_spread.py's check and bounds as they stand
Both are also held to lh_count_le / lh_spread on a live snapshot that received the same handles through Kept.add_to: integers
equal, floats each within the bounds above of the exact value.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import bisect

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_across import P_MAIN
from tests.test_gpu_count_le import engine, take_of
from tests.test_gpu_kept import BIG, K, LISTS, crafted, shape, tile  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_spread import Exact, check as check_spread

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
W = 1 << 64
KINDS = ("wave", "block")
INF = float("inf")
SP_FIELDS = dict(count=U64, sum=np.float64, m2=np.float64, pkeys=np.int16, pvalid=np.uint8, count_le=U64, sum_le=np.float64)
SP_PER_P = ("pkeys", "pvalid", "count_le", "sum_le")
SP_LISTS = [[0], [0, 1, 2], [BIG, BIG], list(range(K)), list(range(K - 1, -1, -1)), LISTS[-1]]
P_ENDS = [0.0, 1.0, 1.5, float("nan")]
_CELLS, _EXACT, _CUM = {}, {}, {}


def value_of(b):
    """decompress(the key of bin b): the bound that takes in exactly the bins 0 .. b (b >= 1: below, the bound saturates)"""
    return oracle.decompress(int(oracle.bin_to_key(int(b))))


# ---- the model -------------------------------------------------------------------------------------------------------------
def cells_of(c, lst):
    """per name (sorted bins, C at those bins) with C the sum over the list modulo 2^64, zeros left out; and the wrapping
    sum of the handles' row sums"""
    key = (c.wide, tuple(lst))
    if key not in _CELLS:
        out = []
        for m in range(c.M):
            tot = {}
            for i in lst:
                for b, v in c.rows[i][m].items():
                    tot[b] = tot.get(b, 0) + v
            bins = sorted(b for b, v in tot.items() if v % W)
            out.append((bins, [tot[b] % W for b in bins], sum(tot.values()) % W))
        _CELLS[key] = out
    return _CELLS[key]


def want_cum(c, lst, bounds, name):
    """(cum[M][nb], total[M]) as Python integers"""
    key = (c.wide, tuple(lst), name)
    if key not in _CUM:
        E = [int(e) for e in take_of(np.asarray(bounds, dtype=np.float64))]
        cum, total = [], []
        for bins, counts, tot in cells_of(c, lst):
            pre = [0]
            for v in counts:
                pre.append(pre[-1] + v)
            cum.append([pre[bisect.bisect_left(bins, e)] % W for e in E])       # the bins below e: the first e of the row
            total.append(tot)
            assert pre[-1] % W == tot
        _CUM[key] = (cum, total)
    return _CUM[key]


def exact_rows(c, lst):
    """tests/test_gpu_spread.py's Exact per name, None where the total passes 2^64"""
    key = (c.wide, tuple(lst))
    if key not in _EXACT:
        _EXACT[key] = [Exact(bins, counts) if sum(counts) < W else None for bins, counts, _ in cells_of(c, lst)]
    return _EXACT[key]


def check_cum(got, c, lst, bounds, name, first=0, n=None, what=""):
    cum, total = want_cum(c, lst, bounds, name)
    n = c.M - first if n is None else n
    assert got["cum"].dtype == U64 and got["cum"].shape == (n, len(bounds)) and got["total"].shape == (n,), what
    assert [[int(x) for x in r] for r in got["cum"]] == cum[first:first + n], what
    assert [int(x) for x in got["total"]] == total[first:first + n], what


def check_spreads(got, c, lst, P, rows=None, what=""):
    """rows: the names of got's entries, in order (None: all)"""
    rows = list(range(c.M)) if rows is None else list(rows)
    ex, cells = exact_rows(c, lst), cells_of(c, lst)
    assert got["count"].dtype == U64 and [int(x) for x in got["count"]] == [cells[m][2] for m in rows], what
    ok = [j for j, m in enumerate(rows) if ex[m] is not None]
    assert len(ok) >= len(rows) - 2, what                                        # the crafted rows wrap in two names at most
    sub = {k: v[ok] for k, v in got.items()}
    check_spread(sub, [ex[rows[j]] for j in ok], P)


def bound_sets(T):
    edges = [value_of(b) for b in (0, 1, T - 1, T, 2 * T - 1, 2 * T, NK - 2, NK - 1)]
    gaps = [value_of(b) for b in (9000, 10000, 10001, 10002, 10001 + T, 20000, 40000, 40001, 50000)]   # far_apart: 10 001 and 40 001
    special = [-INF, -1e200, -0.0, 0.0, 0.0, 1e200, 1e200, INF, INF]
    rng = np.random.default_rng(64)
    many = [value_of(b) for b in rng.integers(0, NK, 40)] + [value_of(b) for b in rng.normal(33000, 60, 12).astype(int)] + \
        special + [value_of(T), value_of(T), -INF]
    sets = {"main": sorted(edges + gaps + special + [edges[3], gaps[2]]), "one": [value_of(T - 1)], "nb64": sorted(many)}
    assert len(sets["nb64"]) == N.MAX_BOUNDS and len(sets["main"]) <= N.MAX_BOUNDS
    return sets


@pytest.fixture(scope="module")
def spare_engine(native_lib, torch_cuda):
    with engine(70, cell_bits=64, num_buffers=2) as e:
        yield e


def le_call(c, lst, bounds, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].count_le(bounds, [c.kept[i] for i in lst[:-1]], c.M - first if nmetrics is None else nmetrics, first, **kw)


def sp_call(c, lst, P, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].spread(P, [c.kept[i] for i in lst[:-1]], c.M - first if nmetrics is None else nmetrics, first, **kw)


# ---- count_le --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_count_le_every_list(crafted, kind):
    c = crafted
    sets = bound_sets(c.T)
    got = {}
    with shape(kind):
        for lst in LISTS:
            for name in ("main", "nb64"):
                got[tuple(lst), name] = le_call(c, lst, sets[name])
        got[tuple(range(K)), "one"] = le_call(c, list(range(K)), sets["one"])
        got[(0, 1), "one"] = le_call(c, [0, 1], sets["one"])
    for (lst, name), g in got.items():
        check_cum(g, c, list(lst), sets[name], name, what=(kind, lst[:8], len(lst), name))
    # what the crafted rows were made for
    main, lo = got[tuple(range(K)), "main"], sets["main"]
    at = {v: j for j, v in enumerate(lo)}                                        # (of equal neighbours the last)
    T = c.T
    for name in ("edges", "edges_in_one"):
        lst = tuple(range(K)) if name == "edges" else (2,)
        g = main if name == "edges" else le_call(c, [2], lo)
        row = g["cum"][c.at[name]]
        # (bin 0 is key -32 768, whose value's extended key passes 32 767: as a bound it saturates and takes in nothing)
        assert [int(row[at[value_of(b)]]) for b in (0, T - 1, T, 2 * T - 1, 2 * T, NK - 1)] == [0, 3, 6, 10, 15, 21], (kind, name, lst)
        assert int(row[at[-INF]]) == 0 and int(row[at[INF]]) == 21 and int(row[at[-1e200]]) == 0 and int(row[at[1e200]]) == 21
    row = main["cum"][c.at["bins_0_65535"]]
    assert int(row[at[value_of(1)]]) == 6 and int(row[at[value_of(NK - 2)]]) == 6 and int(row[at[value_of(NK - 1)]]) == 14
    row = got[(0, 1), "main"]["cum"][c.at["far_apart"]]
    assert [int(row[at[value_of(b)]]) for b in (9000, 10000, 10001, 10002, 10001 + T, 20000, 40000, 40001, 50000)] == \
        [0, 0, 1, 1, 1, 1, 1, 2, 2]
    assert int(row[at[-0.0]]) == int(row[at[0.0]]) == 1                          # bin 32 768, between the two cells
    m = c.at["total_2^64-1"]
    assert int(got[(BIG,), "main"]["total"][m]) == W - 1 and int(got[(BIG,), "main"]["cum"][m][at[INF]]) == W - 1
    m = c.at["half_of_2^64"]
    assert int(got[(BIG, BIG), "main"]["total"][m]) == 14 and int(got[(BIG, BIG), "main"]["cum"][m][at[INF]]) == 14
    assert not main["cum"][c.at["never"]].any() and not main["cum"][c.at["marked_zero"]].any()


def test_count_le_shapes_agree_and_equal_the_snapshot_route(crafted, spare_engine):
    c = crafted
    sets = bound_sets(c.T)
    for lst in ([0, 1, 2], [BIG, BIG], list(range(K)), LISTS[-1]):
        res = {}
        for kind in KINDS:
            with shape(kind):
                res[kind] = le_call(c, lst, sets["nb64"])
        assert res["wave"]["cum"].tobytes() == res["block"]["cum"].tobytes()
        assert res["wave"]["total"].tobytes() == res["block"]["total"].tobytes()
        with spare_engine.flip() as spare:
            for i in lst:
                c.kept[i].add_to(spare)
            dense = spare.count_le(sets["nb64"], c.M)
        assert np.array_equal(dense["cum"], res["wave"]["cum"]) and np.array_equal(dense["total"], res["wave"]["total"]), lst[:8]


# ---- spread ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_spread_lists_and_percentiles(crafted, kind):
    c = crafted
    got = {}
    with shape(kind):
        for lst in SP_LISTS:
            got[tuple(lst)] = sp_call(c, lst, P_MAIN)
        ends = sp_call(c, list(range(K)), P_ENDS)
        none = sp_call(c, [0, 1, 2], [])
    for lst in SP_LISTS:
        check_spreads(got[tuple(lst)], c, lst, P_MAIN, what=(kind, lst[:8], len(lst)))
    check_spreads(ends, c, list(range(K)), P_ENDS, what=(kind, "ends"))
    assert not ends["pvalid"][:, 2:].any() and ends["pvalid"][c.at["plain"], 0] == 1 and ends["pvalid"][c.at["plain"], 1] == 1
    check_spreads(none, c, [0, 1, 2], [], what=(kind, "np=0"))
    assert none["pkeys"].shape == (c.M, 0) and none["upper"].shape == (c.M, 0)
    for f in ("count", "sum", "m2"):                                             # the moments do not depend on the percentiles
        assert none[f].tobytes() == got[(0, 1, 2)][f].tobytes(), f
    # names whose samples share one bucket: a spread of (numerically) zero, within the one-bucket bound 2 (1e-12 A)^2 / count
    a = got[tuple(range(K))]
    D = oracle.decompress_table()
    for name, b, n in (("one_bin", 5000, 6), ("one_bin_65535", NK - 1, 3)):
        m = c.at[name]
        assert int(a["count"][m]) == n and 0.0 <= a["m2"][m] <= 2 * (1e-12 * n * abs(D[b])) ** 2 / n, (name, a["m2"][m])
    # the order of the list moves nothing: integer cell sums, one fixed walk
    b = got[tuple(range(K - 1, -1, -1))]
    for f in SP_FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f
    assert int(got[(BIG, BIG)]["count"][c.at["half_of_2^64"]]) == 14 and int(got[(BIG, BIG)]["count_le"][c.at["half_of_2^64"], 1]) == 14


@pytest.mark.parametrize("kind", KINDS)
def test_spread_thresholds_at_the_edges_of_a_tile(crafted, kind):
    """Cells at bins 0, T - 1, T, 2T - 1, 2T and 65 535 with counts 1 .. 6 (prefix 1 3 6 10 15 21): p = s / 21 has the threshold s."""
    c, T = crafted, crafted.T
    P = [s / 21 for s in range(22)]
    prefix = [1, 3, 6, 10, 15, 21]
    bins = [0, T - 1, T, 2 * T - 1, 2 * T, NK - 1]
    want_at = [bisect.bisect_left(prefix, max(s, 1)) for s in range(22)]
    with shape(kind):
        for lst, name in ((list(range(K)), "edges"), ([5, 3, 1, 0, 2, 4], "edges"), ([2], "edges_in_one"), ([0, 2, 3, 4, 5], "edges")):
            m = c.at[name]
            got = sp_call(c, lst, P, 1, m)
            check_spreads(got, c, lst, P, rows=[m], what=(kind, lst, name))
            if len(lst) != 5:
                assert [int(oracle.key_to_bin(int(k))) for k in got["pkeys"][0]] == [bins[j] for j in want_at]
                assert [int(x) for x in got["count_le"][0]] == [prefix[j] for j in want_at] and got["pvalid"].all()
        full = sp_call(c, list(range(K)), P)
        check_spreads(full, c, list(range(K)), P, what=(kind, "all rows"))


def test_spread_shapes_agree_bit_for_bit_and_match_the_snapshot_route(crafted, spare_engine):
    c = crafted
    for lst in ([0, 1, 2], [BIG, BIG], list(range(K)), LISTS[-1]):
        res = {}
        for kind in KINDS:
            with shape(kind):
                res[kind] = sp_call(c, lst, P_MAIN)
        for f in SP_FIELDS:
            assert res["wave"][f].tobytes() == res["block"][f].tobytes(), (lst[:8], f)
        with spare_engine.flip() as spare:
            for i in lst:
                c.kept[i].add_to(spare)
            dense = spare.spread(P_MAIN, c.M)
        ok = [m for m, r in enumerate(exact_rows(c, lst)) if r is not None]
        for f in ("count", "pkeys", "pvalid", "count_le"):
            assert np.array_equal(dense[f][ok], res["wave"][f][ok]), (lst[:8], f)
        assert np.array_equal(dense["count"], res["wave"]["count"])
        check_spreads(dense, c, lst, P_MAIN, what=("the snapshot route", lst[:8]))   # its floats within the same bounds of the exact values


# ---- both readers: rows, ids, device forms, ranges, release ----------------------------------------------------------------------
def _le_out(torch, n, nb, pad=3):
    back = dict(cum=torch.full(((n + pad) * nb,), 77, dtype=torch.int64, device="cuda"),
                total=torch.full((n + pad,), 77, dtype=torch.int64, device="cuda"))
    return back, dict(cum=back["cum"][:n * nb], total=back["total"][:n])


def _sp_out(torch, n, np_, names=tuple(SP_FIELDS), pad=3):
    kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8, count_le=torch.int64,
                 sum_le=torch.float64)
    back = {k: torch.full(((n + pad) * (np_ if k in SP_PER_P else 1),), 77, dtype=kinds[k], device="cuda") for k in SP_FIELDS}
    return back, {k: back[k][:n * (np_ if k in SP_PER_P else 1)] for k in names}


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _same_sp(back, n, np_, want, names, what):
    """the device arrays hold want's rows; behind them, and in the arrays not asked for, the sentinel stands"""
    for k, dt in SP_FIELDS.items():
        per = np_ if k in SP_PER_P else 1
        h = _host(back[k], dt)
        if k in names:
            assert h[:n * per].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)
            assert np.all(h[n * per:] == 77), (what, k)
        else:
            assert np.all(h == 77), (what, k, "not asked for")


@pytest.mark.parametrize("kind", KINDS)
def test_rows_ids_and_device_forms(crafted, kind):
    import loghisto_amd
    c, torch, lst = crafted, crafted.torch, [0, 1, 2, BIG]
    bounds = bound_sets(c.T)["main"]
    nb, npct = len(bounds), len(P_MAIN)
    ids = [c.at["edges"], 0, c.M - 1, c.at["dense300"], 0, c.at["eight_tiles"], 5, 4, 3, c.at["edges"], c.at["never"], c.at["far_apart"]]
    st = torch.cuda.Stream()
    with shape(kind):
        le, sp = le_call(c, lst, bounds), sp_call(c, lst, P_MAIN)
        check_cum(le, c, lst, bounds, "main", what=kind)
        check_spreads(sp, c, lst, P_MAIN, what=kind)
        # sub-ranges
        for first, n in ((1, 1), (2, 3), (3, 4), (c.M - 5, 5), (0, 5), (7, 1)):
            part = le_call(c, lst, bounds, n, first)
            assert part["cum"].tobytes() == le["cum"][first:first + n].tobytes() and part["total"].tobytes() == le["total"][first:first + n].tobytes()
            part = sp_call(c, lst, P_MAIN, n, first)
            for f in SP_FIELDS:
                assert part[f].tobytes() == sp[f][first:first + n].tobytes(), (first, n, f)
        # a host id list: shuffled, repeated (both calls are pinned to one shape, so the bits agree)
        got = le_call(c, lst, bounds, ids=ids)
        assert got["cum"].tobytes() == le["cum"][ids].tobytes() and got["total"].tobytes() == le["total"][ids].tobytes()
        gsp = sp_call(c, lst, P_MAIN, ids=ids)
        for f in SP_FIELDS:
            assert gsp[f].tobytes() == sp[f][ids].tobytes(), f
        check_spreads(gsp, c, lst, P_MAIN, rows=ids, what=(kind, "ids"))
        assert le_call(c, lst, bounds, ids=[])["total"].shape == (0,) and sp_call(c, lst, P_MAIN, ids=[])["count"].shape == (0,)
        # device forms on a caller's stream, whole block and sub-range: sentinel-filled arrays, written up to the rows asked for
        for first, n in ((0, c.M), (2, c.M - 5)):
            back, out = _le_out(torch, n, nb)
            sback, sout = _sp_out(torch, n, npct)
            torch.cuda.synchronize()
            assert le_call(c, lst, bounds, n, first, out=out, stream=st)["cum"] is out["cum"]
            assert sp_call(c, lst, P_MAIN, n, first, out=sout, stream=st)["m2"] is sout["m2"]
            st.synchronize()
            assert _host(back["cum"], U64)[:n * nb].tobytes() == le["cum"][first:first + n].tobytes()
            assert _host(back["total"], U64)[:n].tobytes() == le["total"][first:first + n].tobytes()
            assert np.all(_host(back["cum"], U64)[n * nb:] == 77) and np.all(_host(back["total"], U64)[n:] == 77)
            _same_sp(sback, n, npct, {k: v[first:first + n] for k, v in sp.items()}, tuple(SP_FIELDS), (kind, first, n))
        # only the requested arrays are written; pageable host arrays == pinned ones
        for names in (("cum",), ("total",)):
            back, out = _le_out(torch, c.M, nb)
            torch.cuda.synchronize()
            le_call(c, lst, bounds, out={k: out[k] for k in names})                  # the null stream
            torch.cuda.synchronize()
            for k in ("cum", "total"):
                h = _host(back[k], U64)
                n = c.M * (nb if k == "cum" else 1)
                assert (h[:n].tobytes() == le[k].tobytes() and np.all(h[n:] == 77)) if k in names else np.all(h == 77), (names, k)
            pageable = {k: np.full((c.M, nb) if k == "cum" else (c.M,), 7, dtype=U64) for k in names}
            res = le_call(c, lst, bounds, out=pageable)
            assert set(res) == set(names) and all(pageable[k].tobytes() == le[k].tobytes() for k in names)
        for names in (("count",), ("m2",), ("pkeys", "sum_le"), ("pvalid", "count_le", "sum"), tuple(k for k in SP_FIELDS if k != "count")):
            sback, sout = _sp_out(torch, c.M, npct, names)
            torch.cuda.synchronize()
            sp_call(c, lst, P_MAIN, out=sout)
            torch.cuda.synchronize()
            _same_sp(sback, c.M, npct, sp, names, (kind, names))
            pageable = {k: np.full((c.M, npct) if k in SP_PER_P else (c.M,), 7, dtype=SP_FIELDS[k]) for k in names}
            res = sp_call(c, lst, P_MAIN, out=pageable)
            assert set(res) - {"std", "mean_le", "upper"} == set(names)
            assert all(pageable[k].tobytes() == sp[k].tobytes() for k in names), names
        # device ids; ids at or beyond the block give the all-zero entry, the others are unaffected
        bad = {2: c.M, 6: c.M + 1000, 9: 0xffffffff}
        dids = [bad.get(j, i) for j, i in enumerate(ids)]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(dids, dtype=torch.int64, device="cuda").to(torch.int32)
        back, out = _le_out(torch, len(ids), nb)
        sback, sout = _sp_out(torch, len(ids), npct)
        torch.cuda.synchronize()
        le_call(c, lst, bounds, ids=d_ids, out=out, stream=st)
        sp_call(c, lst, P_MAIN, ids=d_ids, out=sout, stream=st)
        st.synchronize()
        zero = lambda a: np.stack([np.zeros_like(a[j]) if j in bad else a[j] for j in range(len(ids))])   # noqa: E731
        assert _host(out["cum"], U64).tobytes() == zero(got["cum"]).tobytes() and _host(out["total"], U64).tobytes() == zero(got["total"]).tobytes()
        _same_sp(sback, len(ids), npct, {k: zero(gsp[k]) for k in SP_FIELDS}, tuple(SP_FIELDS), (kind, "device ids"))
        # ... and so does an id that ONE handle of the list does not hold (the sub-block handle has rows 3 .. 7)
        sub = c.extra["sub"][0]
        ref_le, ref_sp = le_call(c, [0, 0], bounds), sp_call(c, [0, 0], P_MAIN)
        some = [3, 2, 7, 8, 5]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(some, dtype=torch.int32, device="cuda")
        back, out = _le_out(torch, 5, nb)
        sback, sout = _sp_out(torch, 5, npct)
        torch.cuda.synchronize()
        sub.count_le(bounds, [c.kept[0]], ids=d_ids, out=out, stream=st)
        sub.spread(P_MAIN, [c.kept[0]], ids=d_ids, out=sout, stream=st)
        st.synchronize()
        pick = lambda a: np.stack([a[i] if 3 <= i < 8 else np.zeros_like(a[i]) for i in some])   # noqa: E731
        assert _host(out["cum"], U64).tobytes() == pick(ref_le["cum"]).tobytes() and _host(out["total"], U64).tobytes() == pick(ref_le["total"]).tobytes()
        _same_sp(sback, 5, npct, {k: pick(ref_sp[k]) for k in SP_FIELDS}, tuple(SP_FIELDS), (kind, "one handle lacks the row"))
        # rows [3, 8) of the sub-block handle: inside it fine (nmetrics=None: up to the end of its block), outside LH_ERANGE
        both = sub.count_le(bounds, [c.kept[0]], first=3)
        assert both["cum"].tobytes() == ref_le["cum"][3:8].tobytes()
        assert sub.spread(P_MAIN, [c.kept[0]], first=3)["m2"].tobytes() == ref_sp["m2"][3:8].tobytes()
        calls = [lambda k, e, **kw: k.count_le(bounds, e, **kw), lambda k, e, **kw: k.spread(P_MAIN, e, **kw)]
        for f in calls:
            for first, n in ((2, 2), (3, 6), (8, 1), (0, c.M), (7, 2)):
                for earlier in ([], [c.kept[0]], [c.kept[1], c.kept[2]]):
                    with pytest.raises(loghisto_amd.LhError) as ei:
                        f(sub, earlier, nmetrics=n, first=first)
                    assert ei.value.code == N.ERANGE, (first, n)
            for first, n in ((0, c.M + 1), (c.M, 1), (1, c.M)):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    f(c.kept[2], [c.kept[0], c.kept[1]], nmetrics=n, first=first)
                assert ei.value.code == N.ERANGE, (first, n)
            # a host id that some handle does not hold: LH_ERANGE, nothing enqueued, nothing written
            for earlier, kk, bad_ids in (([c.kept[0], c.kept[1]], c.kept[2], [0, c.M, 1]), ([c.kept[0]], sub, [3, 4, 2]),
                                         ([c.kept[0]], sub, [8]), ([sub], c.kept[0], [7, 0xffffffff])):
                if f is calls[0]:
                    out = dict(cum=np.full((len(bad_ids), nb), 7, dtype=U64), total=np.full(len(bad_ids), 7, dtype=U64))
                else:
                    out = {k: np.full((len(bad_ids), npct) if k in SP_PER_P else (len(bad_ids),), 7, dtype=t) for k, t in SP_FIELDS.items()}
                with pytest.raises(loghisto_amd.LhError) as ei:
                    f(kk, earlier, ids=bad_ids, out=out)
                assert ei.value.code == N.ERANGE
                assert all(np.all(v == 7) for v in out.values())
        with pytest.raises(ValueError):
            c.kept[0].count_le(np.zeros((c.M, 2)))                                   # a row of bounds per name: not over handles


@pytest.mark.parametrize("kind", KINDS)
def test_close_right_after_a_device_form_call_waits_for_it(crafted, kind):
    c, torch = crafted, crafted.torch
    bounds = bound_sets(c.T)["nb64"]
    nb, npct = len(bounds), len(P_MAIN)
    lst = [0, 1, 2, BIG]
    with shape(kind):
        le, sp = le_call(c, lst, bounds), sp_call(c, lst, P_MAIN)
        for reader in ("count_le", "spread"):
            fresh = [c.kept[i].merge() for i in lst]                                 # the same cells in handles to be closed at once
            st = torch.cuda.Stream()
            back, out = _le_out(torch, c.M, nb)
            _, junk = _le_out(torch, c.M, nb)
            sback, sout = _sp_out(torch, c.M, npct)
            _, sjunk = _sp_out(torch, c.M, npct)
            torch.cuda.synchronize()
            for _ in range(20):                                                      # work ahead of the call on the same stream
                if reader == "count_le":
                    fresh[-1].count_le(bounds, fresh[:-1], c.M, out=junk, stream=st)
                else:
                    fresh[-1].spread(P_MAIN, fresh[:-1], c.M, out=sjunk, stream=st)
            if reader == "count_le":
                fresh[-1].count_le(bounds, fresh[:-1], c.M, out=out, stream=st)
            else:
                fresh[-1].spread(P_MAIN, fresh[:-1], c.M, out=sout, stream=st)
            for k_ in fresh:
                k_.close()                                                           # waits for the enqueued kernels
            st.synchronize()
            if reader == "count_le":
                assert _host(out["cum"], U64).tobytes() == le["cum"].tobytes() and _host(out["total"], U64).tobytes() == le["total"].tobytes()
            else:
                _same_sp(sback, c.M, npct, sp, tuple(SP_FIELDS), (kind, "closed at once"))
