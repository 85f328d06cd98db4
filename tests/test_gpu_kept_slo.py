"""GPU tests of lh_kept_slo* and lh_kept_burn*: lh_kept_heat* with a row of bounds PER NAME, and the multi-window burn-rate alert.
slo runs on the crafted fixture of tests/test_gpu_kept.py (70 names x 6 handles, engines of 64- and of 32-bit cells, the BIG list)
with the window sets of tests/test_gpu_kept_series.py under both kernel shapes: every entry against the Python-integer model on the
row's own bounds (want_cum) and byte for byte against Kept.heat with that row for that name; rows, ids and device forms; device
arrays the host never sees (an id outside a block, a NaN, a decreasing row).  burn runs on a small engine built here, so that ties
exist by construction: total 1024 and bad 256 against a budget of 0.25 and of the double just below it."""
import ctypes as C
import types

import numpy as np
import pytest

import loghisto_amd
from loghisto_amd import _native as N
from tests.test_gpu_compare import _import
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import K, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_readers import bound_sets, value_of, want_cum
from tests.test_gpu_kept_series import CASES, KINDS, WINDOWS, _heat_out, _host, _same_device, heat

pytestmark = pytest.mark.gpu

U64 = np.uint64
INF = float("inf")
V = 4                      # name m takes variant m % V of a set's rows: neighbouring names differ
SLO_FIELDS = dict(cum=U64, total=U64)


def row_sets(T):
    """name -> V sorted rows of bounds of one length, drawn from bound_sets: +-Inf, -0.0, values beyond the int16 key range (1e200),
    equal neighbours; nb = 1, len(main) and 64."""
    sets = bound_sets(T)
    pool = sets["main"] + sets["nb64"]
    rng = np.random.default_rng(7)
    out = {"one": [[INF], [-0.0], list(sets["one"]), [1e200]]}
    for name in ("main", "nb64"):
        rows = [list(sets[name])]
        while len(rows) < V:
            rows.append(sorted(float(x) for x in rng.choice(pool, len(sets[name]))))
        out[name] = rows
    assert all(len(v) == V and len({tuple(r) for r in v}) == V for v in out.values())
    return out


def rows_of(variants, n):
    return np.array([variants[m % V] for m in range(n)], dtype=np.float64)


def slo(c, lst, windows, bounds, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].slo(bounds, [c.kept[i] for i in lst[:-1]], windows, c.M - first if nmetrics is None else nmetrics, first, **kw)


def model(c, sl, variants, name, rows):
    """(cum[n][nb], total[n]) for entry j = name rows[j] with variant j % V, as Python integers"""
    per = [want_cum(c, sl, variants[v], f"slo:{name}:{v}") for v in range(V)]
    return [per[j % V][0][m] for j, m in enumerate(rows)], [per[0][1][m] for m in rows]


def same(got, ref, what):
    for f in SLO_FIELDS:
        assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), (what, f)


# ---- 1. every window set against the model and against heat, in both shapes ---------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_slo_every_window_set(crafted, kind):
    c = crafted
    sets = row_sets(c.T)
    with shape(kind):
        for lst, windows, name in CASES:
            for bname in ("main", "nb64", "one") if name in ("rolling", "big") else ("main",):
                variants = sets[bname]
                nb = len(variants[0])
                got = slo(c, lst, windows, rows_of(variants, c.M))
                assert got["cum"].dtype == U64 and got["cum"].shape == (len(windows), c.M, nb), (name, bname)
                assert got["total"].dtype == U64 and got["total"].shape == (len(windows), c.M), (name, bname)
                for w, (lo, hi) in enumerate(windows):
                    cum, total = model(c, lst[lo:hi], variants, bname, range(c.M))           # exact, modulo 2^64
                    assert [[int(x) for x in r] for r in got["cum"][w]] == cum, (kind, name, bname, w)
                    assert [int(x) for x in got["total"][w]] == total, (kind, name, bname, w)
                # byte for byte heat with the row for the name: all names that have variant v in ONE heat call by id ...
                for v in range(V):
                    ids = list(range(v, c.M, V))
                    same({f: got[f][:, ids] for f in SLO_FIELDS}, heat(c, lst, windows, variants[v], ids=ids), (kind, name, bname, v))
                # ... and, as the contract says it, one name and its one row a call
                if bname == "main" and name in ("rolling", "big"):
                    for m in (c.at["edges"], c.at["far_apart"], c.at["total_2^64-1"], c.at["half_of_2^64"], c.M - 1, 0):
                        ref = heat(c, lst, windows, variants[m % V], ids=[m])
                        same({f: got[f][:, m:m + 1] for f in SLO_FIELDS}, ref, (kind, name, m))
    # a 1-D bounds array is one bound a name
    one = slo(c, list(range(K)), WINDOWS["halves"], np.array([sets["one"][m % V][0] for m in range(c.M)]))
    same(one, slo(c, list(range(K)), WINDOWS["halves"], rows_of(sets["one"], c.M)), "1-D")
    assert one["cum"].shape == (2, c.M, 1)


def test_the_two_shapes_give_identical_bytes(crafted):
    c = crafted
    sets = row_sets(c.T)
    for lst, windows, name in CASES:
        for bname in ("main", "one"):
            res = {}
            for kind in KINDS:
                with shape(kind):
                    res[kind] = slo(c, lst, windows, rows_of(sets[bname], c.M))
            same(res["wave"], res["block"], (name, bname))


# ---- 2. rows, ids, device forms, device arrays the host never sees ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_slo_rows_ids_and_device_forms(crafted, kind):
    c, torch, lst = crafted, crafted.torch, list(range(K))
    windows = WINDOWS["rolling"] + WINDOWS["repeated"]
    nw = len(windows)
    variants = row_sets(c.T)["main"]
    nb = len(variants[0])
    ids = [c.at["edges"], 0, c.M - 1, c.at["dense300"], 0, c.at["eight_tiles"], 5, 4, 3, c.at["edges"], c.at["never"], c.at["far_apart"]]
    st = torch.cuda.Stream()

    def against_model(got, rows, what):
        for w, (lo, hi) in enumerate(windows):
            cum, total = model(c, lst[lo:hi], variants, "main", rows)
            assert [[int(x) for x in r] for r in got["cum"][w]] == cum and [int(x) for x in got["total"][w]] == total, (kind, what, w)

    with shape(kind):
        # rows with first > 0: entry j is name 7 + j with ROW j of the call's bounds
        part = slo(c, lst, windows, rows_of(variants, 9), nmetrics=9, first=7)
        assert part["cum"].shape == (nw, 9, nb) and part["total"].shape == (nw, 9)
        against_model(part, range(7, 16), "first=7")
        for v in range(V):
            js = list(range(v, 9, V))
            same({f: part[f][:, js] for f in SLO_FIELDS}, heat(c, lst, windows, variants[v], ids=[7 + j for j in js]), (kind, "first=7", v))
        # a host id list: arbitrary order, repeats -- a repeated name meets another row of bounds each time
        by_id = slo(c, lst, windows, rows_of(variants, len(ids)), ids=ids)
        assert by_id["cum"].shape == (nw, len(ids), nb)
        against_model(by_id, ids, "ids")
        for v in range(V):
            js = list(range(v, len(ids), V))
            same({f: by_id[f][:, js] for f in SLO_FIELDS}, heat(c, lst, windows, variants[v], ids=[ids[j] for j in js]), (kind, "ids", v))
        assert slo(c, lst, windows, np.zeros((0, nb)), ids=[])["total"].shape == (nw, 0)
        # device forms on a caller's stream, padded outputs: rows, then device ids with some outside every block
        whole = slo(c, lst, windows, rows_of(variants, c.M))
        with torch.cuda.stream(st):
            d_rows = torch.tensor(rows_of(variants, c.M), dtype=torch.float64, device="cuda")
            d_few = torch.tensor(rows_of(variants, len(ids)), dtype=torch.float64, device="cuda")
        back, out = _heat_out(torch, nw * c.M, nb)
        torch.cuda.synchronize()
        assert slo(c, lst, windows, d_rows, out=out, stream=st)["cum"] is out["cum"]
        st.synchronize()
        _same_device(back, SLO_FIELDS, whole, dict(cum=nb), (kind, "device form"))
        bad = {2: c.M, 6: c.M + 1000, 9: 0xffffffff}
        with torch.cuda.stream(st):
            d_ids = torch.tensor([bad.get(j, i) for j, i in enumerate(ids)], dtype=torch.int64, device="cuda").to(torch.int32)
        back, out = _heat_out(torch, nw * len(ids), nb)
        torch.cuda.synchronize()
        slo(c, lst, windows, d_few, ids=d_ids, out=out, stream=st)
        st.synchronize()

        def zero(a):
            a = a.copy()
            a[:, list(bad)] = 0
            return a
        _same_device(back, SLO_FIELDS, {k: zero(by_id[k]) for k in SLO_FIELDS}, dict(cum=nb), (kind, "device ids"))
        # a device array is any bytes: a NaN takes in nothing, a decreasing row is answered bound by bound -- every column against
        # ONE-bound host calls (a NaN's column entry: -Inf, which takes in nothing either)
        rows = rows_of(variants, c.M)
        rows[3, 2] = rows[c.at["edges"], 0] = rows[c.M - 1, nb - 1] = np.nan
        rows[5] = rows[5][::-1]
        rows[c.at["dense300"]] = rows[c.at["dense300"]][::-1]
        rows[11, [4, 9]] = rows[11, [9, 4]]
        assert rows[5, 0] > rows[5, -1]
        with torch.cuda.stream(st):
            d_any = torch.tensor(rows, dtype=torch.float64, device="cuda")
        back, out = _heat_out(torch, nw * c.M, nb)
        torch.cuda.synchronize()
        slo(c, lst, windows, d_any, out=out, stream=st)
        st.synchronize()
        got = _host(out["cum"], U64).reshape(nw, c.M, nb)
        for m, j in ((3, 2), (c.at["edges"], 0), (c.M - 1, nb - 1)):
            assert not got[:, m, j].any(), (kind, "NaN", m, j)
        for j in range(nb):
            col = np.where(np.isnan(rows[:, j]), -INF, rows[:, j])
            ref = slo(c, lst, windows, col)
            assert got[:, :, j].tobytes() == np.ascontiguousarray(ref["cum"][:, :, 0]).tobytes(), (kind, "bound by bound", j)
            assert _host(out["total"], U64).tobytes() == ref["total"].tobytes(), (kind, j)
        assert np.all(_host(back["cum"], U64)[nw * c.M * nb:] == 77) and np.all(_host(back["total"], U64)[nw * c.M:] == 77)
        # host rows are checked: a NaN or a decreasing row in the LAST row is LH_EINVAL; rows outside a block LH_ERANGE; nothing written
        o = dict(cum=np.full((nw, c.M, nb), 7, dtype=U64), total=np.full((nw, c.M), 7, dtype=U64))
        for r in (3, c.M - 1):
            for fix in (lambda a: a.__setitem__((r, 2), np.nan), lambda a: a.__setitem__(r, a[r][::-1].copy())):
                hostile = rows_of(variants, c.M)
                fix(hostile)
                with pytest.raises(loghisto_amd.LhError) as ei:
                    slo(c, lst, windows, hostile, out=o)
                assert ei.value.code == N.EINVAL, r
        with pytest.raises(loghisto_amd.LhError) as ei:
            slo(c, lst, windows, rows_of(variants, 3), ids=[0, c.M, 1], out={k: v[:, :3].copy() for k, v in o.items()})
        assert ei.value.code == N.ERANGE
        assert all(np.all(v == 7) for v in o.values())


# ---- 3. burn: ties by construction -----------------------------------------------------------------------------------------------
NAMES = ("tie", "fires", "short_only", "long_only", "empty_in_short", "never", "all_bad", "fires_too", "no_bad", "fires_three")


@pytest.fixture(scope="module")
def alerts(native_lib, torch_cuda):
    """Three handles of ten names.  bound = value_of(1000) takes in bins 0 .. 1000: `good` samples lie in bin 900, `bad` ones in
    bin 1100.  Windows: short = the last handle, long = all three.  Every cell is a power of two, so every total is 1024 or a
    small multiple and rate * budget * total is exact where the tests need a tie."""
    def cells(total, bad):
        return {b: v for b, v in ((900, total - bad), (1100, bad)) if v}
    #                       handle 0          handle 1         handle 2 (the short window)
    per = dict(tie=[cells(1024, 256), cells(1024, 256), cells(1024, 256)],           # 1/4 bad everywhere
               fires=[cells(1024, 256), cells(1024, 256), cells(1024, 256)],         # the same cells, a budget just below 1/4
               short_only=[cells(1024, 0), cells(1024, 0), cells(1024, 512)],        # short 1/2; long 512 / 3072 = 1/6
               long_only=[cells(1024, 1024), cells(1024, 1024), cells(1024, 128)],   # short 1/8; long 2176 / 3072
               empty_in_short=[cells(1024, 1024), cells(1024, 1024), {}],            # no sample in the short window
               never=[{}, {}, {}],
               all_bad=[cells(8, 8), {}, cells(2, 2)],
               fires_too=[cells(1024, 512), cells(1024, 512), cells(1024, 512)],
               no_bad=[cells(1024, 0), cells(1024, 0), cells(1024, 0)],
               fires_three=[cells(4096, 2048), cells(2048, 2048), cells(1024, 1024)])
    M = len(NAMES)
    kept = []
    with engine(M, cell_bits=64, num_buffers=2) as e:
        for i in range(3):
            with e.flip() as s:
                rows = [per[n][i] for n in NAMES]
                _import(s, rows, ["tight" if r else None for r in rows])
                kept.append(s.keep(M))
        bound = value_of(1000)
        below = float(np.nextafter(0.25, 0.0))
        budget = dict(tie=0.25, fires=below, short_only=0.25, long_only=0.25, empty_in_short=0.25, never=0.0, all_bad=0.5, fires_too=0.25,
                      no_bad=0.0, fires_three=0.25)
        yield types.SimpleNamespace(kept=kept, M=M, torch=torch_cuda, windows=[(2, 3), (0, 3)], rates=[1.0, 1.0],
                                    bounds=np.full(M, bound), budget=np.array([budget[n] for n in NAMES]),
                                    reported=[NAMES.index(n) for n in ("fires", "all_bad", "fires_too", "fires_three")])
    for k in kept:
        k.close()


def burn(a, k, **kw):
    kw.setdefault("windows", a.windows)
    kw.setdefault("rates", a.rates)
    bounds, budget, rates = kw.pop("bounds", a.bounds), kw.pop("budget", a.budget), kw.pop("rates")
    return a.kept[-1].burn(bounds, budget, rates, k, a.kept[:-1], **kw)


def test_burn_ties_windows_and_k(alerts):
    a = alerts
    at = {n: m for m, n in enumerate(NAMES)}
    res = {}
    for kind in KINDS:
        with shape(kind):
            full = burn(a, a.M, counts=True)
            # the device's decisions are the NumPy rule's on the call's own counts, and the counts are slo's
            fires = loghisto_amd.burn_fires(full["cum"], full["total"], a.budget, a.rates)
            assert np.flatnonzero(fires.all(axis=0)).tolist() == full["entry"].tolist() == a.reported, kind
            assert full["n"] == len(a.reported) and full["row"].tolist() == a.reported and full["entry"].dtype == np.uint32
            ref = a.kept[-1].slo(a.bounds, a.kept[:-1], a.windows)
            assert full["cum"].tobytes() == ref["cum"].tobytes() and full["total"].tobytes() == ref["total"].tobytes(), kind
            assert full["cum"].shape == (2, a.M) and full["total"].shape == (2, a.M)
            # what the fixture was built for
            assert [int(x) for x in full["total"][:, at["tie"]]] == [1024, 3072] and [int(x) for x in full["cum"][:, at["tie"]]] == [768, 2304]
            assert not fires[:, at["tie"]].any() and fires[:, at["fires"]].all()                # a tie does not fire; just below does
            assert fires[:, at["short_only"]].tolist() == [True, False] and fires[:, at["long_only"]].tolist() == [False, True]
            assert fires[:, at["empty_in_short"]].tolist() == [False, True] and int(full["total"][0, at["empty_in_short"]]) == 0
            assert not fires[:, at["never"]].any() and not fires[:, at["no_bad"]].any()
            # k below the number reported: the full count, the first k in ascending m
            for k in (1, 2, 3):
                few = burn(a, k)
                assert few["n"] == len(a.reported) and few["entry"].tolist() == a.reported[:k] and "cum" not in few, (kind, k)
            count_only = burn(a, 0)
            assert count_only["n"] == len(a.reported) and count_only["entry"].size == 0
            # rates: at 2.0 in the long window `fires_too` ties there (1536 against 2 * 0.25 * 3072) and leaves; a zero rate takes
            # every name with a bad sample in both windows
            assert burn(a, a.M, rates=[1.0, 2.0])["entry"].tolist() == [at["fires_three"]]     # (all_bad ties too: 10 against 1.0 * 10)
            assert burn(a, a.M, rates=[0.0, 0.0])["entry"].tolist() == [at[n] for n in ("tie", "fires", "short_only", "long_only",
                                                                                          "all_bad", "fires_too", "fires_three")]
            # one window only: the short one
            short = burn(a, a.M, windows=[(2, 3)], rates=[1.0])
            assert short["entry"].tolist() == [at[n] for n in ("fires", "short_only", "all_bad", "fires_too", "fires_three")]
            res[kind] = (full, short)
    for x, y in zip(res["wave"], res["block"]):
        assert x["n"] == y["n"] and all(x[f].tobytes() == y[f].tobytes() for f in ("entry", "row", "cum", "total") if f in x)


@pytest.mark.parametrize("kind", KINDS)
def test_burn_ids_and_device_forms(alerts, kind):
    a, torch = alerts, alerts.torch
    at = {n: m for m, n in enumerate(NAMES)}
    L = N.lib()
    st = torch.cuda.Stream()
    order = ["fires_too", "tie", "fires", "never", "fires", "long_only", "all_bad", "fires_three", "short_only", "fires"]
    ids = [at[n] for n in order]
    budget = a.budget[ids].copy()
    budget[4] = 0.25                                                   # `fires` again, with the tie's budget this time
    want = [j for j, n in enumerate(order) if n in ("fires_too", "fires", "all_bad", "fires_three") and j != 4]
    with shape(kind):
        got = burn(a, len(ids), ids=ids, bounds=a.bounds[ids], budget=budget, counts=True)
        assert got["entry"].tolist() == want and got["row"].tolist() == [ids[j] for j in want] and got["n"] == len(want)
        fires = loghisto_amd.burn_fires(got["cum"], got["total"], budget, a.rates)
        assert np.flatnonzero(fires.all(axis=0)).tolist() == want
        assert got["cum"].tobytes() == a.kept[-1].slo(a.bounds[ids], a.kept[:-1], a.windows, ids=ids)["cum"].tobytes()
        # the rest of out is left untouched, in the host form (the library's) ...
        hits = np.full(8, 7, dtype=N.BURN_HIT)
        n_out = np.zeros(1, dtype=U64)
        handles, nkept = a.kept[-1]._list(a.kept[:-1])
        win, nwin = a.kept[-1]._windows(a.windows, nkept)
        ida, rates = np.array(ids, dtype=np.uint32), np.array(a.rates)
        b = np.ascontiguousarray(a.bounds[ids])
        N.check(L.lh_kept_burn_ids(C.addressof(handles), nkept, C.addressof(win), nwin, ida.ctypes.data, len(ids), rates.ctypes.data,
                                   b.ctypes.data, budget.ctypes.data, 3, 0, None, hits.ctypes.data, n_out.ctypes.data, None, None), "burn")
        assert int(n_out[0]) == len(want) and hits["entry"][:3].tolist() == want[:3] and np.all(hits["entry"][3:] == 7) and \
            np.all(hits["row"][3:] == 7)
        # ... and in the device form: padded outputs, device bounds, budgets and ids -- one of them outside every block, one budget NaN
        dids = list(ids)
        dids[6] = a.M + 5                                              # all_bad's entry: never fires, the empty entry in cum / total
        dbud = budget.copy()
        dbud[0] = np.nan                                               # fires_too's entry: the comparison is false
        dwant = [j for j in want if j not in (0, 6)]
        for k in (len(ids), 2, 0):
            with torch.cuda.stream(st):
                d_ids = torch.tensor(dids, dtype=torch.int32, device="cuda")
                d_b = torch.tensor(a.bounds[ids], dtype=torch.float64, device="cuda")
                d_g = torch.tensor(dbud, dtype=torch.float64, device="cuda")
                d_hits = torch.full((2 * (len(ids) + 3),), 77, dtype=torch.int32, device="cuda")
                d_n = torch.full((2,), 77, dtype=torch.int64, device="cuda")
                d_cum = torch.full((2 * len(ids) + 3,), 77, dtype=torch.int64, device="cuda")
                d_tot = torch.full((2 * len(ids) + 3,), 77, dtype=torch.int64, device="cuda")
            st.synchronize()
            out = dict(n=d_n[:1], cum=d_cum[:2 * len(ids)], total=d_tot[:2 * len(ids)])
            if k:
                out["hits"] = d_hits[:2 * k]
            assert burn(a, k, ids=d_ids, bounds=d_b, budget=d_g, out=out, stream=st) is out
            st.synchronize()
            h = d_hits.cpu().numpy().view(np.uint32).reshape(-1, 2)
            wrote = min(k, len(dwant))
            assert [int(x) for x in d_n.cpu().numpy()] == [len(dwant), 77], (kind, k)
            assert h[:wrote, 0].tolist() == dwant[:wrote] and h[:wrote, 1].tolist() == [dids[j] for j in dwant[:wrote]], (kind, k)
            assert np.all(h[wrote:] == 77), (kind, k)
            cum, tot = _host(d_cum, U64), _host(d_tot, U64)
            assert np.all(cum[2 * len(ids):] == 77) and np.all(tot[2 * len(ids):] == 77)
            ref_cum, ref_tot = got["cum"].copy(), got["total"].copy()
            ref_cum[:, 6] = ref_tot[:, 6] = 0
            assert cum[:2 * len(ids)].tobytes() == ref_cum.tobytes() and tot[:2 * len(ids)].tobytes() == ref_tot.tobytes(), (kind, k)
        # rows with first > 0, host and device
        part = burn(a, a.M, nmetrics=a.M - 1, first=1, bounds=a.bounds[1:], budget=a.budget[1:])
        assert part["row"].tolist() == a.reported and part["entry"].tolist() == [m - 1 for m in a.reported]
        with torch.cuda.stream(st):
            d_b = torch.tensor(a.bounds[1:], dtype=torch.float64, device="cuda")
            d_g = torch.tensor(a.budget[1:], dtype=torch.float64, device="cuda")
            d_hits = torch.full((2 * a.M,), 77, dtype=torch.int32, device="cuda")
            d_n = torch.zeros((1,), dtype=torch.int64, device="cuda")
        st.synchronize()
        burn(a, a.M, nmetrics=a.M - 1, first=1, bounds=d_b, budget=d_g, out=dict(hits=d_hits, n=d_n), stream=st)
        st.synchronize()
        h = d_hits.cpu().numpy().view(np.uint32).reshape(-1, 2)
        assert int(d_n.item()) == len(a.reported) and h[:len(a.reported), 1].tolist() == a.reported and np.all(h[len(a.reported):] == 77)
    # the rolling window delegates
    w = loghisto_amd.KeptWindow(3)
    w.handles.extend(a.kept)
    assert w.burn(a.bounds, a.budget, a.rates, a.M, windows=a.windows)["entry"].tolist() == a.reported
    assert w.slo(a.bounds, windows=a.windows)["cum"].shape == (2, a.M, 1)
    w.handles.clear()
