"""lh_kept_series* and lh_kept_heat* (Kept.series, Kept.heat, KeptWindow.series / heat): lh_kept_across' and lh_kept_count_le's
outputs per WINDOW of a list of kept intervals, in one call.

On the crafted fixture of tests/test_gpu_kept.py (70 names x 6 handles, engines of 64- and of 32-bit cells), under both kernel
shapes (lh_tool_kept_switch, which here takes the ENTRIES of a call).  Two references per window [lo, hi):
  the model      Python integers over the recorded rows of the slice: test_gpu_kept.check64 as it stands for series (integers
                 exact, sum within 1e-12 x the sum of |terms|), test_gpu_kept_readers.want_cum exact modulo 2^64 for heat
  the readers    Kept.across / Kept.count_le over the slice: every array byte-equal (tobytes), sum included; present_bits after
                 the shift by lo
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import numpy as np
import pytest

from loghisto_amd import _native as N
from tests.test_gpu_across import P_MAIN
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import BIG, FIELDS, K, LISTS, PER_P, check64, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_readers import bound_sets, cells_of, want_cum  # noqa: F401

pytestmark = pytest.mark.gpu

U64 = np.uint64
KINDS = ("wave", "block")
HEAT_FIELDS = dict(cum=U64, total=U64)
WINDOWS = {
    "singletons": [(i, i + 1) for i in range(K)],
    "whole": [(0, K)],
    "halves": [(0, 3), (3, 6)],
    "rolling": [(i, i + 2) for i in range(K - 1)],
    "repeated": [(2, 5), (0, 1), (2, 5)],
}
BIG_LIST, BIG_WINDOWS = [BIG, BIG, 0, 1], [(0, 2), (1, 3), (0, 4)]
CASES = [(list(range(K)), w, name) for name, w in WINDOWS.items()] + [(BIG_LIST, BIG_WINDOWS, "big")]
assert list(range(K)) in LISTS and [BIG, BIG] in LISTS


def series(c, lst, windows, P=P_MAIN, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].series(P, [c.kept[i] for i in lst[:-1]], windows, c.M - first if nmetrics is None else nmetrics, first, **kw)


def heat(c, lst, windows, bounds, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].heat(bounds, [c.kept[i] for i in lst[:-1]], windows, c.M - first if nmetrics is None else nmetrics, first, **kw)


def across(c, lst, P=P_MAIN, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].across([c.kept[i] for i in lst[:-1]], P, c.M - first if nmetrics is None else nmetrics, first, **kw)


def count_le(c, lst, bounds, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].count_le(bounds, [c.kept[i] for i in lst[:-1]], c.M - first if nmetrics is None else nmetrics, first, **kw)


def shifted(ref, lo):
    """a slice call's arrays as the window's block holds them: present_bits speaks of the whole list"""
    return dict(ref, present_bits=ref["present_bits"] << U64(lo)) if "present_bits" in ref else ref


def same_block(got, w, ref, fields, what):
    for f in fields:
        assert np.ascontiguousarray(got[f][w]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), (what, w, f)


# ---- 1. against the model, and against the parent's readers -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_series_every_window_set(crafted, kind):
    c = crafted
    with shape(kind):
        for lst, windows, name in CASES:
            got = series(c, lst, windows)
            assert got["count"].shape == (len(windows), c.M) and got["pkeys"].shape == (len(windows), c.M, len(P_MAIN)), name
            assert got["avg"].shape == (len(windows), c.M) and got["pvals"].shape == got["pkeys"].shape, name
            for w, (lo, hi) in enumerate(windows):
                sl = lst[lo:hi]
                block = {f: v[w] for f, v in got.items()}                                     # avg and pvals too
                assert not np.any(block["present_bits"] & U64((1 << lo) - 1)), (name, w)      # no bit below the window
                assert not np.any(block["present_bits"] >> U64(hi)), (name, w)                # ... or at and above its end
                check64(dict(block, present_bits=block["present_bits"] >> U64(lo)), c.want(sl), P_MAIN, (kind, name, w))
                same_block(got, w, shifted(across(c, sl), lo), FIELDS, (kind, name))


@pytest.mark.parametrize("kind", KINDS)
def test_heat_every_window_set(crafted, kind):
    c = crafted
    sets = bound_sets(c.T)
    with shape(kind):
        for lst, windows, name in CASES:
            for bname in ("main", "nb64") if name in ("rolling", "big") else ("main",):
                bounds = sets[bname]
                got = heat(c, lst, windows, bounds)
                assert got["cum"].dtype == U64 and got["cum"].shape == (len(windows), c.M, len(bounds)), name
                assert got["total"].shape == (len(windows), c.M), name
                for w, (lo, hi) in enumerate(windows):
                    sl = lst[lo:hi]
                    cum, total = want_cum(c, sl, bounds, bname)                              # exact, modulo 2^64
                    assert [[int(x) for x in r] for r in got["cum"][w]] == cum, (kind, name, bname, w)
                    assert [int(x) for x in got["total"][w]] == total, (kind, name, bname, w)
                    same_block(got, w, count_le(c, sl, bounds), HEAT_FIELDS, (kind, name, bname))


def test_the_two_shapes_give_identical_bytes(crafted):
    c = crafted
    bounds = bound_sets(c.T)["main"]
    for lst, windows, name in CASES:
        res = {}
        for kind in KINDS:
            with shape(kind):
                res[kind] = (series(c, lst, windows), heat(c, lst, windows, bounds))
        for f in FIELDS:
            assert res["wave"][0][f].tobytes() == res["block"][0][f].tobytes(), (name, f)
        for f in HEAT_FIELDS:
            assert res["wave"][1][f].tobytes() == res["block"][1][f].tobytes(), (name, f)


# ---- 2. rows, ids, device forms, refusals -------------------------------------------------------------------------------------
def _series_out(torch, n, np_, pad=3):
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int64, pkeys=torch.int16,
                 pvalid=torch.uint8)
    back = {k: torch.full(((n + pad) * (np_ if k in PER_P else 1),), 77, dtype=kinds[k], device="cuda") for k in FIELDS}
    return back, {k: back[k][:n * (np_ if k in PER_P else 1)] for k in FIELDS}


def _heat_out(torch, n, nb, pad=3):
    back = dict(cum=torch.full(((n + pad) * nb,), 77, dtype=torch.int64, device="cuda"),
                total=torch.full((n + pad,), 77, dtype=torch.int64, device="cuda"))
    return back, dict(cum=back["cum"][:n * nb], total=back["total"][:n])


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _same_device(back, fields, want, per, what):
    """the device arrays hold want (window-major) and the sentinel behind it"""
    for k, dt in fields.items():
        h, w = _host(back[k], dt), np.ascontiguousarray(want[k])
        assert h[:w.size].tobytes() == w.tobytes(), (what, k)
        assert h.size == w.size + 3 * per.get(k, 1) and np.all(h[w.size:] == 77), (what, k)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_ids_and_device_forms(crafted, kind):
    import loghisto_amd
    c, torch, lst = crafted, crafted.torch, list(range(K))
    windows = WINDOWS["rolling"] + WINDOWS["repeated"]
    nw = len(windows)
    bounds = bound_sets(c.T)["main"]
    nb, npct = len(bounds), len(P_MAIN)
    ids = [c.at["edges"], 0, c.M - 1, c.at["dense300"], 0, c.at["eight_tiles"], 5, 4, 3, c.at["edges"], c.at["never"], c.at["far_apart"]]
    st = torch.cuda.Stream()
    with shape(kind):
        se, he = series(c, lst, windows), heat(c, lst, windows, bounds)
        # a sub-block
        part, hpart = series(c, lst, windows, nmetrics=9, first=7), heat(c, lst, windows, bounds, nmetrics=9, first=7)
        assert part["count"].shape == (nw, 9) and hpart["cum"].shape == (nw, 9, nb)
        for w, (lo, hi) in enumerate(windows):
            same_block(part, w, shifted(across(c, lst[lo:hi], nmetrics=9, first=7), lo), FIELDS, (kind, "first=7"))
            same_block(hpart, w, count_le(c, lst[lo:hi], bounds, nmetrics=9, first=7), HEAT_FIELDS, (kind, "first=7"))
        for f in FIELDS:
            assert part[f].tobytes() == np.ascontiguousarray(se[f][:, 7:16]).tobytes(), f
        # a host id list: permuted, repeated
        gse, ghe = series(c, lst, windows, ids=ids), heat(c, lst, windows, bounds, ids=ids)
        assert gse["count"].shape == (nw, len(ids)) and ghe["cum"].shape == (nw, len(ids), nb)
        for w, (lo, hi) in enumerate(windows):
            same_block(gse, w, shifted(across(c, lst[lo:hi], ids=ids), lo), FIELDS, (kind, "ids"))
            same_block(ghe, w, count_le(c, lst[lo:hi], bounds, ids=ids), HEAT_FIELDS, (kind, "ids"))
        for f in FIELDS:
            assert gse[f].tobytes() == np.ascontiguousarray(se[f][:, ids]).tobytes(), f
        assert series(c, lst, windows, ids=[])["count"].shape == (nw, 0) and heat(c, lst, windows, bounds, ids=[])["total"].shape == (nw, 0)
        # device forms on a caller's stream: rows, then device ids with some beyond every block
        back, out = _series_out(torch, nw * c.M, npct)
        hback, hout = _heat_out(torch, nw * c.M, nb)
        torch.cuda.synchronize()
        assert series(c, lst, windows, out=out, stream=st)["sum"] is out["sum"]
        assert heat(c, lst, windows, bounds, out=hout, stream=st)["cum"] is hout["cum"]
        st.synchronize()
        _same_device(back, FIELDS, se, {k: npct for k in PER_P}, (kind, "device form"))
        _same_device(hback, HEAT_FIELDS, he, dict(cum=nb), (kind, "device form"))
        for w, (lo, hi) in enumerate(windows):                                   # ... against the parent's device form
            ref = {k: torch.full((c.M, npct) if k in PER_P else (c.M,), 77, dtype=out[k].dtype, device="cuda") for k in FIELDS}
            across(c, lst[lo:hi], out=ref, stream=st)
            st.synchronize()
            same_block({f: _host(out[f], FIELDS[f]).reshape(nw, -1) for f in FIELDS}, w,
                       shifted({f: _host(ref[f], FIELDS[f]).reshape(-1) for f in FIELDS}, lo), FIELDS, (kind, "device forms"))
        bad = {2: c.M, 6: c.M + 1000, 9: 0xffffffff}
        dids = [bad.get(j, i) for j, i in enumerate(ids)]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(dids, dtype=torch.int64, device="cuda").to(torch.int32)
        back, out = _series_out(torch, nw * len(ids), npct)
        hback, hout = _heat_out(torch, nw * len(ids), nb)
        torch.cuda.synchronize()
        series(c, lst, windows, ids=d_ids, out=out, stream=st)
        heat(c, lst, windows, bounds, ids=d_ids, out=hout, stream=st)
        st.synchronize()

        def zero(a):
            a = a.copy()
            a[:, list(bad)] = 0
            return a
        _same_device(back, FIELDS, {k: zero(gse[k]) for k in FIELDS}, {k: npct for k in PER_P}, (kind, "device ids"))
        _same_device(hback, HEAT_FIELDS, {k: zero(ghe[k]) for k in HEAT_FIELDS}, dict(cum=nb), (kind, "device ids"))
        # a host id outside any listed handle, or rows beyond it: LH_ERANGE, nothing written
        for kw in (dict(ids=[0, c.M, 1]), dict(ids=[0xffffffff]), dict(nmetrics=c.M + 1), dict(nmetrics=1, first=c.M)):
            n = len(kw["ids"]) if "ids" in kw else kw["nmetrics"]
            o = {k: np.full((nw, n, npct) if k in PER_P else (nw, n), 7, dtype=t) for k, t in FIELDS.items()}
            ho = dict(cum=np.full((nw, n, nb), 7, dtype=U64), total=np.full((nw, n), 7, dtype=U64))
            for call, arrays in ((lambda: series(c, lst, windows, out=o, **kw), o), (lambda: heat(c, lst, windows, bounds, out=ho, **kw), ho)):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    call()
                assert ei.value.code == N.ERANGE, kw
                assert all(np.all(v == 7) for v in arrays.values()), kw


@pytest.mark.parametrize("kind", KINDS)
def test_a_shorter_handle_empties_only_the_windows_that_hold_it(crafted, kind):
    """A device id one past the block of a shorter handle gives the empty entry in exactly the windows that contain the handle; a
    host id there, or rows beyond it, are refused whether or not a window names the handle."""
    import loghisto_amd
    c, torch = crafted, crafted.torch
    bounds = bound_sets(c.T)["main"]
    nb, npct = len(bounds), len(P_MAIN)
    end = c.at["eight_tiles"]                                                    # a name every handle holds cells of
    short = c.kept[1].merge(nmetrics=end, first=0)                               # rows 0 .. end - 1 of handle 1
    try:
        kept = [c.kept[0], short, c.kept[2], c.kept[3]]                          # the list; `short` at position 1
        windows = [(0, 1), (0, 2), (1, 2), (2, 4), (1, 4), (3, 4)]
        holds = [lo <= 1 < hi for lo, hi in windows]
        some = [end - 1, end, 3, end]                                            # end: one past the short handle's block
        with shape(kind):
            full = {lohi: (kept[lohi[1] - 1].across(kept[lohi[0]:lohi[1] - 1], P_MAIN, ids=[end - 1, 3]),
                           kept[lohi[1] - 1].count_le(bounds, kept[lohi[0]:lohi[1] - 1], ids=[end - 1, 3])) for lohi in windows}
            wide = {lohi: (kept[lohi[1] - 1].across(kept[lohi[0]:lohi[1] - 1], P_MAIN, ids=some),
                           kept[lohi[1] - 1].count_le(bounds, kept[lohi[0]:lohi[1] - 1], ids=some)) for lohi, h in zip(windows, holds) if not h}
            d_ids = torch.tensor(some, dtype=torch.int32, device="cuda")
            back, out = _series_out(torch, len(windows) * 4, npct)
            hback, hout = _heat_out(torch, len(windows) * 4, nb)
            torch.cuda.synchronize()
            kept[-1].series(P_MAIN, kept[:-1], windows, ids=d_ids, out=out)
            kept[-1].heat(bounds, kept[:-1], windows, ids=d_ids, out=hout)
            torch.cuda.synchronize()
            for w, (lohi, h) in enumerate(zip(windows, holds)):
                for fields, o, which, per in ((FIELDS, out, 0, npct), (HEAT_FIELDS, hout, 1, nb)):
                    for f, dt in fields.items():
                        got = _host(o[f], dt).reshape(len(windows), 4, -1)[w]
                        if h:                                                    # entries 1 and 3 empty, 0 and 2 the slice's
                            ref = full[lohi][which][f].reshape(2, -1)
                            ref = ref << U64(lohi[0]) if f == "present_bits" else ref
                            assert got[0].tobytes() == ref[0].tobytes() and got[2].tobytes() == ref[1].tobytes(), (kind, w, f)
                            assert not got[1].any() and not got[3].any(), (kind, w, f)
                        else:
                            ref = wide[lohi][which][f].reshape(4, -1)
                            ref = ref << U64(lohi[0]) if f == "present_bits" else ref
                            assert got.tobytes() == ref.tobytes(), (kind, w, f)
            assert all(_host(out["count"], U64).reshape(len(windows), 4)[w, 1] for w, h in enumerate(holds) if not h)
            # on the host: refused even for windows that leave the short handle out
            for kw in (dict(ids=some), dict(nmetrics=end + 1), dict(nmetrics=1, first=end)):
                n = len(kw["ids"]) if "ids" in kw else kw["nmetrics"]
                o = {k: np.full((2, n, npct) if k in PER_P else (2, n), 7, dtype=t) for k, t in FIELDS.items()}
                ho = dict(cum=np.full((2, n, nb), 7, dtype=U64), total=np.full((2, n), 7, dtype=U64))
                for call, arrays in ((lambda: kept[-1].series(P_MAIN, kept[:-1], [(0, 1), (2, 4)], out=o, **kw), o),
                                     (lambda: kept[-1].heat(bounds, kept[:-1], [(0, 1), (2, 4)], out=ho, **kw), ho)):
                    with pytest.raises(loghisto_amd.LhError) as ei:
                        call()
                    assert ei.value.code == N.ERANGE, kw
                    assert all(np.all(v == 7) for v in arrays.values()), kw
    finally:
        short.close()


# ---- 3. the limits: 64 handles, 128 windows -----------------------------------------------------------------------------------
def test_64_handles_and_128_windows(native_lib, torch_cuda):
    M, n, k = 3, 300, 64
    rng = np.random.default_rng(6400)
    bounds = [1.0, 10.0, 20.0, 50.0, 1e3]
    kept = []
    with engine(M, cell_bits=64, num_buffers=2) as e:
        for i in range(k):
            ids = rng.integers(0, M, n).astype(np.uint32)
            e.submit_pairs(ids[ids != i % 5], rng.lognormal(3.0 + 0.01 * i, 1.0, n)[ids != i % 5])   # a name missing from most
            with e.flip() as s:
                kept.append(s.keep(M))
    try:
        windows = [(i, i + 1) for i in range(k)] + [(i, min(i + 7, k)) for i in range(k)]
        assert len(windows) == N.MAX_WINDOWS
        res = {}
        for kind in KINDS:
            with shape(kind):
                se, he = kept[-1].series(P_MAIN, kept[:-1], windows), kept[-1].heat(bounds, kept[:-1], windows)
                assert se["count"].shape == (128, M) and he["cum"].shape == (128, M, len(bounds))
                for w, (lo, hi) in enumerate(windows):
                    same_block(se, w, shifted(kept[hi - 1].across(kept[lo:hi - 1], P_MAIN), lo), FIELDS, (kind, "64 x 128"))
                    same_block(he, w, kept[hi - 1].count_le(bounds, kept[lo:hi - 1]), HEAT_FIELDS, (kind, "64 x 128"))
                res[kind] = se
                none = kept[-1].series(P_MAIN, kept[:-1])                        # windows=None: one per handle
                for f in FIELDS:
                    assert none[f].tobytes() == np.ascontiguousarray(se[f][:k]).tobytes(), f
        assert int(res["wave"]["present_bits"][63, 0]) in (0, 1 << 63) and res["wave"]["count"].sum() > 0.5 * k * n
        for f in FIELDS:
            assert res["wave"][f].tobytes() == res["block"][f].tobytes(), f
        with pytest.raises(ValueError):
            kept[-1].series(P_MAIN, kept[:-1], [(0, -1)])
    finally:
        for kk in kept:
            kk.close()


# ---- 4. lifetime ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_close_right_after_a_device_form_call_waits_for_it(crafted, kind):
    c, torch = crafted, crafted.torch
    bounds = bound_sets(c.T)["nb64"]
    nb, npct = len(bounds), len(P_MAIN)
    lst, windows = [0, 1, 2, BIG], [(0, 4), (1, 3), (3, 4), (0, 1)]
    nw = len(windows)
    with shape(kind):
        se, he = series(c, lst, windows), heat(c, lst, windows, bounds)
        for reader in ("series", "heat"):
            fresh = [c.kept[i].merge() for i in lst]                             # the same cells in handles to be closed at once
            st = torch.cuda.Stream()
            back, out = _series_out(torch, nw * c.M, npct)
            hback, hout = _heat_out(torch, nw * c.M, nb)
            torch.cuda.synchronize()
            if reader == "series":
                fresh[-1].series(P_MAIN, fresh[:-1], windows, c.M, out=out, stream=st)
            else:
                fresh[-1].heat(bounds, fresh[:-1], windows, c.M, out=hout, stream=st)
            for k_ in fresh:
                k_.close()                                                       # waits for the enqueued kernel
            st.synchronize()
            if reader == "series":
                _same_device(back, FIELDS, se, {k: npct for k in PER_P}, (kind, "closed at once"))
            else:
                _same_device(hback, HEAT_FIELDS, he, dict(cum=nb), (kind, "closed at once"))


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------------
def test_window_class_and_lines(native_lib, torch_cuda):
    import loghisto_amd
    torch = torch_cuda
    M, n = 12, 4000
    rng = np.random.default_rng(12)
    bounds = [5.0, 20.0, 100.0]
    with engine(M, cell_bits=64, num_buffers=2) as e, loghisto_amd.KeptWindow(3) as win:
        for m in range(M):
            assert e.intern(f"svc_{m}") == m
        kept = []
        for i in range(4):                                                       # 4 pushes into a window of 3
            ids = rng.integers(0, M - 1, n).astype(np.uint32)                    # the last name stays empty
            e.submit_pairs(ids, rng.lognormal(2.0 + 0.3 * i, 1.0, n))
            with e.flip() as s:
                kept.append(s.keep(M))
            old = win.push(kept[-1])
            assert (old is kept[0]) == (i == 3)
        handles = list(win.handles)
        assert handles == kept[1:]
        for windows in (None, [(0, 3), (1, 3), (2, 3)]):
            a, b = win.series(P_MAIN, windows), handles[-1].series(P_MAIN, handles[:-1], windows)
            assert set(a) == set(FIELDS) | {"avg", "pvals"} and a["count"].shape == (3, M)
            for f in FIELDS:
                assert a[f].tobytes() == b[f].tobytes(), f
            a, b = win.heat(bounds, windows), handles[-1].heat(bounds, handles[:-1], windows)
            assert set(a) == {"cum", "total"} and a["cum"].shape == (3, M, 3) and a["total"].shape == (3, M)
            assert a["cum"].tobytes() == b["cum"].tobytes() and a["total"].tobytes() == b["total"].tobytes()
        whole = win.series(P_MAIN, [(0, 3)], ids=[3, 1])                          # the window's total holds the same cells
        tot = win.total.across((), P_MAIN, ids=[3, 1])
        assert whole["count"][0].tobytes() == tot["count"].tobytes() and whole["pkeys"][0].tobytes() == tot["pkeys"].tobytes()
        # window w's device block of cum is a column lh_lines takes as it is
        windows = [(0, 2), (1, 3)]
        cum = torch.full((2, M, 3), 77, dtype=torch.int64, device="cuda")
        total = torch.full((2, M), 77, dtype=torch.int64, device="cuda")
        win.heat(bounds, windows, out=dict(cum=cum.view(-1), total=total.view(-1)))
        with e.device_names() as names:
            for w, (lo, hi) in enumerate(windows):
                rcum = torch.full((M, 3), 77, dtype=torch.int64, device="cuda")
                rtotal = torch.full((M,), 77, dtype=torch.int64, device="cuda")
                handles[hi - 1].count_le(bounds, handles[lo:hi - 1], out=dict(cum=rcum.view(-1), total=rtotal))
                spec = lambda cu, to: [dict(label="%s_le_" + "%g" % b, a=cu[:, j]) for j, b in enumerate(bounds)] + \
                    [dict(label="%s_le_+Inf", a=to)]                             # noqa: E731
                got = names.lines(spec(cum[w], total[w]), row_count=total[w], sep=" ", suffix="\n")
                want = names.lines(spec(rcum, rtotal), row_count=rtotal, sep=" ", suffix="\n")
                assert got == want and got.count(b"\n") == (M - 1) * 4 and b"svc_0_le_5 " in got, w
        for k_ in kept:
            k_.close()
