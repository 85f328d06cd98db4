"""lh_kept_spread_series* and lh_kept_drift* (Kept.spread_series, Kept.drift, KeptWindow.spread_series / drift): lh_kept_spread's
and lh_kept_compare's outputs per WINDOW of a list of kept intervals, in one call.

On the crafted fixture of tests/test_gpu_kept.py (70 names x 6 handles) and on the compare fixture of
tests/test_gpu_kept_compare.py, each on engines of 64- and of 32-bit cells, under both kernel shapes (lh_tool_kept_switch, which
here takes the ENTRIES of a call).  Two references per window:
  the model      spread: tests/test_gpu_kept_readers.check_spreads over the recorded rows of the slice [lo, hi); drift:
                 tests/test_gpu_compare.model / check over the summed rows of the two slices (counts, key and prefixes exact, ks
                 bit-equal, w1 and shift within that file's bound 4 n 2^-53 (1 + w1)); a side whose total passes 2^64 has no model
  the readers    Kept.spread over the slice, Kept.compare over the two slices: every array byte-equal (tobytes), floats included
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import math

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_across import P_MAIN
from tests.test_gpu_compare import FIELDS as CMP_FIELDS, model
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import BIG, K, LISTS, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_compare import check_rows, kept, models  # noqa: F401  (kept: the compare fixture)
from tests.test_gpu_kept_readers import SP_FIELDS, SP_PER_P, check_spreads
from tests.test_gpu_kept_series import CASES

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
KINDS = ("wave", "block")
ALL = list(range(K))
LIST64 = LISTS[-1]
assert len(LIST64) == 64 and LIST64[:K] == ALL
DRIFT = {                                                                        # name -> (list, windows)
    "fixed_baseline": (ALL, [((0, 2), (i, i + 1)) for i in range(K)]),
    "consecutive": (ALL, [((i, i + 1), (i + 1, i + 2)) for i in range(K - 1)]),
    "base_after_cur": (ALL, [((3, 6), (0, 3)), ((5, 6), (0, 1)), ((1, 6), (0, 1))]),
    "overlapping": (ALL, [((0, 4), (2, 6)), ((1, 3), (2, 4)), ((0, 6), (2, 3))]),
    "identical": (ALL, [((0, 6), (0, 6)), ((2, 3), (2, 3)), ((BIG, BIG + 1), (BIG, BIG + 1))]),
    "repeated": (ALL, [((0, 2), (2, 4)), ((4, 5), (0, 1)), ((0, 2), (2, 4))]),
    "32+32": (LIST64, [((0, 32), (32, 64))]),
    "empty_side": (ALL, [((4, 5), (0, 1)), ((4, 5), (3, 5)), ((0, 1), (4, 5))]),
}
_DRIFT_MODEL = {}


def spread_series(c, lst, windows, P=P_MAIN, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].spread_series(P, [c.kept[i] for i in lst[:-1]], windows, c.M - first if nmetrics is None else nmetrics,
                                         first, **kw)


def spread(c, lst, P=P_MAIN, nmetrics=None, first=0, **kw):
    return c.kept[lst[-1]].spread(P, [c.kept[i] for i in lst[:-1]], c.M - first if nmetrics is None else nmetrics, first, **kw)


def drift(c, lst, windows, nmetrics=None, first=0, against=None, **kw):
    return c.kept[lst[-1]].drift(windows, [c.kept[i] for i in lst[:-1]], against, c.M - first if nmetrics is None else nmetrics,
                                 first, **kw)


def compare(c, base, cur, nmetrics=None, first=0, **kw):
    return c.kept[cur[-1]].compare([c.kept[i] for i in base], c.M - first if nmetrics is None else nmetrics, first,
                                   earlier=[c.kept[i] for i in cur[:-1]], **kw)


def drift_models(c, base, cur):
    """the compare model of every name for the handles `base` against `cur`; None where a side's total passes 2^64"""
    key = (c.wide, tuple(base), tuple(cur))
    if key not in _DRIFT_MODEL:
        out = []
        for m in range(c.M):
            sides = []
            for lst in (base, cur):
                cells = {}
                for i in lst:
                    for b, v in c.rows[i][m].items():
                        cells[b] = cells.get(b, 0) + v
                sides.append(cells)
            out.append(None if any(sum(s.values()) >= 1 << 64 for s in sides) else model(*sides))
        _DRIFT_MODEL[key] = out
    return _DRIFT_MODEL[key]


def same_block(got, w, ref, fields, what):
    for f in fields:
        assert np.ascontiguousarray(got[f][w]).tobytes() == np.ascontiguousarray(ref[f]).tobytes(), (what, w, f)


def sides(lst, window):
    (blo, bhi), (clo, chi) = window
    return lst[blo:bhi], lst[clo:chi]


# ---- 1. against the model, and against the parents' readers ------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_spread_series_every_window_set(crafted, kind):
    c = crafted
    with shape(kind):
        for lst, windows, name in CASES:
            got = spread_series(c, lst, windows)
            nw = len(windows)
            assert got["count"].shape == (nw, c.M) and got["sum_le"].shape == (nw, c.M, len(P_MAIN)), name
            assert got["std"].shape == (nw, c.M) and got["mean_le"].shape == got["upper"].shape == got["pkeys"].shape, name
            for w, (lo, hi) in enumerate(windows):
                sl = lst[lo:hi]
                check_spreads({f: v[w] for f, v in got.items()}, c, sl, P_MAIN, what=(kind, name, w))
                ref = spread(c, sl)
                same_block(got, w, ref, SP_FIELDS, (kind, name))
                for f in ("std", "mean_le", "upper"):                            # the derived fields too
                    assert got[f][w].tobytes() == ref[f].tobytes(), (kind, name, w, f)
        # np == 0: moments only
        lst, windows, name = CASES[3]
        none = spread_series(c, lst, windows, P=[])
        assert none["pkeys"].shape == (len(windows), c.M, 0) and none["upper"].shape == (len(windows), c.M, 0)
        full = spread_series(c, lst, windows)
        for w, (lo, hi) in enumerate(windows):
            check_spreads({f: v[w] for f, v in none.items()}, c, lst[lo:hi], [], what=(kind, "np=0", w))
            same_block(none, w, spread(c, lst[lo:hi], P=[]), ("count", "sum", "m2"), (kind, "np=0"))
        for f in ("count", "sum", "m2"):                                         # the moments do not depend on the percentiles
            assert none[f].tobytes() == full[f].tobytes(), f


@pytest.mark.parametrize("kind", KINDS)
def test_spread_series_thresholds_at_the_edges_of_a_tile_in_a_window_with_lo_above_0(crafted, kind):
    """test_spread_thresholds_at_the_edges_of_a_tile's row (cells at bins 0, T - 1, T, 2T - 1, 2T and 65 535 with counts 1 .. 6) read
    through windows that start behind the head of the list."""
    import bisect
    c, T = crafted, crafted.T
    P = [s / 21 for s in range(22)]
    prefix = [1, 3, 6, 10, 15, 21]
    bins = [0, T - 1, T, 2 * T - 1, 2 * T, NK - 1]
    want_at = [bisect.bisect_left(prefix, max(s, 1)) for s in range(22)]
    with shape(kind):
        for lst, windows, name in (([1] + ALL, [(1, 7), (0, 1), (1, 7)], "edges"), ([4, 5, 3, 1, 0, 2, 4], [(0, 2), (1, 7)], "edges"),
                                   ([0, 1, 2, 3], [(2, 3), (0, 4)], "edges_in_one")):
            m = c.at[name]
            got = spread_series(c, lst, windows, P, 1, m)
            for w, (lo, hi) in enumerate(windows):
                sl = lst[lo:hi]
                block = {f: v[w] for f, v in got.items()}
                check_spreads(block, c, sl, P, rows=[m], what=(kind, lst, name, w))
                same_block(got, w, spread(c, sl, P, 1, m), SP_FIELDS, (kind, name))
                if sorted(sl) == ALL or (name == "edges_in_one" and 2 in sl):
                    assert [int(oracle.key_to_bin(int(k))) for k in block["pkeys"][0]] == [bins[j] for j in want_at], (name, w)
                    assert [int(x) for x in block["count_le"][0]] == [prefix[j] for j in want_at] and block["pvalid"].all()


@pytest.mark.parametrize("kind", KINDS)
def test_drift_every_window_set(crafted, kind):
    c = crafted
    with shape(kind):
        for name, (lst, windows) in DRIFT.items():
            got = drift(c, lst, windows)
            assert got["ks"].shape == (len(windows), c.M) and got["ks_value"].shape == (len(windows), c.M), name
            for w, window in enumerate(windows):
                base, cur = sides(lst, window)
                check_rows({f: v[w] for f, v in got.items()}, drift_models(c, base, cur), (kind, name, w))
                same_block(got, w, compare(c, base, cur), list(CMP_FIELDS) + ["ks_value"], (kind, name))
        # against= and the defaults build the same windows
        lst, windows = DRIFT["fixed_baseline"]
        got = drift(c, lst, windows)
        for other in (drift(c, lst, None, against=(0, 2)), drift(c, lst, [(i, i + 1) for i in range(K)], against=(0, 2))):
            for f in CMP_FIELDS:
                assert other[f].tobytes() == got[f].tobytes(), f
        got, other = drift(c, *DRIFT["consecutive"]), drift(c, ALL, None)
        assert other["ks"].shape == (K - 1, c.M)
        for f in CMP_FIELDS:
            assert other[f].tobytes() == got[f].tobytes(), f
        # identical slices: exact zeros for every non-empty name
        lst, windows = DRIFT["identical"]
        got = drift(c, lst, windows)
        for w, window in enumerate(windows):
            for m, want in enumerate(drift_models(c, *sides(lst, window))):
                if want is None:
                    continue
                assert int(got["count_a"][w, m]) == int(got["count_b"][w, m]) == want["count_a"], (w, m)
                if want["count_a"]:
                    assert got["ks"][w, m] == 0 and got["w1"][w, m] == 0 and got["shift"][w, m] == 0 and got["key"][w, m] == 0, (w, m)
                    assert got["below_a"][w, m] == 0 and got["below_b"][w, m] == 0, (w, m)
                else:
                    assert math.isnan(got["ks"][w, m]) and math.isnan(got["w1"][w, m]) and math.isnan(got["shift"][w, m]), (w, m)
        # a name that is empty on one side of a window: NaN with key and prefixes 0 there, and only there
        got = drift(c, *DRIFT["empty_side"])
        m = c.at["only_in_4"]
        for w, (na, nb) in enumerate(((6, 0), (6, 6), (0, 6))):
            assert (int(got["count_a"][w, m]), int(got["count_b"][w, m])) == (na, nb), w
            empty = na == 0 or nb == 0
            for f in ("ks", "w1", "shift", "ks_value"):
                assert math.isnan(got[f][w, m]) == empty, (w, f)
            if empty:
                assert got["key"][w, m] == 0 and got["below_a"][w, m] == 0 and got["below_b"][w, m] == 0, w
        # more than LH_MAX_KEPT handles in the two slices of a window, and malformed windows
        import loghisto_amd
        with pytest.raises(loghisto_amd.LhError) as ei:
            drift(c, LIST64, [((0, 32), (32, 64)), ((0, 33), (32, 64))])
        assert ei.value.code == N.EINVAL
        for bad in ([((0, 1), (0, -1))], [((0, 1),)]):
            with pytest.raises((ValueError, TypeError)):
                drift(c, ALL, bad)
        with pytest.raises(ValueError):
            drift(c, [0], None)


@pytest.mark.parametrize("kind", KINDS)
def test_drift_on_the_compare_fixture(kept, kind):
    """The crafted pairs and tile cases of lh_kept_compare's own tests, base and cur as two slices of ONE list."""
    c, M = kept, kept.M
    LA, LB = c.lists[3]
    both = LA + LB + [c.A, c.B]                                                  # positions 0 .. 2 | 3 .. 5 | 6 | 7
    windows = [((0, 3), (3, 6)), ((3, 6), (0, 3)), ((6, 7), (7, 8)), ((6, 7), (3, 6)), ((0, 3), (0, 3)), ((0, 3), (3, 6)),
               ((0, 7), (3, 8))]
    with shape(kind):
        got = both[-1].k.drift(windows, [h.k for h in both[:-1]], nmetrics=M)
        for w, ((blo, bhi), (clo, chi)) in enumerate(windows):
            base, cur = both[blo:bhi], both[clo:chi]
            check_rows({f: v[w] for f, v in got.items()}, models(c, base, cur), (kind, "compare fixture", w))
            ref = cur[-1].k.compare([h.k for h in base], M, earlier=[h.k for h in cur[:-1]])
            same_block(got, w, ref, list(CMP_FIELDS) + ["ks_value"], (kind, "compare fixture"))
        for f in CMP_FIELDS:                                                     # dealt over three handles or in one: the same sums
            assert got[f][0].tobytes() == got[f][2].tobytes() == got[f][5].tobytes(), f
        for k, na, nb in (("a_empty", 0, 1), ("b_empty", 3, 0), ("both_empty", 0, 0)):
            m = c.at[k]
            assert (int(got["count_a"][0, m]), int(got["count_b"][0, m])) == (na, nb), k
            assert (int(got["count_a"][1, m]), int(got["count_b"][1, m])) == (nb, na), k
            assert math.isnan(got["ks"][0, m]) and math.isnan(got["w1"][1, m]) and got["key"][0, m] == 0, k


def test_the_two_shapes_give_identical_bytes(crafted):
    c = crafted
    for lst, windows, name in CASES:
        res = {}
        for kind in KINDS:
            with shape(kind):
                res[kind] = spread_series(c, lst, windows)
        for f in SP_FIELDS:
            assert res["wave"][f].tobytes() == res["block"][f].tobytes(), (name, f)
    for name, (lst, windows) in DRIFT.items():
        res = {}
        for kind in KINDS:
            with shape(kind):
                res[kind] = drift(c, lst, windows)
        for f in CMP_FIELDS:
            assert res["wave"][f].tobytes() == res["block"][f].tobytes(), (name, f)


# ---- 2. rows, ids, device forms, refusals -------------------------------------------------------------------------------------
SP_TORCH = dict(count="int64", sum="float64", m2="float64", pkeys="int16", pvalid="uint8", count_le="int64", sum_le="float64")
CMP_TORCH = dict(count_a="int64", count_b="int64", ks="float64", key="int16", below_a="int64", below_b="int64", w1="float64",
                 shift="float64")
PAD = 3


def _out(torch, kinds, n, per, pad=PAD):
    """(the padded arrays filled with 77, their leading n entries: what the call is given)"""
    back = {k: torch.full(((n + pad) * per.get(k, 1),), 77, dtype=getattr(torch, t), device="cuda") for k, t in kinds.items()}
    return back, {k: back[k][:n * per.get(k, 1)] for k in kinds}


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _same_device(back, fields, want, per, what):
    """the device arrays hold want (window-major) and the sentinel behind it"""
    for k, dt in fields.items():
        h, w = _host(back[k], dt), np.ascontiguousarray(want[k])
        assert h[:w.size].tobytes() == w.tobytes(), (what, k)
        assert h.size == w.size + PAD * per.get(k, 1) and np.all(h[w.size:] == 77), (what, k)


def _emptied(res, fields, cols, never):
    """res with the entries `cols` of every window replaced by the entry of the name that never has a sample"""
    out = {}
    for f in fields:
        a = res[f].copy()
        for j in cols:
            a[:, j] = a[:, never]
        out[f] = a
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_rows_ids_and_device_forms(crafted, kind):
    import loghisto_amd
    c, torch = crafted, crafted.torch
    npct = len(P_MAIN)
    sper = {k: npct for k in SP_PER_P}
    swin = [(i, i + 2) for i in range(K - 1)] + [(2, 5), (0, 1), (2, 5)]
    dwin = DRIFT["overlapping"][1] + DRIFT["repeated"][1] + DRIFT["consecutive"][1]
    ids = [c.at["edges"], 0, c.M - 1, c.at["dense300"], 0, c.at["eight_tiles"], 5, 4, 3, c.at["edges"], c.at["never"], c.at["far_apart"]]
    never = ids.index(c.at["never"])
    st = torch.cuda.Stream()
    with shape(kind):
        sp, dr = spread_series(c, ALL, swin), drift(c, ALL, dwin)
        # a sub-block
        part, dpart = spread_series(c, ALL, swin, nmetrics=9, first=7), drift(c, ALL, dwin, nmetrics=9, first=7)
        assert part["count"].shape == (len(swin), 9) and dpart["ks"].shape == (len(dwin), 9)
        for w, (lo, hi) in enumerate(swin):
            same_block(part, w, spread(c, ALL[lo:hi], nmetrics=9, first=7), SP_FIELDS, (kind, "first=7"))
        for w, window in enumerate(dwin):
            same_block(dpart, w, compare(c, *sides(ALL, window), nmetrics=9, first=7), CMP_FIELDS, (kind, "first=7"))
        for f in SP_FIELDS:
            assert part[f].tobytes() == np.ascontiguousarray(sp[f][:, 7:16]).tobytes(), f
        for f in CMP_FIELDS:
            assert dpart[f].tobytes() == np.ascontiguousarray(dr[f][:, 7:16]).tobytes(), f
        # a host id list: permuted, repeated
        gsp, gdr = spread_series(c, ALL, swin, ids=ids), drift(c, ALL, dwin, ids=ids)
        assert gsp["count"].shape == (len(swin), len(ids)) and gdr["ks"].shape == (len(dwin), len(ids))
        for w, (lo, hi) in enumerate(swin):
            same_block(gsp, w, spread(c, ALL[lo:hi], ids=ids), SP_FIELDS, (kind, "ids"))
        for w, window in enumerate(dwin):
            same_block(gdr, w, compare(c, *sides(ALL, window), ids=ids), CMP_FIELDS, (kind, "ids"))
        for f in SP_FIELDS:
            assert gsp[f].tobytes() == np.ascontiguousarray(sp[f][:, ids]).tobytes(), f
        for f in CMP_FIELDS:
            assert gdr[f].tobytes() == np.ascontiguousarray(dr[f][:, ids]).tobytes(), f
        assert spread_series(c, ALL, swin, ids=[])["count"].shape == (len(swin), 0) and drift(c, ALL, dwin, ids=[])["ks"].shape == (len(dwin), 0)
        # device forms on a caller's stream: rows, then device ids with some beyond every block
        sback, sout = _out(torch, SP_TORCH, len(swin) * c.M, sper)
        dback, dout = _out(torch, CMP_TORCH, len(dwin) * c.M, {})
        torch.cuda.synchronize()
        assert spread_series(c, ALL, swin, out=sout, stream=st)["sum"] is sout["sum"]
        assert drift(c, ALL, dwin, out=dout, stream=st)["ks"] is dout["ks"]
        st.synchronize()
        _same_device(sback, SP_FIELDS, sp, sper, (kind, "device form"))
        _same_device(dback, CMP_FIELDS, dr, {}, (kind, "device form"))
        bad = {2: c.M, 6: c.M + 1000, 9: 0xffffffff}
        dids = [bad.get(j, i) for j, i in enumerate(ids)]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(dids, dtype=torch.int64, device="cuda").to(torch.int32)
        sback, sout = _out(torch, SP_TORCH, len(swin) * len(ids), sper)
        dback, dout = _out(torch, CMP_TORCH, len(dwin) * len(ids), {})
        torch.cuda.synchronize()
        spread_series(c, ALL, swin, ids=d_ids, out=sout, stream=st)
        drift(c, ALL, dwin, ids=d_ids, out=dout, stream=st)
        st.synchronize()
        assert not gsp["count"][:, never].any() and not gsp["sum_le"][:, never].any() and np.isnan(gdr["ks"][:, never]).all()
        assert not gdr["count_a"][:, never].any() and not gdr["count_b"][:, never].any() and not gdr["key"][:, never].any()
        _same_device(sback, SP_FIELDS, _emptied(gsp, SP_FIELDS, bad, never), sper, (kind, "device ids"))
        _same_device(dback, CMP_FIELDS, _emptied(gdr, CMP_FIELDS, bad, never), {}, (kind, "device ids"))
        # a host id outside any listed handle, or rows beyond it: LH_ERANGE, nothing written
        for kw in (dict(ids=[0, c.M, 1]), dict(ids=[0xffffffff]), dict(nmetrics=c.M + 1), dict(nmetrics=1, first=c.M)):
            n = len(kw["ids"]) if "ids" in kw else kw["nmetrics"]
            so = {k: np.full((len(swin), n, npct) if k in SP_PER_P else (len(swin), n), 7, dtype=t) for k, t in SP_FIELDS.items()}
            do = {k: np.full((len(dwin), n), 7, dtype=t) for k, t in CMP_FIELDS.items()}
            for call, arrays in ((lambda: spread_series(c, ALL, swin, out=so, **kw), so), (lambda: drift(c, ALL, dwin, out=do, **kw), do)):
                with pytest.raises(loghisto_amd.LhError) as ei:
                    call()
                assert ei.value.code == N.ERANGE, kw
                assert all(np.all(v == 7) for v in arrays.values()), kw


@pytest.mark.parametrize("kind", KINDS)
def test_a_shorter_handle_empties_only_the_windows_that_hold_it(crafted, kind):
    """A device id one past the block of a shorter handle gives the empty entry in exactly the windows whose slices contain the
    handle; a host id there, or rows beyond it, are refused whether or not a window names the handle."""
    import loghisto_amd
    c, torch = crafted, crafted.torch
    npct = len(P_MAIN)
    sper = {k: npct for k in SP_PER_P}
    end = c.at["eight_tiles"]                                                    # a name every handle holds cells of
    short = c.kept[1].merge(nmetrics=end, first=0)                               # rows 0 .. end - 1 of handle 1
    try:
        kl = [c.kept[0], short, c.kept[2], c.kept[3]]                            # the list; `short` at position 1
        swin = [(0, 1), (0, 2), (1, 2), (2, 4), (1, 4), (3, 4)]
        dwin = [((0, 1), (2, 3)), ((0, 2), (2, 3)), ((2, 4), (1, 2)), ((2, 3), (3, 4)), ((1, 2), (1, 2)), ((3, 4), (0, 1))]
        some = [end - 1, end, 3, end]                                            # end: one past the short handle's block
        d_ids = torch.tensor(some, dtype=torch.int32, device="cuda")
        with shape(kind):
            sback, sout = _out(torch, SP_TORCH, len(swin) * 4, sper)
            dback, dout = _out(torch, CMP_TORCH, len(dwin) * 4, {})
            torch.cuda.synchronize()
            kl[-1].spread_series(P_MAIN, kl[:-1], swin, ids=d_ids, out=sout)
            kl[-1].drift(dwin, kl[:-1], ids=d_ids, out=dout)
            torch.cuda.synchronize()
            for w, (lo, hi) in enumerate(swin):
                holds = lo <= 1 < hi
                ref = kl[hi - 1].spread(P_MAIN, kl[lo:hi - 1], ids=[end - 1, 3] if holds else some)
                for f, dt in SP_FIELDS.items():
                    got = _host(sout[f], dt).reshape(len(swin), 4, -1)[w]
                    if holds:                                                    # entries 1 and 3 all zero, 0 and 2 the slice's
                        r = ref[f].reshape(2, -1)
                        assert got[0].tobytes() == r[0].tobytes() and got[2].tobytes() == r[1].tobytes(), (kind, w, f)
                        assert not got[1].any() and not got[3].any(), (kind, w, f)
                    else:
                        assert got.tobytes() == ref[f].tobytes(), (kind, w, f)
                if not holds:
                    assert _host(sout["count"], U64).reshape(len(swin), 4)[w, 1], w
            for w, ((blo, bhi), (clo, chi)) in enumerate(dwin):
                holds = blo <= 1 < bhi or clo <= 1 < chi
                ref = kl[chi - 1].compare(kl[blo:bhi], ids=[end - 1, 3] if holds else some, earlier=kl[clo:chi - 1])
                for f, dt in CMP_FIELDS.items():
                    got = _host(dout[f], dt).reshape(len(dwin), 4)[w]
                    if holds:                                                    # entries 1 and 3: two empty sides
                        assert got[[0, 2]].tobytes() == ref[f].tobytes(), (kind, w, f)
                        if f in ("ks", "w1", "shift"):
                            assert np.isnan(got[[1, 3]]).all(), (kind, w, f)
                        else:
                            assert not got[[1, 3]].any(), (kind, w, f)
                    else:
                        assert got.tobytes() == ref[f].tobytes(), (kind, w, f)
                if not holds:
                    assert _host(dout["count_a"], U64).reshape(len(dwin), 4)[w, 1], w
            # on the host: refused even for windows that leave the short handle out
            for kw in (dict(ids=some), dict(nmetrics=end + 1), dict(nmetrics=1, first=end)):
                n = len(kw["ids"]) if "ids" in kw else kw["nmetrics"]
                so = {k: np.full((2, n, npct) if k in SP_PER_P else (2, n), 7, dtype=t) for k, t in SP_FIELDS.items()}
                do = {k: np.full((2, n), 7, dtype=t) for k, t in CMP_FIELDS.items()}
                for call, arrays in ((lambda: kl[-1].spread_series(P_MAIN, kl[:-1], [(0, 1), (2, 4)], out=so, **kw), so),
                                     (lambda: kl[-1].drift([((0, 1), (2, 3)), ((2, 3), (3, 4))], kl[:-1], out=do, **kw), do)):
                    with pytest.raises(loghisto_amd.LhError) as ei:
                        call()
                    assert ei.value.code == N.ERANGE, kw
                    assert all(np.all(v == 7) for v in arrays.values()), kw
    finally:
        short.close()


# ---- 3. the limits: 64 handles, 128 windows -----------------------------------------------------------------------------------
def test_64_handles_and_128_windows(native_lib, torch_cuda):
    M, n, k = 3, 300, 64
    rng = np.random.default_rng(6401)
    handles = []
    with engine(M, cell_bits=64, num_buffers=2) as e:
        for i in range(k):
            ids = rng.integers(0, M, n).astype(np.uint32)
            e.submit_pairs(ids[ids != i % 5], rng.lognormal(3.0 + 0.01 * i, 1.0, n)[ids != i % 5])   # a name missing from most
            with e.flip() as s:
                handles.append(s.keep(M))
    try:
        swin = [(i, i + 1) for i in range(k)] + [(i, min(i + 7, k)) for i in range(k)]
        dwin = [((0, 10), (i, i + 1)) for i in range(k)] + [((i, i + 1), (i + 1, i + 2)) for i in range(k - 1)] + [((0, 32), (32, 64))]
        assert len(swin) == len(dwin) == N.MAX_WINDOWS
        res = {}
        for kind in KINDS:
            with shape(kind):
                sp, dr = handles[-1].spread_series(P_MAIN, handles[:-1], swin), handles[-1].drift(dwin, handles[:-1])
                assert sp["count"].shape == (128, M) and dr["ks"].shape == (128, M)
                for w, (lo, hi) in enumerate(swin):
                    same_block(sp, w, handles[hi - 1].spread(P_MAIN, handles[lo:hi - 1]), SP_FIELDS, (kind, "64 x 128"))
                for w, ((blo, bhi), (clo, chi)) in enumerate(dwin):
                    same_block(dr, w, handles[chi - 1].compare(handles[blo:bhi], earlier=handles[clo:chi - 1]), CMP_FIELDS, (kind, "64 x 128"))
                res[kind] = (sp, dr)
                none = handles[-1].spread_series(P_MAIN, handles[:-1])           # windows=None: one per handle
                for f in SP_FIELDS:
                    assert none[f].tobytes() == np.ascontiguousarray(sp[f][:k]).tobytes(), f
                fixed = handles[-1].drift(None, handles[:-1], against=(0, 10))   # ... against a fixed baseline
                pairs = handles[-1].drift(None, handles[:-1])                    # ... each against the one before it
                for f in CMP_FIELDS:
                    assert fixed[f].tobytes() == np.ascontiguousarray(dr[f][:k]).tobytes(), f
                    assert pairs[f].tobytes() == np.ascontiguousarray(dr[f][k:2 * k - 1]).tobytes(), f
        assert res["wave"][0]["count"].sum() > 0.5 * k * n and np.isfinite(res["wave"][1]["w1"]).sum() > 100
        for f in SP_FIELDS:
            assert res["wave"][0][f].tobytes() == res["block"][0][f].tobytes(), f
        for f in CMP_FIELDS:
            assert res["wave"][1][f].tobytes() == res["block"][1][f].tobytes(), f
    finally:
        for kk in handles:
            kk.close()


# ---- 4. lifetime ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_close_right_after_a_device_form_call_waits_for_it(crafted, kind):
    c, torch = crafted, crafted.torch
    npct = len(P_MAIN)
    sper = {k: npct for k in SP_PER_P}
    lst, swin = [0, 1, 2, BIG], [(0, 4), (1, 3), (3, 4), (0, 1)]
    dwin = [((0, 2), (2, 4)), ((3, 4), (0, 1)), ((0, 4), (1, 3))]
    with shape(kind):
        sp, dr = spread_series(c, lst, swin), drift(c, lst, dwin)
        for reader in ("spread_series", "drift"):
            fresh = [c.kept[i].merge() for i in lst]                             # the same cells in handles to be closed at once
            st = torch.cuda.Stream()
            sback, sout = _out(torch, SP_TORCH, len(swin) * c.M, sper)
            dback, dout = _out(torch, CMP_TORCH, len(dwin) * c.M, {})
            torch.cuda.synchronize()
            if reader == "spread_series":
                fresh[-1].spread_series(P_MAIN, fresh[:-1], swin, c.M, out=sout, stream=st)
            else:
                fresh[-1].drift(dwin, fresh[:-1], None, c.M, out=dout, stream=st)
            for k_ in fresh:
                k_.close()                                                       # waits for the enqueued kernel
            st.synchronize()
            if reader == "spread_series":
                _same_device(sback, SP_FIELDS, sp, sper, (kind, "closed at once"))
            else:
                _same_device(dback, CMP_FIELDS, dr, {}, (kind, "closed at once"))


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------------
def test_window_class(native_lib, torch_cuda):
    import loghisto_amd
    M, n = 12, 4000
    rng = np.random.default_rng(13)
    with engine(M, cell_bits=64, num_buffers=2) as e, loghisto_amd.KeptWindow(3) as win:
        made = []
        for i in range(4):                                                       # 4 pushes into a window of 3
            ids = rng.integers(0, M - 1, n).astype(np.uint32)                    # the last name stays empty
            e.submit_pairs(ids, rng.lognormal(2.0 + 0.3 * i, 1.0, n))
            with e.flip() as s:
                made.append(s.keep(M))
            win.push(made[-1])
        handles = list(win.handles)
        assert handles == made[1:]
        for windows in (None, [(0, 3), (1, 3), (2, 3)]):
            a, b = win.spread_series(P_MAIN, windows), handles[-1].spread_series(P_MAIN, handles[:-1], windows)
            assert set(a) == set(SP_FIELDS) | {"std", "mean_le", "upper"} and a["count"].shape == (3, M)
            for f in SP_FIELDS:
                assert a[f].tobytes() == b[f].tobytes(), f
        for windows, against, nw in ((None, None, 2), (None, (0, 1), 3), ([(1, 3)], (0, 1), 1), ([((0, 1), (1, 3)), ((2, 3), (0, 2))], None, 2)):
            a, b = win.drift(windows, against), handles[-1].drift(windows, handles[:-1], against)
            assert set(a) == set(CMP_FIELDS) | {"ks_value"} and a["ks"].shape == (nw, M)
            for f in CMP_FIELDS:
                assert a[f].tobytes() == b[f].tobytes(), f
            assert np.isnan(a["ks"][:, M - 1]).all() and np.isfinite(a["w1"][:, :M - 1]).all()
        whole = win.spread_series(P_MAIN, [(0, 3)], ids=[3, 1])                  # the window's total holds the same cells
        tot = win.total.spread(P_MAIN, (), ids=[3, 1])
        assert whole["count"][0].tobytes() == tot["count"].tobytes() and whole["pkeys"][0].tobytes() == tot["pkeys"].tobytes()
        for k_ in made:
            k_.close()
