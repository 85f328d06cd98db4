"""lh_kept_top* and lh_kept_movers* (Kept.top, Kept.movers): lh_top's and lh_movers' selections over lists of kept intervals.

The yardstick for a selection is the already-tested per-name kept readers plus an exact host sort: Kept.across, Kept.count_le or
Kept.compare over the same lists give every name's score, (score, id) pairs are sorted in Python by the documented total order --
descending or ascending score with -0.0 == +0.0, ties by lowest id, empty rows never ranked -- and k entries are taken.  Ids and
integer fields must be equal; `sum` and the movers' `score` are compared as BITS.
A name whose total passes 2^64 in a list has an unspecified rank: for every `by` except "count" the tests rank the sub-ranges
that leave such names out (the model, cells_of, says which they are: two per list at most), and by="count" ranks the whole block
against the model modulo 2^64.  On the crafted fixture of tests/test_gpu_kept.py (70 names x 6 handles, engines of 64- and of
32-bit cells) under both kernel shapes, and on 4 097 names x 3 handles for the select pass's sizes under the default switch.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import ctypes as C
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_compare import EPS, _import, model as pair_model
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import BIG, K, LISTS, arrays_of, crafted, crafted_names, shape, tile  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_readers import cells_of, value_of
from tests.test_gpu_movers import DOZEN, M_ROWS, NONE_FROM, NONE_TO, dozen_rows
from tests.test_gpu_spread import Exact

pytestmark = pytest.mark.gpu

U64 = np.uint64
W = 1 << 64
KINDS = ("wave", "block")
INF = float("inf")
PCTS = [0.0, 0.5, 0.99, 1.0]
KS = (1, 2, 69, 70, 71, 1024)
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
MOVER_BYS = [("ks", None), ("w1", None), ("shift", None)] + [("percentile", p) for p in PCTS]
SPLITS = [([0], [1]), ([0, 1, 2], [3, 4, 5]), ([BIG], [BIG, BIG]), ([0, 1, 2], [0, 1, 2]), ([3], [3]),
          (([0, 1, 2] * 11)[:32], ([3, 4, 5] * 11)[:32])]


def aboves(T):
    return sorted([250.0, value_of(T - 1), value_of(T), -5.0, INF, -INF, 1e200])


def top_bys(T):
    return [("count", None), ("sum", None)] + [("percentile", p) for p in PCTS] + [("count_above", a) for a in aboves(T)]


def bin_of(keys):
    return (np.asarray(keys).astype(np.int64) & 0xffff) ^ 0x8000


def kept_of(c, lst):
    return [c.kept[i] for i in lst]


# ---- which names are ranked ---------------------------------------------------------------------------------------------------
def wrapped_in(rows_by_handle, lists, M):
    """the names whose total passes 2^64 in one of the lists"""
    out = set()
    for lst in lists:
        for m in range(M):
            tot = {}
            for i in lst:
                for b, v in rows_by_handle[i][m].items():
                    tot[b] = tot.get(b, 0) + v
            if sum(v % W for v in tot.values()) >= W:
                out.add(m)
    return sorted(out)


def ranges_without(bad, M):
    """the sub-ranges [first, first + n) of [0, M) that leave the names `bad` out"""
    out, at = [], 0
    for m in list(bad) + [M]:
        if m > at:
            out.append((at, m - at))
        at = m + 1
    return out


def test_the_crafted_rows_wrap_in_two_names_a_list_at_most():
    """A property of the fixture, from its rows alone (no GPU is needed for it): at most two names per list are left out of the
    ranked ranges, every other name lies in one, and the model agrees with cells_of."""
    T = 1024
    names = crafted_names(T)
    M = len(names)
    rows = [[dict(per.get(i, ({}, None))[0]) for _, per in names] for i in range(K)]
    c = types.SimpleNamespace(wide="model", M=M, rows=rows)
    for lst in LISTS + [a + b for a, b in SPLITS]:
        bad = wrapped_in(rows, [lst], M)
        assert bad == [m for m, (_, counts, _) in enumerate(cells_of(c, lst)) if sum(counts) >= W]
        assert len(bad) <= 2, lst
        covered = set()
        for first, n in ranges_without(bad, M):
            covered |= set(range(first, first + n))
        assert covered == set(range(M)) - set(bad)
    assert not wrapped_in(rows, [[0, 1, 2]], M)


# ---- the yardstick: the per-name readers, then an exact sort --------------------------------------------------------------------
def top_scores(k_last, earlier, M, T, first=0):
    """every name's fields and scores of block [first, first + M) from Kept.across and Kept.count_le over the same list"""
    ab = aboves(T)
    acr = k_last.across(earlier, PCTS, M, first)
    le = k_last.count_le(ab, earlier, M, first)
    assert np.array_equal(acr["count"], le["total"])
    return types.SimpleNamespace(count=[int(x) for x in acr["count"]], sum=acr["sum"].copy(), pkeys=acr["pkeys"].copy(),
                                 pvalid=acr["pvalid"].copy(),
                                 above={a: [(int(t) - int(x)) % W for t, x in zip(le["total"], le["cum"][:, j])] for j, a in enumerate(ab)},
                                 first=first)


def top_want(s, by, arg, k, asc, first, n):
    """the expected entries of rows [first, first + n) (absolute), from the scores s of a block that holds them"""
    rows = []
    for m in range(first - s.first, first - s.first + n):
        if s.count[m] == 0:
            continue
        j = PCTS.index(arg) if by == "percentile" else 0
        if by == "percentile":
            assert s.pvalid[m, j]
        score = {"count": s.count[m], "sum": float(s.sum[m]), "percentile": int(bin_of(s.pkeys[m, j])),
                 "count_above": s.above[arg][m] if by == "count_above" else 0}[by]
        assert score == score
        rows.append((score if asc else -score, m + s.first, m, j))
    rows.sort(key=lambda r: r[:2])
    want = np.zeros(min(k, len(rows)), dtype=N.TOP_ENTRY)
    for t, (_, mid, m, j) in enumerate(rows[:k]):
        want[t] = (mid, s.pkeys[m, j] if by == "percentile" else 0, 0, s.count[m], s.sum[m], s.above[arg][m] if by == "count_above" else 0)
    return want


def same_entries(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for f in got.dtype.names:
        a, b = got[f], want[f]
        if a.dtype == np.float64:
            a, b = a.view(U64), b.view(U64)
        assert np.array_equal(a, b), (what, f, got[:8], want[:8])


def movers_scores(base, cur, M, first=0):
    """base, cur: lists of Kept.  Every name's fields and scores from Kept.compare and Kept.across over the same lists."""
    cmp_ = cur[-1].compare(base, M, first, earlier=cur[:-1])
    pa = base[-1].across(base[:-1], PCTS, M, first)
    pb = cur[-1].across(cur[:-1], PCTS, M, first)
    assert np.array_equal(cmp_["count_a"], pa["count"]) and np.array_equal(cmp_["count_b"], pb["count"])
    return types.SimpleNamespace(cmp=cmp_, ka=pa["pkeys"].copy(), kb=pb["pkeys"].copy(), first=first,
                                 cand=(cmp_["count_a"] != 0) & (cmp_["count_b"] != 0))


def movers_want(s, by, arg, k, asc, first, n):
    rows = []
    for m in range(first - s.first, first - s.first + n):
        if not s.cand[m]:
            continue
        key = key_base = 0
        if by == "percentile":
            j = PCTS.index(arg)
            key, key_base = int(s.kb[m, j]), int(s.ka[m, j])
            score = float(int(bin_of(key)) - int(bin_of(key_base)))
        else:
            score = float(s.cmp[by][m])
            key = int(s.cmp["key"][m]) if by == "ks" else 0
        assert score == score                                                    # a NaN is never ranked
        rows.append((score if asc else -score, m + s.first, m, key, key_base, score))
    rows.sort(key=lambda r: r[:2])
    want = np.zeros(min(k, len(rows)), dtype=N.MOVER_ENTRY)
    for t, (_, mid, m, key, key_base, score) in enumerate(rows[:k]):
        want[t] = (mid, key, key_base, s.cmp["count_a"][m], s.cmp["count_b"][m], score)
    return want


# ---- 1. every list x every by, both directions, every k -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_top_every_list_every_by(crafted, kind):
    c = crafted
    with shape(kind):
        for lst in LISTS:
            kept = kept_of(c, lst)
            s = top_scores(kept[-1], kept[:-1], c.M, c.T)
            cells = cells_of(c, lst)
            assert s.count == [tot for _, _, tot in cells]                       # count: the model modulo 2^64, wrapped names included
            bad = [m for m, (_, counts, _) in enumerate(cells) if sum(counts) >= W]
            assert len(bad) <= 2
            for by, arg in top_bys(c.T):
                spans = [(0, c.M)] if by == "count" else ranges_without(bad, c.M)
                assert sum(n for _, n in spans) == c.M - (0 if by == "count" else len(bad))
                for first, n in spans:
                    for asc in (False, True):
                        for k in KS:
                            got = kept[-1].top(k, by, arg, asc, kept[:-1], n, first)
                            same_entries(got, top_want(s, by, arg, k, asc, first, n), (kind, lst[:8], len(lst), by, arg, asc, k, first, n))
    # what the crafted rows were made for: the take on a tile's edge, and in the gap of far_apart (bins 10 001 and 40 001)
    s = top_scores(c.kept[1], [c.kept[0]], c.M, c.T)
    m = c.at["far_apart"]
    assert s.above[250.0][m] == 1 and s.above[value_of(c.T)][m] == 2 and s.above[-INF][m] == 2 and s.above[INF][m] == 0
    e = top_scores(c.kept[K - 1], c.kept[:K - 1], c.M, c.T)
    m = c.at["edges"]
    assert e.above[value_of(c.T - 1)][m] == 18 and e.above[value_of(c.T)][m] == 15 and e.above[1e200][m] == 0


# ---- 2. movers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_movers_every_split_every_by(crafted, kind):
    c = crafted
    with shape(kind):
        for la, lb in SPLITS:
            base, cur = kept_of(c, la), kept_of(c, lb)
            s = movers_scores(base, cur, c.M)
            bad = sorted(set(m for lst in (la, lb) for m, (_, counts, _) in enumerate(cells_of(c, lst)) if sum(counts) >= W))
            assert len(bad) <= 4
            ca, cb = cells_of(c, la), cells_of(c, lb)
            model_cand = [m for m in range(c.M) if ca[m][2] != 0 and cb[m][2] != 0]
            assert list(np.nonzero(s.cand)[0]) == model_cand
            for by, arg in MOVER_BYS:
                for first, n in ranges_without(bad, c.M):
                    for asc in (False, True):
                        for k in KS:
                            got = cur[-1].movers(base, k, by, arg, asc, cur[:-1], n, first)
                            what = (kind, la[:4], lb[:4], len(la) + len(lb), by, arg, asc, k, first, n)
                            same_entries(got, movers_want(s, by, arg, k, asc, first, n), what)
                            if k == 1024:                                        # names empty on a side are never returned
                                assert [int(x) for x in np.sort(got["id"])] == [m for m in model_cand if first <= m < first + n], what
                            if la == lb:                                         # a list against itself: all scores exactly 0, lowest ids first
                                assert np.all(got["score"] == 0) and list(got["id"]) == sorted(got["id"]), what
    assert len(SPLITS[-1][0]) + len(SPLITS[-1][1]) == N.MAX_KEPT


# ---- 3. the shapes agree ---------------------------------------------------------------------------------------------------------
def test_the_two_shapes_return_identical_bytes(crafted):
    c = crafted
    got = {}
    for kind in KINDS:
        with shape(kind):
            out = []
            for lst in (LISTS[5], LISTS[7], LISTS[-1]):
                kept = kept_of(c, lst)
                for by, arg in top_bys(c.T):
                    out.append(kept[-1].top(70, by, arg, False, kept[:-1], c.M, 0).tobytes())
            for la, lb in SPLITS[:3] + SPLITS[-1:]:
                for by, arg in MOVER_BYS:
                    out.append(c.kept[lb[-1]].movers(kept_of(c, la), 70, by, arg, True, kept_of(c, lb[:-1]), c.M, 0).tobytes())
            got[kind] = out
    assert got["wave"] == got["block"] and all(len(x) for x in got["wave"][:3])


# ---- 4. select edges: 4 097 names x 3 handles, the default switch ----------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled(native_lib, torch_cuda):
    """handles 0 and 1: tests/test_gpu_movers.py's DOZEN pairs, cyclically (base / cur); handle 2: the base rows one name on.
    Kept besides: two handles of other blocks with first != 0."""
    ra, rb = dozen_rows()
    rc = [dict(DOZEN[(m + 1) % len(DOZEN)][0]) for m in range(M_ROWS)]
    kept, parts = [], []
    with engine(M_ROWS, cell_bits=64, num_buffers=2) as e:
        for rows in (ra, rb, rc):
            with e.flip() as s:
                _import(s, rows, ["tight"] * M_ROWS)
                kept.append(s.keep(M_ROWS))
                if rows is ra:
                    parts = [s.keep(100, 50), s.keep(200, 20)]                   # rows 50 .. 149 and 20 .. 219
        t = types.SimpleNamespace(kept=kept, parts=parts, rows=[ra, rb, rc], torch=torch_cuda, e=e)
        t.top = top_scores(kept[1], [kept[0]], M_ROWS, tile())                   # list [0, 1]
        t.mov = movers_scores([kept[0]], [kept[1], kept[2]], M_ROWS)             # [0] against [1, 2]
        yield t
    for k_ in kept + parts:
        k_.close()


@pytest.mark.parametrize("nmetrics", SIZES)
def test_sizes_under_the_default_switch(tiled, nmetrics):
    t = tiled
    T = tile()
    for first in (0, M_ROWS - nmetrics):
        for k in (1, 64, 1024):
            for asc in (False, True):
                for by, arg in (("count", None), ("sum", None), ("percentile", 0.5), ("count_above", value_of(T))):
                    got = t.kept[1].top(k, by, arg, asc, [t.kept[0]], nmetrics, first)
                    same_entries(got, top_want(t.top, by, arg, k, asc, first, nmetrics), ("top", by, k, asc, first, nmetrics))
                for by, arg in (("ks", None), ("shift", None), ("percentile", 0.99)):
                    got = t.kept[2].movers(t.kept[0], k, by, arg, asc, [t.kept[1]], nmetrics, first)
                    same_entries(got, movers_want(t.mov, by, arg, k, asc, first, nmetrics), ("movers", by, k, asc, first, nmetrics))


def test_ties_at_the_cut_fewer_candidates_and_none(tiled):
    t = tiled
    # a tie group straddling the cut: by count some 340 rows share each value, far more than k leaves room for
    for asc in (False, True):
        got = t.kept[1].top(100, "count", None, asc, [t.kept[0]], M_ROWS, 0)
        assert len(set(int(x) for x in got["count"])) <= 2
        same_entries(got, top_want(t.top, "count", None, 100, asc, 0, M_ROWS), ("tie", asc))
        got = t.kept[2].movers(t.kept[0], 100, "ks", None, asc, [t.kept[1]], M_ROWS, 0)
        same_entries(got, movers_want(t.mov, "ks", None, 100, asc, 0, M_ROWS), ("tie", asc))
    # fewer candidates than k
    for first, n in ((0, 63), (NONE_FROM - 20, 150), (NONE_TO - 1, 2)):
        have = sum(1 for x in t.top.count[first:first + n] if x)
        got = t.kept[1].top(1024, "sum", None, False, [t.kept[0]], n, first)
        assert 0 < len(got) == have < 1024
        havem = int(t.mov.cand[first:first + n].sum())
        got = t.kept[2].movers(t.kept[0], 1024, "w1", None, False, [t.kept[1]], n, first)
        assert len(got) == havem < n
    # no candidate at all: n_out == 0 and `out` untouched
    empty = [m for m in range(M_ROWS) if t.top.count[m] == 0]
    assert empty
    out = np.zeros(8, dtype=N.TOP_ENTRY)
    out.view(np.uint8)[:] = 0x5a
    got = t.kept[1].top(8, "count", None, False, [t.kept[0]], 1, empty[0], out=out)
    assert got.shape == (0,) and np.all(out.view(np.uint8) == 0x5a)
    pair = movers_scores([t.kept[0]], [t.kept[1]], NONE_TO - NONE_FROM, NONE_FROM)
    assert not pair.cand.any()
    mout = np.zeros(8, dtype=N.MOVER_ENTRY)
    mout.view(np.uint8)[:] = 0x5a
    got = t.kept[1].movers(t.kept[0], 8, "ks", None, False, (), NONE_TO - NONE_FROM, NONE_FROM, out=mout)
    assert got.shape == (0,) and np.all(mout.view(np.uint8) == 0x5a)


# ---- 5. absolute ids and ranges --------------------------------------------------------------------------------------------------
def test_blocks_with_first_not_zero_and_range_errors(tiled):
    import loghisto_amd
    t, torch = tiled, tiled.torch
    a, b = t.parts                                                               # rows 50 .. 149 and 20 .. 219 of handle 0
    s = top_scores(t.kept[0], [t.kept[0]], M_ROWS, tile())                       # the same cells twice
    for first, n in ((50, 100), (60, 80), (147, 3), (149, 1)):
        for by, arg in (("count", None), ("sum", None), ("percentile", 0.99)):
            got = a.top(30, by, arg, False, [b], n, first)
            same_entries(got, top_want(s, by, arg, 30, False, first, n), (by, first, n))
            assert all(first <= int(i) < first + n for i in got["id"]) and len(got) == min(30, sum(1 for x in s.count[first:first + n] if x))
    got = a.top(5)                                                               # the defaults: this handle's block
    same_entries(got, top_want(top_scores(t.kept[0], [], M_ROWS, tile()), "count", None, 5, False, 50, 100), "defaults")
    got = t.kept[1].movers([a, b], 30, "shift", None, True, [b], 80, 60)         # base: handle 0's cells twice, cur: handle 1 + handle 0
    assert got["id"].min() >= 60 and got["id"].max() < 140 and len(got) == min(30, sum(1 for x in s.count[60:140] if x))
    got = a.movers(b, 7, "percentile", 0.5)                                      # the defaults; identical cells: score 0, lowest ids
    assert np.all(got["score"] == 0) and list(got["id"]) == [m for m in range(50, 150) if s.count[m]][:7]
    # a range outside one handle's block: LH_ERANGE, and out / n_out untouched
    ent = np.zeros(4, dtype=N.TOP_ENTRY)
    ent.view(np.uint8)[:] = 0x5a
    for first, n in ((49, 2), (50, 101), (149, 2), (20, 10), (0, 1), (150, 1)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            a.top(4, "count", None, False, [b], n, first, out=ent)
        assert ei.value.code == N.ERANGE and np.all(ent.view(np.uint8) == 0x5a), (first, n)
        with pytest.raises(loghisto_amd.LhError) as ei:
            t.kept[1].movers([a], 4, "ks", None, False, [b], n, first)
        assert ei.value.code == N.ERANGE, (first, n)
    dent = torch.full((4 * 32,), 0x5a, dtype=torch.uint8, device="cuda")
    dn = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(loghisto_amd.LhError) as ei:
        a.top(4, "count", None, False, [b], 2, 49, out=(dent, dn))
    torch.cuda.synchronize()
    assert ei.value.code == N.ERANGE and int(dn.cpu()[0]) == -7 and bool((dent == 0x5a).all())
    # the device-form empty call zeroes d_n_out (and writes no entry)
    a.top(4, "count", None, False, [b], 0, 60, out=(dent, dn))
    torch.cuda.synchronize()
    assert int(dn.cpu()[0]) == 0 and bool((dent == 0x5a).all())
    dn.fill_(-7)
    t.kept[1].movers([a], 4, "ks", None, False, [b], 0, 60, out=(dent, dn))
    torch.cuda.synchronize()
    assert int(dn.cpu()[0]) == 0 and bool((dent == 0x5a).all())
    assert a.top(4, "count", None, False, [b], 0, 60).shape == (0,)


# ---- 6. forms and lifetime -------------------------------------------------------------------------------------------------------
def _device_pair(torch, k):
    return (torch.full((k * 32,), 0x77, dtype=torch.uint8, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda"))


def _entries(pair, dtype):
    ent, n = pair
    return ent.cpu().numpy().view(dtype)[:int(n.cpu()[0])]


@pytest.mark.parametrize("kind", KINDS)
def test_device_form_pinned_and_pageable_out(crafted, kind):
    c, torch = crafted, crafted.torch
    with shape(kind):
        for lst, k in ((LISTS[5], 20), (LISTS[-1], 1024)):
            kept = kept_of(c, lst)
            for by, arg in (("sum", None), ("percentile", 0.99), ("count_above", 250.0)):
                host = kept[-1].top(k, by, arg, False, kept[:-1], c.M, 0)
                pair = _device_pair(torch, k)
                assert kept[-1].top(k, by, arg, False, kept[:-1], c.M, 0, out=pair, stream=torch.cuda.current_stream()) is pair
                torch.cuda.synchronize()
                assert _entries(pair, N.TOP_ENTRY).tobytes() == host.tobytes() and len(host)
                pinned = torch.zeros((k * 32,), dtype=torch.uint8, pin_memory=True).numpy().view(N.TOP_ENTRY)
                pageable = np.zeros(k, dtype=N.TOP_ENTRY)
                p = kept[-1].top(k, by, arg, False, kept[:-1], c.M, 0, out=pinned)
                q = kept[-1].top(k, by, arg, False, kept[:-1], c.M, 0, out=pageable)
                assert p.tobytes() == q.tobytes() == host.tobytes()
        base, cur = kept_of(c, [0, 1, 2]), kept_of(c, [3, 4, 5])
        for by, arg in MOVER_BYS:
            host = cur[-1].movers(base, 40, by, arg, True, cur[:-1], c.M, 0)
            pair = _device_pair(torch, 40)
            cur[-1].movers(base, 40, by, arg, True, cur[:-1], c.M, 0, out=pair)
            torch.cuda.synchronize()
            assert _entries(pair, N.MOVER_ENTRY).tobytes() == host.tobytes() and len(host)


@pytest.mark.parametrize("bits", (64, 32))
def test_release_waits_for_device_form_calls_on_two_streams(native_lib, torch_cuda, bits):
    """Device-form calls on TWO caller streams, with work ahead on the first, followed at once by close() of every listed handle
    (of both lists): close() waits for both streams' readers, and the results are what the same calls return with nothing in flight."""
    torch = torch_cuda
    M, n, k = 70, 50_000, 25
    rng = np.random.default_rng(23)
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
        for kind in KINDS:
            with shape(kind):
                want_a = ref[2].top(k, "percentile", 0.99, False, ref[:2], M, 0)
                want_b = ref[2].movers(ref[:1], k, "w1", None, False, ref[1:2], M - 3, 3)
                fresh = three(e)
                a, b = torch.cuda.Stream(), torch.cuda.Stream()
                out_a, out_b, junk = _device_pair(torch, k), _device_pair(torch, k), _device_pair(torch, k)
                torch.cuda.synchronize()
                for _ in range(20):                                              # work ahead on the first stream
                    fresh[2].top(k, "sum", None, False, fresh[:2], M, 0, out=junk, stream=a)
                fresh[2].top(k, "percentile", 0.99, False, fresh[:2], M, 0, out=out_a, stream=a)
                fresh[2].movers(fresh[:1], k, "w1", None, False, fresh[1:2], M - 3, 3, out=out_b, stream=b)
                for k_ in fresh:
                    k_.close()                                                   # waits for the readers on both streams
                a.synchronize()
                b.synchronize()
                assert _entries(out_a, N.TOP_ENTRY).tobytes() == want_a.tobytes() and len(want_a) == k, kind
                assert _entries(out_b, N.MOVER_ENTRY).tobytes() == want_b.tobytes() and len(want_b) == k, kind
        for k_ in ref:
            k_.close()


def test_the_records_block_regrows_behind_a_pending_device_form_call(tiled, crafted):
    """A small call, then -- nothing waited for -- a device-form call on a stream of its own, then a host-form call of more rows than
    the records block has held so far in this unit (it is freed and allocated again behind the pending passes): all three are what
    the same calls return afterwards."""
    t, c, torch = tiled, crafted, tiled.torch
    big_e = 12000
    with engine(big_e, cell_bits=64, num_buffers=2) as e:
        rng = np.random.default_rng(3)
        e.submit_pairs(rng.integers(0, big_e, 60_000).astype(np.uint32), rng.lognormal(3.0, 1.0, 60_000))
        with e.flip() as s:
            big = s.keep(big_e)
    try:
        kept = kept_of(c, LISTS[5])
        st = torch.cuda.Stream()
        pair = _device_pair(torch, 50)
        torch.cuda.synchronize()
        small = kept[-1].top(50, "sum", None, False, kept[:-1], c.M, 0).copy()
        t.kept[2].movers(t.kept[0], 50, "shift", None, False, [t.kept[1]], M_ROWS, 0, out=pair, stream=st)
        large = big.top(50, "sum", None, False, (), big_e, 0).copy()
        st.synchronize()
        mid = _entries(pair, N.MOVER_ENTRY)
        torch.cuda.synchronize()
        assert len(small) == 50 and len(mid) == 50 and len(large) == 50
        assert small.tobytes() == kept[-1].top(50, "sum", None, False, kept[:-1], c.M, 0).tobytes()
        assert mid.tobytes() == t.kept[2].movers(t.kept[0], 50, "shift", None, False, [t.kept[1]], M_ROWS, 0).tobytes()
        assert large.tobytes() == big.top(50, "sum", None, False, (), big_e, 0).tobytes()
        assert list(large["sum"]) == sorted(large["sum"], reverse=True)
    finally:
        big.close()


# ---- 7. equal to the import route --------------------------------------------------------------------------------------------------
def _agree(a, b, exact, tol, what):
    """two full rankings of the same candidates: the same ids; where the order differs, the two names' exact scores are closer than
    their bounds allow to tell apart"""
    assert sorted(a["id"]) == sorted(b["id"]), what
    for x, y in zip(a["id"], b["id"]):
        if x != y:
            assert abs(exact[int(x)] - exact[int(y)]) <= tol[int(x)] + tol[int(y)], (what, int(x), int(y))


def test_equal_to_the_import_route(crafted):
    c = crafted
    with engine(c.M, cell_bits=64, num_buffers=3) as e2:
        for la, lb in (([0, 1, 2], [3, 4, 5]), ([0], [1]), ([BIG], [BIG, BIG])):
            with e2.flip() as sa, e2.flip() as sb:
                for i in la:
                    c.kept[i].add_to(sa)
                for i in lb:
                    c.kept[i].add_to(sb)
                base, cur = kept_of(c, la), kept_of(c, lb)
                ca, cb = cells_of(c, la), cells_of(c, lb)
                bad = sorted(set(m for cells in (ca, cb) for m, (_, counts, _) in enumerate(cells) if sum(counts) >= W))
                for first, n in ranges_without(bad, c.M):
                    ex = {m: Exact(cb[m][0], cb[m][1]) for m in range(first, first + n)}
                    for by, arg in top_bys(c.T):
                        got = cur[-1].top(1024, by, arg, False, cur[:-1], n, first)
                        ref = sb.top(1024, by, arg, False, n, first)
                        what = ("top", lb, by, arg, first, n)
                        if by == "sum":
                            _agree(got, ref, {m: x.S for m, x in ex.items()}, {m: Fraction(1e-12) * x.A for m, x in ex.items()}, what)
                        else:
                            assert list(got["id"]) == list(ref["id"]), what
                        by_id = {int(r["id"]): r for r in ref}
                        for g in got:
                            r, x = by_id[int(g["id"])], ex[int(g["id"])]
                            assert (g["pkey"], g["count"], g["above"]) == (r["pkey"], r["count"], r["above"]), what
                            for v in (g["sum"], r["sum"]):
                                assert abs(Fraction(float(v)) - x.S) <= Fraction(1e-12) * x.A, what
                    models = {m: pair_model(dict(zip(ca[m][0], ca[m][1])), dict(zip(cb[m][0], cb[m][1]))) for m in range(first, first + n)}
                    for by, arg in MOVER_BYS:
                        got = cur[-1].movers(base, 1024, by, arg, False, cur[:-1], n, first)
                        ref = sb.movers(sa, 1024, by, arg, False, n, first)
                        what = ("movers", la, lb, by, arg, first, n)
                        if by in ("w1", "shift"):
                            tol = {m: 4 * w["n"] * EPS * (1 + w["w1"]) for m, w in models.items() if w["w1"] is not None}
                            exact = {m: w[by] for m, w in models.items() if w["w1"] is not None}
                            _agree(got, ref, exact, tol, what)
                            for res in (got, ref):
                                for g in res:
                                    assert abs(Fraction(float(g["score"])) - exact[int(g["id"])]) <= tol[int(g["id"])], what
                        else:
                            assert got.tobytes() == ref.tobytes(), what          # ks: a fixed function of exact integers
                        by_id = {int(r["id"]): r for r in ref}
                        for g in got:
                            r = by_id[int(g["id"])]
                            assert (g["key"], g["key_base"], g["count_a"], g["count_b"]) == (r["key"], r["key_base"], r["count_a"], r["count_b"]), what


# ---- 8. read-only ----------------------------------------------------------------------------------------------------------------
def test_read_only(crafted):
    c, torch = crafted, crafted.torch
    before = [[a.tobytes() for a in arrays_of(k_)] for k_ in c.kept]
    for kind in KINDS:
        with shape(kind):
            c.kept[K - 1].top(70, "percentile", 0.5, False, c.kept[:K - 1], c.M, 0)
            c.kept[5].movers(c.kept[:3], 70, "w1", None, False, c.kept[3:5], c.M, 0)
            pair = _device_pair(torch, 10)
            c.kept[K - 1].top(10, "count_above", 250.0, True, c.kept[:K - 1], c.M, 0, out=pair)
    torch.cuda.synchronize()
    assert [[a.tobytes() for a in arrays_of(k_)] for k_ in c.kept] == before


# ---- 9. the timing hooks ---------------------------------------------------------------------------------------------------------
def test_the_timing_hooks_run_both_passes(tiled):
    t = tiled
    L = N.lib()
    one = (C.c_void_p * 2)(t.kept[0]._h.value, t.kept[1]._h.value)
    two = (C.c_void_p * 1)(t.kept[2]._h.value)
    for by in range(4):
        a, b = C.c_float(-1.0), C.c_float(-1.0)
        assert L.lh_tool_kept_top_passes_ms(C.addressof(one), 2, 0, M_ROWS, by, 0.5, 20, 0, None, C.byref(a), C.byref(b)) == 0
        assert a.value > 0 and b.value > 0 and math.isfinite(a.value + b.value)
        a, b = C.c_float(-1.0), C.c_float(-1.0)
        assert L.lh_tool_kept_movers_passes_ms(C.addressof(one), 2, C.addressof(two), 1, 0, M_ROWS, by, 0.5, 20, 0, None, C.byref(a),
                                               C.byref(b)) == 0
        assert a.value > 0 and b.value > 0 and math.isfinite(a.value + b.value)
