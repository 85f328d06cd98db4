"""lh_kept_slide (Kept.slide, KeptWindow): a rolling window of kept intervals advanced exactly -- one new handle that holds,
per row and bin, the 64-bit sum over the `add` handles minus the sum over the `sub` handles: bit for bit what lh_kept_merge
gives for the new window's handles.

The inputs are the crafted handles of tests/test_gpu_kept.py (70 rows, 6 handles, engines of 64- and of 32-bit cells) and a
few small handles of this file's own (add_buckets + keep): cells at either side of every edge of the two-tile width
(lh_tool_kept_compare_tile) on opposite sides of the call, more than 64 entries of one handle in one tile, an empty stretch
between tiles, bins 0 and 65 535, and subtrahends that go below zero in chosen cells.  The references are lh_kept_merge of the
same window, Python integers over the fixture's rows, and loghisto_amd.keptfile.combine over the saved blobs.  Every check
runs under both kernel shapes (lh_tool_kept_switch) and the two shapes' bytes are compared.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib
import ctypes as C
import itertools
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from loghisto_amd import keptfile
from tests.test_gpu_across import P_MAIN
from tests.test_gpu_compare import _import
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import K, LISTS, arrays_of, crafted, same_listing, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_merge import listing, summed

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
WRAP = 1 << 64
KINDS = ("wave", "block")
SENTINEL = 0x77


def key_of(b):
    return int(oracle.bin_to_key(b))


def bytes_of(k):
    return [a.tobytes() for a in arrays_of(k)]


def merge(handles, **kw):
    return handles[-1].merge(handles[:-1], **kw)


def slide(add, sub=(), **kw):
    return add[0].slide(add[1:], sub, **kw)


def raw(add, sub, first, n):
    """lh_kept_slide itself -> (code, why's bytes before, why's bytes after, why, out): out starts as SENTINEL"""
    VP = C.c_void_p
    a = (VP * len(add))(*[k._h.value for k in add])
    s = (VP * max(len(sub), 1))(*[k._h.value for k in sub])
    why = N.LhKeptUnder(struct_size=16, row=0x11223344, key=-77, reserved0=0x5566, reserved1=0x778899aa)
    was = bytes(why)
    out = VP(SENTINEL)
    rc = N.lib().lh_kept_slide(a, len(add), s if sub else None, len(sub), first, n, 0, None, C.byref(why), C.byref(out))
    return rc, was, bytes(why), why, out


def diff_model(add_rows, sub_rows, M):
    """Python integers: per row {bin: A - S} of the sums mod 2^64 (zeros dropped), or ("under", row, bin) of the lowest row's
    lowest bin with S > A.  add_rows / sub_rows: per handle its rows [{bin: count}]."""
    out = []
    for m in range(M):
        A, S = {}, {}
        for side, lst in ((A, add_rows), (S, sub_rows)):
            for rows in lst:
                for b, x in rows[m].items():
                    side[b] = (side.get(b, 0) + x) % WRAP
        under = sorted(b for b, x in S.items() if x > A.get(b, 0))
        if under:
            return ("under", m, under[0])
        out.append({b: A[b] - S.get(b, 0) for b in A if A[b] - S.get(b, 0)})
    return out


def refused(add, sub, first, n, row, b, what=""):
    """An underflow refusal, through the library and through Kept.slide: LH_ERANGE, the cell named, out untouched."""
    import loghisto_amd
    rc, was, now, why, out = raw(add, sub, first, n)
    assert rc == N.ERANGE and out.value == SENTINEL, (what, rc)
    assert (why.struct_size, why.row, why.key, why.reserved0, why.reserved1) == (16, row, key_of(b), 0, 0), (what, why.row, why.key)
    with pytest.raises(loghisto_amd.KeptUnderflow) as e:
        slide(add, sub, first=first, nmetrics=n)
    assert (e.value.row, e.value.key) == (row, key_of(b)), what


# ---- this file's own handles ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own(native_lib, torch_cuda):
    t = C.c_uint32(0)
    assert N.lib().lh_tool_kept_compare_tile(C.byref(t)) == 0 and 256 <= t.value <= 4096
    T = int(t.value)
    M = 6
    edges = [0, T - 1, T, 2 * T - 1, 2 * T, NK - 1]
    rows = {
        # P: the window.  Row 0: a cell either side of every edge; row 1: 200 entries in one tile; row 2: two tiles far apart;
        # row 3: nothing; row 4: a cell per tile over five tiles; row 5 (the last): bin 65 535 and one more
        "P": [{b: 5 + 2 * i for i, b in enumerate(edges)}, {b: 3 for b in range(20000, 20200)}, {10001: 4, 40001: 6}, {},
              {1000 + i * T: 2 for i in range(5)}, {100: 1, NK - 1: 15}],
        # Q: taken away from P without going below zero: the edge cells alternately in full and in part (so that of two cells
        # either side of an edge one goes and one stays), 100 of the 200, the far tile's cell
        "Q": [{0: 1, T - 1: 7, T: 2, 2 * T - 1: 11, 2 * T: 1, NK - 1: 15}, {b: 3 for b in range(20050, 20150)}, {40001: 6}, {},
              {1000 + 2 * T: 2, 1000 + 4 * T: 1}, {NK - 1: 15}],
        "last_cell": [{}, {}, {}, {}, {}, {NK - 1: 16}],                       # one more than P's, in the last bin of the last row
        "absent": [{}, {12345: 1}, {}, {}, {}, {}],                            # a bin P's row does not hold
        "two_rows": [{}, {}, {10001: 5}, {}, {1000: 3, 1000 + T: 3}, {}],      # rows 2 and 4 go below zero
        "later_tile": [{}, {}, {10001: 4, 40001: 7}, {}, {}, {}],              # the first tile's cell is fine, the second's is not
        "empty_row": [{}, {}, {}, {7: 1}, {}, {}],                             # P's row 3 has no cell at all
    }
    kept = {}
    with engine(M, cell_bits=64) as e:
        for name, r in rows.items():
            with e.flip() as s:
                _import(s, r, [None] * M)
                kept[name] = s.keep(M)
    yield types.SimpleNamespace(kept=kept, rows=rows, M=M, T=T, edges=edges)
    for k in kept.values():
        k.close()


# ---- 1. without sub: the merge -------------------------------------------------------------------------------------------------
def test_without_sub_it_is_the_merge(crafted):
    c = crafted
    got = {}
    for kind in KINDS:
        with shape(kind), contextlib.ExitStack() as stack:
            for lst in LISTS:
                hs = [c.kept[i] for i in lst]
                s, m = stack.enter_context(slide(hs)), stack.enter_context(merge(hs))
                assert bytes_of(s) == bytes_of(m) and s.info == m.info, (kind, lst[:8], len(lst))
                got[kind, tuple(lst)] = bytes_of(s)
    for lst in LISTS:
        assert got["wave", tuple(lst)] == got["block", tuple(lst)], lst[:8]


# ---- 2. every split of the six handles -----------------------------------------------------------------------------------------
def test_every_split_gives_the_merge_of_what_stays(crafted):
    c = crafted
    everything = list(range(K))
    exact = [not wrapped for _, wrapped in summed(c, everything)]
    assert exact.count(False) <= 3                                           # the rows built to pass 2^64, if listed often enough
    runs = [(g[0], len(g)) for ok, g in ((ok, list(g)) for ok, g in itertools.groupby(range(c.M), key=lambda m: exact[m])) if ok]
    assert sum(n for _, n in runs) >= c.M - 3
    got = {}
    for kind in KINDS:
        with shape(kind):
            for first, n in runs:
                blk = dict(first=first, nmetrics=n)
                with merge([c.kept[i] for i in everything], **blk) as whole:
                    for r in range(1, K + 1):
                        for A in itertools.combinations(everything, r):
                            B = [i for i in everything if i not in A]
                            hA, hB = [c.kept[i] for i in A], [c.kept[i] for i in B]
                            with merge(hA, **blk) as want, slide([whole], hB, **blk) as one, slide(hA + hB, hB, **blk) as two:
                                w = bytes_of(want)
                                assert bytes_of(one) == w and one.info == want.info, (kind, A, first)
                                assert bytes_of(two) == w and two.info == want.info, (kind, A, first)
                                got[kind, A, first] = w
    assert all(got["wave", A, f] == v for (kind, A, f), v in got.items() if kind == "block")


# ---- 3. against the integer model and keptfile.combine ---------------------------------------------------------------------------
def test_against_the_model_and_the_numpy_reference(crafted):
    import loghisto_amd
    c = crafted
    blobs = [k.to_bytes() for k in c.kept]
    cases = [([0, 1, 2], [1]), ([0, 0], [0])] + [([k], [k]) for k in range(K)]
    got = {}
    for kind in KINDS:
        with shape(kind):
            for add, sub in cases:
                what = (kind, add, sub)
                want = diff_model([c.rows[i] for i in add], [c.rows[i] for i in sub], c.M)
                assert isinstance(want, list), what
                with slide([c.kept[i] for i in add], [c.kept[i] for i in sub]) as s:
                    same_listing(s, listing(want), what)
                    assert s.info["first"] == 0 and s.info["device"] == 0
                    if add == sub:
                        assert s.info["cells"] == 0 and s.info["samples"] == 0 and s.info["bytes"] == 8 * (2 * c.M + 1), what
                    blob = s.to_bytes()
                    assert blob == keptfile.combine([blobs[i] for i in add], [blobs[i] for i in sub]), what
                    with loghisto_amd.Kept.from_bytes(blob) as back:
                        assert bytes_of(back) == bytes_of(s) and back.info == s.info, what
                    got[kind, tuple(add), tuple(sub)] = blob
    assert all(got["wave", a, s] == v for (kind, a, s), v in got.items() if kind == "block")


# ---- 4. this file's own handles: the tile edges, and going below zero -------------------------------------------------------------
def test_cells_either_side_of_the_tile_edges(own):
    o, T = own, own.T
    P, Q = o.kept["P"], o.kept["Q"]
    want = diff_model([o.rows["P"]], [o.rows["Q"]], o.M)
    assert want[0] == {0: 4, T: 7, 2 * T: 12} and len(want[1]) == 100 and want[2] == {10001: 4} and want[3] == {}
    assert want[4] == {1000: 2, 1000 + T: 2, 1000 + 3 * T: 2, 1000 + 4 * T: 1} and want[5] == {100: 1}
    got = {}
    for kind in KINDS:
        with shape(kind):
            with slide([P], [Q]) as s, slide([P, Q], [Q, Q]) as s2, slide([P, P, Q], [P, Q, Q]) as s3:
                same_listing(s, listing(want), kind)
                assert bytes_of(s2) == bytes_of(s) and bytes_of(s3) == bytes_of(s) and s2.info == s.info == s3.info
                assert s.to_bytes() == keptfile.combine([P.to_bytes()], [Q.to_bytes()])
                got[kind] = bytes_of(s)
            with slide([P, Q], [Q]) as s, merge([P]) as m:                     # on both sides: it cancels
                assert bytes_of(s) == bytes_of(m) and s.info == m.info
            with slide([P, Q]) as s:
                same_listing(s, listing(diff_model([o.rows["P"], o.rows["Q"]], [], o.M)), kind)
    assert got["wave"] == got["block"]


def test_underflow_is_refused_with_the_lowest_row_and_bin(crafted, own):
    c, o, T = crafted, own, own.T
    P, blobs = o.kept["P"], {k: v.to_bytes() for k, v in own.kept.items()}
    m01 = diff_model([c.rows[0]], [c.rows[1]], c.M)
    assert m01[0] == "under"
    own_cases = [("last_cell", o.M - 1, NK - 1), ("absent", 1, 12345), ("two_rows", 2, 10001), ("later_tile", 2, 40001),
                 ("empty_row", 3, 7)]
    for kind in KINDS:
        with shape(kind):
            refused([c.kept[0]], [c.kept[1]], 0, c.M, m01[1], m01[2], kind)    # the crafted pair, by the model
            with slide([c.kept[0], c.kept[1]], [c.kept[1]]) as s, merge([c.kept[0]]) as m:      # a valid call right behind it
                assert bytes_of(s) == bytes_of(m)
            for name, row, b in own_cases:
                assert diff_model([o.rows["P"]], [o.rows[name]], o.M) == ("under", row, b), name
                with pytest.raises(keptfile.KeptUnderflow) as e:
                    keptfile.combine([blobs["P"]], [blobs[name]])
                assert (e.value.row, e.value.key) == (row, key_of(b)), name
                refused([P], [o.kept[name]], 0, o.M, row, b, (kind, name))
                with slide([P, o.kept[name]], [o.kept[name]]) as s, merge([P]) as m:
                    assert bytes_of(s) == bytes_of(m), (kind, name)
            # what the own cases were made for
            assert o.rows["later_tile"][2][10001] <= o.rows["P"][2][10001] and 40001 - 10001 > 2 * T
            assert 12345 not in o.rows["P"][1] and not o.rows["P"][3]
            # the rows asked for alone decide: "two_rows" without row 2 names row 4's lowest bin, without either none
            refused([P], [o.kept["two_rows"]], 3, 3, 4, 1000, kind)
            with slide([P], [o.kept["two_rows"]], first=0, nmetrics=2) as s, merge([P], first=0, nmetrics=2) as m:
                assert bytes_of(s) == bytes_of(m)
            # a sub-block: `row` is the metric id, not the row within the block
            refused([P], [o.kept["last_cell"]], o.M - 1, 1, o.M - 1, NK - 1, kind)
            # the 2^64 corner: the add side wraps to 0 (2^63 twice), so any subtrahend looks too large -- refused like any other
            m = c.at["half_of_2^64"]
            refused([c.kept[3], c.kept[3]], [c.kept[3]], m, 1, m, 100, kind)


# ---- 5. blocks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_blocks(crafted, kind):
    import loghisto_amd
    c = crafted
    sub, _ = c.extra["sub"]                                                       # rows [3, 8) of handle 0
    with shape(kind):
        with slide([sub, c.kept[1]], [c.kept[1]], first=3, nmetrics=5) as s:
            assert bytes_of(s) == bytes_of(sub) and s.info == sub.info
        with slide([c.kept[0], c.kept[1]], [sub], first=3, nmetrics=5) as s, merge([c.kept[1]], first=3, nmetrics=5) as m:
            assert bytes_of(s) == bytes_of(m) and s.info == m.info and s.info["first"] == 3
        with sub.slide() as s:                                                    # first=None, nmetrics=None: the handle's own block
            assert bytes_of(s) == bytes_of(sub) and s.info == sub.info
        with slide([c.kept[0]], first=c.M - 1) as s, merge([c.kept[0]], first=c.M - 1) as m:
            assert bytes_of(s) == bytes_of(m) and s.info["nrows"] == 1
        for add, subs in (([sub, c.kept[1]], [c.kept[1]]), ([c.kept[1]], [sub]), ([c.kept[0], sub], [])):
            for first, n in ((2, 5), (3, 6), (0, c.M), (8, 1)):
                rc, was, now, _, out = raw(add, subs, first, n)
                assert rc == N.ERANGE and now == was and out.value == SENTINEL, (first, n)
                with pytest.raises(loghisto_amd.LhError) as ei:
                    slide(add, subs, first=first, nmetrics=n)
                assert ei.value.code == N.ERANGE and not isinstance(ei.value, loghisto_amd.KeptUnderflow), (first, n)


# ---- 6. the readers over the slid handle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_readers_over_the_slid_handle_equal_readers_over_the_merge(crafted, kind):
    c = crafted
    bounds = [-5.0, 0.0, 1.0, 80.0, 1e3, 1e12]
    with shape(kind), contextlib.ExitStack() as stack:
        for window, newest, oldest in (([0, 1, 2], 3, 0), ([1, 2, 3], 4, 1), ([2, 3, 4], 5, 2)):
            old = stack.enter_context(merge([c.kept[i] for i in window]))
            slid = stack.enter_context(slide([old, c.kept[newest]], [c.kept[oldest]]))
            want = stack.enter_context(merge([c.kept[i] for i in window[1:] + [newest]]))
            assert bytes_of(slid) == bytes_of(want) and slid.info == want.info
            for a, b in ((slid.across((), P_MAIN), want.across((), P_MAIN)), (slid.count_le(bounds), want.count_le(bounds)),
                         (slid.spread(P_MAIN), want.spread(P_MAIN))):
                assert set(a) == set(b)
                for f in a:
                    assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), (window, f)


# ---- 7. the window ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_window_of_four_over_nine_intervals(native_lib, torch_cuda, kind):
    import loghisto_amd
    M, n, size = 9, 3000, 4
    rng = np.random.default_rng(23)
    kept = []
    with engine(M, cell_bits=32) as e:
        for i in range(9):
            e.submit_pairs(rng.integers(0, M - 1, n).astype(np.uint32), rng.lognormal(3.0 + 0.2 * i, 1.0, n))   # the last name: none
            with e.flip() as s:
                kept.append(s.keep(M))
    before = [bytes_of(k) for k in kept]
    with shape(kind), loghisto_amd.KeptWindow(size) as w:
        for i, k in enumerate(kept):
            gone = w.push(k)
            live = kept[max(0, i + 1 - size):i + 1]
            assert gone is (kept[i - size] if i >= size else None), i
            assert list(w.handles) == live
            with merge(live) as want:
                assert bytes_of(w.total) == bytes_of(want) and w.total.info == want.info, i
            assert w.total.info["samples"] == n * len(live)
        total = w.total
    assert w.total is None and total._h is None and not w.handles                  # close() released what the window made
    assert [bytes_of(k) for k in kept] == before                                    # ... and the caller's handles are usable
    with merge(kept[-size:]) as m:
        assert m.info["samples"] == size * n
    for k in kept:
        k.close()
