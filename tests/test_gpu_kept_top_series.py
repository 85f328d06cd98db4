"""lh_kept_top_series* and lh_kept_movers_series* (Kept.top_series, Kept.movers_series, KeptWindow.top_series / movers_series):
lh_kept_top's and lh_kept_movers' selections per WINDOW of a list of kept intervals, in one call.

The yardstick is the parent: per window, Kept.top over the slice -- Kept.movers over the two slices -- gives the expected entries
and their number, and the window's block is compared with it as BYTES (tobytes: sum and score included).  On the crafted fixture of
tests/test_gpu_kept.py (70 names x 6 handles, engines of 64- and of 32-bit cells) under both kernel shapes (lh_tool_kept_switch,
which here takes the ENTRIES of a call), and on the 4 097 names x 3 handles of tests/test_gpu_kept_select.py for the select pass's
sizes under the default switch.  A name whose total passes 2^64 in some window's slice has an unspecified rank in the parents and
therefore here: for every `by` but "count" the ranked ranges leave such names out (ranges_without).
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import ctypes as C
import contextlib
import math

import numpy as np
import pytest

from loghisto_amd import _native as N
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import BIG, K, LISTS, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_drift import DRIFT, sides
from tests.test_gpu_kept_readers import cells_of, value_of
from tests.test_gpu_kept_select import KS, MOVER_BYS, SIZES, kept_of, ranges_without, tiled, top_bys  # noqa: F401  (tiled: the fixture)
from tests.test_gpu_kept_series import CASES, WINDOWS
from tests.test_gpu_movers import M_ROWS

pytestmark = pytest.mark.gpu

W = 1 << 64
KINDS = ("wave", "block")
PATTERN = 0x5a
ALL = list(range(K))
ENTRY = {"top": N.TOP_ENTRY, "movers": N.MOVER_ENTRY}
_BAD = {}


# ---- the one call and the parent, on handle numbers of the crafted fixture (or on Kept objects: of=) --------------------------------
def top_series(kept, windows, k, by, arg, asc, n, first, **kw):
    return kept[-1].top_series(k, by, arg, asc, kept[:-1], windows, n, first, **kw)


def movers_series(kept, windows, k, by, arg, asc, n, first, **kw):
    return kept[-1].movers_series(k, by, arg, asc, kept[:-1], windows, None, n, first, **kw)


def top(kept, window, k, by, arg, asc, n, first):
    sl = kept[window[0]:window[1]]
    return sl[-1].top(k, by, arg, asc, sl[:-1], n, first)


def movers(kept, window, k, by, arg, asc, n, first):
    base, cur = sides(kept, window)
    return cur[-1].movers(base, k, by, arg, asc, cur[:-1], n, first)


CALL = {"top": (top_series, top), "movers": (movers_series, movers)}


def check_windows(which, kept, windows, k, by, arg, asc, n, first, what):
    """the one call against the parent, window by window, through a pattern-filled `out`: bytes, lengths, and nothing written at or
    beyond n_out[w] in any window's block; -> the per-window arrays"""
    series, parent = CALL[which]
    out = np.zeros(len(windows) * k, dtype=ENTRY[which])
    out.view(np.uint8)[:] = PATTERN
    got = series(kept, windows, k, by, arg, asc, n, first, out=out)
    assert len(got) == len(windows), what
    raw = out.view(np.uint8).reshape(len(windows), k * 32)
    for w, window in enumerate(windows):
        want = parent(kept, window, k, by, arg, asc, n, first)
        assert len(got[w]) == len(want) and got[w].tobytes() == want.tobytes(), (what, w, window, got[w][:4], want[:4])
        assert raw[w, :len(want) * 32].tobytes() == want.tobytes(), (what, w)
        assert np.all(raw[w, len(want) * 32:] == PATTERN), (what, w)
    return got


def wrapped(c, lists):
    """the names whose total passes 2^64 in one of the lists of handle numbers"""
    bad = set()
    for lst in lists:
        key = (c.wide, tuple(lst))
        if key not in _BAD:
            _BAD[key] = [m for m, (_, counts, _) in enumerate(cells_of(c, lst)) if sum(counts) >= W]
        bad |= set(_BAD[key])
    return sorted(bad)


def spans_of(bad, M):
    """the ranked ranges, and a sub-range with first > 0 inside the longest"""
    spans = ranges_without(bad, M)
    first, n = max(spans, key=lambda s: s[1])
    return spans + [(first + 3, n - 7)]


# ---- 1. every window set x every by, both directions, every k ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_top_series_every_window_set(crafted, kind):
    c = crafted
    with shape(kind):
        for lst, windows, name in CASES:
            kept = kept_of(c, lst)
            bad = wrapped(c, [lst[lo:hi] for lo, hi in windows])
            for by, arg in top_bys(c.T):
                for first, n in spans_of([] if by == "count" else bad, c.M):
                    for asc in (False, True):
                        for k in KS:
                            got = check_windows("top", kept, windows, k, by, arg, asc, n, first, (kind, name, by, arg, asc, k, first, n))
                            if name == "repeated":                                   # windows 0 and 2 are the same slice
                                assert got[0].tobytes() == got[2].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_movers_series_every_window_set(crafted, kind):
    c = crafted
    short = 0
    with shape(kind):
        for name, (lst, windows) in DRIFT.items():
            kept = kept_of(c, lst)
            bad = wrapped(c, [s for window in windows for s in sides(lst, window)])
            for by, arg in MOVER_BYS:
                for first, n in spans_of(bad, c.M):
                    for asc in (False, True):
                        for k in KS:
                            got = check_windows("movers", kept, windows, k, by, arg, asc, n, first, (kind, name, by, arg, asc, k, first, n))
                            if name == "repeated":
                                assert got[0].tobytes() == got[2].tobytes()
                            if name == "identical":                                  # score 0 everywhere: the lowest ids win
                                for g in got:
                                    assert np.all(g["score"] == 0) and list(g["id"]) == sorted(g["id"])
                            if name == "empty_side":
                                short += sum(1 for g in got if 0 < len(g) < min(k, n))
    assert short                                                                     # windows with fewer candidates than k (none at all: below)
    assert sum(hi - lo for s in DRIFT["32+32"][1][0] for lo, hi in [s]) == N.MAX_KEPT


def test_the_two_shapes_give_identical_bytes(crafted):
    c = crafted
    got = {}
    for kind in KINDS:
        with shape(kind):
            out = []
            for lst, windows, name in CASES:
                for by, arg in top_bys(c.T):
                    out += [g.tobytes() for g in top_series(kept_of(c, lst), windows, 70, by, arg, False, c.M, 0)]
            for name, (lst, windows) in DRIFT.items():
                for by, arg in MOVER_BYS:
                    out += [g.tobytes() for g in movers_series(kept_of(c, lst), windows, 70, by, arg, True, c.M, 0)]
            got[kind] = out
    assert got["wave"] == got["block"] and all(len(x) for x in got["wave"][:3])


# ---- 2. a window without candidates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_window_without_candidates_is_left_untouched(crafted, kind):
    """One name, a window per handle: the handles that hold no sample of it have n_out[w] = 0 and an untouched block, between
    windows that have the name."""
    c, torch = crafted, crafted.torch
    kept = kept_of(c, ALL)
    per = [k_.across((), [0.5], c.M, 0)["count"] for k_ in kept]
    m = next(m for m in range(c.M) if any(p[m] == 0 for p in per) and per[0][m] and per[K - 1][m])
    empty = [i for i in range(K) if per[i][m] == 0]
    singles = WINDOWS["singletons"]
    with shape(kind):
        got = check_windows("top", kept, singles, 4, "sum", None, False, 1, m, (kind, "none"))
        assert [len(g) for g in got] == [0 if i in empty else 1 for i in range(K)] and empty
        pairs = [((0, 1), (i, i + 1)) for i in range(K)]
        got = check_windows("movers", kept, pairs, 4, "ks", None, False, 1, m, (kind, "none"))
        assert [len(g) for g in got] == [0 if i in empty else 1 for i in range(K)]
        # the device form: the same counts, and the blocks of the empty windows keep their bytes
        ent = torch.full((K * 4 * 32,), PATTERN, dtype=torch.uint8, device="cuda")
        cnt = torch.full((K + 2,), -7, dtype=torch.int32, device="cuda")
        top_series(kept, singles, 4, "sum", None, False, 1, m, out=(ent, cnt[:K]))
        torch.cuda.synchronize()
        assert list(cnt.cpu().numpy()) == [0 if i in empty else 1 for i in range(K)] + [-7, -7]
        blocks = ent.cpu().numpy().reshape(K, 4 * 32)
        for i in range(K):
            assert np.all(blocks[i, (0 if i in empty else 32):] == PATTERN), i


# ---- 3. select sizes: 4 097 names x 3 handles, the default switch ------------------------------------------------------------------
TOP3 = [(0, 2), (2, 3), (0, 3)]
MOV3 = [((0, 1), (1, 3)), ((2, 3), (0, 2)), ((1, 2), (1, 2))]


@pytest.mark.parametrize("nmetrics", SIZES)
def test_sizes_under_the_default_switch(tiled, nmetrics):
    """the per-window offset w * npad: nmetrics that are no multiple of 4, a record tile boundary at 4 096"""
    t = tiled
    for first in (0, M_ROWS - nmetrics):
        for k in (1, 1024):
            for asc in (False, True):
                for by, arg in (("count", None), ("sum", None), ("percentile", 0.5), ("count_above", value_of(512))):
                    check_windows("top", t.kept, TOP3, k, by, arg, asc, nmetrics, first, ("top", by, k, asc, first, nmetrics))
                for by, arg in (("ks", None), ("shift", None), ("percentile", 0.99)):
                    check_windows("movers", t.kept, MOV3, k, by, arg, asc, nmetrics, first, ("movers", by, k, asc, first, nmetrics))


# ---- 4. the most windows a call takes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_128_windows_of_one_handle_each(crafted, kind):
    c = crafted
    kept = kept_of(c, ALL)
    singles = [(i % K, i % K + 1) for i in range(N.MAX_WINDOWS)]
    pairs = [((i % K, i % K + 1), ((i + 1) % K, (i + 1) % K + 1)) for i in range(N.MAX_WINDOWS)]
    bad = wrapped(c, [[i] for i in ALL])
    with shape(kind):
        check_windows("top", kept, singles, 3, "count", None, False, c.M, 0, (kind, "128"))
        for first, n in ranges_without(bad, c.M):
            for asc in (False, True):
                check_windows("top", kept, singles, 3, "percentile", 0.99, asc, n, first, (kind, "128", first, n))
                check_windows("movers", kept, pairs, 3, "w1", None, asc, n, first, (kind, "128", first, n))
        with pytest.raises(Exception):
            top_series(kept, singles + [(0, 1)], 3, "count", None, False, c.M, 0)


# ---- 5. chunks ----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def select_bytes(value):
    prev, now = C.c_uint64(0), C.c_uint64(0)
    assert N.lib().lh_tool_kept_select_bytes(value, C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_kept_select_bytes(prev.value, C.byref(now)) == 0 and now.value == value


@pytest.mark.parametrize("kind", KINDS)
def test_chunks_of_one_and_of_two_windows_give_the_bytes_of_one_chunk(crafted, kind):
    c, torch = crafted, crafted.torch
    kept = kept_of(c, ALL)
    record = 5 * 8 * 72                                                              # 70 names padded to four, five fields of 8 bytes
    tops = WINDOWS["rolling"]
    pairs = DRIFT["consecutive"][1]
    assert len(tops) == len(pairs) == 5
    bad = wrapped(c, [ALL[lo:hi] for lo, hi in tops] + [[i] for i in ALL])
    first, n = max(ranges_without(bad, c.M), key=lambda s: s[1])

    def both():
        out = [g.tobytes() for g in top_series(kept, tops, 20, "percentile", 0.99, False, n, first)]
        out += [g.tobytes() for g in top_series(kept, tops, 1024, "count", None, True, c.M, 0)]
        out += [g.tobytes() for g in movers_series(kept, pairs, 20, "ks", None, False, n, first)]
        ent = torch.full((5 * 20 * 32,), PATTERN, dtype=torch.uint8, device="cuda")
        cnt = torch.full((5,), -1, dtype=torch.int32, device="cuda")
        movers_series(kept, pairs, 20, "shift", None, True, n, first, out=(ent, cnt))
        torch.cuda.synchronize()
        return out + [ent.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()]

    with shape(kind):
        want = both()
        assert any(len(x) for x in want[:5])
        for windows_a_chunk in (1, 2):
            with select_bytes(windows_a_chunk * record + (windows_a_chunk - 1) * 8):
                assert both() == want, windows_a_chunk
                # the passes tool sums its times over the chunks
                a, b = C.c_float(-1.0), C.c_float(-1.0)
                hs = (C.c_void_p * K)(*[k_._h.value for k_ in kept])
                win = (C.c_uint32 * 10)(*[v for p in tops for v in p])
                assert N.lib().lh_tool_kept_top_series_passes_ms(C.addressof(hs), K, C.addressof(win), 5, 0, c.M, 0, 0.0, 20, 0, None,
                                                                 C.byref(a), C.byref(b)) == 0
                assert a.value > 0 and b.value > 0 and math.isfinite(a.value + b.value)
        assert both() == want


# ---- 6. forms, streams and lifetime -------------------------------------------------------------------------------------------------
def _device_pair(torch, nwin, k):
    return (torch.full((nwin * k * 32,), 0x77, dtype=torch.uint8, device="cuda"), torch.full((nwin,), -1, dtype=torch.int32, device="cuda"))


def _blocks(pair, dtype, nwin, k):
    ent, n = pair
    e, n = ent.cpu().numpy().view(dtype), n.cpu().numpy()
    return [e[w * k:w * k + int(n[w])].tobytes() for w in range(nwin)]


@pytest.mark.parametrize("kind", KINDS)
def test_device_form_equals_host_form_and_a_second_stream_right_behind(crafted, kind):
    c, torch = crafted, crafted.torch
    kept = kept_of(c, ALL)
    tops, pairs = WINDOWS["rolling"], DRIFT["overlapping"][1]
    bad = wrapped(c, [ALL[lo:hi] for lo, hi in tops] + [s for window in pairs for s in sides(ALL, window)])
    first, n = max(ranges_without(bad, c.M), key=lambda s: s[1])
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with shape(kind):
        for k in (7, 1024):
            host_t = [g.tobytes() for g in top_series(kept, tops, k, "sum", None, False, n, first)]
            host_m = [g.tobytes() for g in movers_series(kept, pairs, k, "w1", None, True, n, first)]
            pt, pm = _device_pair(torch, len(tops), k), _device_pair(torch, len(pairs), k)
            torch.cuda.synchronize()
            assert top_series(kept, tops, k, "sum", None, False, n, first, out=pt, stream=a) is pt
            movers_series(kept, pairs, k, "w1", None, True, n, first, out=pm, stream=b)   # the ONE records block: b waits for a's passes
            a.synchronize()
            b.synchronize()
            assert _blocks(pt, N.TOP_ENTRY, len(tops), k) == host_t and any(host_t), (kind, k)
            assert _blocks(pm, N.MOVER_ENTRY, len(pairs), k) == host_m and any(host_m), (kind, k)
            pinned = torch.zeros((len(tops) * k * 32,), dtype=torch.uint8, pin_memory=True).numpy().view(N.TOP_ENTRY)
            assert [g.tobytes() for g in top_series(kept, tops, k, "sum", None, False, n, first, out=pinned)] == host_t


@pytest.mark.parametrize("bits", (64, 32))
def test_handles_are_releasable_straight_after_a_device_form_call(native_lib, torch_cuda, bits):
    torch = torch_cuda
    M, n, k = 70, 50_000, 25
    rng = np.random.default_rng(29)
    sets = [(rng.integers(0, M, n).astype(np.uint32), rng.lognormal(2.0 + i, 1.5, n)) for i in range(4)]
    tops = [(0, 1), (1, 3), (0, 4), (3, 4)]
    pairs = [((0, 2), (2, 4)), ((3, 4), (0, 1)), ((0, 4), (1, 2))]

    def four(e):
        kept = []
        for ids, v in sets:
            e.submit_pairs(ids, v)
            with e.flip() as s:
                kept.append(s.keep(M))
        return kept

    with engine(M, cell_bits=bits) as e:
        ref = four(e)
        for kind in KINDS:
            with shape(kind):
                want_t = [g.tobytes() for g in top_series(ref, tops, k, "percentile", 0.99, False, M, 0)]
                want_m = [g.tobytes() for g in movers_series(ref, pairs, k, "ks", None, False, M - 3, 3)]
                fresh = four(e)
                a, b = torch.cuda.Stream(), torch.cuda.Stream()
                pt, pm = _device_pair(torch, len(tops), k), _device_pair(torch, len(pairs), k)
                torch.cuda.synchronize()
                top_series(fresh, tops, k, "percentile", 0.99, False, M, 0, out=pt, stream=a)
                movers_series(fresh, pairs, k, "ks", None, False, M - 3, 3, out=pm, stream=b)
                for k_ in fresh:
                    k_.close()                                                       # waits for the readers on both streams
                a.synchronize()
                b.synchronize()
                assert _blocks(pt, N.TOP_ENTRY, len(tops), k) == want_t and all(len(x) == k * 32 for x in want_t), kind
                assert _blocks(pm, N.MOVER_ENTRY, len(pairs), k) == want_m and all(len(x) == k * 32 for x in want_m), kind
        for k_ in ref:
            k_.close()


def test_rows_outside_a_handle_no_window_names_are_refused(tiled):
    """The rows must lie inside EVERY listed handle's block, whether or not a window names the handle; nothing is written."""
    import loghisto_amd
    t, torch = tiled, tiled.torch
    a, b = t.parts                                                                   # rows 50 .. 149 and 20 .. 219
    kept = [t.kept[0], a, b]
    out = np.zeros(2 * 4, dtype=N.TOP_ENTRY)
    out.view(np.uint8)[:] = PATTERN
    for first, n in ((49, 2), (149, 2), (20, 10), (0, 1)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            top_series(kept, [(0, 1), (2, 3)], 4, "count", None, False, n, first, out=out)   # handle 1 is in no window
        assert ei.value.code == N.ERANGE and np.all(out.view(np.uint8) == PATTERN), (first, n)
        with pytest.raises(loghisto_amd.LhError) as ei:
            movers_series(kept, [((0, 1), (2, 3))], 4, "ks", None, False, n, first)
        assert ei.value.code == N.ERANGE, (first, n)
    got = check_windows("top", kept, [(0, 1), (2, 3), (0, 3)], 4, "sum", None, False, 100, 50, "inside")
    assert all(50 <= int(i) < 150 for g in got for i in g["id"])
    # the device form's empty call zeroes nwin counts and writes no entry
    ent = torch.full((2 * 4 * 32,), PATTERN, dtype=torch.uint8, device="cuda")
    cnt = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    top_series(kept, [(0, 1), (2, 3)], 4, "count", None, False, 0, 60, out=(ent, cnt[:2]))
    torch.cuda.synchronize()
    assert list(cnt.cpu().numpy()) == [0, 0, -7] and bool((ent == PATTERN).all())
    assert [len(g) for g in top_series(kept, [(0, 1), (2, 3)], 4, "count", None, False, 0, 60)] == [0, 0]


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_windows_against_and_the_window_class(native_lib, torch_cuda):
    import loghisto_amd
    M, n = 12, 4000
    rng = np.random.default_rng(12)
    with engine(M, cell_bits=64, num_buffers=2) as e, loghisto_amd.KeptWindow(4) as win:
        kept = []
        for i in range(4):
            e.submit_pairs(rng.integers(0, M - 1, n).astype(np.uint32), rng.lognormal(2.0 + 0.3 * i, 1.0, n))   # the last name stays empty
            with e.flip() as s:
                kept.append(s.keep(M))
            win.push(kept[-1])
        last, earlier = kept[-1], kept[:-1]
        # windows=None: one window per handle, as Kept.series resolves it
        got = last.top_series(5, "percentile", 0.99, earlier=earlier)
        assert len(got) == 4 and all(g.dtype == N.TOP_ENTRY and len(g) == 5 for g in got)
        for i, g in enumerate(got):
            assert g.tobytes() == kept[i].top(5, "percentile", 0.99).tobytes()
        got = last.top_series(1024, "count", earlier=earlier, windows=[(0, 4), (1, 3)])
        assert [len(g) for g in got] == [M - 1, M - 1]
        assert got[1].tobytes() == kept[2].top(1024, "count", earlier=[kept[1]]).tobytes()
        # movers: with neither, each handle against the one before it; against= a fixed baseline, one window per handle
        got = last.movers_series(3, "shift", earlier=earlier)
        assert len(got) == 3 and all(g.dtype == N.MOVER_ENTRY and len(g) == 3 for g in got)
        for i, g in enumerate(got):
            assert g.tobytes() == kept[i + 1].movers(kept[i], 3, "shift").tobytes()
        got = last.movers_series(3, "ks", earlier=earlier, against=(0, 2))
        assert len(got) == 4
        for i, g in enumerate(got):
            assert g.tobytes() == kept[i].movers(kept[:2], 3, "ks").tobytes()
        got = last.movers_series(3, "percentile", 0.5, True, earlier, [(1, 4)], (0, 1))
        assert len(got) == 1 and got[0].tobytes() == kept[3].movers(kept[0], 3, "percentile", 0.5, True, kept[1:3]).tobytes()
        # by / arg go through the one set of checks
        for bad in (lambda: last.top_series(3, "median"), lambda: last.top_series(3, "percentile"), lambda: last.movers_series(3, "percentile")):
            with pytest.raises(ValueError):
                bad()
        # the window class: the same calls over its intervals, the oldest first
        assert list(win.handles) == kept
        for windows in (None, [(0, 4), (2, 3)]):
            a, b = win.top_series(4, "sum", windows=windows), last.top_series(4, "sum", earlier=earlier, windows=windows)
            assert len(a) == len(b) and [x.tobytes() for x in a] == [x.tobytes() for x in b] and all(len(x) == 4 for x in a)
        a, b = win.movers_series(4, "w1", against=(0, 1)), last.movers_series(4, "w1", earlier=earlier, against=(0, 1))
        assert len(a) == 4 and [x.tobytes() for x in a] == [x.tobytes() for x in b]
        a, b = win.movers_series(4), last.movers_series(4, earlier=earlier)
        assert len(a) == 3 and [x.tobytes() for x in a] == [x.tobytes() for x in b]
        for k_ in kept:
            k_.close()
