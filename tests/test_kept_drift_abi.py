"""CPU tests of lh_kept_spread_series* and lh_kept_drift* (lh_kept_spread's and lh_kept_compare's outputs per WINDOW of a list of
kept intervals, in one call): declared, exported, bound with the header's prototypes, and every LH_EINVAL -- the windows' rules,
the list's, each family's own --, the early LH_ERANGE and the empty call decided on the host before any handle is looked at -- the
handle pointers below are fakes that are never dereferenced -- with no output written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_kept_readers_abi import BIG, CTYPES, VP, _header, _lists
from tests.test_kept_series_abi import LIST, ROWS, _forms, _id_errors, _window_and_list_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD = ("const double *p, size_t np, uint32_t flags, void *stream, uint64_t *{0}count, double *{0}sum, double *{0}m2, "
          "int16_t *{0}pkeys, uint8_t *{0}pvalid, uint64_t *{0}count_le, double *{0}sum_le")
DRIFT = ("uint32_t flags, void *stream, uint64_t *{0}count_a, uint64_t *{0}count_b, double *{0}ks, int16_t *{0}ks_key, "
         "uint64_t *{0}ks_below_a, uint64_t *{0}ks_below_b, double *{0}w1, double *{0}shift")
PROTOS = {}
for _family, _tail in (("lh_kept_spread_series", SPREAD), ("lh_kept_drift", DRIFT)):
    for _rows, _text in ROWS.items():
        for _dev, _d in (("", ""), ("_device", "d_")):
            PROTOS[_family + _rows + _dev] = LIST + _text.format(_d) + _tail.format(_d)
CONTRACT = (
    "This lifts spread / compare per window from the out-of-scope list of the block above; top per window stays out",
    "Window w's block of every output of lh_kept_spread_series* is byte for byte what lh_kept_spread* (the same form, the same "
    "rows or ids, p, np) writes for the list (kept + lo_w, hi_w - lo_w).",
    "This includes sum, m2 and sum_le: they are taken in the same fixed order, the same in both kernel shapes.",
    "Wrapped totals behave as lh_kept_spread*'s do; np == 0 is allowed; a handle listed twice counts twice.",
    "Window w's block of every output of lh_kept_drift* is byte for byte what lh_kept_compare* (the same form, the same rows or "
    "ids) writes for the lists (kept + base_lo, base_hi - base_lo) and (kept + cur_lo, cur_hi - cur_lo).",
    "This covers all eight outputs, w1 and shift among them, in both kernel shapes.",
    "A name with no samples on one side of a window has NaN distances with key and prefixes 0 in that window, and only there.",
    "Identical slices give exact zeros for non-empty names.",
    "The two slices may overlap, coincide and stand in either order in the list.",
    "A fixed baseline is the same base slice in every window.",
    "(base_hi - base_lo) + (cur_hi - cur_lo) <= LH_MAX_KEPT",
)


def test_the_eight_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    assert len(PROTOS) == 8
    src = _header()
    raw = C.CDLL(_native.LIB_PATH)
    for name, proto in PROTOS.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert decl, f"{name} is not declared"
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == proto, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        restype, argtypes = _native.SIGNATURES[name]
        want = [C.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in proto.split(", ")]
        assert restype is C.c_int and argtypes == want, name
    # adding functions is backward compatible: no new limit, version or error code
    assert re.search(r"#define\s+LH_MAX_WINDOWS\s+128\b", src) and _native.MAX_WINDOWS == 128
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    # the contract stands in the header in its own words; the series block keeps its list
    flat = lambda s: re.sub(r"\s+\*?\s*(- )?", " ", s)                       # noqa: E731  (comment stars, bullets, line breaks)
    text = flat(open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    for sentence in CONTRACT:
        assert flat(sentence) in text, sentence
    assert "spread / compare / top per window; more than LH_MAX_KEPT handles per call." in text
    assert "OUT OF SCOPE: top and movers per window" in text


def test_spread_series_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    p = np.array([0.5, 0.99, 1.5, np.nan])
    pp = p.ctypes.data
    p33 = np.zeros(33)
    fields = dict(count=np.uint64, sum=np.float64, m2=np.float64, pkeys=np.int16, pvalid=np.uint8, count_le=np.uint64,
                  sum_le=np.float64)
    arrays = {k: np.full(32, 7, dtype=t) for k, t in fields.items()}
    outs = [a.ctypes.data for a in arrays.values()]
    widths = [a.itemsize for a in arrays.values()]
    for fn in _forms(L, "lh_kept_spread_series", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _window_and_list_errors(fn, n, (pp, 4, 0, None, *outs), EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                assert fn(k, nk, wp, nw, n, p33.ctypes.data, 33, 0, None, *outs) == EINVAL   # np <= LH_MAX_PERCENTILES
                assert fn(k, nk, wp, nw, n, None, 4, 0, None, *outs) == EINVAL    # np > 0 with NULL p
                assert fn(k, nk, wp, nw, n, pp, 4, 0, None, *[None] * 7) == EINVAL   # all outputs NULL
                assert fn(k, nk, wp, nw, n, None, 0, 0, None, None, None, None, *outs[3:]) == EINVAL   # np == 0: the last four count for nothing
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(k, nk, wp, nw, n, pp, 4, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):
                    assert fn(k, nk, wp, nw, n, pp + off, 1, 0, None, *outs) == EINVAL, off
                for j, width in enumerate(widths):                            # an output off its element's alignment
                    for off in range(1, width):
                        bad = list(outs)
                        bad[j] += off
                        assert fn(k, nk, wp, nw, n, pp, 4, 0, None, *bad) == EINVAL, (j, off)
                        only = [None] * 7
                        only[j] = bad[j]
                        assert fn(k, nk, wp, nw, n, pp, 4, 0, None, *only) == EINVAL, (j, off)
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(k, nk, wp, nw, BIG, pp, 4, 0, None, *outs) == ERANGE
            assert fn(k, nk, wp, nw, (1 << 64) - 1, None, 0, 0, None, None, outs[1], *[None] * 5) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes); np == 0 is allowed
            assert fn(k, nk, wp, nw, 0, pp, 4, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, None, 0, 0, 0x10, outs[0], None, None, 1, 1, 1, 1) == 0
            assert fn(k, nk, wp, nw, 0, p33.ctypes.data, 32, 0, None, *[None] * 4, outs[4], None, None) == 0
    _id_errors(L, "lh_kept_spread_series", good, (pp, 4, 0, None, *outs), ids, EINVAL)
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written


def _quads(*quads):
    return np.array([v for q in quads for v in q], dtype=np.uint32)


def _drift_window_and_list_errors(fn, n, tail, EINVAL):
    """every window rule and every list rule -> LH_EINVAL; returns good (list, nkept, windows, nwin) sets"""
    good, h65, holes = _lists()
    one = _quads((0, 1, 0, 1))
    w1 = one.ctypes.data
    odd = (C.c_char * 64)()
    # ---- the list rules, with a window that fits any list
    assert fn(None, 1, w1, 1, n, *tail) == EINVAL and fn(None, 0, w1, 1, n, *tail) == EINVAL
    for off in range(1, C.sizeof(VP)):
        assert fn(C.addressof(odd) + off, 1, w1, 1, n, *tail) == EINVAL, off
    for h in holes:                                                           # a NULL entry, wherever
        assert fn(h, len(h), w1, 1, n, *tail) == EINVAL
    assert fn(good[0][0], 0, w1, 1, n, *tail) == EINVAL                       # an empty list
    assert fn(h65, 65, w1, 1, n, *tail) == EINVAL and fn(h65, (1 << 64) - 1, w1, 1, n, *tail) == EINVAL
    # ---- the window rules, for lists of 1, 2 and 64 handles: every bad slice on either side of a window
    w129 = _quads(*[(0, 1, 0, 1)] * 129)
    for k, nk in good:
        for bad in ((0, 0), (nk, nk), (1, 1),                                 # lo == hi
                    (1, 0), (nk, 0), (0xffffffff, 1),                         # lo > hi
                    (0, nk + 1), (nk, nk + 1), (0, 0xffffffff)):              # hi == nkept + 1, and far beyond
            for quad in ((*bad, 0, 1), (0, 1, *bad), (*bad, *bad)):
                w = _quads(quad)
                assert fn(k, nk, w.ctypes.data, 1, n, *tail) == EINVAL, (nk, quad)
                w = _quads((0, 1, 0, 1), (0, min(nk, 63), 0, 1), quad)                 # ... behind good ones
                assert fn(k, nk, w.ctypes.data, 3, n, *tail) == EINVAL, (nk, quad)
        assert fn(k, nk, w1, 0, n, *tail) == EINVAL                           # nwin == 0
        assert fn(k, nk, w129.ctypes.data, 129, n, *tail) == EINVAL           # nwin == LH_MAX_WINDOWS + 1
        assert fn(k, nk, w129.ctypes.data, (1 << 64) - 1, n, *tail) == EINVAL
        assert fn(k, nk, None, 1, n, *tail) == EINVAL                         # NULL win
        assert fn(k, nk, None, 0, n, *tail) == EINVAL
        for off in (1, 2, 3):                                                 # misaligned win
            assert fn(k, nk, w129.ctypes.data + off, 1, n, *tail) == EINVAL, off
    # ---- the two slices of a window hold LH_MAX_KEPT handles at most: a sum of 65, in a list of 64
    k, nk = good[2]
    for quad in ((0, 33, 32, 64), (0, 32, 31, 64), (0, 64, 0, 1), (63, 64, 0, 64), (0, 64, 0, 64), (1, 34, 0, 32)):
        assert sum(quad[1::2]) - sum(quad[0::2]) > 64
        assert fn(k, nk, _quads(quad).ctypes.data, 1, n, *tail) == EINVAL, quad
        assert fn(k, nk, _quads((0, 32, 32, 64), quad).ctypes.data, 2, n, *tail) == EINVAL, quad
    w128 = _quads(*[(0, 1, 0, 1)] * 128)
    full = [(k, nk, _quads((0, min(nk, 63), nk - 1, nk), (nk - 1, nk, 0, 1), (0, 1, 0, 1), (nk - 1, nk, 0, nk - 1 or 1)), 4)
            for k, nk in good]
    sums64 = _quads((0, 32, 32, 64), (0, 63, 63, 64), (0, 1, 1, 64), (16, 48, 0, 32), (0, 32, 0, 32))   # exactly LH_MAX_KEPT
    return full + [(good[0][0], 1, w128, 128), (good[2][0], 64, sums64, 5),
                   (good[2][0], 64, _quads(*([(i, 64, 0, i) for i in range(1, 64)] + [(0, 32, 32, 64)]) * 2), 128)]


def test_drift_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    fields = dict(count_a=np.uint64, count_b=np.uint64, ks=np.float64, ks_key=np.int16, ks_below_a=np.uint64, ks_below_b=np.uint64,
                  w1=np.float64, shift=np.float64)
    arrays = {k: np.full(32, 7, dtype=t) for k, t in fields.items()}
    outs = [a.ctypes.data for a in arrays.values()]
    widths = [a.itemsize for a in arrays.values()]
    for fn in _forms(L, "lh_kept_drift", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _drift_window_and_list_errors(fn, n, (0, None, *outs), EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(k, nk, wp, nw, n, flags, None, *outs) == EINVAL, flags
                assert fn(k, nk, wp, nw, n, 0, None, *[None] * 8) == EINVAL   # all outputs NULL
                for j, width in enumerate(widths):                            # an output off its element's alignment
                    for off in range(1, width):
                        bad = list(outs)
                        bad[j] += off
                        assert fn(k, nk, wp, nw, n, 0, None, *bad) == EINVAL, (j, off)
                        only = [None] * 8
                        only[j] = bad[j]
                        assert fn(k, nk, wp, nw, n, 0, None, *only) == EINVAL, (j, off)
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(k, nk, wp, nw, BIG, 0, None, *outs) == ERANGE
            assert fn(k, nk, wp, nw, (1 << 64) - 1, 0, None, None, None, outs[2], *[None] * 5) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes)
            assert fn(k, nk, wp, nw, 0, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, 0, 0x10, *[None] * 7, outs[7]) == 0
    _id_errors(L, "lh_kept_drift", good, (0, None, *outs), ids, EINVAL)
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written


def test_python_wrapper_has_the_two_readers():
    import loghisto_amd
    rest = ["nmetrics", "first", "ids", "out", "stream"]
    K, W = loghisto_amd.Kept, loghisto_amd.KeptWindow
    assert list(inspect.signature(K.spread_series).parameters) == ["self", "percentiles", "earlier", "windows", *rest]
    assert list(inspect.signature(W.spread_series).parameters) == ["self", "percentiles", "windows", *rest]
    assert list(inspect.signature(K.drift).parameters) == ["self", "windows", "earlier", "against", *rest]
    assert list(inspect.signature(W.drift).parameters) == ["self", "windows", "against", *rest]
    for fn in (K.spread_series, W.spread_series, K.drift, W.drift):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items()}
        assert d["windows"] is None and d["nmetrics"] is None and d["first"] == 0, fn
        assert d["ids"] is None and d["out"] is None and d["stream"] is None, fn
        assert d.get("earlier", ()) == () and d.get("against") is None, fn
    # a window of more intervals than a call reads is refused before any call
    w = W(100)
    w.handles.extend([None] * 65)
    for read in (lambda: w.spread_series([0.5]), lambda: w.drift(), lambda: w.drift(against=(0, 1))):
        with pytest.raises(ValueError):
            read()
    # the windows Kept.drift builds: explicit pairs, a fixed baseline, each handle against the one before it
    make = K._drift_windows
    assert list(make(None)([((0, 2), (2, 3)), ((4, 5), (0, 1))], 6)[0]) == [0, 2, 2, 3, 4, 5, 0, 1]
    assert list(make((1, 3))(None, 3)[0]) == [1, 3, 0, 1, 1, 3, 1, 2, 1, 3, 2, 3] and make((1, 3))(None, 3)[1] == 3
    assert list(make((1, 3))([(0, 2)], 3)[0]) == [1, 3, 0, 2]
    assert list(make(None)(None, 4)[0]) == [0, 1, 1, 2, 1, 2, 2, 3, 2, 3, 3, 4] and make(None)(None, 4)[1] == 3
    for bad in (lambda: make(None)(None, 1), lambda: make(None)([((0, 1), (0, -1))], 3), lambda: make(None)([((0, 1), (0, 1 << 32))], 3)):
        with pytest.raises(ValueError):
            bad()
    # the earlier per-window readers keep their signatures
    assert list(inspect.signature(K.series).parameters) == ["self", "percentiles", "earlier", "windows", *rest]
