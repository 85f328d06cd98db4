"""CPU tests of lh_kept_series* and lh_kept_heat* (lh_kept_across' and lh_kept_count_le's outputs per WINDOW of a list of kept
intervals, in one call): declared, exported, bound with the header's prototypes, and every LH_EINVAL -- the windows' rules, the
list's, each family's own --, the early LH_ERANGE and the empty call decided on the host before any handle is looked at -- the
handle pointers below are fakes that are never dereferenced -- with no output written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_kept_readers_abi import BIG, CTYPES, VP, _header, _lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = "lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, "
ROWS = {"": "uint32_t first, size_t nmetrics, ", "_ids": "const uint32_t *{}ids, size_t n, "}
SERIES = ("const double *p, size_t np, uint32_t flags, void *stream, uint64_t *{0}count, double *{0}sum, uint32_t *{0}nbuckets, "
          "uint64_t *{0}present_bits, int16_t *{0}pkeys, uint8_t *{0}pvalid")
HEAT = "const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *{0}cum, uint64_t *{0}total"
PROTOS = {}
for _family, _tail in (("lh_kept_series", SERIES), ("lh_kept_heat", HEAT)):
    for _rows, _text in ROWS.items():
        for _dev, _d in (("", ""), ("_device", "d_")):
            PROTOS[_family + _rows + _dev] = LIST + _text.format(_d) + _tail.format(_d)
CONTRACT = (
    "Window w's block of every output of lh_kept_series* is byte for byte what lh_kept_across* (the same form, the same rows or "
    "ids, p, np) writes for the list (kept + lo_w, hi_w - lo_w).",
    "The one exception is present_bits: bit i means kept[i] of the WHOLE list, which is the slice call's value shifted left by lo_w.",
    "Window w's block of lh_kept_heat* is byte for byte lh_kept_count_le*'s cum / total for that slice.",
    "This includes sum: it is taken in the same fixed order, the same in both kernel shapes and independent of timing.",
    "A handle listed twice counts twice.",
    "A name with no sample in a window has the empty entry there.",
    "A DEVICE id outside the block of some handle of window w yields the empty entry in that window, and nothing is read for it.",
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
    # adding functions is backward compatible: one new limit, no new version or error code
    assert re.search(r"#define\s+LH_MAX_WINDOWS\s+128\b", src) and _native.MAX_WINDOWS == 128
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    # the contract stands in the header in its own words
    flat = lambda s: re.sub(r"\s+\*?\s*(- )?", " ", s)                       # noqa: E731  (comment stars, bullets, line breaks)
    text = flat(open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    for sentence in CONTRACT:
        assert flat(sentence) in text, sentence
    assert "OUT OF SCOPE: sharing cell reads between overlapping windows" in text


def _win(*pairs):
    return np.array([v for p in pairs for v in p], dtype=np.uint32)


def _forms(L, family, ids):
    """call(kept, nkept, win, nwin, n, *tail) for the family's four entry points (tail: everything behind the rows)"""
    for dev in ("", "_device"):
        yield lambda k, nk, w, nw, n, *t, fn=getattr(L, family + dev): fn(k, nk, w, nw, 0, n, *t)
        yield lambda k, nk, w, nw, n, *t, fn=getattr(L, family + "_ids" + dev): fn(k, nk, w, nw, ids.ctypes.data, n, *t)


def _window_and_list_errors(fn, n, tail, EINVAL):
    """every window rule and every list rule -> LH_EINVAL; returns good (list, nkept, windows, nwin) sets"""
    good, h65, holes = _lists()
    one = _win((0, 1))
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
    # ---- the window rules, for lists of 1, 2 and 64 handles
    w129 = _win(*[(0, 1)] * 129)
    for k, nk in good:
        for bad in ((0, 0), (nk, nk), (1, 1),                                 # lo == hi
                    (1, 0), (nk, 0), (0xffffffff, 1),                         # lo > hi
                    (0, nk + 1), (nk, nk + 1), (0, 0xffffffff)):              # hi == nkept + 1, and far beyond
            w = _win(bad)
            assert fn(k, nk, w.ctypes.data, 1, n, *tail) == EINVAL, (nk, bad)
            w = _win((0, 1), (0, nk), bad)                                    # ... behind good ones
            assert fn(k, nk, w.ctypes.data, 3, n, *tail) == EINVAL, (nk, bad)
        assert fn(k, nk, w1, 0, n, *tail) == EINVAL                           # nwin == 0
        assert fn(k, nk, w129.ctypes.data, 129, n, *tail) == EINVAL           # nwin == LH_MAX_WINDOWS + 1
        assert fn(k, nk, w129.ctypes.data, (1 << 64) - 1, n, *tail) == EINVAL
        assert fn(k, nk, None, 1, n, *tail) == EINVAL                         # NULL win
        assert fn(k, nk, None, 0, n, *tail) == EINVAL
        for off in (1, 2, 3):                                                 # misaligned win
            assert fn(k, nk, w129.ctypes.data + off, 1, n, *tail) == EINVAL, off
    w128 = _win(*[(0, 1)] * 128)
    full = [(k, nk, _win((0, nk), (nk - 1, nk), (0, 1), (0, nk)), 4) for k, nk in good]
    return full + [(good[0][0], 1, w128, 128), (good[2][0], 64, _win(*[(i, 64) for i in range(64)] * 2), 128)]


def _id_errors(L, family, good, tail, ids, EINVAL):
    for fn in (getattr(L, family + "_ids"), getattr(L, family + "_ids_device")):
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            assert fn(k, nk, wp, nw, None, 1, *tail) == EINVAL                # ids NULL with n > 0
            assert fn(k, nk, wp, nw, None, BIG, *tail) == EINVAL              # ... wins over the early LH_ERANGE
            assert fn(k, nk, wp, nw, None, 0, *tail) == 0                     # n == 0: no list is needed
            for off in (1, 2, 3):                                             # ids misaligned
                for n in (0, 1, BIG):
                    assert fn(k, nk, wp, nw, ids.ctypes.data + off, n, *tail) == EINVAL, (off, n)


def test_series_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    p = np.array([0.5, 0.99, 1.5, np.nan])
    pp = p.ctypes.data
    p33 = np.zeros(33)
    fields = dict(count=np.uint64, sum=np.float64, nbuckets=np.uint32, present_bits=np.uint64, pkeys=np.int16, pvalid=np.uint8)
    arrays = {k: np.full(32, 7, dtype=t) for k, t in fields.items()}
    outs = [a.ctypes.data for a in arrays.values()]
    widths = [a.itemsize for a in arrays.values()]
    for fn in _forms(L, "lh_kept_series", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _window_and_list_errors(fn, n, (pp, 4, 0, None, *outs), EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                assert fn(k, nk, wp, nw, n, p33.ctypes.data, 33, 0, None, *outs) == EINVAL   # np <= LH_MAX_PERCENTILES
                assert fn(k, nk, wp, nw, n, None, 4, 0, None, *outs) == EINVAL    # np > 0 with NULL p
                assert fn(k, nk, wp, nw, n, pp, 4, 0, None, *[None] * 6) == EINVAL   # all outputs NULL
                assert fn(k, nk, wp, nw, n, None, 0, 0, None, None, None, None, None, *outs[4:]) == EINVAL   # np == 0: the last two count for nothing
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(k, nk, wp, nw, n, pp, 4, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):
                    assert fn(k, nk, wp, nw, n, pp + off, 1, 0, None, *outs) == EINVAL, off
                for j, width in enumerate(widths):                            # an output off its element's alignment
                    for off in range(1, width):
                        bad = list(outs)
                        bad[j] += off
                        assert fn(k, nk, wp, nw, n, pp, 4, 0, None, *bad) == EINVAL, (j, off)
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(k, nk, wp, nw, BIG, pp, 4, 0, None, *outs) == ERANGE
            assert fn(k, nk, wp, nw, (1 << 64) - 1, None, 0, 0, None, None, outs[1], *[None] * 4) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes); np == 0 is allowed
            assert fn(k, nk, wp, nw, 0, pp, 4, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, None, 0, 0, 0x10, outs[0], None, None, None, 1, 1) == 0
            assert fn(k, nk, wp, nw, 0, p33.ctypes.data, 32, 0, None, *[None] * 4, outs[4], None) == 0
    _id_errors(L, "lh_kept_series", good, (pp, 4, 0, None, *outs), ids, EINVAL)
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written


def test_heat_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    bounds = np.array([-np.inf, -1.0, -0.0, 0.0, 0.25, 0.25, 1e200, np.inf])
    b = bounds.ctypes.data
    b65 = np.arange(65, dtype=np.float64)
    cum, total = np.full(8 * 64, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64)
    outs = (cum.ctypes.data, total.ctypes.data)
    nan, down, neg0 = np.array([0.0, np.nan, 1.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, -0.0, 0.0])
    for fn in _forms(L, "lh_kept_heat", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _window_and_list_errors(fn, n, (b, 8, 0, None, *outs), EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                assert fn(k, nk, wp, nw, n, b, 0, 0, None, *outs) == EINVAL   # nb in 1 .. LH_MAX_BOUNDS
                assert fn(k, nk, wp, nw, n, b65.ctypes.data, 65, 0, None, *outs) == EINVAL
                assert fn(k, nk, wp, nw, n, None, 8, 0, None, *outs) == EINVAL   # NULL bounds
                assert fn(k, nk, wp, nw, n, nan.ctypes.data, 3, 0, None, *outs) == EINVAL   # a NaN bound
                assert fn(k, nk, wp, nw, n, nan.ctypes.data + 8, 1, 0, None, *outs) == EINVAL
                assert fn(k, nk, wp, nw, n, down.ctypes.data, 3, 0, None, *outs) == EINVAL   # a decreasing row
                assert fn(k, nk, wp, nw, n, b, 8, 0, None, None, None) == EINVAL   # both outputs NULL
                for flags in (_native.LE_PER_METRIC, 2, 0x80000000, 3):       # flags must be 0
                    assert fn(k, nk, wp, nw, n, b, 8, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):                                       # arrays off their alignment
                    assert fn(k, nk, wp, nw, n, b + off, 2, 0, None, *outs) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, outs[0] + off, outs[1]) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, outs[0], outs[1] + off) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, None, outs[1] + off) == EINVAL, off
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            assert fn(k, nk, wp, nw, BIG, b, 8, 0, None, *outs) == ERANGE
            assert fn(k, nk, wp, nw, (1 << 64) - 1, b, 8, 0, None, None, outs[1]) == ERANGE
            # an empty call: LH_OK before any handle is looked at; equal neighbours, both zeros, one bound
            assert fn(k, nk, wp, nw, 0, b, 8, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, b, 8, 0, 0x10, outs[0], None) == 0
            assert fn(k, nk, wp, nw, 0, neg0.ctypes.data, 3, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, b65.ctypes.data, 64, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, b, 1, 0, None, *outs) == 0
    _id_errors(L, "lh_kept_heat", good, (b, 8, 0, None, *outs), ids, EINVAL)
    assert np.all(cum == 7) and np.all(total == 7)                            # nothing was written


def test_python_wrapper_has_the_two_readers():
    import loghisto_amd
    for cls, skip in ((loghisto_amd.Kept, ["earlier"]), (loghisto_amd.KeptWindow, [])):
        for name, lead in (("series", "percentiles"), ("heat", "bounds")):
            sig = inspect.signature(getattr(cls, name))
            assert list(sig.parameters) == ["self", lead, *skip, "windows", "nmetrics", "first", "ids", "out", "stream"], (cls, name)
            d = {k: v.default for k, v in sig.parameters.items()}
            assert d["windows"] is None and d["nmetrics"] is None and d["first"] == 0, name
            assert d["ids"] is None and d["out"] is None and d["stream"] is None, name
    assert inspect.signature(loghisto_amd.Kept.series).parameters["earlier"].default == ()
    # a window of more intervals than a call reads is refused before any call
    w = loghisto_amd.KeptWindow(100)
    w.handles.extend([None] * 65)
    for read in (lambda: w.series([0.5]), lambda: w.heat([1.0])):
        with pytest.raises(ValueError):
            read()
    # the earlier kept readers keep their signatures
    assert list(inspect.signature(loghisto_amd.Kept.count_le).parameters) == ["self", "bounds", "earlier", "nmetrics", "first", "ids",
                                                                               "out", "stream"]
