"""CPU tests of lh_kept_top_series* and lh_kept_movers_series* (lh_kept_top's and lh_kept_movers' selections per WINDOW of a list of
kept intervals, in one call): declared, exported, bound with the header's prototypes, and every LH_EINVAL -- the list's rules, the
windows' of either kind, then `by`, flags, arg, k, out, n_out --, the early LH_ERANGE and the host forms' empty call decided on the
host, in the documented order, before any handle is looked at -- the handle pointers below are fakes that are never dereferenced --
with no output written."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_kept_drift_abi import _drift_window_and_list_errors
from tests.test_kept_select_abi import BIG, CTYPES, PATTERN, Out, _common_errors, _handles, _header
from tests.test_kept_series_abi import _window_and_list_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD = ("lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics, uint32_t by, "
        "double arg, size_t k, uint32_t flags, void *stream, ")
PROTOS = {
    "lh_kept_top_series": LEAD + "lh_top_entry *out, size_t *n_out",
    "lh_kept_top_series_device": LEAD + "lh_top_entry *d_out, uint32_t *d_n_out",
    "lh_kept_movers_series": LEAD + "lh_mover_entry *out, size_t *n_out",
    "lh_kept_movers_series_device": LEAD + "lh_mover_entry *d_out, uint32_t *d_n_out",
}
TOOLS = {
    "lh_tool_kept_top_series_passes_ms": LEAD + "float *score_ms, float *select_ms",
    "lh_tool_kept_movers_series_passes_ms": LEAD + "float *score_ms, float *select_ms",
    "lh_tool_kept_select_bytes": "uint64_t bytes, uint64_t *previous",
}
TYPES = dict(CTYPES, uint64_t=C.c_uint64)
CONTRACT = (
    "This lifts top and movers per window from the out-of-scope lists of the two blocks above",
    "n_out is an array of nwin counts: size_t in the host forms, uint32_t in the device forms.",
    "Window w's entries lie at out[w * k .. w * k + n_out[w]).",
    "Entries of a window's block at and beyond n_out[w] are never written.",
    "Window w's block of out and n_out[w] are byte for byte what lh_kept_top* (the same form, the same first, nmetrics, by, arg, k, "
    "flags) writes for the list (kept + lo_w, hi_w - lo_w).",
    "For lh_kept_movers_series* they are what lh_kept_movers* writes for base = (kept + base_lo, base_hi - base_lo) and "
    "cur = (kept + cur_lo, cur_hi - cur_lo).",
    "This holds for sum and score, in both kernel shapes.",
    "A window with no candidate has n_out[w] = 0, and nothing of its block is written.",
    "A handle listed twice counts twice.",
    "Wrapped totals behave as the parents' do.",
    "Nothing is summed across names and no new statistic is defined.",
    "OUT OF SCOPE: sharing cell reads between overlapping windows; a select that spreads ONE window over several workgroups; _ids "
    "forms; more than LH_MAX_KEPT handles a call.",
)
PINNED = (
    "top per window stays out",
    "OUT OF SCOPE: top and movers per window",
    "spread / compare / top per window; more than LH_MAX_KEPT handles per call.",
)


def test_the_four_symbols_and_the_three_tools_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    raw = C.CDLL(_native.LIB_PATH)
    for protos, header, table in ((PROTOS, "loghisto_gpu.h", _native.SIGNATURES), (TOOLS, "loghisto_gpu_tuning.h", _native.TUNING_SIGNATURES)):
        src = _header(header)
        for name, proto in protos.items():
            decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
            assert decl, f"{name} is not declared"
            assert re.sub(r"\s+", " ", decl.group(1)).strip() == proto, name
            assert hasattr(raw, name), f"{name} is not exported"
            assert name in table and getattr(native_lib, name).restype is C.c_int, name
            restype, argtypes = table[name]
            want = [(C.POINTER(C.c_float) if a.startswith("float") else C.POINTER(C.c_uint64) if a.startswith("uint64_t *") else C.c_void_p)
                    if "*" in a else TYPES[a.split()[0]] for a in proto.split(", ")]
            assert restype is C.c_int and argtypes == want, name
    # adding functions is backward compatible: no new version, limit, entry type or error code
    src = _header()
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_WINDOWS\s+128\b", src) and _native.MAX_WINDOWS == 128
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert re.search(r"#define\s+LH_MAX_TOP\s+1024\b", src) and _native.MAX_TOP == 1024
    assert len(re.findall(r"typedef\s+struct\s+lh_top_entry\b", src)) == 1 and len(re.findall(r"typedef\s+struct\s+lh_mover_entry\b", src)) == 1
    assert not re.search(r"\blh_kept_(top|movers)_series_ids", src)               # no _ids forms
    # the contract stands in the header in its own words; the two older blocks keep their sentences
    flat = lambda s: re.sub(r"\s+\*?\s*(- )?", " ", s)                           # noqa: E731  (comment stars, bullets, line breaks)
    text = flat(open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    for sentence in CONTRACT + PINNED:
        assert flat(sentence) in text, sentence


def _forms(L, family):
    """(call(kept, nkept, win, nwin, nmetrics, by, arg, k, flags, stream, out, n_out), alignment of n_out, host form?)"""
    for name, align in ((family, C.sizeof(C.c_size_t)), (family + "_device", 4)):
        yield (lambda k, nk, w, nw, n, *t, fn=getattr(L, name): fn(k, nk, w, nw, 0, n, *t)), align, name == family


NAN, INF = float("nan"), float("inf")


def _early_errors(L, family, window_errors, by_last, needs_arg, ascending, range_cases):
    from loghisto_amd import _native
    EINVAL, ERANGE = _native.EINVAL, _native.ERANGE
    o = Out()
    for fn, align, host in _forms(L, family):
        for n in (1, BIG):                                                        # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = window_errors(fn, n, (0, 0.0, 3, 0, None, o.e, o.pn), EINVAL)  # the list's rules, then the windows'
            for k, nk, w, nw in good:
                _common_errors(lambda n_, by, arg, kk, flags, out, n_out: fn(k, nk, w.ctypes.data, nw, n_, by, arg, kk, flags, None, out, n_out),
                               align, n, o, EINVAL, by_last, needs_arg, ascending)
        for k, nk, w, nw in good:
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            for by, arg in range_cases:
                assert fn(k, nk, w.ctypes.data, nw, BIG, by, arg, 1024, ascending, None, o.e, o.pn) == ERANGE, (by, arg)
            assert fn(k, nk, w.ctypes.data, nw, (1 << 64) - 1, 0, 0.0, 1, 0, None, o.e, o.pn) == ERANGE
        assert o.untouched()
    # the host form's empty call: nwin zeros to n_out and nothing else, before any handle is looked at (the handles are fakes)
    width = C.sizeof(C.c_size_t)
    for k, nk, w, nw in good:
        entries = np.full(64, PATTERN, dtype=np.uint8)
        counts = np.full((nw + 2) * width, 0xff, dtype=np.uint8)
        assert getattr(L, family)(k, nk, w.ctypes.data, nw, 0, 0, 0, 0.0, 20, 0, None, entries.ctypes.data, counts.ctypes.data) == 0
        assert np.all(counts[:nw * width] == 0) and np.all(counts[nw * width:] == 0xff) and np.all(entries == PATTERN), nw
        assert getattr(L, family)(k, nk, w.ctypes.data, nw, 12345, 0, by_last, 0.5, 1024, ascending, 0x10, entries.ctypes.data,
                                  counts.ctypes.data) == 0


def test_top_series_early_errors_are_decided_on_the_host_in_the_documented_order(native_lib):
    from loghisto_amd import _native
    _early_errors(native_lib, "lh_kept_top_series", _window_and_list_errors, _native.TOP_BY_COUNT_ABOVE,
                  ((_native.TOP_BY_PERCENTILE, (NAN, -0.25, 1.0000001, INF, -INF)), (_native.TOP_BY_COUNT_ABOVE, (NAN,))),
                  _native.TOP_ASCENDING, ((0, NAN), (1, NAN), (2, 0.0), (2, 1.0), (3, INF), (3, -INF), (3, 1e200)))


def test_movers_series_early_errors_are_decided_on_the_host_in_the_documented_order(native_lib):
    from loghisto_amd import _native
    _early_errors(native_lib, "lh_kept_movers_series", _drift_window_and_list_errors, _native.MOVERS_BY_PERCENTILE,
                  ((_native.MOVERS_BY_PERCENTILE, (NAN, -0.25, 1.0000001, INF, -INF)),), _native.MOVERS_ASCENDING,
                  ((0, NAN), (1, NAN), (2, INF), (3, 0.0), (3, 1.0)))


def test_a_window_of_the_other_kind_is_refused(native_lib):
    """lh_kept_top_series* reads pairs, lh_kept_movers_series* quads: the same words mean different windows"""
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    o = Out()
    h2 = _handles(0x1000, 0x2000)
    quad = np.array([0, 1, 1, 1], dtype=np.uint32)                                # a fine pair (0, 1); as a quad, cur is empty
    assert L.lh_kept_movers_series(h2, 2, quad.ctypes.data, 1, 0, BIG, 0, 0.0, 3, 0, None, o.e, o.pn) == EINVAL
    assert L.lh_kept_top_series(h2, 2, quad.ctypes.data, 2, 0, BIG, 0, 0.0, 3, 0, None, o.e, o.pn) == EINVAL   # (1, 1): lo == hi
    assert L.lh_kept_top_series(h2, 2, quad.ctypes.data, 1, 0, BIG, 0, 0.0, 3, 0, None, o.e, o.pn) == _native.ERANGE
    assert o.untouched()


def test_the_timing_hooks_refuse_what_the_calls_refuse(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    h1 = _handles(0x1000)
    pair, quad = np.array([0, 1], dtype=np.uint32), np.array([0, 1, 0, 1], dtype=np.uint32)
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    for fn, w in ((L.lh_tool_kept_top_series_passes_ms, pair), (L.lh_tool_kept_movers_series_passes_ms, quad)):
        wp = w.ctypes.data
        assert fn(None, 1, wp, 1, 0, 1, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
        assert fn(h1, 1, None, 1, 0, 1, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
        assert fn(h1, 1, wp, 0, 0, 1, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
        assert fn(h1, 1, wp, 1, 0, 1, 9, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
        assert fn(h1, 1, wp, 1, 0, BIG, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == ERANGE
        assert fn(h1, 1, wp, 1, 0, 0, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL      # nmetrics >= 1
        assert fn(h1, 1, wp, 1, 0, 1, 0, 0.0, 3, 0, None, None, C.byref(b)) == EINVAL
    assert a.value == -1.0 and b.value == -1.0
    # the records' bytes: 0 restores the default, the value before comes back
    was, now = C.c_uint64(0), C.c_uint64(0)
    assert L.lh_tool_kept_select_bytes(4096, C.byref(was)) == 0 and was.value == 64 << 20
    assert L.lh_tool_kept_select_bytes(0, C.byref(now)) == 0 and now.value == 4096
    assert L.lh_tool_kept_select_bytes(0, None) == 0
    assert L.lh_tool_kept_select_bytes(0, C.byref(now)) == 0 and now.value == 64 << 20


def test_python_wrapper_has_the_two_readers():
    import loghisto_amd
    K, W = loghisto_amd.Kept, loghisto_amd.KeptWindow
    lead, rest = ["self", "k", "by", "arg", "ascending"], ["nmetrics", "first", "out", "stream"]
    assert list(inspect.signature(K.top_series).parameters) == [*lead, "earlier", "windows", *rest]
    assert list(inspect.signature(K.movers_series).parameters) == [*lead, "earlier", "windows", "against", *rest]
    assert list(inspect.signature(W.top_series).parameters) == [*lead, "windows", *rest]
    assert list(inspect.signature(W.movers_series).parameters) == [*lead, "windows", "against", *rest]
    for fn, by in ((K.top_series, "count"), (W.top_series, "count"), (K.movers_series, "ks"), (W.movers_series, "ks")):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items()}
        assert d["by"] == by and d["arg"] is None and d["ascending"] is False and d["windows"] is None, fn
        assert d["nmetrics"] is None and d["first"] is None and d["out"] is None and d["stream"] is None, fn
        assert d.get("earlier", ()) == () and d.get("against") is None, fn
    # one copy of the by / arg checks: all six selecting readers go through the one _leaders
    src = inspect.getsource(loghisto_amd.engine)
    assert len(re.findall(r"def _leaders\(", src)) == 1 and len(re.findall(r"Snapshot\._leaders\(|self\._leaders\(", src)) == 5
    assert len(re.findall(r"by is one of", src)) == 1 and len(re.findall(r"takes an arg", src)) == 1
    # a window of more intervals than a call reads is refused before any call
    w = W(100)
    w.handles.extend([None] * 65)
    for read in (lambda: w.top_series(3), lambda: w.movers_series(3), lambda: w.movers_series(3, against=(0, 1))):
        with pytest.raises(ValueError):
            read()
