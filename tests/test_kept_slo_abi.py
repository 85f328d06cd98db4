"""CPU tests of lh_kept_slo* and lh_kept_burn* (lh_kept_heat* with a row of bounds PER ENTRY, and the multi-window burn-rate alert
over one bound and one budget per entry): declared, exported, bound with the header's prototypes, the record 8 bytes, and every
refusal that is decided on the host before any handle is looked at -- the handle pointers below are fakes that are never
dereferenced -- in its documented order and with no output written.  burn_fires, the NumPy statement of the rule, is held to its
own definition here: strictly above the product, ties and empty names do not fire, a NaN budget never does."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_kept_readers_abi import BIG, CTYPES, _header
from tests.test_kept_series_abi import _forms, _id_errors, _window_and_list_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = "lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, "
ROWS = {"": "uint32_t first, size_t nmetrics, ", "_ids": "const uint32_t *{}ids, size_t n, "}
SLO = "const double *{0}bounds, size_t nb, uint32_t flags, void *stream, uint64_t *{0}cum, uint64_t *{0}total"
BURN = ("const double *rate, const double *{0}bounds, const double *{0}budget, size_t k, uint32_t flags, void *stream, "
        "lh_burn_hit *{0}out, uint64_t *{0}n_out, uint64_t *{0}cum, uint64_t *{0}total")
PROTOS = {}
for _family, _tail in (("lh_kept_slo", SLO), ("lh_kept_burn", BURN)):
    for _rows, _text in ROWS.items():
        for _dev, _d in (("", ""), ("_device", "d_")):
            PROTOS[_family + _rows + _dev] = LIST + _text.format(_d) + _tail.format(_d)
CONTRACT = (
    "Entry (w, m) of cum and total is byte for byte what lh_kept_heat_ids* writes for window w and the one row of entry m with "
    "bounds + m * nb, nb.",
    "This holds in both kernel shapes, which agree exactly: only integers are involved.",
    "A DEVICE id outside some handle's block gives the empty entry in that window.",
    "each bound is taken on its own, so a decreasing device row is simply answered bound by bound, and a NaN bound takes in no bin "
    "and gives cum 0.",
    "fires = total != 0 && (double)bad > t * (double)total",
    "A NaN in a device budget never fires",
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
    # the record: two uint32, 8 bytes, in the header and in the binding
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+entry\s*,\s*row\s*;\s*\}\s*lh_burn_hit\s*;", src)
    assert _native.BURN_HIT.itemsize == 8 and _native.BURN_HIT.names == ("entry", "row")
    assert all(_native.BURN_HIT[f] == np.dtype("<u4") for f in ("entry", "row"))
    # adding functions is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_MAX_BOUNDS\s+64\b", src) and re.search(r"#define\s+LH_MAX_WINDOWS\s+128\b", src)
    # the contract stands in the header in its own words; the earlier readers keep their refusal, with a pointer to these
    flat = lambda s: re.sub(r"\s+\*?\s*(- )?", " ", s)                       # noqa: E731  (comment stars, bullets, line breaks)
    text = flat(open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    for sentence in CONTRACT:
        assert flat(sentence) in text, sentence
    assert "LH_LE_PER_METRIC is NOT supported here and returns LH_EINVAL" in text
    assert "per name over kept intervals is lh_kept_slo*" in text
    for out_of_scope in ("sharing cell reads between overlapping windows; more than LH_MAX_KEPT handles a call; per-name bounds for "
                         "lh_kept_top*'s count-above", "an OR or a per-pair rule across windows", "retuning the shape switch",
                         "any change to the snapshot-side lh_count_le"):
        assert out_of_scope in text, out_of_scope


def test_slo_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    row = [-np.inf, -1.0, -0.0, 0.0, 0.25, 0.25, 1e200, np.inf]
    bounds = np.array([row, row, [0.0] * 8])                  # three good rows of eight
    b = bounds.ctypes.data
    b65 = np.arange(65, dtype=np.float64)
    cum, total = np.full(3 * 128 * 64, 7, dtype=np.uint64), np.full(3 * 128, 7, dtype=np.uint64)
    outs = (cum.ctypes.data, total.ctypes.data)
    for fn in _forms(L, "lh_kept_slo", ids):
        for n in (1, 3, BIG):                                                 # each of these wins over the early LH_ERANGE
            good = _window_and_list_errors(fn, n, (b, 8, 0, None, *outs), EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                assert fn(k, nk, wp, nw, n, b, 0, 0, None, *outs) == EINVAL   # nb in 1 .. LH_MAX_BOUNDS
                assert fn(k, nk, wp, nw, n, b65.ctypes.data, 65, 0, None, *outs) == EINVAL
                assert fn(k, nk, wp, nw, n, None, 8, 0, None, *outs) == EINVAL   # NULL bounds
                assert fn(k, nk, wp, nw, n, b, 8, 0, None, None, None) == EINVAL   # both outputs NULL
                for flags in (_native.LE_PER_METRIC, 2, 0x80000000, 3):       # flags must be 0: the rows are the layout already
                    assert fn(k, nk, wp, nw, n, b, 8, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):                                       # arrays off their alignment
                    assert fn(k, nk, wp, nw, n, b + off, 2, 0, None, *outs) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, outs[0] + off, outs[1]) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, outs[0], outs[1] + off) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, b, 8, 0, None, None, outs[1] + off) == EINVAL, off
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            # more rows than any engine can have: LH_ERANGE before a handle is looked at and before a bound is read
            assert fn(k, nk, wp, nw, BIG, b, 8, 0, None, *outs) == ERANGE
            assert fn(k, nk, wp, nw, (1 << 64) - 1, b, 1, 0, None, None, outs[1]) == ERANGE
            # an empty call: LH_OK before any handle is looked at
            assert fn(k, nk, wp, nw, 0, b, 8, 0, None, *outs) == 0
            assert fn(k, nk, wp, nw, 0, b, 8, 0, 0x10, outs[0], None) == 0
            assert fn(k, nk, wp, nw, 0, b65.ctypes.data, 64, 0, None, *outs) == 0
    _id_errors(L, "lh_kept_slo", good, (b, 8, 0, None, *outs), ids, EINVAL)
    # ---- the rows of a HOST array, each by lh_count_le's rule, before any handle is looked at (the handles are fakes): a NaN or a
    #      decreasing pair in ANY row, the last one included; equal neighbours and -0.0 next to 0.0 are fine and reach the handles'
    #      checks, which these tests cannot go through -- so only the refusals are called
    host_forms = [f for i, f in enumerate(_forms(L, "lh_kept_slo", ids)) if i < 2]
    for fn in host_forms:
        for k, nk, w, nw in good[:2]:
            wp = w.ctypes.data
            for m in range(3):
                for j, v in ((0, np.nan), (7, np.nan), (3, np.nan)):
                    bad = bounds.copy()
                    bad[m, j] = v
                    assert fn(k, nk, wp, nw, 3, bad.ctypes.data, 8, 0, None, *outs) == EINVAL, (m, j)
                    assert fn(k, nk, wp, nw, 1, bad.ctypes.data + 8 * (8 * m + j), 1, 0, None, *outs) == EINVAL, (m, j)   # nb == 1
                down = bounds.copy()
                down[m, 5] = 0.2                                              # 0.25, 0.2: a decreasing pair inside row m
                assert fn(k, nk, wp, nw, 3, down.ctypes.data, 8, 0, None, *outs) == EINVAL, m
            # ... while the last bound of a row above the first of the next is no decreasing pair: rows are checked one by one.
            #     (Seen from nb = 4, rows 0 and 1 of `bounds` are {-inf, -1, -0, 0} and {0.25, 0.25, 1e200, inf}; as nb = 16 the
            #     array's first row decreases at its middle.)
            assert fn(k, nk, wp, nw, 1, bounds.ctypes.data, 16, 0, None, *outs) == EINVAL
    assert np.all(cum == 7) and np.all(total == 7)                            # nothing was written


def _burn_tail(rate, bounds, budget, k, flags, out, n_out, cum, total):
    return (rate, bounds, budget, k, flags, None, out, n_out, cum, total)


def test_burn_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    rate = np.full(128, 14.4)
    rate[1] = 0.0                                                             # a zero rate, and -0.0, are allowed
    rate[2] = -0.0
    bounds, budget = np.array([0.25, -np.inf, np.inf, -0.0]), np.array([0.001, 0.0, 1.0, -0.0])
    hits = np.full(8, 7, dtype=_native.BURN_HIT)
    n_out = np.full(2, 7, dtype=np.uint64)
    cum, total = np.full(4 * 128, 7, dtype=np.uint64), np.full(4 * 128, 7, dtype=np.uint64)
    r, b, g, o, no, cu, to = (a.ctypes.data for a in (rate, bounds, budget, hits, n_out, cum, total))
    ok = _burn_tail(r, b, g, 4, 0, o, no, cu, to)
    for fn in _forms(L, "lh_kept_burn", ids):
        for n in (1, 4, BIG):                                                 # each of these wins over the early LH_ERANGE
            good = _window_and_list_errors(fn, n, ok, EINVAL)
            for k, nk, w, nw in good:
                wp = w.ctypes.data
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, flags, o, no, cu, to)) == EINVAL, flags
                assert fn(k, nk, wp, nw, n, *_burn_tail(None, b, g, 4, 0, o, no, cu, to)) == EINVAL   # NULL rate, bounds, budget
                assert fn(k, nk, wp, nw, n, *_burn_tail(r, None, g, 4, 0, o, no, cu, to)) == EINVAL
                assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, None, 4, 0, o, no, cu, to)) == EINVAL
                assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, o, None, cu, to)) == EINVAL   # NULL n_out
                assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, None, no, cu, to)) == EINVAL   # k > 0 with NULL out
                assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 1, 0, None, no, None, None)) == EINVAL
                for off in range(1, 8):                                       # arrays off their alignment
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r + off, b, g, 4, 0, o, no, cu, to)) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b + off, g, 4, 0, o, no, cu, to)) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g + off, 4, 0, o, no, cu, to)) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, o, no + off, cu, to)) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, o, no, cu + off, to)) == EINVAL, off
                    assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, o, no, cu, to + off)) == EINVAL, off
                    if off < 4:
                        assert fn(k, nk, wp, nw, n, *_burn_tail(r, b, g, 4, 0, o + off, no, cu, to)) == EINVAL, off
                for at in sorted({0, nw - 1}):                                # a NaN or negative rate, in ALL forms, at either end
                    for v in (np.nan, -1.0, -np.inf, -5e-324):
                        bad = rate.copy()
                        bad[at] = v
                        assert fn(k, nk, wp, nw, n, *_burn_tail(bad.ctypes.data, b, g, 4, 0, o, no, cu, to)) == EINVAL, (at, v)
        for k, nk, w, nw in good:
            wp = w.ctypes.data
            assert fn(k, nk, wp, nw, BIG, *ok) == ERANGE                      # ... before a bound or a budget is read
            assert fn(k, nk, wp, nw, (1 << 64) - 1, *_burn_tail(r, b, g, 0, 0, None, no, None, None)) == ERANGE
            # an empty call: LH_OK before any handle is looked at, nothing written -- n_out included; a count-only call
            assert fn(k, nk, wp, nw, 0, *ok) == 0
            assert fn(k, nk, wp, nw, 0, *_burn_tail(r, b, g, 0, 0, None, no, None, None)) == 0
            assert fn(k, nk, wp, nw, 0, *_burn_tail(r, b, g, 1 << 40, 0, o, no, None, to)) == 0
    _id_errors(L, "lh_kept_burn", good, ok, ids, EINVAL)
    # ---- the per-entry HOST arrays, before any handle is looked at: a NaN or negative budget, a NaN bound, wherever
    host_forms = [f for i, f in enumerate(_forms(L, "lh_kept_burn", ids)) if i < 2]
    for fn in host_forms:
        for k, nk, w, nw in good[:2]:
            wp = w.ctypes.data
            for m in range(4):
                for v in (np.nan, -0.001, -np.inf):
                    bad = budget.copy()
                    bad[m] = v
                    assert fn(k, nk, wp, nw, 4, *_burn_tail(r, b, bad.ctypes.data, 4, 0, o, no, cu, to)) == EINVAL, (m, v)
                bad = bounds.copy()
                bad[m] = np.nan
                assert fn(k, nk, wp, nw, 4, *_burn_tail(r, bad.ctypes.data, g, 4, 0, o, no, cu, to)) == EINVAL, m
    assert np.all(hits["entry"] == 7) and np.all(hits["row"] == 7) and np.all(n_out == 7)   # nothing was written
    assert np.all(cum == 7) and np.all(total == 7)


def test_burn_fires_is_the_rule():
    from loghisto_amd import burn_fires
    below = np.nextafter(0.25, 0.0)
    total = np.array([1024, 1024, 1024, 0, 1024, 1 << 60, 3], dtype=np.uint64)
    cum = np.array([768, 768, 768, 0, 1024, (1 << 60) - (1 << 58), 2], dtype=np.uint64)     # bad: 256, 256, 256, 0, 0, 2^58, 1
    budget = np.array([0.25, below, np.nan, 0.0, 0.0, below, 1.0 / 3.0])
    got = burn_fires(cum, total, budget, 1.0)
    #   a tie does not fire; strictly above does; a NaN budget never does; no samples: never, whatever the budget; no bad sample
    #   against a zero budget: 0 > 0 is false; the same tie and step at 2^60; 1 > (1/3 rounded down) * 3 -- 0.333...31 * 3 rounds
    #   to 1.0 exactly, so this is a tie of the ROUNDED product and does not fire
    assert (1.0 / 3.0) * 3.0 == 1.0
    assert got.dtype == np.bool_ and got.tolist() == [False, True, False, False, False, True, False]
    # the first product is rounded on its own: rate * budget, then times total
    rate, bud, tot = 14.4, 0.001, np.array([1000000], dtype=np.uint64)
    t = rate * bud
    edge = int(np.floor(t * 1e6))                                            # bad == edge may tie or fall below; edge + 1 is above
    for bad in (edge - 1, edge, edge + 1):
        want = float(bad) > t * 1e6
        assert burn_fires(tot - np.uint64(bad), tot, np.array([bud]), rate).tolist() == [want], bad
    assert burn_fires(tot - np.uint64(edge + 1), tot, np.array([bud]), rate).tolist() == [True]
    # windows: cum / total (nwin, n), one rate per window; reported = fires in every window
    cum2 = np.array([[768, 768, 0], [0, 1000, 0]], dtype=np.uint64)
    total2 = np.array([[1024, 1024, 0], [1024, 1024, 5]], dtype=np.uint64)
    f = burn_fires(cum2, total2, np.array([0.2, 0.2, 0.2]), [1.0, 2.0])
    assert f.shape == (2, 3) and f.tolist() == [[True, True, False], [True, False, True]]
    assert f.all(axis=0).tolist() == [True, False, False]
    # a zero rate: any bad sample fires; uint64 -> float64 is the language's conversion (round to nearest even)
    assert burn_fires(np.array([0, 1], dtype=np.uint64), np.array([1, 1], dtype=np.uint64), np.array([0.5, 0.5]), 0.0).tolist() == [True, False]
    big = np.array([(1 << 64) - 1], dtype=np.uint64)
    assert burn_fires(np.array([0], dtype=np.uint64), big, np.array([1.0]), 1.0).tolist() == [False]    # 2^64 > 2^64 is false


def test_python_wrapper_has_the_two_readers():
    import loghisto_amd
    for cls, skip in ((loghisto_amd.Kept, ["earlier"]), (loghisto_amd.KeptWindow, [])):
        sig = inspect.signature(cls.slo)
        assert list(sig.parameters) == ["self", "bounds", *skip, "windows", "nmetrics", "first", "ids", "out", "stream"], cls
        d = {k: v.default for k, v in sig.parameters.items()}
        assert d["windows"] is None and d["nmetrics"] is None and d["first"] == 0 and d["ids"] is None and d["out"] is None
        sig = inspect.signature(cls.burn)
        assert list(sig.parameters) == ["self", "bounds", "budget", "rates", "k", *skip, "windows", "nmetrics", "first", "ids", "counts",
                                        "out", "stream"], cls
        d = {k: v.default for k, v in sig.parameters.items()}
        assert d["windows"] is None and d["counts"] is False and d["out"] is None and d["stream"] is None
    assert inspect.signature(loghisto_amd.Kept.slo).parameters["earlier"].default == ()
    assert "burn_fires" in loghisto_amd.__all__ and callable(loghisto_amd.burn_fires)
    # a window of more intervals than a call reads is refused before any call
    w = loghisto_amd.KeptWindow(100)
    w.handles.extend([None] * 65)
    for read in (lambda: w.slo([1.0]), lambda: w.burn([1.0], [0.1], [1.0], 1)):
        with pytest.raises(ValueError):
            read()
    # the earlier readers keep their signatures
    assert list(inspect.signature(loghisto_amd.Kept.heat).parameters) == ["self", "bounds", "earlier", "windows", "nmetrics", "first",
                                                                           "ids", "out", "stream"]
