"""CPU tests of lh_kept_count_le* and lh_kept_spread* (lh_count_le's and lh_spread's outputs over a list of kept intervals):
declared, exported, bound with the header's prototypes, and every LH_EINVAL, the early LH_ERANGE and the empty call decided on
the host before any handle is looked at -- the handle pointers below are fakes that are never dereferenced -- with no output
written."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = "lh_kept *const *kept, size_t nkept, "
ROWS = {"": "uint32_t first, size_t nmetrics, ", "_ids": "const uint32_t *{}ids, size_t n, "}
LE = "const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *{0}cum, uint64_t *{0}total"
SP = ("const double *p, size_t np, uint32_t flags, void *stream, uint64_t *{0}count, double *{0}sum, double *{0}m2, "
      "int16_t *{0}pkeys, uint8_t *{0}pvalid, uint64_t *{0}count_le, double *{0}sum_le")
PROTOS = {}
for _family, _tail in (("lh_kept_count_le", LE), ("lh_kept_spread", SP)):
    for _rows, _text in ROWS.items():
        for _dev, _d in (("", ""), ("_device", "d_")):
            PROTOS[_family + _rows + _dev] = LIST + _text.format(_d) + _tail.format(_d)
CTYPES = {"size_t": C.c_size_t, "uint32_t": C.c_uint32}            # every pointer is bound as c_void_p
VP = C.c_void_p
BIG = 1 << 32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)


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
    # adding functions is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert re.search(r"#define\s+LH_MAX_BOUNDS\s+64\b", src) and _native.MAX_BOUNDS == 64
    # what is out of scope, and what the two shapes promise, stand in the header
    text = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    assert "LH_LE_PER_METRIC is NOT supported here and returns LH_EINVAL" in text
    assert "agree BIT FOR BIT on every output" in text


def _handles(*addrs):
    return (VP * len(addrs))(*addrs)


def _lists():
    one, h64 = _handles(0x1000), _handles(*[0x1000 * (i + 1) for i in range(64)])
    good = ((one, 1), (_handles(0x1000, 0x2000), 2), (h64, 64))
    h65 = _handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [_handles(None), _handles(None, 0x2000), _handles(0x1000, None), _handles(*([0x1000] * 63 + [None]))]
    return good, h65, holes


def _forms(L, family, ids):
    """call(kept, nkept, n, *tail) for the family's four entry points (tail: everything behind the rows)"""
    for dev in ("", "_device"):
        yield lambda k, nk, n, *t, fn=getattr(L, family + dev): fn(k, nk, 0, n, *t)
        yield lambda k, nk, n, *t, fn=getattr(L, family + "_ids" + dev): fn(k, nk, ids.ctypes.data, n, *t)


def _list_errors(fn, n, tail, EINVAL):
    good, h65, holes = _lists()
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    assert fn(None, 1, n, *tail) == EINVAL and fn(None, 0, n, *tail) == EINVAL
    for off in range(1, C.sizeof(VP)):
        assert fn(C.addressof(odd) + off, 1, n, *tail) == EINVAL, off
    for h in holes:                                                           # a NULL entry, wherever
        assert fn(h, len(h), n, *tail) == EINVAL
    assert fn(good[0][0], 0, n, *tail) == EINVAL                              # an empty list
    assert fn(h65, 65, n, *tail) == EINVAL and fn(h65, (1 << 64) - 1, n, *tail) == EINVAL
    return good


def _id_errors(L, family, good, tail, ids, EINVAL):
    for fn in (getattr(L, family + "_ids"), getattr(L, family + "_ids_device")):
        for k, nk in good:
            assert fn(k, nk, None, 1, *tail) == EINVAL                        # ids NULL with n > 0
            assert fn(k, nk, None, BIG, *tail) == EINVAL                      # ... wins over the early LH_ERANGE
            assert fn(k, nk, None, 0, *tail) == 0                             # n == 0: no list is needed
            for off in (1, 2, 3):                                             # ids misaligned
                for n in (0, 1, BIG):
                    assert fn(k, nk, ids.ctypes.data + off, n, *tail) == EINVAL, (off, n)


def test_count_le_early_errors_are_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    ids = np.arange(4, dtype=np.uint32)
    bounds = np.array([-np.inf, -1.0, -0.0, 0.0, 0.25, 0.25, 1e200, np.inf])
    b = bounds.ctypes.data
    b65 = np.arange(65, dtype=np.float64)
    cum, total = np.full(8 * 64, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint64)
    outs = (cum.ctypes.data, total.ctypes.data)
    nan, down, neg0 = np.array([0.0, np.nan, 1.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, -0.0, 0.0])
    for fn in _forms(L, "lh_kept_count_le", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _list_errors(fn, n, (b, 8, 0, None, *outs), EINVAL)
            for k, nk in good:
                assert fn(k, nk, n, b, 0, 0, None, *outs) == EINVAL           # nb in 1 .. LH_MAX_BOUNDS
                assert fn(k, nk, n, b65.ctypes.data, 65, 0, None, *outs) == EINVAL
                assert fn(k, nk, n, None, 8, 0, None, *outs) == EINVAL        # NULL bounds
                assert fn(k, nk, n, nan.ctypes.data, 3, 0, None, *outs) == EINVAL          # a NaN bound
                assert fn(k, nk, n, nan.ctypes.data + 8, 1, 0, None, *outs) == EINVAL
                assert fn(k, nk, n, down.ctypes.data, 3, 0, None, *outs) == EINVAL         # a decreasing row
                assert fn(k, nk, n, b, 8, 0, None, None, None) == EINVAL      # both outputs NULL
                for flags in (_native.LE_PER_METRIC, 2, 0x80000000, 3):       # flags must be 0: a row of bounds per name is out of scope
                    assert fn(k, nk, n, b, 8, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):                                       # arrays off their alignment
                    assert fn(k, nk, n, b + off, 2, 0, None, *outs) == EINVAL, off
                    assert fn(k, nk, n, b, 8, 0, None, outs[0] + off, outs[1]) == EINVAL, off
                    assert fn(k, nk, n, b, 8, 0, None, outs[0], outs[1] + off) == EINVAL, off
                    assert fn(k, nk, n, b, 8, 0, None, None, outs[1] + off) == EINVAL, off
        for k, nk in _lists()[0]:
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(k, nk, BIG, b, 8, 0, None, *outs) == ERANGE
            assert fn(k, nk, (1 << 64) - 1, b, 8, 0, None, None, outs[1]) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes); equal neighbours, both zeros, one bound
            assert fn(k, nk, 0, b, 8, 0, None, *outs) == 0
            assert fn(k, nk, 0, b, 8, 0, 0x10, outs[0], None) == 0
            assert fn(k, nk, 0, neg0.ctypes.data, 3, 0, None, *outs) == 0
            assert fn(k, nk, 0, b65.ctypes.data, 64, 0, None, *outs) == 0
            assert fn(k, nk, 0, b, 1, 0, None, *outs) == 0
    _id_errors(L, "lh_kept_count_le", _lists()[0], (b, 8, 0, None, *outs), ids, EINVAL)
    assert np.all(cum == 7) and np.all(total == 7)                            # nothing was written


def test_spread_early_errors_are_decided_on_the_host(native_lib):
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
    for fn in _forms(L, "lh_kept_spread", ids):
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            good = _list_errors(fn, n, (pp, 4, 0, None, *outs), EINVAL)
            for k, nk in good:
                assert fn(k, nk, n, p33.ctypes.data, 33, 0, None, *outs) == EINVAL         # np <= LH_MAX_PERCENTILES
                assert fn(k, nk, n, None, 4, 0, None, *outs) == EINVAL        # np > 0 with NULL p
                assert fn(k, nk, n, pp, 4, 0, None, *[None] * 7) == EINVAL    # all outputs NULL
                assert fn(k, nk, n, None, 0, 0, None, None, None, None, *outs[3:]) == EINVAL   # np == 0: the last four count for nothing
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(k, nk, n, pp, 4, flags, None, *outs) == EINVAL, flags
                for off in range(1, 8):
                    assert fn(k, nk, n, pp + off, 1, 0, None, *outs) == EINVAL, off
                for j, width in enumerate(widths):                            # an output off its element's alignment
                    for off in range(1, width):
                        bad = list(outs)
                        bad[j] += off
                        assert fn(k, nk, n, pp, 4, 0, None, *bad) == EINVAL, (j, off)
                        only = [None] * 7
                        only[j] = bad[j]
                        assert fn(k, nk, n, pp, 4, 0, None, *only) == EINVAL, (j, off)
        for k, nk in _lists()[0]:
            assert fn(k, nk, BIG, pp, 4, 0, None, *outs) == ERANGE
            assert fn(k, nk, (1 << 64) - 1, None, 0, 0, None, None, outs[1], *[None] * 5) == ERANGE
            # an empty call: LH_OK before any handle is looked at; np == 0 is allowed (moments only), and p is then not looked at
            assert fn(k, nk, 0, pp, 4, 0, None, *outs) == 0
            assert fn(k, nk, 0, None, 0, 0, 0x10, outs[0], None, None, 1, 1, 1, 1) == 0
            assert fn(k, nk, 0, p33.ctypes.data, 32, 0, None, *[None] * 4, outs[4], None, None) == 0
    _id_errors(L, "lh_kept_spread", _lists()[0], (pp, 4, 0, None, *outs), ids, EINVAL)
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written


def test_python_wrapper_has_the_two_readers():
    import loghisto_amd
    for name, lead in (("count_le", "bounds"), ("spread", "percentiles")):
        sig = inspect.signature(getattr(loghisto_amd.Kept, name))
        assert list(sig.parameters) == ["self", lead, "earlier", "nmetrics", "first", "ids", "out", "stream"], name
        d = {k: v.default for k, v in sig.parameters.items()}
        assert d["earlier"] == () and d["nmetrics"] is None and d["first"] == 0, name
        assert d["ids"] is None and d["out"] is None and d["stream"] is None, name
    # the snapshot readers and the earlier kept readers keep their signatures
    assert list(inspect.signature(loghisto_amd.Snapshot.spread).parameters) == ["self", "percentiles", "nmetrics", "first", "out"]
    assert list(inspect.signature(loghisto_amd.Snapshot.count_le).parameters) == ["self", "bounds", "nmetrics", "first", "out"]
    assert list(inspect.signature(loghisto_amd.Kept.across).parameters)[:7] == ["self", "earlier", "percentiles", "nmetrics", "first",
                                                                                 "ids", "out"]
