"""CPU tests of lh_kept_top* and lh_kept_movers* (lh_top's and lh_movers' selections over lists of kept intervals): declared,
exported, bound with the header's prototypes, and every LH_EINVAL, the early LH_ERANGE and the host forms' empty call decided on
the host, in the documented order, before any handle is looked at -- the handle pointers below are fakes that are never
dereferenced -- with no output written."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = "lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, "
MOV = ("lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics, uint32_t by, "
       "double arg, size_t k, uint32_t flags, void *stream, ")
PROTOS = {
    "lh_kept_top": TOP + "lh_top_entry *out, size_t *n_out",
    "lh_kept_top_device": TOP + "lh_top_entry *d_out, uint32_t *d_n_out",
    "lh_kept_movers": MOV + "lh_mover_entry *out, size_t *n_out",
    "lh_kept_movers_device": MOV + "lh_mover_entry *d_out, uint32_t *d_n_out",
}
TOOLS = {
    "lh_tool_kept_top_passes_ms": TOP + "float *score_ms, float *select_ms",
    "lh_tool_kept_movers_passes_ms": MOV + "float *score_ms, float *select_ms",
}
CTYPES = {"size_t": C.c_size_t, "uint32_t": C.c_uint32, "double": C.c_double}
VP = C.c_void_p
BIG = 1 << 32
PATTERN = 0x5a


def _header(name="loghisto_gpu.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_six_symbols_are_declared_exported_and_bound(native_lib):
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
            want = [(C.POINTER(C.c_float) if a.startswith("float") else C.c_void_p) if "*" in a else CTYPES[a.split()[0]]
                    for a in proto.split(", ")]
            assert restype is C.c_int and argtypes == want, name
    # adding functions is backward compatible: no new version, limit, entry type or error code
    src = _header()
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert re.search(r"#define\s+LH_MAX_TOP\s+1024\b", src) and _native.MAX_TOP == 1024
    assert len(re.findall(r"typedef\s+struct\s+lh_top_entry\b", src)) == 1 and len(re.findall(r"typedef\s+struct\s+lh_mover_entry\b", src)) == 1
    assert not re.search(r"\blh_kept_(top|movers)_ids", src)                      # no _ids forms
    # what is bit-equal to what stands in the header
    text = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    assert "sum is BIT-EQUAL to lh_kept_across' sum for the same list and row" in text
    assert "BIT-EQUAL to lh_kept_compare's ks, w1 and shift for the same lists" in text
    assert "ORDER OF THE CHECKS" in text


def _handles(*addrs):
    return (VP * len(addrs))(*addrs)


def _lists():
    one, h64 = _handles(0x1000), _handles(*[0x1000 * (i + 1) for i in range(64)])
    good = ((one, 1), (_handles(0x1000, 0x2000), 2), (h64, 64))
    h65 = _handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [_handles(None), _handles(None, 0x2000), _handles(0x1000, None), _handles(*([0x1000] * 63 + [None]))]
    return good, h65, holes


class Out:
    """entries and n_out, pre-filled with a pattern"""

    def __init__(self):
        self.entries = np.full(32 * 1024 + 8, PATTERN, dtype=np.uint8)
        self.n = np.full(16, PATTERN, dtype=np.uint8)
        self.e, self.pn = self.entries.ctypes.data, self.n.ctypes.data
        assert self.e % 8 == 0 and self.pn % 8 == 0

    def untouched(self):
        return bool(np.all(self.entries == PATTERN) and np.all(self.n == PATTERN))


def _top_forms(L):
    """(call(kept, nkept, nmetrics, by, arg, k, flags, out, n_out), alignment of n_out, host form?)"""
    for name, align in (("lh_kept_top", C.sizeof(C.c_size_t)), ("lh_kept_top_device", 4)):
        yield (lambda kept, nk, n, by, arg, k, flags, out, n_out, fn=getattr(L, name): fn(kept, nk, 0, n, by, arg, k, flags, None, out, n_out),
               align, name == "lh_kept_top")


def _movers_forms(L):
    """(call(base, nbase, cur, ncur, nmetrics, by, arg, k, flags, out, n_out), alignment of n_out, host form?)"""
    for name, align in (("lh_kept_movers", C.sizeof(C.c_size_t)), ("lh_kept_movers_device", 4)):
        yield (lambda b, nb, c, nc, n, by, arg, k, flags, out, n_out, fn=getattr(L, name): fn(b, nb, c, nc, 0, n, by, arg, k, flags, None, out,
                                                                                             n_out),
               align, name == "lh_kept_movers")


def _common_errors(call, align, n, o, EINVAL, by_last, needs_arg, ascending):
    """the causes of LH_EINVAL behind the lists: call(nmetrics, by, arg, k, flags, out, n_out)"""
    nan = float("nan")
    for by in (by_last + 1, 7, 0xffffffff):                                       # unknown by
        assert call(n, by, 0.5, 3, 0, o.e, o.pn) == EINVAL, by
    for flags in (2, 3, 4, 0x80000000, ascending | 0x100):                        # unknown flag bits
        assert call(n, 0, 0.0, 3, flags, o.e, o.pn) == EINVAL, flags
    for by, bad in needs_arg:                                                     # lh_top's / lh_movers' rules for arg
        for arg in bad:
            assert call(n, by, arg, 3, 0, o.e, o.pn) == EINVAL, (by, arg)
            assert call(n, by, arg, 3, ascending, o.e, o.pn) == EINVAL, (by, arg)
    assert call(n, 0, nan, 0, 0, o.e, o.pn) == EINVAL                             # k in 1 .. LH_MAX_TOP
    assert call(n, 0, nan, 1025, 0, o.e, o.pn) == EINVAL and call(n, 0, 0.0, (1 << 64) - 1, 0, o.e, o.pn) == EINVAL
    assert call(n, 0, 0.0, 3, 0, None, o.pn) == EINVAL and call(n, 0, 0.0, 3, 0, o.e, None) == EINVAL
    for off in range(1, 8):                                                       # out off its 8 bytes
        assert call(n, 0, 0.0, 3, 0, o.e + off, o.pn) == EINVAL, off
    for off in range(1, align):                                                   # n_out off its type's alignment
        assert call(n, 0, 0.0, 3, 0, o.e, o.pn + off) == EINVAL, off


def test_top_early_errors_are_decided_on_the_host_in_the_documented_order(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    nan, inf = float("nan"), float("inf")
    o = Out()
    odd = (C.c_char * 64)()
    for fn, align, host in _top_forms(L):
        for n in (1, BIG):                                                        # each cause of LH_EINVAL wins over the early LH_ERANGE
            good, h65, holes = _lists()
            assert fn(None, 1, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL and fn(None, 0, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL
            for off in range(1, C.sizeof(VP)):
                assert fn(C.addressof(odd) + off, 1, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL, off
            assert fn(good[0][0], 0, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL        # an empty list
            assert fn(h65, 65, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL and fn(h65, (1 << 64) - 1, n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL
            for h in holes:                                                       # a NULL entry, wherever
                assert fn(h, len(h), n, 0, 0.0, 3, 0, o.e, o.pn) == EINVAL
            for kept, nk in good:
                _common_errors(lambda *a: fn(kept, nk, *a), align, n, o, EINVAL, _native.TOP_BY_COUNT_ABOVE,
                               ((_native.TOP_BY_PERCENTILE, (nan, -0.25, 1.0000001, inf, -inf)), (_native.TOP_BY_COUNT_ABOVE, (nan,))),
                               _native.TOP_ASCENDING)
        for kept, nk in _lists()[0]:
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            for by, arg in ((0, nan), (1, nan), (2, 0.0), (2, 1.0), (3, inf), (3, -inf), (3, 1e200)):
                assert fn(kept, nk, BIG, by, arg, 1024, _native.TOP_ASCENDING, o.e, o.pn) == ERANGE, (by, arg)
            assert fn(kept, nk, (1 << 64) - 1, 0, 0.0, 1, 0, o.e, o.pn) == ERANGE
        assert o.untouched()
    # the host form's empty call: *n_out = 0 and nothing else, before any handle is looked at (the handles are fakes)
    for kept, nk in _lists()[0]:
        o = Out()
        o.n[:] = 0xff
        assert L.lh_kept_top(kept, nk, 0, 0, 2, 0.99, 20, 0, None, o.e, o.pn) == 0
        assert np.all(o.n[:C.sizeof(C.c_size_t)] == 0) and np.all(o.n[C.sizeof(C.c_size_t):] == 0xff) and np.all(o.entries == PATTERN)
        assert L.lh_kept_top(kept, nk, 12345, 0, 0, nan, 1024, 1, 0x10, o.e, o.pn) == 0


def test_movers_early_errors_are_decided_on_the_host_in_the_documented_order(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    nan, inf = float("nan"), float("inf")
    o = Out()
    odd = (C.c_char * 64)()
    h1, h32, h33, h63, h64 = (_handles(*[0x1000 * (i + 1) for i in range(n)]) for n in (1, 32, 33, 63, 64))
    pairs = ((h1, 1, h1, 1), (h32, 32, h32, 32), (h1, 1, h63, 63), (h63, 63, h1, 1))
    for fn, align, host in _movers_forms(L):
        for n in (1, BIG):
            tail = (n, 0, 0.0, 3, 0, o.e, o.pn)
            assert fn(None, 1, h1, 1, *tail) == EINVAL and fn(h1, 1, None, 1, *tail) == EINVAL     # a NULL list
            for off in range(1, C.sizeof(VP)):                                    # a list off its alignment
                assert fn(C.addressof(odd) + off, 1, h1, 1, *tail) == EINVAL and fn(h1, 1, C.addressof(odd) + off, 1, *tail) == EINVAL
            assert fn(h1, 0, h1, 1, *tail) == EINVAL and fn(h1, 1, h1, 0, *tail) == EINVAL         # an empty side
            assert fn(h32, 32, h33, 33, *tail) == EINVAL and fn(h33, 33, h32, 32, *tail) == EINVAL  # more than 64 in all
            assert fn(h64, 64, h1, 1, *tail) == EINVAL and fn(h1, 1, h64, 64, *tail) == EINVAL
            assert fn(h1, (1 << 64) - 1, h1, 2, *tail) == EINVAL and fn(h1, 1, h1, (1 << 64) - 1, *tail) == EINVAL
            hole = _handles(0x1000, None)
            assert fn(hole, 2, h1, 1, *tail) == EINVAL and fn(h1, 1, hole, 2, *tail) == EINVAL      # a NULL entry
            assert fn(_handles(None), 1, h1, 1, *tail) == EINVAL
            for b, nb, c, nc in pairs:
                _common_errors(lambda *a: fn(b, nb, c, nc, *a), align, n, o, EINVAL, _native.MOVERS_BY_PERCENTILE,
                               ((_native.MOVERS_BY_PERCENTILE, (nan, -0.25, 1.0000001, inf, -inf)),), _native.MOVERS_ASCENDING)
        for b, nb, c, nc in pairs:
            for by, arg in ((0, nan), (1, nan), (2, inf), (3, 0.0), (3, 1.0)):    # arg is ignored for the three distances
                assert fn(b, nb, c, nc, BIG, by, arg, 1024, _native.MOVERS_ASCENDING, o.e, o.pn) == ERANGE, (by, arg)
            assert fn(b, nb, c, nc, (1 << 64) - 1, 0, 0.0, 1, 0, o.e, o.pn) == ERANGE
        assert o.untouched()
    for b, nb, c, nc in pairs:
        o = Out()
        o.n[:] = 0xff
        assert L.lh_kept_movers(b, nb, c, nc, 0, 0, 3, 0.5, 20, 0, None, o.e, o.pn) == 0
        assert np.all(o.n[:C.sizeof(C.c_size_t)] == 0) and np.all(o.n[C.sizeof(C.c_size_t):] == 0xff) and np.all(o.entries == PATTERN)


def test_the_timing_hooks_refuse_what_the_calls_refuse(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    h1 = _handles(0x1000)
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    assert L.lh_tool_kept_top_passes_ms(None, 1, 0, 1, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
    assert L.lh_tool_kept_top_passes_ms(h1, 1, 0, 1, 9, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
    assert L.lh_tool_kept_top_passes_ms(h1, 1, 0, BIG, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == ERANGE
    assert L.lh_tool_kept_top_passes_ms(h1, 1, 0, 0, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL      # nmetrics >= 1
    assert L.lh_tool_kept_movers_passes_ms(h1, 1, h1, 0, 0, 1, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
    assert L.lh_tool_kept_movers_passes_ms(h1, 1, h1, 1, 0, 1, 3, 2.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
    assert L.lh_tool_kept_movers_passes_ms(h1, 1, h1, 1, 0, 0, 0, 0.0, 3, 0, None, C.byref(a), C.byref(b)) == EINVAL
    assert L.lh_tool_kept_movers_passes_ms(h1, 1, h1, 1, 0, 1, 0, 0.0, 3, 0, None, None, C.byref(b)) == EINVAL
    assert a.value == -1.0 and b.value == -1.0


def test_python_wrapper_has_the_two_selecting_readers():
    import loghisto_amd
    top = inspect.signature(loghisto_amd.Kept.top)
    assert list(top.parameters) == ["self", "k", "by", "arg", "ascending", "earlier", "nmetrics", "first", "out", "stream"]
    mov = inspect.signature(loghisto_amd.Kept.movers)
    assert list(mov.parameters) == ["self", "base", "k", "by", "arg", "ascending", "earlier", "nmetrics", "first", "out", "stream"]
    for sig, by in ((top, "count"), (mov, "ks")):
        d = {k: v.default for k, v in sig.parameters.items()}
        assert d["by"] == by and d["arg"] is None and d["ascending"] is False and d["earlier"] == ()
        assert d["nmetrics"] is None and d["first"] is None and d["out"] is None and d["stream"] is None
    # the snapshot's two keep their signatures, and all four go through one _leaders
    assert list(inspect.signature(loghisto_amd.Snapshot.top).parameters) == ["self", "k", "by", "arg", "ascending", "nmetrics", "first", "out"]
    assert list(inspect.signature(loghisto_amd.Snapshot.movers).parameters) == ["self", "base", "k", "by", "arg", "ascending", "nmetrics",
                                                                               "first", "out"]
    src = inspect.getsource(loghisto_amd.engine)
    assert len(re.findall(r"def _leaders\(", src)) == 1 and len(re.findall(r"_leaders\(\"lh_", src)) == 4
