"""CPU tests of lh_top / lh_top_device (the k names that lead by count, sum, percentile bucket or count above a value):
declared, exported, bound, the entry's layout, and every LH_EINVAL check runs on the host before the snapshot is looked at
-- the snapshot pointer below is a fake that is never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_top", "lh_top_device"]


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == 9
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible
    consts = dict(re.findall(r"\b(LH_(?:MAX_TOP|TOP_[A-Z_]+))\s*=?\s*(\d+)", src))
    assert consts == dict(LH_MAX_TOP="1024", LH_TOP_BY_COUNT="0", LH_TOP_BY_SUM="1", LH_TOP_BY_PERCENTILE="2",
                          LH_TOP_BY_COUNT_ABOVE="3", LH_TOP_ASCENDING="1")
    assert (_native.MAX_TOP, _native.TOP_ASCENDING) == (1024, 1)
    assert (_native.TOP_BY_COUNT, _native.TOP_BY_SUM, _native.TOP_BY_PERCENTILE, _native.TOP_BY_COUNT_ABOVE) == (0, 1, 2, 3)


def test_the_entry_is_32_bytes_and_the_dtype_is_the_struct():
    from loghisto_amd import _native
    src = open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read()
    body = re.search(r"typedef struct lh_top_entry \{(.*?)\} lh_top_entry;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    ctype = dict(uint32_t=C.c_uint32, int16_t=C.c_int16, uint16_t=C.c_uint16, uint64_t=C.c_uint64, double=C.c_double)

    class Entry(C.Structure):                                                  # the header's struct, laid out by the C rules
        _fields_ = [(name, ctype[t]) for t, name in fields]
    assert [name for _, name in fields] == ["id", "pkey", "reserved", "count", "sum", "above"]
    assert C.sizeof(Entry) == 32 and _native.TOP_ENTRY.itemsize == 32
    assert [_native.TOP_ENTRY.fields[name][1] for _, name in fields] == [0, 4, 6, 8, 16, 24]
    for t, name in fields:
        assert getattr(Entry, name).offset == _native.TOP_ENTRY.fields[name][1], name
        assert _native.TOP_ENTRY.fields[name][0].itemsize == C.sizeof(ctype[t]), name
    assert _native.TOP_ENTRY.fields["pkey"][0].kind == "i" and _native.TOP_ENTRY.fields["sum"][0].kind == "f"


def test_every_einval_case_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    fake = C.c_void_p(0x1000)              # never dereferenced: the argument checks come first
    out = np.zeros(8, dtype=_native.TOP_ENTRY)
    n = np.zeros(4, dtype=np.uint64)
    o, pn = out.ctypes.data, n.ctypes.data
    nan = float("nan")
    COUNT, SUM, PCT, ABOVE = range(4)
    for fn, n_align in ((L.lh_top, C.sizeof(C.c_size_t)), (L.lh_top_device, 4)):
        assert fn(None, 0, 1, COUNT, 0.0, 4, 0, o, pn) == EINVAL                # NULL snapshot
        assert fn(None, 0, 0, COUNT, 0.0, 4, 0, o, pn) == EINVAL                # ... whatever nmetrics
        assert fn(fake, 0, 1, COUNT, 0.0, 0, 0, o, pn) == EINVAL                # k == 0
        assert fn(fake, 0, 1, COUNT, 0.0, 1025, 0, o, pn) == EINVAL             # k > LH_MAX_TOP
        assert fn(fake, 0, 1, COUNT, 0.0, (1 << 64) - 1, 0, o, pn) == EINVAL
        assert fn(fake, 0, 1, 4, 0.0, 4, 0, o, pn) == EINVAL                    # unknown `by`
        assert fn(fake, 0, 1, 0xffffffff, 0.0, 4, 0, o, pn) == EINVAL
        assert fn(fake, 0, 1, COUNT, 0.0, 4, 2, o, pn) == EINVAL                # unknown flag bits
        assert fn(fake, 0, 1, COUNT, 0.0, 4, 3, o, pn) == EINVAL
        assert fn(fake, 0, 1, COUNT, 0.0, 4, 0x80000000, o, pn) == EINVAL
        assert fn(fake, 0, 1, COUNT, 0.0, 4, 0, None, pn) == EINVAL             # NULL out / n_out
        assert fn(fake, 0, 1, COUNT, 0.0, 4, 0, o, None) == EINVAL
        for off in (1, 2, 4):
            assert fn(fake, 0, 1, COUNT, 0.0, 4, 0, o + off, pn) == EINVAL, off  # out not 8-byte aligned
        for off in range(1, n_align):
            assert fn(fake, 0, 1, COUNT, 0.0, 4, 0, o, pn + off) == EINVAL, off  # n_out not aligned to its type
        for by in (PCT, ABOVE):
            assert fn(fake, 0, 1, by, nan, 4, 0, o, pn) == EINVAL               # NaN where arg is used
        for p in (-0.25, 1.0000000000000002, 2.0, float("inf"), float("-inf")):
            assert fn(fake, 0, 1, PCT, p, 4, 0, o, pn) == EINVAL, p             # no bucket to rank by
        # an EINVAL cause wins over the early LH_ERANGE
        assert fn(fake, 0, 1 << 32, COUNT, 0.0, 0, 0, o, pn) == EINVAL
        # more rows than any engine can have: LH_ERANGE, decided before the snapshot is looked at -- for every `by`, and
        # with the args that are ignored for BY_COUNT / BY_SUM set to anything
        for by, arg in ((COUNT, nan), (SUM, 7.0), (PCT, 0.0), (PCT, 1.0), (ABOVE, float("inf")), (ABOVE, -1e300)):
            for flags in (0, 1):
                assert fn(fake, 0, 1 << 32, by, arg, 1024, flags, o, pn) == ERANGE, (by, arg)
                assert fn(fake, 1, (1 << 64) - 1, by, arg, 1, flags, o, pn) == ERANGE, (by, arg)
    assert not out.view(np.uint8).any() and not n.any()                         # nothing was written


def test_the_timing_hook_checks_its_arguments(native_lib):
    from loghisto_amd import _native
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    fake = C.c_void_p(0x1000)
    L = native_lib
    assert "lh_tool_top_passes_ms" in _native.TUNING_SIGNATURES
    assert L.lh_tool_top_passes_ms(None, 0, 1, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == _native.EINVAL
    assert L.lh_tool_top_passes_ms(fake, 0, 1, 0, 0.0, 0, 0, C.byref(a), C.byref(b)) == _native.EINVAL
    assert L.lh_tool_top_passes_ms(fake, 0, 1, 2, 1.5, 4, 0, C.byref(a), C.byref(b)) == _native.EINVAL
    assert L.lh_tool_top_passes_ms(fake, 0, 1, 0, 0.0, 4, 0, None, C.byref(b)) == _native.EINVAL
    assert L.lh_tool_top_passes_ms(fake, 0, 0, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == _native.EINVAL
    assert L.lh_tool_top_passes_ms(fake, 0, 1 << 32, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == _native.ERANGE
    assert (a.value, b.value) == (-1.0, -1.0)


def test_python_wrapper_has_top():
    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "top"))
