"""CPU tests of lh_movers / lh_movers_device (the k names whose distribution moved most between two snapshots): declared,
exported, bound, the entry's layout, and every LH_EINVAL check and the early LH_ERANGE run on the host before either snapshot
is looked at -- the snapshot pointers below are fakes that are never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_movers", "lh_movers_device"]


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == 10
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible
    consts = dict(re.findall(r"\b(LH_MOVERS_[A-Z0-9_]+)\s*=\s*(\d+)", src))
    assert consts == dict(LH_MOVERS_BY_KS="0", LH_MOVERS_BY_W1="1", LH_MOVERS_BY_SHIFT="2", LH_MOVERS_BY_PERCENTILE="3",
                          LH_MOVERS_ASCENDING="1")
    assert (_native.MOVERS_BY_KS, _native.MOVERS_BY_W1, _native.MOVERS_BY_SHIFT, _native.MOVERS_BY_PERCENTILE) == (0, 1, 2, 3)
    assert _native.MOVERS_ASCENDING == 1 and _native.MAX_TOP == 1024           # k is limited by LH_MAX_TOP: no constant of its own


def test_the_entry_is_32_bytes_and_the_dtype_is_the_struct():
    from loghisto_amd import _native
    src = open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read()
    body = re.search(r"typedef struct lh_mover_entry \{(.*?)\} lh_mover_entry;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    ctype = dict(uint32_t=C.c_uint32, int16_t=C.c_int16, uint16_t=C.c_uint16, uint64_t=C.c_uint64, double=C.c_double)

    class Entry(C.Structure):                                                  # the header's struct, laid out by the C rules
        _fields_ = [(name, ctype[t]) for t, name in fields]
    assert [name for _, name in fields] == ["id", "key", "key_base", "count_a", "count_b", "score"]
    assert C.sizeof(Entry) == 32 and _native.MOVER_ENTRY.itemsize == 32
    assert [_native.MOVER_ENTRY.fields[name][1] for _, name in fields] == [0, 4, 6, 8, 16, 24]
    for t, name in fields:
        assert getattr(Entry, name).offset == _native.MOVER_ENTRY.fields[name][1], name
        assert _native.MOVER_ENTRY.fields[name][0].itemsize == C.sizeof(ctype[t]), name
    kinds = {name: _native.MOVER_ENTRY.fields[name][0].kind for _, name in fields}
    assert kinds == dict(id="u", key="i", key_base="i", count_a="u", count_b="u", score="f")


def test_every_early_error_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    fake, fake2 = C.c_void_p(0x1000), C.c_void_p(0x2000)    # never dereferenced: the argument checks come first
    out = np.zeros(8, dtype=_native.MOVER_ENTRY)
    n = np.zeros(4, dtype=np.uint64)
    o, pn = out.ctypes.data, n.ctypes.data
    nan, inf = float("nan"), float("inf")
    KS, W1, SHIFT, PCT = range(4)
    for fn, n_align in ((L.lh_movers, C.sizeof(C.c_size_t)), (L.lh_movers_device, 4)):
        for by in (KS, W1, SHIFT, PCT):
            arg = 0.5
            assert fn(None, fake, 0, 1, by, arg, 4, 0, o, pn) == EINVAL             # NULL base / cur
            assert fn(fake, None, 0, 1, by, arg, 4, 0, o, pn) == EINVAL
            assert fn(None, None, 0, 0, by, arg, 4, 0, o, pn) == EINVAL             # ... whatever nmetrics
            assert fn(fake, fake2, 0, 1, by, arg, 0, 0, o, pn) == EINVAL            # k == 0
            assert fn(fake, fake2, 0, 1, by, arg, 1025, 0, o, pn) == EINVAL         # k > LH_MAX_TOP
            assert fn(fake, fake2, 0, 1, by, arg, (1 << 64) - 1, 0, o, pn) == EINVAL
            for flags in (2, 3, 0x80000000):                                        # unknown flag bits
                assert fn(fake, fake2, 0, 1, by, arg, 4, flags, o, pn) == EINVAL, flags
            assert fn(fake, fake2, 0, 1, by, arg, 4, 0, None, pn) == EINVAL         # NULL out / n_out
            assert fn(fake, fake2, 0, 1, by, arg, 4, 0, o, None) == EINVAL
            for off in (1, 2, 4):
                assert fn(fake, fake2, 0, 1, by, arg, 4, 0, o + off, pn) == EINVAL, off   # out not 8-byte aligned
            for off in range(1, n_align):
                assert fn(fake, fake2, 0, 1, by, arg, 4, 0, o, pn + off) == EINVAL, off   # n_out not aligned to its type
            # a cause of LH_EINVAL wins over the early LH_ERANGE
            assert fn(fake, fake2, 0, 1 << 32, by, arg, 0, 0, o, pn) == EINVAL
            assert fn(fake, fake2, 0, 1 << 32, by, arg, 4, 2, o, pn) == EINVAL
            assert fn(fake, None, 0, 1 << 32, by, arg, 4, 0, o, pn) == EINVAL
        for by in (4, 5, 0xffffffff):                                               # unknown `by`
            assert fn(fake, fake2, 0, 1, by, 0.5, 4, 0, o, pn) == EINVAL, by
        for p in (nan, -0.25, 1.0000000000000002, 2.0, inf, -inf):
            assert fn(fake, fake2, 0, 1, PCT, p, 4, 0, o, pn) == EINVAL, p          # no bucket to rank by
            assert fn(fake, fake2, 0, 1 << 32, PCT, p, 4, 0, o, pn) == EINVAL, p
        # more rows than any engine can have: LH_ERANGE, decided before a snapshot is looked at -- for every `by`, and with
        # the arg that is ignored for the first three set to anything
        for by, arg in ((KS, nan), (W1, 7.0), (SHIFT, -inf), (PCT, 0.0), (PCT, 0.5), (PCT, 1.0)):
            for flags in (0, 1):
                assert fn(fake, fake2, 0, 1 << 32, by, arg, 1024, flags, o, pn) == ERANGE, (by, arg)
                assert fn(fake, fake, 1, (1 << 64) - 1, by, arg, 1, flags, o, pn) == ERANGE, (by, arg)
    assert not out.view(np.uint8).any() and not n.any()                             # nothing was written


def test_the_timing_hook_checks_its_arguments(native_lib):
    from loghisto_amd import _native
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    fake = C.c_void_p(0x1000)
    L, EINVAL = native_lib, _native.EINVAL
    assert "lh_tool_movers_passes_ms" in _native.TUNING_SIGNATURES
    assert len(_native.TUNING_SIGNATURES["lh_tool_movers_passes_ms"][1]) == 10
    fn = L.lh_tool_movers_passes_ms
    assert fn(None, fake, 0, 1, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, None, 0, 1, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 0, 0.0, 0, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 0, 0.0, 1025, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 4, 0.0, 4, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 0, 0.0, 4, 2, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 3, 1.5, 4, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 0, 0.0, 4, 0, None, C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1, 0, 0.0, 4, 0, C.byref(a), None) == EINVAL
    assert fn(fake, fake, 0, 0, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == EINVAL
    assert fn(fake, fake, 0, 1 << 32, 0, 0.0, 4, 0, C.byref(a), C.byref(b)) == _native.ERANGE
    assert (a.value, b.value) == (-1.0, -1.0)


def test_python_wrapper_has_movers():
    import inspect

    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "movers"))
    assert list(inspect.signature(loghisto_amd.Snapshot.movers).parameters) == ["self", "base", "k", "by", "arg", "ascending",
                                                                                "nmetrics", "first", "out"]
