"""CPU tests of lh_keep / lh_kept_* (intervals kept in compact form on the device, and lh_across' outputs over a list of
them): declared, exported, bound, and every LH_EINVAL check and the early LH_ERANGE run on the host before any handle is
looked at -- the handle pointers below are fakes that are never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"lh_keep": 5, "lh_kept_release": 1, "lh_kept_info_get": 2, "lh_kept_arrays": 5, "lh_kept_hold": 2, "lh_kept_across": 14,
        "lh_kept_across_device": 14, "lh_kept_across_ids": 14, "lh_kept_across_ids_device": 14}
TOOLS = {"lh_tool_kept_switch": 2, "lh_tool_kept_tile": 1}


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return src, set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    raw = C.CDLL(_native.LIB_PATH)
    for header, table, names in (("loghisto_gpu.h", _native.SIGNATURES, ARGS),
                                 ("loghisto_gpu_tuning.h", _native.TUNING_SIGNATURES, TOOLS)):
        src, declared = _declared(header)
        for name, nargs in names.items():
            assert name in declared, name
            assert hasattr(raw, name), f"{name} is not exported"
            assert name in table and getattr(native_lib, name).restype is C.c_int, name
            assert len(table[name][1]) == nargs, name
            decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
            assert len(decl.split(",")) == nargs, decl
    src, _ = _declared("loghisto_gpu.h")
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert re.search(r"typedef\s+struct\s+lh_kept\s+lh_kept\s*;", src)
    assert C.sizeof(_native.LhKeptInfo) == 40
    fields = re.search(r"typedef\s+struct\s+lh_kept_info\s*\{(.*?)\}\s*lh_kept_info\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == [k for k, _ in _native.LhKeptInfo._fields_]


def test_every_early_error_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two = handles(0x1000), handles(0x1000, 0x2000)
    full = handles(*[0x1000 * (i + 1) for i in range(64)])
    too_many = handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 63 + [None])),
             handles(*([0x1000] * 31 + [None] + [0x1000] * 32))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    p = np.array([0.5, 0.99, 1.0, float("nan")])
    count, total = np.full(8, 7, dtype=np.uint64), np.full(8, 7.0)
    nb, bits = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint64)
    keys, valid = np.full(64, 7, dtype=np.int16), np.full(64, 7, dtype=np.uint8)
    ids = np.arange(4, dtype=np.uint32)
    outs = [a.ctypes.data for a in (count, total, nb, bits, keys, valid)]
    pp = p.ctypes.data

    def forms():
        """(call(list, nkept, n, p, np, flags, *outs, first=0, ids=...), by id?) for the four entry points, the stream NULL"""
        for fn in (L.lh_kept_across, L.lh_kept_across_device):
            yield (lambda h, nk, n, p_, np_, fl, *o, fn=fn: fn(h, nk, 0, n, p_, np_, fl, None, *o)), False
        for fn in (L.lh_kept_across_ids, L.lh_kept_across_ids_device):
            yield (lambda h, nk, n, p_, np_, fl, *o, fn=fn, ids=ids.ctypes.data: fn(h, nk, ids, n, p_, np_, fl, None, *o)), True

    for fn, by_id in forms():
        assert fn(None, 1, 1, pp, 4, 0, *outs) == EINVAL                          # NULL list
        assert fn(None, 0, 0, pp, 4, 0, *outs) == EINVAL                          # ... whatever the rest
        for h in holes:                                                           # a NULL entry, wherever
            assert fn(h, len(h), 1, pp, 4, 0, *outs) == EINVAL
            assert fn(h, len(h), 0, pp, 4, 0, *outs) == EINVAL
        assert fn(one, 0, 1, pp, 4, 0, *outs) == EINVAL                           # nkept 0
        assert fn(too_many, 65, 1, pp, 4, 0, *outs) == EINVAL                     # nkept too large
        assert fn(full, (1 << 64) - 1, 1, pp, 4, 0, *outs) == EINVAL
        for off in range(1, C.sizeof(VP)):                                        # the list itself off its alignment
            assert fn(C.addressof(odd) + off, 1, 1, pp, 4, 0, *outs) == EINVAL, off
        for s, n in ((one, 1), (two, 2), (full, 64)):
            assert fn(s, n, 1, pp, 33, 0, *outs) == EINVAL                        # np too large
            assert fn(s, n, 1, pp, (1 << 64) - 1, 0, *outs) == EINVAL
            assert fn(s, n, 1, None, 1, 0, *outs) == EINVAL                       # np > 0 with NULL p
            assert fn(s, n, 1, pp, 4, 0, None, None, None, None, None, None) == EINVAL      # all outputs NULL
            assert fn(s, n, 1, None, 0, 0, None, None, None, None, outs[4], outs[5]) == EINVAL   # np == 0: those two are ignored
            for flags in (1, 2, 0x80000000):                                      # unknown flag bits
                assert fn(s, n, 1, pp, 4, flags, *outs) == EINVAL, flags
            for k, width in enumerate((8, 8, 4, 8, 2)):                           # arrays not aligned to their element size
                for off in range(1, width):
                    bad = list(outs)
                    bad[k] += off
                    assert fn(s, n, 1, pp, 4, 0, *bad) == EINVAL, (k, off)
                    only = [None] * 6
                    only[k] = bad[k]
                    assert fn(s, n, 1, pp, 4, 0, *only) == EINVAL, (k, off)
            for off in (1, 2, 4):
                assert fn(s, n, 1, pp + off, 3, 0, *outs) == EINVAL, off          # p not 8-byte aligned
            # a cause of LH_EINVAL wins over the early LH_ERANGE
            assert fn(s, n, 1 << 32, pp, 33, 0, *outs) == EINVAL
            assert fn(s, n, 1 << 32, pp, 4, 1, *outs) == EINVAL
            assert fn(s, n, 1 << 32, pp, 4, 0, outs[0] + 4, *outs[1:]) == EINVAL
            assert fn(s, 0, 1 << 32, pp, 4, 0, *outs) == EINVAL
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(s, n, 1 << 32, pp, 4, 0, *outs) == ERANGE
            assert fn(s, n, (1 << 64) - 1, pp, 4, 0, *outs) == ERANGE
            assert fn(s, n, 1 << 32, None, 0, 0, outs[0], None, None, None, None, None) == ERANGE
            assert fn(s, n, 1 << 32, pp, 32, 0, None, None, None, None, None, outs[5]) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes)
            assert fn(s, n, 0, pp, 4, 0, *outs) == 0
            assert fn(s, n, 0, None, 0, 0, outs[0], None, None, None, None, None) == 0
        assert fn(holes[2], 2, 1 << 32, pp, 4, 0, *outs) == EINVAL
    # the id forms' own causes
    for fn in (L.lh_kept_across_ids, L.lh_kept_across_ids_device):
        for s, n in ((one, 1), (full, 64)):
            assert fn(s, n, None, 1, pp, 4, 0, None, *outs) == EINVAL             # ids NULL with n > 0
            assert fn(s, n, None, 1 << 32, pp, 4, 0, None, *outs) == EINVAL       # ... wins over the early LH_ERANGE
            assert fn(s, n, None, 0, pp, 4, 0, None, *outs) == 0                  # n == 0: no list is needed
            for off in (1, 2, 3):
                assert fn(s, n, ids.ctypes.data + off, 1, pp, 4, 0, None, *outs) == EINVAL, off   # ids misaligned
                assert fn(s, n, ids.ctypes.data + off, 0, pp, 4, 0, None, *outs) == EINVAL, off
                assert fn(s, n, ids.ctypes.data + off, 1 << 32, pp, 4, 0, None, *outs) == EINVAL, off
    assert np.all(count == 7) and np.all(total == 7.0) and np.all(nb == 7) and np.all(bits == 7)   # nothing was written
    assert np.all(keys == 7) and np.all(valid == 7)


def test_keep_and_the_handle_calls_check_their_arguments(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    out = C.c_void_p(0x77)
    fake = C.c_void_p(0x1000)
    assert L.lh_keep(None, 0, 1, 0, C.byref(out)) == EINVAL                      # NULL snapshot
    assert L.lh_keep(fake, 0, 1, 0, None) == EINVAL                               # NULL out
    for flags in (1, 2, 0x80000000):
        assert L.lh_keep(fake, 0, 1, flags, C.byref(out)) == EINVAL               # flags must be 0
    assert L.lh_keep(fake, 0, 0, 0, C.byref(out)) == EINVAL                       # nmetrics == 0
    assert L.lh_keep(fake, 5, 0, 0, C.byref(out)) == EINVAL
    assert out.value == 0x77                                                      # *out untouched
    assert L.lh_kept_release(None) == EINVAL
    info = _native.LhKeptInfo(struct_size=C.sizeof(_native.LhKeptInfo))
    assert L.lh_kept_info_get(None, C.byref(info)) == EINVAL and L.lh_kept_info_get(fake, None) == EINVAL
    assert L.lh_kept_arrays(None, None, None, None, None) == EINVAL
    assert L.lh_kept_hold(None, None) == EINVAL


def test_the_tool_hooks_check_their_arguments(native_lib):
    src = open(os.path.join(ROOT, "include", "loghisto_gpu_tuning.h")).read()
    assert re.search(r"\bint\s+lh_tool_kept_switch\s*\(\s*uint32_t\s+wave_from_rows\s*,\s*uint32_t\s*\*\s*previous\s*\)\s*;", src)
    assert re.search(r"\bint\s+lh_tool_kept_tile\s*\(\s*uint32_t\s*\*\s*bins\s*\)\s*;", src)
    fn = native_lib.lh_tool_kept_switch
    prev = C.c_uint32(0)
    assert fn(0, C.byref(prev)) == 0
    default = C.c_uint32(0)
    assert fn(7, C.byref(default)) == 0 and default.value == 1024               # lh_spread's default
    assert fn(1 << 30, C.byref(prev)) == 0 and prev.value == 7
    assert fn(0, None) == 0                                                      # previous may be NULL; 0 restores the default
    assert fn(0, C.byref(prev)) == 0 and prev.value == default.value
    tile = C.c_uint32(0)
    assert native_lib.lh_tool_kept_tile(None) == 1                               # LH_EINVAL
    assert native_lib.lh_tool_kept_tile(C.byref(tile)) == 0
    assert tile.value % 256 == 0 and 256 <= tile.value and tile.value * 8 <= 65536   # whole steps, at most 64 KiB of LDS


def test_python_wrapper_has_kept():
    import inspect

    import loghisto_amd
    assert "Kept" in loghisto_amd.__all__
    sig = inspect.signature(loghisto_amd.Snapshot.keep)
    assert list(sig.parameters) == ["self", "nmetrics", "first"]
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default == 0
    sig = inspect.signature(loghisto_amd.Kept.across)
    assert list(sig.parameters)[:7] == ["self", "earlier", "percentiles", "nmetrics", "first", "ids", "out"]
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default == 0
    assert sig.parameters["ids"].default is None and sig.parameters["out"].default is None
    for name in ("arrays", "add_to", "close", "__enter__", "__exit__"):
        assert callable(getattr(loghisto_amd.Kept, name)), name
