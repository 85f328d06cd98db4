"""CPU tests of lh_across / lh_across_device (stats and percentiles of a name over several snapshots at once): declared,
exported, bound, and every LH_EINVAL check and the early LH_ERANGE run on the host before any snapshot is looked at -- the
snapshot pointers below are fakes that are never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_across", "lh_across_device"]


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == 13
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == 13, decl
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible
    assert re.search(r"#define\s+LH_MAX_ACROSS\s+16\b", src) and _native.MAX_ACROSS == 16
    assert re.search(r"#define\s+LH_MAX_PERCENTILES\s+32\b", src) and _native.MAX_PERCENTILES == 32


def test_every_early_error_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p

    def snaps(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two, full = snaps(0x1000), snaps(0x1000, 0x2000), snaps(*[0x1000 * (i + 1) for i in range(16)])
    too_many = snaps(*[0x1000 * (i + 1) for i in range(17)])
    holes = [snaps(None), snaps(None, 0x2000), snaps(0x1000, None), snaps(*([0x1000] * 15 + [None]))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    p = np.array([0.5, 0.99, 1.0, float("nan")])
    count, total = np.full(8, 7, dtype=np.uint64), np.full(8, 7.0)
    nb, bits = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    keys, valid = np.full(64, 7, dtype=np.int16), np.full(64, 7, dtype=np.uint8)
    outs = [a.ctypes.data for a in (count, total, nb, bits, keys, valid)]
    pp = p.ctypes.data
    for fn in (L.lh_across, L.lh_across_device):
        assert fn(None, 1, 0, 1, pp, 4, 0, *outs) == EINVAL                       # NULL snaps
        assert fn(None, 0, 0, 0, pp, 4, 0, *outs) == EINVAL                       # ... whatever the rest
        for h in holes:                                                           # a NULL entry, wherever
            assert fn(h, len(h), 0, 1, pp, 4, 0, *outs) == EINVAL
            assert fn(h, len(h), 0, 0, pp, 4, 0, *outs) == EINVAL
        assert fn(one, 0, 0, 1, pp, 4, 0, *outs) == EINVAL                        # nsnaps 0
        assert fn(too_many, 17, 0, 1, pp, 4, 0, *outs) == EINVAL                  # nsnaps too large
        assert fn(full, (1 << 64) - 1, 0, 1, pp, 4, 0, *outs) == EINVAL
        for off in range(1, C.sizeof(VP)):                                        # the list itself off its alignment
            assert fn(C.addressof(odd) + off, 1, 0, 1, pp, 4, 0, *outs) == EINVAL, off
        for s, n in ((one, 1), (two, 2), (full, 16)):
            assert fn(s, n, 0, 1, pp, 33, 0, *outs) == EINVAL                     # np too large
            assert fn(s, n, 0, 1, pp, (1 << 64) - 1, 0, *outs) == EINVAL
            assert fn(s, n, 0, 1, None, 1, 0, *outs) == EINVAL                    # np > 0 with NULL p
            assert fn(s, n, 0, 1, pp, 4, 0, None, None, None, None, None, None) == EINVAL   # all outputs NULL
            assert fn(s, n, 0, 1, None, 0, 0, None, None, None, None, outs[4], outs[5]) == EINVAL   # np == 0: those two are ignored
            for flags in (1, 2, 0x80000000):                                      # unknown flag bits
                assert fn(s, n, 0, 1, pp, 4, flags, *outs) == EINVAL, flags
            for k, width in enumerate((8, 8, 4, 4, 2)):                           # arrays not aligned to their element size
                for off in range(1, width):
                    bad = list(outs)
                    bad[k] += off
                    assert fn(s, n, 0, 1, pp, 4, 0, *bad) == EINVAL, (k, off)
                    only = [None] * 6
                    only[k] = bad[k]
                    assert fn(s, n, 0, 1, pp, 4, 0, *only) == EINVAL, (k, off)
            for off in (1, 2, 4):
                assert fn(s, n, 0, 1, pp + off, 3, 0, *outs) == EINVAL, off       # p not 8-byte aligned
            # a cause of LH_EINVAL wins over the early LH_ERANGE
            assert fn(s, n, 0, 1 << 32, pp, 33, 0, *outs) == EINVAL
            assert fn(s, n, 0, 1 << 32, pp, 4, 1, *outs) == EINVAL
            assert fn(s, n, 0, 1 << 32, pp, 4, 0, outs[0] + 4, *outs[1:]) == EINVAL
            assert fn(s, 0, 0, 1 << 32, pp, 4, 0, *outs) == EINVAL
            # more rows than any engine can have: LH_ERANGE, decided before a snapshot is looked at
            assert fn(s, n, 0, 1 << 32, pp, 4, 0, *outs) == ERANGE
            assert fn(s, n, 1, (1 << 64) - 1, pp, 4, 0, *outs) == ERANGE
            assert fn(s, n, 0, 1 << 32, None, 0, 0, outs[0], None, None, None, None, None) == ERANGE
            assert fn(s, n, 0, 1 << 32, pp, 32, 0, None, None, None, None, None, outs[5]) == ERANGE
        assert fn(holes[2], 2, 0, 1 << 32, pp, 4, 0, *outs) == EINVAL
    assert np.all(count == 7) and np.all(total == 7.0) and np.all(nb == 7) and np.all(bits == 7)   # nothing was written
    assert np.all(keys == 7) and np.all(valid == 7)


def test_the_switch_hook_checks_its_arguments(native_lib):
    from loghisto_amd import _native
    assert "lh_tool_across_switch" in _native.TUNING_SIGNATURES
    assert len(_native.TUNING_SIGNATURES["lh_tool_across_switch"][1]) == 2
    src = open(os.path.join(ROOT, "include", "loghisto_gpu_tuning.h")).read()
    assert re.search(r"\bint\s+lh_tool_across_switch\s*\(\s*uint32_t\s+wave_from_rows\s*,\s*uint32_t\s*\*\s*previous\s*\)\s*;", src)
    fn = native_lib.lh_tool_across_switch
    prev = C.c_uint32(0)
    assert fn(0, C.byref(prev)) == 0
    default = C.c_uint32(0)
    assert fn(7, C.byref(default)) == 0 and default.value == 1024               # lh_spread's default
    sp = C.c_uint32(0)
    assert native_lib.lh_tool_spread_switch(0, C.byref(sp)) == 0 and sp.value == default.value
    assert fn(1 << 30, C.byref(prev)) == 0 and prev.value == 7
    assert fn(0, None) == 0                                                      # previous may be NULL; 0 restores the default
    assert fn(0, C.byref(prev)) == 0 and prev.value == default.value


def test_python_wrapper_has_across():
    import inspect

    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "across"))
    sig = inspect.signature(loghisto_amd.Snapshot.across)
    assert list(sig.parameters) == ["self", "earlier", "percentiles", "nmetrics", "first", "out"]
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default == 0
    assert sig.parameters["out"].default is None
