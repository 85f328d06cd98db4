"""CPU tests of lh_count_le / lh_count_le_device (counts at or below given values, per name: the running count of
percentile()'s bucket walk, metrics.go:389-418, read at a value): declared, exported, bound, and every LH_EINVAL check runs
on the host before the snapshot is looked at -- the snapshot pointer below is a fake that is never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_count_le", "lh_count_le_device"]


def test_the_two_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read()
    assert re.search(r"#define\s+LH_MAX_BOUNDS\s+64\b", src) and re.search(r"LH_LE_PER_METRIC\s*=\s*1\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
    assert _native.MAX_BOUNDS == 64 and _native.LE_PER_METRIC == 1
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible


def test_every_einval_case_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    fake = C.c_void_p(0x1000)              # never dereferenced: the argument checks come first
    b = np.array([-1.0, 0.0, 0.0, 2.5, np.inf], dtype=np.float64)
    per = np.array([[0.0, 1.0], [-5.0, 5.0], [-np.inf, np.inf]], dtype=np.float64)
    cum = np.zeros(64 * 4, dtype=np.uint64)
    total = np.zeros(4, dtype=np.uint64)
    bp, cp, tp = b.ctypes.data, cum.ctypes.data, total.ctypes.data
    for fn in (L.lh_count_le, L.lh_count_le_device):
        assert fn(None, 0, 1, bp, b.size, 0, cp, tp) == EINVAL                 # NULL snapshot
        assert fn(None, 0, 0, bp, b.size, 0, cp, tp) == EINVAL                 # ... whatever nmetrics
        assert fn(fake, 0, 1, bp, 0, 0, cp, tp) == EINVAL                      # nb == 0
        assert fn(fake, 0, 1, bp, 65, 0, cp, tp) == EINVAL                     # nb > LH_MAX_BOUNDS
        assert fn(fake, 0, 1, None, b.size, 0, cp, tp) == EINVAL               # NULL bounds
        assert fn(fake, 0, 1, bp, b.size, 0, None, None) == EINVAL             # both outputs NULL
        for bad in ([0.0, np.nan], [np.nan], [1.0, 0.5], [0.0, -1e-300], [np.inf, 1.0], [1.0, 2.0, -np.inf]):
            x = np.array(bad, dtype=np.float64)                                # a NaN bound / a decreasing row
            assert fn(fake, 0, 1, x.ctypes.data, x.size, 0, cp, tp) == EINVAL, bad
            assert fn(fake, 0, 1, x.ctypes.data, x.size, 0, None, tp) == EINVAL, bad
        for flags in (2, 4, 3, 0x80000000):                                    # unknown flag bits
            assert fn(fake, 0, 1, bp, b.size, flags, cp, tp) == EINVAL, flags
        assert fn(fake, 0, 1, bp + 4, 1, 0, cp, tp) == EINVAL                  # arrays not 8-byte aligned
        assert fn(fake, 0, 1, bp, b.size, 0, cp + 4, tp) == EINVAL
        assert fn(fake, 0, 1, bp, b.size, 0, cp, tp + 4) == EINVAL
        assert fn(fake, 0, 1, bp, b.size, 0, cp + 2, None) == EINVAL
        # per-metric rows: each is checked on its own (row 1 may start below row 0's end) ...
        bad = per.copy()
        bad[2] = [np.inf, 1e308]                                                # ... and the LAST row decreases
        assert fn(fake, 0, 3, bad.ctypes.data, 2, _native.LE_PER_METRIC, cp, tp) == EINVAL
        bad = per.copy()
        bad[1, 0] = np.nan
        assert fn(fake, 0, 3, bad.ctypes.data, 2, _native.LE_PER_METRIC, cp, tp) == EINVAL
        # the same six doubles as ONE shared row decrease (1.0 -> -5.0)
        assert fn(fake, 0, 1, per.ctypes.data, 6, 0, cp, tp) == EINVAL
        # more rows than any engine can have: LH_ERANGE before a row of bounds is read (these arrays hold 3 rows, not 2^32)
        assert fn(fake, 0, 1 << 32, per.ctypes.data, 2, _native.LE_PER_METRIC, cp, tp) == _native.ERANGE
        assert fn(fake, 1, (1 << 64) - 1, bp, b.size, 0, cp, tp) == _native.ERANGE
    assert not cum.any() and not total.any()                                    # nothing was written


def test_python_wrapper_has_count_le():
    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "count_le"))
