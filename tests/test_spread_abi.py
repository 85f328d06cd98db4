"""CPU tests of lh_spread / lh_spread_device (std and percentile-trimmed sums per name: the weighted walk of
metrics.go:342-346 cut where percentile(), metrics.go:406-418, cuts): declared, exported, bound, and every LH_EINVAL check
runs on the host before the snapshot is looked at -- the snapshot pointer below is a fake that is never dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_spread", "lh_spread_device"]


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == 12
    tuning = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu_tuning.h")).read(), flags=re.S)
    assert re.search(r"\blh_tool_spread_switch\s*\(", tuning) and hasattr(raw, "lh_tool_spread_switch")
    assert "lh_tool_spread_switch" in _native.TUNING_SIGNATURES
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible


def test_the_switch_hook_reports_the_previous_value(native_lib):
    prev = C.c_uint32(0)
    assert native_lib.lh_tool_spread_switch(0, C.byref(prev)) == 0
    default = prev.value
    assert default >= 1
    try:
        assert native_lib.lh_tool_spread_switch(77, C.byref(prev)) == 0 and prev.value == default
        assert native_lib.lh_tool_spread_switch(1 << 30, None) == 0
        assert native_lib.lh_tool_spread_switch(0, C.byref(prev)) == 0 and prev.value == 1 << 30     # 0: the default
    finally:
        assert native_lib.lh_tool_spread_switch(0, C.byref(prev)) == 0 and prev.value == default


def test_every_einval_case_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    fake = C.c_void_p(0x1000)              # never dereferenced: the argument checks come first
    p = np.array([0.5, 0.9, 0.99, 1.5, np.nan], dtype=np.float64)
    many = np.linspace(0.0, 1.0, 33)
    n = 4
    count, sums, m2 = np.zeros(n, dtype=np.uint64), np.zeros(n), np.zeros(n)
    keys, valid = np.zeros(n * 32 + 1, dtype=np.int16), np.zeros(n * 32, dtype=np.uint8)
    cle, sle = np.zeros(n * 32, dtype=np.uint64), np.zeros(n * 32)
    outs = [a.ctypes.data for a in (count, sums, m2, keys, valid, cle, sle)]
    pp = p.ctypes.data
    for fn in (L.lh_spread, L.lh_spread_device):
        assert fn(None, 0, 1, pp, p.size, *outs) == EINVAL                      # NULL snapshot
        assert fn(None, 0, 0, pp, p.size, *outs) == EINVAL                      # ... whatever nmetrics
        assert fn(None, 0, 1, None, 0, *outs) == EINVAL
        assert fn(fake, 0, 1, many.ctypes.data, 33, *outs) == EINVAL            # np > LH_MAX_PERCENTILES
        assert fn(fake, 0, 1, None, 1, *outs) == EINVAL                         # np > 0 with NULL p
        assert fn(fake, 0, 1, pp, p.size, *([None] * 7)) == EINVAL              # all outputs NULL
        assert fn(fake, 0, 1, None, 0, *([None] * 7)) == EINVAL
        # np == 0: the per-percentile outputs are ignored, so they do not count as outputs
        assert fn(fake, 0, 1, None, 0, None, None, None, *outs[3:]) == EINVAL
        assert fn(fake, 0, 1, pp, 0, None, None, None, *outs[3:]) == EINVAL
        assert fn(fake, 0, 1, pp + 4, 1, *outs) == EINVAL                       # arrays not aligned to their element size
        for k, width in ((0, 8), (1, 8), (2, 8), (3, 2), (5, 8), (6, 8)):
            for off in {1, width // 2}:
                bad = list(outs)
                bad[k] += off
                assert fn(fake, 0, 1, pp, p.size, *bad) == EINVAL, (k, off)
                alone = [None] * 7
                alone[k] = bad[k]
                assert fn(fake, 0, 1, pp, p.size, *alone) == EINVAL, (k, off)
        # more rows than any engine can have: LH_ERANGE, decided before the snapshot is looked at
        assert fn(fake, 0, 1 << 32, pp, p.size, *outs) == _native.ERANGE
        assert fn(fake, 1, (1 << 64) - 1, None, 0, *outs) == _native.ERANGE
    for a in (count, sums, m2, keys, valid, cle, sle):
        assert not a.any()                                                      # nothing was written


def test_python_wrapper_has_spread():
    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "spread"))
