"""CPU tests of lh_compare / lh_compare_device (per-name distribution shift between two snapshots: percentile()'s bucket
walk, metrics.go:389-418, over two rows at once): declared, exported, bound, and every LH_EINVAL check and both early
LH_ERANGE checks run on the host before either snapshot is looked at -- the snapshot pointers below are fakes that are never
dereferenced."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_compare", "lh_compare_device"]


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
    tuning = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu_tuning.h")).read(), flags=re.S)
    assert re.search(r"\blh_tool_compare_switch\s*\(", tuning) and hasattr(raw, "lh_tool_compare_switch")
    assert "lh_tool_compare_switch" in _native.TUNING_SIGNATURES
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible


def test_the_switch_hook_reports_the_previous_value(native_lib):
    prev = C.c_uint32(0)
    assert native_lib.lh_tool_compare_switch(0, C.byref(prev)) == 0
    default = prev.value
    assert default >= 1
    try:
        assert native_lib.lh_tool_compare_switch(77, C.byref(prev)) == 0 and prev.value == default
        assert native_lib.lh_tool_compare_switch(1 << 30, None) == 0
        assert native_lib.lh_tool_compare_switch(0, C.byref(prev)) == 0 and prev.value == 1 << 30    # 0: the default
    finally:
        assert native_lib.lh_tool_compare_switch(0, C.byref(prev)) == 0 and prev.value == default


def test_every_einval_case_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)      # never dereferenced: the argument checks come first
    n = 4
    widths = (8, 8, 8, 2, 8, 8, 8, 8)                         # count_a, count_b, ks, ks_key, ks_below_a, ks_below_b, w1, shift
    arrays = [np.zeros(n * w + 8, dtype=np.uint8) for w in widths]
    outs = [a.ctypes.data for a in arrays]
    assert all(p % 8 == 0 for p in outs)
    for fn in (L.lh_compare, L.lh_compare_device):
        assert fn(None, fake, 0, 1, 0, *outs) == EINVAL                         # NULL base
        assert fn(fake, None, 0, 1, 0, *outs) == EINVAL                         # NULL cur
        assert fn(None, None, 0, 0, 0, *outs) == EINVAL                         # ... whatever nmetrics
        assert fn(None, fake, 0, 1 << 32, 0, *outs) == EINVAL                   # ... and before the range
        for a, b in ((fake, other), (fake, fake)):
            assert fn(a, b, 0, 1, 0, *([None] * 8)) == EINVAL                   # all outputs NULL
            assert fn(a, b, 0, 0, 0, *([None] * 8)) == EINVAL
            for flags in (1, 2, 1 << 31, 0xffffffff):                           # unknown flag bits
                assert fn(a, b, 0, 1, flags, *outs) == EINVAL, flags
            for k, width in enumerate(widths):                                  # arrays not aligned to their element size
                for off in {1, width // 2}:
                    bad = list(outs)
                    bad[k] += off
                    assert fn(a, b, 0, 1, 0, *bad) == EINVAL, (k, off)
                    alone = [None] * 8
                    alone[k] = bad[k]
                    assert fn(a, b, 0, 1, 0, *alone) == EINVAL, (k, off)
            # more rows than any engine can have: LH_ERANGE, decided before either snapshot is looked at
            assert fn(a, b, 0, 1 << 32, 0, *outs) == _native.ERANGE
            assert fn(a, b, 1, (1 << 64) - 1, 0, *outs) == _native.ERANGE
            assert fn(a, b, 0, 1 << 32, 0, None, None, None, outs[3], None, None, None, None) == _native.ERANGE
    for a in arrays:
        assert not a.any()                                                      # nothing was written


def test_python_wrapper_has_compare():
    import loghisto_amd
    assert callable(getattr(loghisto_amd.Snapshot, "compare"))
