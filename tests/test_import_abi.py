"""CPU tests of the cell-import entry points (lh_snapshot_add_buckets*, the inverse of lh_buckets_all;
RawMetricSet.Histograms, metrics.go:54-60): declared, exported, bound, and their argument checks need no GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lh_snapshot_add_buckets", "lh_snapshot_add_buckets_csr", "lh_snapshot_add_buckets_csr_device",
         "lh_snapshot_add_buckets_device"]


def test_the_four_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible


def test_null_arguments_are_einval_without_a_device(native_lib):
    from loghisto_amd import _native
    ids = np.zeros(4, dtype=np.uint32)
    keys = np.zeros(4, dtype=np.int16)
    counts = np.ones(4, dtype=np.uint64)
    offsets = np.array([0, 4], dtype=np.uint64)
    fake = C.c_void_p(0x1000)      # never dereferenced: the array checks come first
    L = native_lib
    for fn in (L.lh_snapshot_add_buckets, L.lh_snapshot_add_buckets_device):
        assert fn(None, ids.ctypes.data, keys.ctypes.data, counts.ctypes.data, 4) == _native.EINVAL
        assert fn(None, None, None, None, 0) == _native.EINVAL                 # a NULL snapshot, whatever n
        assert fn(fake, None, keys.ctypes.data, counts.ctypes.data, 4) == _native.EINVAL
        assert fn(fake, ids.ctypes.data, None, counts.ctypes.data, 4) == _native.EINVAL
        assert fn(fake, ids.ctypes.data, keys.ctypes.data, None, 4) == _native.EINVAL
        # misaligned: counts 8, ids 4, keys 2 bytes
        assert fn(fake, ids.ctypes.data, keys.ctypes.data, counts.ctypes.data + 4, 1) == _native.EINVAL
        assert fn(fake, ids.ctypes.data + 2, keys.ctypes.data, counts.ctypes.data, 1) == _native.EINVAL
        assert fn(fake, ids.ctypes.data, keys.ctypes.data + 1, counts.ctypes.data, 1) == _native.EINVAL
    for fn in (L.lh_snapshot_add_buckets_csr, L.lh_snapshot_add_buckets_csr_device):
        assert fn(None, 0, 1, offsets.ctypes.data, keys.ctypes.data, counts.ctypes.data) == _native.EINVAL
        assert fn(None, 0, 0, None, None, None) == _native.EINVAL
        assert fn(fake, 0, 1, None, keys.ctypes.data, counts.ctypes.data) == _native.EINVAL
        assert fn(fake, 0, 1, offsets.ctypes.data + 4, keys.ctypes.data, counts.ctypes.data) == _native.EINVAL
        assert fn(fake, 0, 1, offsets.ctypes.data, keys.ctypes.data + 1, counts.ctypes.data) == _native.EINVAL
        assert fn(fake, 0, 1, offsets.ctypes.data, keys.ctypes.data, counts.ctypes.data + 4) == _native.EINVAL


def test_python_wrapper_has_the_three_methods():
    import loghisto_amd
    for m in ("add_buckets", "add_buckets_csr", "add_raw"):
        assert callable(getattr(loghisto_amd.Snapshot, m))
