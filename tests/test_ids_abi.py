"""CPU tests of the id-list forms lh_across_ids*, lh_count_le_ids*, lh_spread_ids* (the base forms' walks over rows ids[0 .. n)
instead of [first, first + nmetrics)): declared, exported, bound, and every LH_EINVAL check and the early LH_ERANGE run on the
host before any snapshot is looked at -- the snapshot pointers below are fakes that are never dereferenced, and the id arrays
hold a few entries whatever n says."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"lh_across_ids": 13, "lh_across_ids_device": 13, "lh_count_le_ids": 8, "lh_count_le_ids_device": 8,
         "lh_spread_ids": 12, "lh_spread_ids_device": 12}
FAKE = 0x1000                                  # never dereferenced: the argument checks come first
BIG = (1 << 32, (1 << 64) - 1)                 # n beyond any uint32 row count


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name, nargs in NARGS.items():
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, decl
        base = name.replace("_ids", "")                                          # (first, nmetrics) became (ids, n): as many
        assert len(_native.SIGNATURES[base][1]) == nargs, base
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7         # adding functions is backward compatible


class Ids:
    """A small id array, and addresses off its 4-byte alignment."""
    def __init__(self):
        self.a = np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
        self.p = self.a.ctypes.data
        self.off = [self.p + k for k in (1, 2, 3)]


def test_across_ids_decides_every_early_error_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p

    def snaps(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two, full = snaps(FAKE), snaps(FAKE, 0x2000), snaps(*[FAKE * (i + 1) for i in range(16)])
    too_many = snaps(*[FAKE * (i + 1) for i in range(17)])
    holes = [snaps(None), snaps(None, 0x2000), snaps(FAKE, None), snaps(*([FAKE] * 15 + [None]))]
    odd = (C.c_char * 64)()
    ids = Ids()
    p = np.array([0.5, 0.99, 1.0, float("nan")])
    count, total = np.full(8, 7, dtype=np.uint64), np.full(8, 7.0)
    nb, bits = np.full(8, 7, dtype=np.uint32), np.full(8, 7, dtype=np.uint32)
    keys, valid = np.full(64, 7, dtype=np.int16), np.full(64, 7, dtype=np.uint8)
    outs = [a.ctypes.data for a in (count, total, nb, bits, keys, valid)]
    pp, ip = p.ctypes.data, ids.p
    for fn in (L.lh_across_ids, L.lh_across_ids_device):
        # ---- every LH_EINVAL of the base form
        assert fn(None, 1, ip, 1, pp, 4, 0, *outs) == EINVAL                      # NULL snaps
        assert fn(None, 0, ip, 0, pp, 4, 0, *outs) == EINVAL
        for h in holes:                                                           # a NULL entry, wherever
            assert fn(h, len(h), ip, 1, pp, 4, 0, *outs) == EINVAL
            assert fn(h, len(h), ip, 0, pp, 4, 0, *outs) == EINVAL
        assert fn(one, 0, ip, 1, pp, 4, 0, *outs) == EINVAL                       # nsnaps 0
        assert fn(too_many, 17, ip, 1, pp, 4, 0, *outs) == EINVAL                 # nsnaps too large
        assert fn(full, (1 << 64) - 1, ip, 1, pp, 4, 0, *outs) == EINVAL
        for off in range(1, C.sizeof(VP)):                                        # the list itself off its alignment
            assert fn(C.addressof(odd) + off, 1, ip, 1, pp, 4, 0, *outs) == EINVAL, off
        for s, n in ((one, 1), (two, 2), (full, 16)):
            assert fn(s, n, ip, 1, pp, 33, 0, *outs) == EINVAL                    # np too large
            assert fn(s, n, ip, 1, pp, (1 << 64) - 1, 0, *outs) == EINVAL
            assert fn(s, n, ip, 1, None, 1, 0, *outs) == EINVAL                   # np > 0 with NULL p
            assert fn(s, n, ip, 1, pp, 4, 0, None, None, None, None, None, None) == EINVAL   # all outputs NULL
            assert fn(s, n, ip, 1, None, 0, 0, None, None, None, None, outs[4], outs[5]) == EINVAL   # np == 0: those two are ignored
            for flags in (1, 2, 0x80000000):                                      # unknown flag bits
                assert fn(s, n, ip, 1, pp, 4, flags, *outs) == EINVAL, flags
            for k, width in enumerate((8, 8, 4, 4, 2)):                           # arrays not aligned to their element size
                for off in range(1, width):
                    bad = list(outs)
                    bad[k] += off
                    assert fn(s, n, ip, 1, pp, 4, 0, *bad) == EINVAL, (k, off)
                    only = [None] * 6
                    only[k] = bad[k]
                    assert fn(s, n, ip, 1, pp, 4, 0, *only) == EINVAL, (k, off)
            for off in (1, 2, 4):
                assert fn(s, n, ip, 1, pp + off, 3, 0, *outs) == EINVAL, off      # p not 8-byte aligned
            # ---- the id list's own
            assert fn(s, n, None, 1, pp, 4, 0, *outs) == EINVAL                   # NULL ids with n > 0
            assert fn(s, n, None, 8, pp, 4, 0, *outs) == EINVAL
            for bad in ids.off:                                                   # ids off 4-byte alignment
                assert fn(s, n, bad, 1, pp, 4, 0, *outs) == EINVAL, bad - ip
                assert fn(s, n, bad, 0, pp, 4, 0, *outs) == EINVAL, bad - ip
            for big in BIG:
                # more entries than a uint32 counts: LH_ERANGE, decided before a snapshot or an id is looked at
                assert fn(s, n, ip, big, pp, 4, 0, *outs) == ERANGE
                assert fn(s, n, ip, big, None, 0, 0, outs[0], None, None, None, None, None) == ERANGE
                assert fn(s, n, ip, big, pp, 32, 0, None, None, None, None, None, outs[5]) == ERANGE
                # a cause of LH_EINVAL wins over it
                assert fn(s, n, ip, big, pp, 33, 0, *outs) == EINVAL
                assert fn(s, n, ip, big, pp, 4, 1, *outs) == EINVAL
                assert fn(s, n, ip, big, pp, 4, 0, outs[0] + 4, *outs[1:]) == EINVAL
                assert fn(s, 0, ip, big, pp, 4, 0, *outs) == EINVAL
                assert fn(s, n, None, big, pp, 4, 0, *outs) == EINVAL
                for bad in ids.off:
                    assert fn(s, n, bad, big, pp, 4, 0, *outs) == EINVAL
        assert fn(holes[2], 2, ip, 1 << 32, pp, 4, 0, *outs) == EINVAL
    assert np.all(count == 7) and np.all(total == 7.0) and np.all(nb == 7) and np.all(bits == 7)   # nothing was written
    assert np.all(keys == 7) and np.all(valid == 7)
    assert np.array_equal(ids.a, np.arange(8, dtype=np.uint32))


def test_count_le_ids_decides_every_early_error_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE, PER = native_lib, _native.EINVAL, _native.ERANGE, _native.LE_PER_METRIC
    fake = C.c_void_p(FAKE)
    ids = Ids()
    b = np.array([-1.0, 0.0, 0.0, 2.5, np.inf], dtype=np.float64)
    per = np.array([[0.0, 1.0], [-5.0, 5.0], [-np.inf, np.inf]], dtype=np.float64)
    cum = np.full(64 * 4, 7, dtype=np.uint64)
    total = np.full(4, 7, dtype=np.uint64)
    bp, cp, tp, ip = b.ctypes.data, cum.ctypes.data, total.ctypes.data, ids.p
    for fn in (L.lh_count_le_ids, L.lh_count_le_ids_device):
        # ---- every LH_EINVAL of the base form
        assert fn(None, ip, 1, bp, b.size, 0, cp, tp) == EINVAL                # NULL snapshot
        assert fn(None, ip, 0, bp, b.size, 0, cp, tp) == EINVAL                # ... whatever n
        assert fn(fake, ip, 1, bp, 0, 0, cp, tp) == EINVAL                     # nb == 0
        assert fn(fake, ip, 1, bp, 65, 0, cp, tp) == EINVAL                    # nb > LH_MAX_BOUNDS
        assert fn(fake, ip, 1, None, b.size, 0, cp, tp) == EINVAL              # NULL bounds
        assert fn(fake, ip, 1, bp, b.size, 0, None, None) == EINVAL            # both outputs NULL
        for bad in ([0.0, np.nan], [np.nan], [1.0, 0.5], [0.0, -1e-300], [np.inf, 1.0], [1.0, 2.0, -np.inf]):
            x = np.array(bad, dtype=np.float64)                                # a NaN bound / a decreasing row
            assert fn(fake, ip, 1, x.ctypes.data, x.size, 0, cp, tp) == EINVAL, bad
            assert fn(fake, ip, 1, x.ctypes.data, x.size, 0, None, tp) == EINVAL, bad
        for flags in (2, 4, 3, 0x80000000):                                    # unknown flag bits
            assert fn(fake, ip, 1, bp, b.size, flags, cp, tp) == EINVAL, flags
        assert fn(fake, ip, 1, bp + 4, 1, 0, cp, tp) == EINVAL                 # arrays not 8-byte aligned
        assert fn(fake, ip, 1, bp, b.size, 0, cp + 4, tp) == EINVAL
        assert fn(fake, ip, 1, bp, b.size, 0, cp, tp + 4) == EINVAL
        assert fn(fake, ip, 1, bp, b.size, 0, cp + 2, None) == EINVAL
        bad = per.copy()                                                       # per-metric rows: each is checked on its own
        bad[2] = [np.inf, 1e308]
        assert fn(fake, ip, 3, bad.ctypes.data, 2, PER, cp, tp) == EINVAL
        bad = per.copy()
        bad[1, 0] = np.nan
        assert fn(fake, ip, 3, bad.ctypes.data, 2, PER, cp, tp) == EINVAL
        assert fn(fake, ip, 1, per.ctypes.data, 6, 0, cp, tp) == EINVAL        # the same six doubles as one shared row decrease
        # ---- the id list's own
        assert fn(fake, None, 1, bp, b.size, 0, cp, tp) == EINVAL              # NULL ids with n > 0
        assert fn(fake, None, 3, per.ctypes.data, 2, PER, cp, tp) == EINVAL
        for bad in ids.off:                                                    # ids off 4-byte alignment
            assert fn(fake, bad, 1, bp, b.size, 0, cp, tp) == EINVAL, bad - ip
            assert fn(fake, bad, 0, bp, b.size, 0, cp, tp) == EINVAL, bad - ip
        for big in BIG:
            # LH_ERANGE before a row of bounds or an id is read (these arrays hold 3 rows and 8 ids, not 2^32)
            assert fn(fake, ip, big, per.ctypes.data, 2, PER, cp, tp) == ERANGE
            assert fn(fake, ip, big, bp, b.size, 0, cp, tp) == ERANGE
            assert fn(fake, ip, big, bp, b.size, 0, None, tp) == ERANGE
            # a cause of LH_EINVAL wins over it
            assert fn(fake, ip, big, bp, 0, 0, cp, tp) == EINVAL
            assert fn(fake, ip, big, bp, b.size, 2, cp, tp) == EINVAL
            assert fn(fake, ip, big, bp, b.size, 0, cp + 4, tp) == EINVAL
            assert fn(None, ip, big, bp, b.size, 0, cp, tp) == EINVAL
            assert fn(fake, None, big, bp, b.size, 0, cp, tp) == EINVAL
            for bad in ids.off:
                assert fn(fake, bad, big, per.ctypes.data, 2, PER, cp, tp) == EINVAL
    assert np.all(cum == 7) and np.all(total == 7)                              # nothing was written


def test_spread_ids_decides_every_early_error_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    fake = C.c_void_p(FAKE)
    ids = Ids()
    p = np.array([0.5, 0.9, 0.99, 1.5, np.nan], dtype=np.float64)
    many = np.linspace(0.0, 1.0, 33)
    n = 4
    count, sums, m2 = np.full(n, 7, dtype=np.uint64), np.full(n, 7.0), np.full(n, 7.0)
    keys, valid = np.full(n * 32 + 1, 7, dtype=np.int16), np.full(n * 32, 7, dtype=np.uint8)
    cle, sle = np.full(n * 32, 7, dtype=np.uint64), np.full(n * 32, 7.0)
    outs = [a.ctypes.data for a in (count, sums, m2, keys, valid, cle, sle)]
    pp, ip = p.ctypes.data, ids.p
    for fn in (L.lh_spread_ids, L.lh_spread_ids_device):
        # ---- every LH_EINVAL of the base form
        assert fn(None, ip, 1, pp, p.size, *outs) == EINVAL                     # NULL snapshot
        assert fn(None, ip, 0, pp, p.size, *outs) == EINVAL                     # ... whatever n
        assert fn(None, ip, 1, None, 0, *outs) == EINVAL
        assert fn(fake, ip, 1, many.ctypes.data, 33, *outs) == EINVAL           # np > LH_MAX_PERCENTILES
        assert fn(fake, ip, 1, None, 1, *outs) == EINVAL                        # np > 0 with NULL p
        assert fn(fake, ip, 1, pp, p.size, *([None] * 7)) == EINVAL             # all outputs NULL
        assert fn(fake, ip, 1, None, 0, *([None] * 7)) == EINVAL
        assert fn(fake, ip, 1, None, 0, None, None, None, *outs[3:]) == EINVAL  # np == 0: the per-percentile outputs do not count
        assert fn(fake, ip, 1, pp, 0, None, None, None, *outs[3:]) == EINVAL
        assert fn(fake, ip, 1, pp + 4, 1, *outs) == EINVAL                      # arrays not aligned to their element size
        for k, width in ((0, 8), (1, 8), (2, 8), (3, 2), (5, 8), (6, 8)):
            for off in {1, width // 2}:
                bad = list(outs)
                bad[k] += off
                assert fn(fake, ip, 1, pp, p.size, *bad) == EINVAL, (k, off)
                alone = [None] * 7
                alone[k] = bad[k]
                assert fn(fake, ip, 1, pp, p.size, *alone) == EINVAL, (k, off)
        # ---- the id list's own
        assert fn(fake, None, 1, pp, p.size, *outs) == EINVAL                   # NULL ids with n > 0
        assert fn(fake, None, 4, None, 0, *outs) == EINVAL
        for bad in ids.off:                                                     # ids off 4-byte alignment
            assert fn(fake, bad, 1, pp, p.size, *outs) == EINVAL, bad - ip
            assert fn(fake, bad, 0, pp, p.size, *outs) == EINVAL, bad - ip
        for big in BIG:
            assert fn(fake, ip, big, pp, p.size, *outs) == ERANGE               # before the snapshot or an id is looked at
            assert fn(fake, ip, big, None, 0, *outs) == ERANGE
            # a cause of LH_EINVAL wins over it
            assert fn(fake, ip, big, many.ctypes.data, 33, *outs) == EINVAL
            assert fn(fake, ip, big, pp, p.size, *([None] * 7)) == EINVAL
            assert fn(fake, ip, big, pp, p.size, outs[0] + 4, *outs[1:]) == EINVAL
            assert fn(None, ip, big, pp, p.size, *outs) == EINVAL
            assert fn(fake, None, big, pp, p.size, *outs) == EINVAL
            for bad in ids.off:
                assert fn(fake, bad, big, pp, p.size, *outs) == EINVAL
    for a in (count, sums, m2, keys, valid, cle, sle):
        assert np.all(a == 7)                                                   # nothing was written


def test_python_wrapper_has_the_three_methods():
    import loghisto_amd
    S = loghisto_amd.Snapshot
    want = {"across_ids": ["self", "ids", "earlier", "percentiles", "out"], "count_le_ids": ["self", "ids", "bounds", "out"],
            "spread_ids": ["self", "ids", "percentiles", "out"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(S, name))
        assert list(sig.parameters) == params, name
        assert sig.parameters["out"].default is None
        assert all(sig.parameters[k].default is inspect.Parameter.empty for k in params[1:-1]), name
    # the base methods keep theirs
    assert list(inspect.signature(S.across).parameters) == ["self", "earlier", "percentiles", "nmetrics", "first", "out"]
    assert list(inspect.signature(S.count_le).parameters) == ["self", "bounds", "nmetrics", "first", "out"]
    assert list(inspect.signature(S.spread).parameters) == ["self", "percentiles", "nmetrics", "first", "out"]
