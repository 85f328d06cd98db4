"""CPU tests of lh_kept_save* / lh_kept_load* / lh_kept_values: declared, exported, bound; every LH_EINVAL / LH_ERANGE that is
decided on the host, with handle pointers that are fakes and never dereferenced and with blobs whose header is wrong in exactly
one field (the cause lands in `why`, *out stays untouched); and loghisto_amd.keptfile, the NumPy restatement of the blob:
pack -> unpack round trips, check() takes what pack() makes and names the expected (cause, row, index) for each single
mutation.  The device's verdict is held to keptfile.check by tests/test_gpu_kept_store.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from loghisto_amd import keptfile as KF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"lh_kept_save_size": 2, "lh_kept_save": 5, "lh_kept_save_device": 5, "lh_kept_load": 7, "lh_kept_load_device": 7,
        "lh_kept_values": 2}
U64 = np.uint64


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)
    return src, set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    raw = C.CDLL(_native.LIB_PATH)
    src, declared = _declared()
    for name, nargs in ARGS.items():
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, decl
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7          # adding functions is backward compatible
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert C.sizeof(_native.LhKeptCheck) == 16
    fields = re.search(r"typedef\s+struct\s+lh_kept_check\s*\{(.*?)\}\s*lh_kept_check\s*;", src, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == [k for k, _ in _native.LhKeptCheck._fields_]
    # the causes and the format's constants: the header and keptfile agree
    enum = dict((k, int(v)) for k, v in re.findall(r"\bLH_KEPT_(BAD_[A-Z_]+)\s*=\s*(\d+)", src))
    assert enum == {k: v for v, k in KF.CAUSES.items()} and len(enum) == 20
    assert re.search(r'#define\s+LH_KEPT_BLOB_MAGIC\s+"LHKEPT\\x1a\\n"', src) and KF.MAGIC == b"LHKEPT\x1a\n"
    assert re.search(r"#define\s+LH_KEPT_BLOB_VERSION\s+1\b", src) and KF.VERSION == 1
    assert re.search(r"#define\s+LH_KEPT_BLOB_HEADER\s+64\b", src) and KF.HEADER == 64
    assert KF.NKEYS == _native.NKEYS and KF.BLOB_MIN == 88


def test_python_wrapper_has_the_store():
    import inspect

    import loghisto_amd
    K = loghisto_amd.Kept
    for name in ("to_bytes", "save", "to_device_blob", "from_bytes", "load", "from_device_blob", "values"):
        assert callable(getattr(K, name)), name
    assert list(inspect.signature(K.from_bytes).parameters)[:2] == ["blob", "device"]
    assert inspect.signature(K.from_bytes).parameters["device"].default == 0
    assert list(inspect.signature(K.load).parameters)[:2] == ["path", "device"]
    assert inspect.signature(K.load).parameters["device"].default == 0
    assert list(inspect.signature(K.from_device_blob).parameters)[:1] == ["t"]


# ---- the entries' own checks: nothing below reaches a device ------------------------------------------------------------------
def crafted():
    """three rows: {bin 0: 3, bin 65535: 4} | empty | {bins 100, 101, 102}; first = 5"""
    keys = np.array([0x8000, 0x7fff, 100 ^ 0x8000, 101 ^ 0x8000, 102 ^ 0x8000], dtype=np.uint16).view(np.int16)
    return KF.pack([0, 2, 2, 5], keys, [3, 4, 1, 1, 1], first=5)


def _load_forms(L):
    return (L.lh_kept_load, L.lh_kept_load_device)


def _why(_native, size=16):
    return _native.LhKeptCheck(struct_size=size, cause=0x77, row=0x77, index=0x77)


def test_save_and_values_check_their_arguments_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    fake = C.c_void_p(0x1000)
    n = C.c_size_t(0x77)
    buf = np.full(256, 7, dtype=np.uint8)
    assert L.lh_kept_save_size(None, C.byref(n)) == EINVAL and L.lh_kept_save_size(fake, None) == EINVAL
    for fn in (L.lh_kept_save, L.lh_kept_save_device):
        assert fn(None, buf.ctypes.data, 256, None, C.byref(n)) == EINVAL         # NULL handle
        assert fn(fake, None, 256, None, C.byref(n)) == EINVAL                    # NULL buffer
        assert fn(None, None, 0, None, None) == EINVAL
        for cap in (0, 1, 63, 64, KF.BLOB_MIN - 1):                               # below the smallest blob there is: LH_ERANGE
            assert fn(fake, buf.ctypes.data, cap, None, C.byref(n)) == ERANGE, cap    # ... before the handle is looked at
        assert fn(None, buf.ctypes.data, 0, None, C.byref(n)) == EINVAL           # a cause of LH_EINVAL wins
    assert n.value == 0x77 and np.all(buf == 7)                                   # nothing was written
    D = np.full(_native.NKEYS + 1, 7.0)
    dp = C.POINTER(C.c_double)
    assert L.lh_kept_values(0, None) == EINVAL
    for off in (1, 2, 4):
        assert L.lh_kept_values(0, C.cast(D.ctypes.data + off, dp)) == EINVAL     # misaligned
    for device in (-1, -2**31, 64, 2**31 - 1):
        assert L.lh_kept_values(device, C.cast(D.ctypes.data, dp)) == EINVAL
    assert np.all(D == 7.0)


def test_load_decides_the_header_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    good = np.frombuffer(crafted(), dtype=np.uint8).copy()
    out = C.c_void_p(0x77)

    def refused(fn, device, addr, length, flags, cause, why="own"):
        w = _why(_native) if why == "own" else why
        assert fn(device, addr, length, flags, None, C.byref(w) if w is not None else None, C.byref(out)) == EINVAL
        assert out.value == 0x77                                                  # *out untouched
        if w is not None:
            assert (w.struct_size, w.cause, w.row, w.index) == (16, cause, 0, 0), (KF.CAUSES.get(w.cause), KF.CAUSES[cause])

    # ---- the causes that need no header: both forms, before any device call (the device pointer is a fake)
    for fn in _load_forms(L):
        addr = good.ctypes.data if fn is L.lh_kept_load else 0x1000
        refused(fn, 0, None, good.size, 0, KF.BAD_ARG)                            # NULL blob
        w = _why(_native)
        assert fn(0, addr, good.size, 0, None, C.byref(w), None) == EINVAL and w.cause == KF.BAD_ARG   # NULL out
        for flags in (1, 2, 0x80000000):
            refused(fn, 0, addr, good.size, flags, KF.BAD_ARG)                    # flags must be 0
        for device in (-1, 64, 2**31 - 1):
            refused(fn, device, addr, good.size, 0, KF.BAD_ARG)
        for length in (0, 1, 63):
            refused(fn, 0, addr, length, 0, KF.BAD_SHORT)
        refused(fn, 0, None, 0, 1, KF.BAD_ARG)                                    # the documented order: arguments first
        refused(fn, 0, addr, good.size, 1, KF.BAD_ARG, why=None)                  # why is optional
        for size in (0, 12, 15, 17, 32):                                          # a why of another size: nothing written
            w = _why(_native, size)
            assert fn(0, addr, good.size, 0, None, C.byref(w), C.byref(out)) == EINVAL
            assert (w.struct_size, w.cause, w.row, w.index) == (size, 0x77, 0x77, 0x77) and out.value == 0x77

    # ---- the header's fields, one wrong at a time (host form: the header is read where it lies)
    def with_field(at, fmt, value, length=None):
        b = good.copy()
        b[at:at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        return b, (good.size if length is None else length)

    nrows, cells = 3, 5
    cases = [(with_field(0, "<8s", b"LHKEPT\x1a\r"), KF.BAD_MAGIC), (with_field(0, "<8s", b"lHKEPT\x1a\n"), KF.BAD_MAGIC),
             (with_field(0, "<8s", bytes(8)), KF.BAD_MAGIC),
             (with_field(8, "<I", 0), KF.BAD_VERSION), (with_field(8, "<I", 2), KF.BAD_VERSION),
             (with_field(12, "<I", 63), KF.BAD_HEADER_SIZE), (with_field(12, "<I", 128), KF.BAD_HEADER_SIZE),
             (with_field(16, "<I", 65535), KF.BAD_NKEYS), (with_field(16, "<I", 0), KF.BAD_NKEYS),
             (with_field(24, "<I", 0), KF.BAD_NROWS),
             (with_field(20, "<I", 2**32 - 2), KF.BAD_FIRST), (with_field(20, "<I", 2**32 - 1), KF.BAD_FIRST),
             (with_field(32, "<Q", nrows * 65536 + 1), KF.BAD_CELLS), (with_field(32, "<Q", 2**64 - 1), KF.BAD_CELLS),
             (with_field(32, "<Q", cells + 1), KF.BAD_BYTES), (with_field(32, "<Q", 0), KF.BAD_BYTES),
             (with_field(24, "<I", nrows + 1), KF.BAD_BYTES),
             (with_field(48, "<Q", good.size - 64 + 1), KF.BAD_BYTES), (with_field(48, "<Q", 0), KF.BAD_BYTES),
             ((good, good.size - 1), KF.BAD_LENGTH), ((good, good.size - 2), KF.BAD_LENGTH), ((good, 64), KF.BAD_LENGTH),
             ((np.concatenate([good, good[:8]]), good.size + 8), KF.BAD_LENGTH),
             (with_field(28, "<I", 1), KF.BAD_RESERVED), (with_field(28, "<I", 0x80000000), KF.BAD_RESERVED)]
    cases += [(with_field(at, "<B", 1), KF.BAD_RESERVED) for at in range(56, 64)]
    for (b, length), cause in cases:
        refused(L.lh_kept_load, 0, b.ctypes.data, length, 0, cause)
        refused(L.lh_kept_load, 63, b.ctypes.data, length, 0, cause)              # whatever the device: it is not opened
        refused(L.lh_kept_load, 0, b.ctypes.data, length, 0, cause, why=None)
        assert KF.check(b[:length].tobytes()) == (cause, 0, 0), KF.CAUSES[cause]   # the reference agrees
    # first + nrows == 2^32 exactly is allowed by the header rule (the next one to fail here is none: check() goes on)
    b, _ = with_field(20, "<I", 2**32 - 3)
    assert KF.check(b.tobytes()) is None
    # two fields wrong: the documented order decides
    b, _ = with_field(8, "<I", 9)
    b[0] = 0
    refused(L.lh_kept_load, 0, b.ctypes.data, good.size, 0, KF.BAD_MAGIC)
    b, _ = with_field(28, "<I", 1)
    refused(L.lh_kept_load, 0, b.ctypes.data, good.size - 1, 0, KF.BAD_LENGTH)


# ---- keptfile -----------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_round_trip():
    blob = crafted()
    assert len(blob) == 64 + (2 * 3 + 1) * 8 + 5 * 10
    u = KF.unpack(blob)
    assert (u["first"], u["nrows"], u["cells"], u["samples"], u["bytes"]) == (5, 3, 5, 10, len(blob) - 64)
    assert u["offsets"].tolist() == [0, 2, 2, 5] and u["row_count"].tolist() == [7, 0, 3]
    assert u["counts"].tolist() == [3, 4, 1, 1, 1] and u["keys"].tolist() == [-32768, 32767, 100 - 32768, 101 - 32768, 102 - 32768]
    assert KF.pack(u["offsets"], u["keys"], u["counts"], first=5) == blob
    assert KF.check(blob) is None
    # counts that wrap: row_count and samples are sums mod 2^64
    big = KF.pack([0, 2, 3], np.array([1, 2, 3], dtype=np.int16), np.array([2**63, 2**63 + 5, 2**64 - 1], dtype=U64))
    u = KF.unpack(big)
    assert u["row_count"].tolist() == [5, 2**64 - 1] and u["samples"] == 4 and KF.check(big) is None
    # no cell at all
    empty = KF.pack([0, 0], np.zeros(0, np.int16), np.zeros(0, U64), first=2**32 - 1)
    assert len(empty) == KF.BLOB_MIN and KF.check(empty) is None and KF.unpack(empty)["cells"] == 0
    with pytest.raises(ValueError):
        KF.unpack(blob[:-1])
    with pytest.raises(ValueError):
        KF.unpack(b"x" * 10)
    assert KF.check(b"") == (KF.BAD_SHORT, 0, 0)


def wide():
    """rows of 1, 0, 63, 64, 65 and 129 cells, then a row whose first key lies below the previous row's last (bin 0)"""
    sizes = [1, 0, 63, 64, 65, 129, 3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    bins = np.concatenate([np.arange(n) * 7 + (1000 if n != 3 else 0) for n in sizes]).astype(np.uint16)
    counts = np.arange(1, bins.size + 1, dtype=U64)
    return off, (bins ^ np.uint16(0x8000)).view(np.int16), counts


def mutate(blob, what, at, value):
    """a copy of `blob` with one element of one array of the block (or the header's samples) replaced"""
    u = KF.unpack(blob)
    b = np.frombuffer(blob, dtype=np.uint8).copy()
    base = {"offsets": 64, "row_count": 64 + 8 * (u["nrows"] + 1), "counts": 64 + 8 * (2 * u["nrows"] + 1),
            "keys": 64 + 8 * (2 * u["nrows"] + 1) + 8 * u["cells"], "samples": 40}[what]
    width = 2 if what == "keys" else 8
    fmt = "<h" if what == "keys" else "<Q"
    b[base + width * at:base + width * (at + 1)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
    return b.tobytes()


def single_mutations():
    """(name, blob, the verdict check() must give) for the refusals the issue lists, over wide()"""
    off, keys, counts = wide()
    blob = KF.pack(off, keys, counts, first=3)
    u = KF.unpack(blob)
    nrows, cells = u["nrows"], u["cells"]
    o = [int(x) for x in off]
    key = lambda i: int(keys[i])                                                  # noqa: E731
    r5 = o[5]                                                                     # the row of 129 cells
    return blob, [
        ("off[1] > off[2]", mutate(blob, "offsets", 2, 0), (KF.BAD_OFFSET_ORDER, 1, 0)),
        ("off[nrows] != cells", mutate(blob, "offsets", nrows, cells - 1), (KF.BAD_OFFSET_LAST, nrows - 1, 0)),
        ("off[0] != 0", mutate(blob, "offsets", 0, 1), (KF.BAD_OFFSET_FIRST, 0, 0)),
        ("an offset beyond cells", mutate(blob, "offsets", 4, cells + 1), (KF.BAD_OFFSET_ORDER, 3, 0)),
        ("off[nrows] beyond cells", mutate(blob, "offsets", nrows, cells + 1), (KF.BAD_OFFSET_ORDER, nrows - 1, 0)),
        ("a huge offset", mutate(blob, "offsets", 3, 2**64 - 1), (KF.BAD_OFFSET_ORDER, 2, 0)),
        ("two equal keys", mutate(blob, "keys", r5 + 10, key(r5 + 9)), (KF.BAD_KEY_ORDER, 5, 10)),
        ("descending inside a step", mutate(blob, "keys", r5 + 70, key(r5 + 60)), (KF.BAD_KEY_ORDER, 5, 70)),
        ("descending across the step boundary", mutate(blob, "keys", r5 + 64, key(r5 + 63) - 1), (KF.BAD_KEY_ORDER, 5, 64)),
        ("descending across the second boundary", mutate(blob, "keys", r5 + 128, key(r5 + 127)), (KF.BAD_KEY_ORDER, 5, 128)),
        ("a zero count", mutate(blob, "counts", o[3] + 63, 0), (KF.BAD_ZERO_COUNT, 3, 63)),
        ("a zero count in a one-cell row", mutate(blob, "counts", 0, 0), (KF.BAD_ZERO_COUNT, 0, 0)),
        ("row_count off by one", mutate(blob, "row_count", 4, int(u["row_count"][4]) + 1), (KF.BAD_ROW_COUNT, 4, 65)),
        ("row_count of an empty row", mutate(blob, "row_count", 1, 1), (KF.BAD_ROW_COUNT, 1, 0)),
        ("samples off by one", mutate(blob, "samples", 0, u["samples"] + 1), (KF.BAD_SAMPLES, nrows, 0)),
    ]


def test_check_names_each_single_mutation():
    blob, cases = single_mutations()
    assert KF.check(blob) is None                                                 # a first key below the previous row's last is fine
    for name, bad, want in cases:
        assert KF.check(bad) == want, (name, KF.check(bad), want)
    # the ordering of the report: the lowest row, then the lowest index, then the lowest cause code
    u = KF.unpack(blob)
    o = [int(x) for x in u["offsets"]]
    two = mutate(mutate(blob, "counts", o[5] + 3, 0), "counts", o[3] + 40, 0)
    assert KF.check(two) == (KF.BAD_ZERO_COUNT, 3, 40)
    two = mutate(mutate(blob, "counts", o[5] + 9, 0), "keys", o[5] + 9, int(u["keys"][o[5] + 8]))
    assert KF.check(two) == (KF.BAD_KEY_ORDER, 5, 9)                              # the same cell: the lower cause code
    two = mutate(mutate(blob, "counts", o[5] + 9, 0), "keys", o[5] + 8, int(u["keys"][o[5] + 7]))
    assert KF.check(two) == (KF.BAD_KEY_ORDER, 5, 8)
    two = mutate(mutate(blob, "counts", o[5] + 9, 0), "row_count", 5, 1)
    assert KF.check(two) == (KF.BAD_ZERO_COUNT, 5, 9)                             # a cell before the row's sum
    two = mutate(mutate(blob, "samples", 0, 0), "row_count", 6, 1)
    assert KF.check(two) == (KF.BAD_ROW_COUNT, 6, 3)                              # a row before the block's sum
    two = mutate(mutate(blob, "offsets", 0, 1), "offsets", 1, 0)
    assert KF.check(two) == (KF.BAD_OFFSET_FIRST, 0, 0)                           # row 0: both offset causes, the lower code
    # a row of more than LH_NKEYS cells (cells <= nrows * LH_NKEYS holds: two rows)
    n = KF.NKEYS + 1
    long_row = KF.pack([0, n, n], np.zeros(n, np.int16), np.ones(n, U64))
    assert KF.check(long_row) == (KF.BAD_ROW_LENGTH, 0, 0)
