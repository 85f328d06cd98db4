"""CPU tests of lh_kept_encode* / lh_kept_decode*: declared, exported, bound; every LH_EINVAL / LH_ERANGE that is decided on the
host, with handle pointers that are fakes and never dereferenced and with encoded blobs whose header is wrong in exactly one
field (the cause lands in `why` in the documented order, *out stays untouched, and loghisto_amd.keptfile.check_encoded agrees);
lh_kept_load still answers LH_KEPT_BAD_MAGIC to an encoded blob.  Nothing here reaches a device."""
import ctypes as C
import os
import re
import struct

import numpy as np

from loghisto_amd import keptfile as KF
from tests.test_keptfile_encode import mutation_rows, raw_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"lh_kept_encode_size": 3, "lh_kept_encode": 5, "lh_kept_encode_device": 5, "lh_kept_decode": 7, "lh_kept_decode_device": 7}


def _source():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)


def test_the_five_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    raw = C.CDLL(_native.LIB_PATH)
    src = _source()
    for name, nargs in ARGS.items():
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs, decl
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7          # entries are only added
    # the format's constants and the new causes: the header and keptfile agree
    assert re.search(r'#define\s+LH_KEPT_ENC_MAGIC\s+"LHKENC\\x1a\\n"', src) and KF.ENC_MAGIC == b"LHKENC\x1a\n"
    assert re.search(r"#define\s+LH_KEPT_ENC_VERSION\s+1\b", src) and KF.ENC_VERSION == 1
    assert re.search(r"#define\s+LH_KEPT_ENC_MIN\s+\(LH_KEPT_BLOB_HEADER \+ 8\)", src) and KF.ENC_MIN == 72
    enc = dict((k, int(v)) for k, v in re.findall(r"#define\s+LH_KEPT_(BAD_ENC_[A-Z_]+)\s+(\d+)", src))
    assert enc == {k: v for v, k in KF.ENC_CAUSES.items() if k.startswith("BAD_ENC_")} and sorted(enc.values()) == [32, 33, 34, 35, 36]


def test_python_wrapper_has_the_codec():
    import inspect

    import loghisto_amd
    K = loghisto_amd.Kept
    for name in ("encode", "encode_device", "decode", "decode_device", "encoded_size"):
        assert callable(getattr(K, name)), name
    assert list(inspect.signature(K.decode).parameters)[:2] == ["data", "device"]
    assert inspect.signature(K.decode).parameters["device"].default == 0
    assert inspect.signature(K.save).parameters["encoded"].default is False
    assert inspect.signature(K.load).parameters["encoded"].default is False
    for name in ("encode", "decode", "check_encoded", "encoded_bound"):
        assert callable(getattr(loghisto_amd.keptfile, name)), name


def _why(_native, size=16):
    return _native.LhKeptCheck(struct_size=size, cause=0x77, row=0x77, index=0x77)


def test_encode_checks_its_arguments_on_the_host(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    fake = C.c_void_p(0x1000)
    n = C.c_size_t(0x77)
    buf = np.full(256, 7, dtype=np.uint8)
    assert L.lh_kept_encode_size(None, None, C.byref(n)) == EINVAL and L.lh_kept_encode_size(fake, None, None) == EINVAL
    for fn in (L.lh_kept_encode, L.lh_kept_encode_device):
        assert fn(None, buf.ctypes.data, 256, None, C.byref(n)) == EINVAL         # NULL handle
        assert fn(fake, None, 256, None, C.byref(n)) == EINVAL                    # NULL buffer
        assert fn(None, None, 0, None, None) == EINVAL
        for cap in (0, 1, 63, 64, 71):                                            # below the smallest encoded blob there is
            assert fn(fake, buf.ctypes.data, cap, None, C.byref(n)) == ERANGE, cap    # ... before the handle is looked at
        assert fn(None, buf.ctypes.data, 0, None, C.byref(n)) == EINVAL           # a cause of LH_EINVAL wins
    assert n.value == 0x77 and np.all(buf == 7)                                   # nothing was written


def test_decode_decides_the_header_on_the_host_in_the_documented_order(native_lib):
    from loghisto_amd import _native
    L, EINVAL = native_lib, _native.EINVAL
    rows = mutation_rows()
    nrows, cells = len(rows), sum(len(b) for b, _ in rows)
    good = np.frombuffer(raw_encode(rows, first=5), dtype=np.uint8).copy()
    assert KF.check_encoded(good.tobytes()) is None
    out = C.c_void_p(0x77)

    def refused(fn, device, addr, length, flags, cause, why="own"):
        w = _why(_native) if why == "own" else why
        assert fn(device, addr, length, flags, None, C.byref(w) if w is not None else None, C.byref(out)) == EINVAL
        assert out.value == 0x77                                                  # *out untouched
        if w is not None:
            assert (w.struct_size, w.cause, w.row, w.index) == (16, cause, 0, 0), (KF.ENC_CAUSES.get(w.cause), KF.ENC_CAUSES[cause])

    # ---- the causes that need no header: both forms, before any device call (the device pointer is a fake)
    for fn in (L.lh_kept_decode, L.lh_kept_decode_device):
        addr = good.ctypes.data if fn is L.lh_kept_decode else 0x1000
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

    # ---- the header's fields: each case has every EARLIER field of the order right and every LATER one wrong as well, so the
    # order itself is what is asserted
    def fields(**kw):
        f = dict(magic=KF.ENC_MAGIC, version=1, header=64, nkeys=65536, first=5, nrows=nrows, r0=0, cells=cells, samples=0,
                 bytes=good.size - 64, r1=bytes(8))
        f.update(kw)
        b = good.copy()
        b[:64] = np.frombuffer(struct.pack("<8sIIIIIIQQQ8s", *f.values()), dtype=np.uint8)
        return b

    bound = 8 * ((nrows + 1) // 2) + 10 * cells + 6 * nrows
    late = dict(version=9, header=0, nkeys=1, nrows=0, cells=2**63, bytes=4, r0=1, r1=b"\x01" * 8)
    order = [("magic", dict(magic=KF.MAGIC), KF.BAD_MAGIC), ("version", dict(version=2), KF.BAD_VERSION),
             ("header", dict(header=128), KF.BAD_HEADER_SIZE), ("nkeys", dict(nkeys=65535), KF.BAD_NKEYS),
             ("nrows", dict(nrows=0), KF.BAD_NROWS), ("first", dict(first=2**32 - nrows + 1), KF.BAD_FIRST),
             ("cells", dict(cells=nrows * 65536 + 1), KF.BAD_CELLS), ("bytes", dict(bytes=good.size - 64 + 4), KF.BAD_BYTES),
             ("r0", dict(r0=1), KF.BAD_RESERVED)]
    names = [x[0] for x in order]
    for i, (name, kw, cause) in enumerate(order):
        alone, with_later = fields(**kw), fields(**{**{k: v for k, v in late.items() if k in names[i + 1:] or k == "r1"}, **kw})
        for b in (alone, with_later):
            refused(L.lh_kept_decode, 0, b.ctypes.data, good.size, 0, cause)
            refused(L.lh_kept_decode, 63, b.ctypes.data, good.size, 0, cause)     # whatever the device: it is not opened
            refused(L.lh_kept_decode, 0, b.ctypes.data, good.size, 0, cause, why=None)
            assert KF.check_encoded(b.tobytes()) == (cause, 0, 0), name           # the reference agrees
    more = [(fields(magic=b"LHKENC\x1a\r"), good.size, KF.BAD_MAGIC), (fields(magic=bytes(8)), good.size, KF.BAD_MAGIC),
            (fields(version=0), good.size, KF.BAD_VERSION), (fields(first=2**32 - 1), good.size, KF.BAD_FIRST),
            (fields(bytes=32), good.size, KF.BAD_BYTES),                          # below the directory's 40
            (fields(bytes=bound // 8 * 8 + 8), good.size, KF.BAD_BYTES),          # above the bound
            (fields(bytes=bound // 8 * 8), good.size, KF.BAD_LENGTH),             # at the bound: the length decides
            (good, good.size - 1, KF.BAD_LENGTH), (good, good.size - 8, KF.BAD_LENGTH), (good, 64, KF.BAD_LENGTH),
            (np.concatenate([good, good[:8]]), good.size + 8, KF.BAD_LENGTH),
            (fields(r0=0x80000000), good.size, KF.BAD_RESERVED), (fields(bytes=good.size - 64 + 8, r0=1), good.size, KF.BAD_LENGTH)]
    more += [(fields(r1=bytes(i) + b"\x01" + bytes(7 - i)), good.size, KF.BAD_RESERVED) for i in range(8)]
    for b, length, cause in more:
        refused(L.lh_kept_decode, 0, b.ctypes.data, length, 0, cause)
        assert KF.check_encoded(b[:length].tobytes()) == (cause, 0, 0), KF.ENC_CAUSES[cause]
    # first + nrows == 2^32 exactly passes the header (keptfile goes on to the payload and takes it)
    assert KF.check_encoded(fields(first=2**32 - nrows, samples=KF.parse_header(good)["samples"]).tobytes()) is None


def test_load_still_refuses_an_encoded_blob_and_decode_a_verbatim_one(native_lib):
    from loghisto_amd import _native
    L = native_lib
    rows = mutation_rows()
    enc = np.frombuffer(raw_encode(rows), dtype=np.uint8).copy()
    out = C.c_void_p(0x77)
    for fn in (L.lh_kept_load,):
        w = _why(_native)
        assert fn(0, enc.ctypes.data, enc.size, 0, None, C.byref(w), C.byref(out)) == _native.EINVAL
        assert (w.cause, w.row, w.index) == (KF.BAD_MAGIC, 0, 0) and out.value == 0x77
    blob = np.frombuffer(KF.decode(enc.tobytes()), dtype=np.uint8).copy()
    w = _why(_native)
    assert L.lh_kept_decode(0, blob.ctypes.data, blob.size, 0, None, C.byref(w), C.byref(out)) == _native.EINVAL
    assert (w.cause, w.row, w.index) == (KF.BAD_MAGIC, 0, 0) and out.value == 0x77
