"""CPU tests of lh_names_* / lh_lines* (wire lines for any per-name device columns): declared, exported, bound, the column's
layout, the constants, and every LH_EINVAL / LH_ERANGE check runs on the host before the handle is looked at -- the handle
below is a fake that is never dereferenced."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lh_names_create": 3, "lh_names_refresh": 2, "lh_names_destroy": 1, "lh_lines": 13, "lh_lines_ids": 14,
         "lh_lines_device": 13, "lh_lines_ids_device": 14}


def _header():
    return open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read()


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(lh_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_native.LIB_PATH)
    for name, nargs in NAMES.items():
        assert name in declared, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        assert len(_native.SIGNATURES[name][1]) == nargs, name
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == nargs, name                             # the header's own argument count
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7       # adding functions is backward compatible


def test_the_constants_match_the_header():
    from loghisto_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    consts = dict(re.findall(r"\b(LH_(?:MAX_COLUMNS|COL_[A-Z0-9]+|OP_[A-Z_]+|LINES_[A-Z_]+))\s*=?\s*(\d+)", src))
    assert consts == dict(LH_MAX_COLUMNS="128", LH_COL_F64="0", LH_COL_U64="1", LH_COL_U32="2", LH_COL_KEY="3", LH_OP_VALUE="0",
                          LH_OP_RATIO="1", LH_OP_SQRT_RATIO="2", LH_OP_DIFF="3", LH_LINES_SKIP_NAN="1")
    assert N.MAX_COLUMNS == 128 and N.LINES_SKIP_NAN == 1
    assert (N.COL_F64, N.COL_U64, N.COL_U32, N.COL_KEY) == (0, 1, 2, 3)
    assert (N.OP_VALUE, N.OP_RATIO, N.OP_SQRT_RATIO, N.OP_DIFF) == (0, 1, 2, 3)


def test_the_column_is_64_bytes_with_the_headers_offsets():
    from loghisto_amd import _native as N
    body = re.search(r"typedef struct lh_column \{(.*?)\} lh_column;", _header(), flags=re.S).group(1)
    fields = re.findall(r"^\s*(const \w+ \*|\w+ )(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    ctype = {"const char *": C.c_char_p, "const void *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint64_t ": C.c_uint64,
             "uint8_t ": C.c_uint8, "uint32_t ": C.c_uint32}

    class Column(C.Structure):                                                 # the header's struct, laid out by the C rules
        _fields_ = [(name, ctype[t]) for t, name in fields]
    want = ["label", "a", "b", "valid", "a_stride", "b_stride", "valid_stride", "a_type", "b_type", "op", "reserved0", "reserved1"]
    assert [name for _, name in fields] == want == [name for name, _ in N.LhColumn._fields_]
    assert C.sizeof(Column) == 64 == C.sizeof(N.LhColumn)
    assert [getattr(Column, n).offset for n in want] == [0, 8, 16, 24, 32, 40, 48, 56, 57, 58, 59, 60]
    for n in want:
        assert getattr(N.LhColumn, n).offset == getattr(Column, n).offset, n
        assert getattr(N.LhColumn, n).size == getattr(Column, n).size, n


def _column(label=b"%s_x", a=0x2000, b=0, valid=0, a_stride=8, b_stride=8, valid_stride=1, a_type=0, b_type=0, op=0, r0=0, r1=0):
    from loghisto_amd import _native as N
    return N.LhColumn(label, a, b, valid, a_stride, b_stride, valid_stride, a_type, b_type, op, r0, r1)


def _forms(L):
    """The four entry points behind one signature: f(nm, n, cols, ncols, fmt, flags, len, ids=, id_stride=, row_count=,
    rc_stride=) -- every pointer but `len` is a fake device address that the checks never follow."""
    def make(fn, by_id):
        def call(nm, n, cols, ncols, fmt, flags, ln, ids=0x3000, id_stride=4, row_count=0, rc_stride=8, first=0):
            rows = (ids, id_stride, n) if by_id else (first, n)
            return fn(nm, *rows, row_count, rc_stride, cols, ncols, fmt, flags, None, None, 0, ln)
        return call
    return [(make(L.lh_lines, False), False, 8), (make(L.lh_lines_ids, True), True, 8),
            (make(L.lh_lines_device, False), False, 8), (make(L.lh_lines_ids_device, True), True, 8)]


def test_every_einval_and_erange_case_is_decided_on_the_host(native_lib):
    from loghisto_amd import _native as N
    L, EINVAL, ERANGE = native_lib, N.EINVAL, N.ERANGE
    fake = C.c_void_p(0x1000)              # never dereferenced: the argument checks come first
    fmt = C.pointer(N.LhLineFormat(b"put ", b" 1 ", b"\n", 0, 0))
    box = (C.c_uint64 * 4)(7, 7, 7, 7)
    ln = C.addressof(box)
    one = (N.LhColumn * 1)(_column())

    def cols(*cs):
        return (N.LhColumn * len(cs))(*cs)
    for f, by_id, len_align in _forms(L):
        assert f(None, 1, one, 1, fmt, 0, ln) == EINVAL                          # NULL handle
        assert f(fake, 1, None, 1, fmt, 0, ln) == EINVAL                         # NULL cols
        assert f(fake, 1, one, 1, None, 0, ln) == EINVAL                         # NULL fmt
        assert f(fake, 1, one, 1, fmt, 0, None) == EINVAL                        # NULL len / d_len
        for off in range(1, len_align):
            assert f(fake, 1, one, 1, fmt, 0, ln + off) == EINVAL, off           # ... misaligned
        for piece in range(3):                                                   # a NULL piece of the format
            parts = [b"a", b"b", b"c"]
            parts[piece] = None
            assert f(fake, 1, one, 1, C.pointer(N.LhLineFormat(*parts, 0, 0)), 0, ln) == EINVAL
        assert f(fake, 1, one, 0, fmt, 0, ln) == EINVAL                          # ncols == 0
        many = (N.LhColumn * 129)(*[_column() for _ in range(129)])
        assert f(fake, 1, many, 129, fmt, 0, ln) == EINVAL                       # ncols > LH_MAX_COLUMNS
        for flags in (2, 3, 0x80000000):
            assert f(fake, 1, one, 1, fmt, flags, ln) == EINVAL                  # unknown flag bits
        for bad in (_column(a_type=4), _column(a_type=255), _column(op=1, b=0x4000, b_type=4), _column(b_type=4),
                    _column(op=4, b=0x4000), _column(op=255, b=0x4000)):
            assert f(fake, 1, cols(bad), 1, fmt, 0, ln) == EINVAL                # unknown type / op
        assert f(fake, 1, cols(_column(r0=1)), 1, fmt, 0, ln) == EINVAL          # non-zero reserved fields
        assert f(fake, 1, cols(_column(r1=1)), 1, fmt, 0, ln) == EINVAL
        for label in (None, b"", b"nope", b"%s_%s", b"%d_%s", b"%s_100%", b"%%s", b"%"):
            assert f(fake, 1, cols(_column(label=label)), 1, fmt, 0, ln) == EINVAL, label   # not exactly one %s
        assert f(fake, 1, cols(_column(), _column(label=b"x")), 2, fmt, 0, ln) == EINVAL    # ... in any column
        # prefix + sep + suffix + all labels above 4 KiB: 8 + 2 + 4086 = 4096 passes the checks (the LH_ERANGE behind them
        # answers), one more byte does not
        assert f(fake, 1 << 32, cols(_column(label=b"%s" + b"y" * 4086)), 1, fmt, 0, ln) == ERANGE
        assert f(fake, 1 << 32, cols(_column(label=b"%s" + b"y" * 4087)), 1, fmt, 0, ln) == EINVAL
        assert f(fake, 1, one, 1, C.pointer(N.LhLineFormat(b"p" * 4097, b"", b"", 0, 0)), 0, ln) == EINVAL
        half = [_column(label=b"%s" + b"z" * 2046) for _ in range(2)]            # 2 x 2048 + 8 > 4096: the labels add up
        assert f(fake, 1, cols(*half), 2, fmt, 0, ln) == EINVAL
        assert f(fake, 1, cols(_column(a=0)), 1, fmt, 0, ln) == EINVAL           # NULL a
        for op in (1, 2, 3):
            assert f(fake, 1, cols(_column(op=op, b=0)), 1, fmt, 0, ln) == EINVAL           # an op other than VALUE, NULL b
        assert f(fake, 1, cols(_column(op=1, a_type=3, a_stride=2, b=0x4000)), 1, fmt, 0, ln) == EINVAL   # KEY under an op
        assert f(fake, 1, cols(_column(op=1, b=0x4000, b_type=3, b_stride=2)), 1, fmt, 0, ln) == EINVAL   # KEY as b
        assert f(fake, 1, cols(_column(b=0x4000, b_type=3, b_stride=2)), 1, fmt, 0, ln) == EINVAL
        for t, size in ((0, 8), (1, 8), (2, 4), (3, 2)):                         # pointer / stride against the element size
            for off in range(1, size):
                assert f(fake, 1, cols(_column(a_type=t, a=0x2000 + off, a_stride=size)), 1, fmt, 0, ln) == EINVAL, (t, off)
                assert f(fake, 1, cols(_column(a_type=t, a_stride=size + off)), 1, fmt, 0, ln) == EINVAL, (t, off)
                if t != 3:
                    assert f(fake, 1, cols(_column(op=3, b_type=t, b=0x4000 + off, b_stride=size)), 1, fmt, 0, ln) == EINVAL
                    assert f(fake, 1, cols(_column(op=3, b_type=t, b=0x4000, b_stride=size + off)), 1, fmt, 0, ln) == EINVAL
        for off in range(1, 8):                                                  # the row counts are uint64
            assert f(fake, 1, one, 1, fmt, 0, ln, row_count=0x5000 + off) == EINVAL
            assert f(fake, 1, one, 1, fmt, 0, ln, row_count=0x5000, rc_stride=8 + off) == EINVAL
        if by_id:
            assert f(fake, 1, one, 1, fmt, 0, ln, ids=0) == EINVAL               # NULL ids with n > 0
            for off in (1, 2, 3):
                assert f(fake, 1, one, 1, fmt, 0, ln, ids=0x3000 + off) == EINVAL
                assert f(fake, 1, one, 1, fmt, 0, ln, id_stride=32 + off) == EINVAL         # id_stride not a multiple of 4
        # more entries than an id is wide: LH_ERANGE before the handle is looked at; a cause of LH_EINVAL wins over it
        for n in (1 << 32, (1 << 64) - 1):
            assert f(fake, n, one, 1, fmt, 0, ln) == ERANGE
            assert f(fake, n, one, 1, fmt, 1, ln) == ERANGE
            assert f(fake, n, one, 1, fmt, 2, ln) == EINVAL
            assert f(fake, n, cols(_column(label=b"x")), 1, fmt, 0, ln) == EINVAL
    assert list(box) == [7, 7, 7, 7]                                             # nothing was written


def test_the_empty_host_call_returns_before_the_handle_is_looked_at(native_lib):
    from loghisto_amd import _native as N
    L = native_lib
    fake = C.c_void_p(0x1000)
    fmt = C.pointer(N.LhLineFormat(b"", b" ", b"\n", 1, 0))
    one = (N.LhColumn * 1)(_column(op=2, b=0x4000, b_type=2, b_stride=4))
    for f, by_id, _ in _forms(L)[:2]:
        ln = C.c_size_t(99)
        assert f(fake, 0, one, 1, fmt, 1, C.addressof(ln)) == N.OK and ln.value == 0
        if by_id:
            ln = C.c_size_t(99)
            assert f(fake, 0, one, 1, fmt, 0, C.addressof(ln), ids=0) == N.OK and ln.value == 0   # NULL ids go with n == 0


def test_names_create_checks_its_arguments(native_lib):
    from loghisto_amd import _native as N
    L = native_lib
    h = C.c_void_p(0x77)
    assert L.lh_names_create(None, 0, C.byref(h)) == N.EINVAL and h.value == 0x77
    assert L.lh_names_create(C.c_void_p(0x1000), 0, None) == N.EINVAL
    assert L.lh_names_create(C.c_void_p(0x1000), -1, C.byref(h)) == N.EINVAL and h.value == 0x77
    assert L.lh_names_refresh(None, None) == N.EINVAL
    assert L.lh_names_destroy(None) == N.EINVAL


def test_python_wrapper_has_the_feature():
    import loghisto_amd
    assert callable(getattr(loghisto_amd.Engine, "device_names"))
    assert callable(getattr(loghisto_amd.Snapshot, "spread_lines"))
    for m in ("lines", "refresh", "close", "__enter__", "__exit__"):
        assert callable(getattr(loghisto_amd.Names, m)), m


def test_host_arrays_are_refused_before_the_library_is_called():
    import numpy as np
    import pytest
    from loghisto_amd import engine
    nm = object.__new__(engine.Names)           # no handle: the checks come before any call
    nm._h, nm.count, nm._buf = None, 4, None
    with pytest.raises(ValueError, match="device"):
        nm.lines([dict(label="%s_x", a=np.zeros(4))], n=4)
    with pytest.raises(ValueError, match="op is one of"):
        nm._column(dict(label="%s_x", a=np.zeros(4), op="plus"), 4)
