"""CPU tests of lh_kept_gather / lh_kept_gather_device (kept rows re-mapped per handle and summed into one kept handle): declared,
exported, bound with the header's prototypes, the ABI version unchanged, and every refusal the host decides before a handle is
looked at -- the handle pointers below are fakes that are never dereferenced -- in the documented order and with *out left as it
was.  What needs a handle (the devices, the host form's rows against the blocks) is in tests/test_gpu_kept_gather.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x77
NO_ROW = 0xffffffff
PROTOS = {
    "lh_kept_gather": "lh_kept *const *kept, size_t nkept, const uint32_t *src, size_t n, uint32_t first_out, uint32_t flags, "
                      "void *stream, lh_kept **out",
    "lh_kept_gather_device": "lh_kept *const *kept, size_t nkept, const uint32_t *d_src, size_t n, uint32_t first_out, uint32_t flags, "
                             "void *stream, lh_kept **out",
}
CTYPES = {"size_t": C.c_size_t, "uint32_t": C.c_uint32}


def _read(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_two_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = re.sub(r"/\*.*?\*/", "", _read("loghisto_gpu.h"), flags=re.S)
    raw = C.CDLL(_native.LIB_PATH)
    for name, proto in PROTOS.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert decl, f"{name} is not declared"
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == proto, name
        assert hasattr(raw, name), f"{name} is not exported"
        restype, argtypes = _native.SIGNATURES[name]
        # a pointer is bound as c_void_p, but for `out`, which the wrappers hand over by reference
        want = [C.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in proto.split(", ")][:-1] + [C.POINTER(C.c_void_p)]
        assert restype is C.c_int and argtypes == want and getattr(native_lib, name).restype is C.c_int, name
    assert re.search(r"#define\s+LH_KEPT_NO_ROW\s+0xffffffffu\b", src) and _native.KEPT_NO_ROW == NO_ROW
    # adding functions is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    # the deliberate difference from the readers, and what is out of scope, stand in the header in their own words
    text = re.sub(r"\s+\*?\s*", " ", _read("loghisto_gpu.h"))
    for sentence in ("makes handle i's segment empty for that output row and nothing else. Nothing is read for it.",
                     "the gather of a list equals lh_kept_merge of the nkept one-handle gathers",
                     "more than LH_MAX_KEPT handles a call (gather in groups, then lh_kept_merge); many-to-one roll-ups of names "
                     "within one handle; names inside the blob"):
        assert sentence in text, sentence
    # the measurement switch that lets tests compare the routes
    tuning = re.sub(r"/\*.*?\*/", "", _read("loghisto_gpu_tuning.h"), flags=re.S)
    assert re.search(r"\bint\s+lh_tool_kept_gather_route\s*\(\s*uint32_t route, uint32_t \*previous\s*\)\s*;", tuning)
    assert hasattr(raw, "lh_tool_kept_gather_route") and "lh_tool_kept_gather_route" in _native.TUNING_SIGNATURES
    prev = C.c_uint32(99)
    assert native_lib.lh_tool_kept_gather_route(_native.GATHER_TILE, C.byref(prev)) == 0 and prev.value == _native.GATHER_DEFAULT
    assert native_lib.lh_tool_kept_gather_route(4, C.byref(prev)) == _native.EINVAL and prev.value == _native.GATHER_DEFAULT
    assert native_lib.lh_tool_kept_gather_route(_native.GATHER_DEFAULT, C.byref(prev)) == 0 and prev.value == _native.GATHER_TILE
    assert native_lib.lh_tool_kept_gather_route(0, None) == 0


def test_every_early_error_is_decided_on_the_host_and_out_is_untouched(native_lib):
    from loghisto_amd import _native
    EINVAL, ERANGE = _native.EINVAL, _native.ERANGE
    VP = C.c_void_p
    out = VP(SENTINEL)
    BIG = 1 << 32
    src = np.full(64 * 4, NO_ROW, dtype=np.uint32)
    sp = src.ctypes.data

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two = handles(0x1000), handles(0x1000, 0x2000)
    full = handles(*[0x1000 * (i + 1) for i in range(64)])
    too_many = handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 63 + [None])),
             handles(*([0x1000] * 31 + [None] + [0x1000] * 32))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment

    for fn in (native_lib.lh_kept_gather, native_lib.lh_kept_gather_device):
        def call(h, nkept, n, flags=0, first_out=0, src_=sp, out_=None, stream=None):
            return fn(h, nkept, src_, n, first_out, flags, stream, C.byref(out) if out_ is None else out_)

        for n, first_out in ((1, 0), (4, 0), (BIG, 0), (4, 0xfffffffd)):      # each cause of LH_EINVAL wins over the early LH_ERANGE
            assert call(None, 1, n, first_out=first_out) == EINVAL            # NULL list
            assert call(None, 0, n, first_out=first_out) == EINVAL
            for h in holes:                                                   # a NULL entry, wherever
                assert call(h, len(h), n, first_out=first_out) == EINVAL
            for off in range(1, C.sizeof(VP)):                                # the list itself off its alignment
                assert fn(C.addressof(odd) + off, 1, sp, n, first_out, 0, None, C.byref(out)) == EINVAL, off
            assert call(one, 0, n, first_out=first_out) == EINVAL             # nkept 0
            assert call(too_many, 65, n, first_out=first_out) == EINVAL       # nkept too large
            assert call(full, (1 << 64) - 1, n, first_out=first_out) == EINVAL
            for s, k in ((one, 1), (two, 2), (full, 64)):
                assert call(s, k, n, first_out=first_out, src_=None) == EINVAL   # NULL src
                for off in (1, 2, 3):                                         # src off its alignment
                    assert call(s, k, n, first_out=first_out, src_=sp + off) == EINVAL, off
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert call(s, k, n, flags, first_out=first_out) == EINVAL, flags
                assert fn(s, k, sp, n, first_out, 0, None, None) == EINVAL    # NULL out
        for s, k in ((one, 1), (two, 2), (full, 64)):
            assert call(s, k, 0) == EINVAL                                    # n == 0
            assert call(s, k, 0, first_out=5) == EINVAL
            # more rows than a handle can have, or rows that end beyond 2^32: LH_ERANGE, decided before a handle is looked at
            assert call(s, k, BIG) == ERANGE
            assert call(s, k, (1 << 64) - 1) == ERANGE
            assert call(s, k, 0xffffffff, first_out=2) == ERANGE
            assert call(s, k, 4, first_out=0xfffffffd) == ERANGE              # first_out + n == 2^32 + 1
            assert call(s, k, 2, first_out=0xffffffff) == ERANGE
            assert call(s, k, BIG, stream=0x10) == ERANGE                     # ... whatever the stream
    assert out.value == SENTINEL                                              # through every failure
    assert np.all(src == NO_ROW)


def test_python_wrapper_has_gather_and_the_fleet_functions():
    import loghisto_amd
    from loghisto_amd import fleet, keptfile
    sig = inspect.signature(loghisto_amd.Kept.gather)
    assert list(sig.parameters) == ["self", "src", "earlier", "first", "stream"]
    assert sig.parameters["earlier"].default == () and sig.parameters["first"].default == 0 and sig.parameters["stream"].default is None
    assert loghisto_amd.union_names is fleet.union_names and loghisto_amd.aggregate is fleet.aggregate
    assert {"union_names", "aggregate"} <= set(loghisto_amd.__all__)
    assert fleet.NO_ROW == keptfile.NO_ROW == NO_ROW
    assert list(inspect.signature(fleet.aggregate).parameters)[:2] == ["kepts", "name_lists"]
    assert list(inspect.signature(keptfile.gather).parameters)[:3] == ["blobs", "src", "first_out"]
    # merge's signature stays as tests/test_kept_merge_abi.py pins it
    assert list(inspect.signature(loghisto_amd.Kept.merge).parameters) == ["self", "earlier", "nmetrics", "first", "stream"]
