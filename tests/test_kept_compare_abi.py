"""CPU tests of lh_kept_compare* (lh_compare's outputs between two lists of kept intervals): declared, exported, bound with
the header's prototypes, and every LH_EINVAL, the early LH_ERANGE and the empty call decided on the host, in that order,
before any handle is looked at -- the handle pointers below are fakes that are never dereferenced -- with no output written."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = ("uint64_t *{}count_a, uint64_t *{}count_b, double *{}ks, int16_t *{}ks_key, uint64_t *{}ks_below_a, "
        "uint64_t *{}ks_below_b, double *{}w1, double *{}shift")
LISTS = "lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, "
PROTOS = {
    "lh_kept_compare": LISTS + "uint32_t first, size_t nmetrics, uint32_t flags, void *stream, " + OUTS.format(*[""] * 8),
    "lh_kept_compare_device": LISTS + "uint32_t first, size_t nmetrics, uint32_t flags, void *stream, " + OUTS.format(*["d_"] * 8),
    "lh_kept_compare_ids": LISTS + "const uint32_t *ids, size_t n, uint32_t flags, void *stream, " + OUTS.format(*[""] * 8),
    "lh_kept_compare_ids_device": LISTS + "const uint32_t *d_ids, size_t n, uint32_t flags, void *stream, " + OUTS.format(*["d_"] * 8),
}
CTYPES = {"size_t": C.c_size_t, "uint32_t": C.c_uint32}            # every pointer is bound as c_void_p


def _header(name="loghisto_gpu.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbols_are_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = _header()
    raw = C.CDLL(_native.LIB_PATH)
    for name, proto in PROTOS.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert decl, f"{name} is not declared"
        assert re.sub(r"\s+", " ", decl.group(1)).strip() == proto, name
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _native.SIGNATURES and getattr(native_lib, name).restype is C.c_int, name
        restype, argtypes = _native.SIGNATURES[name]
        want = [C.c_void_p if "*" in a else CTYPES[a.split()[0]] for a in proto.split(", ")]
        assert restype is C.c_int and argtypes == want, name
    # adding functions is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    # the cap and its reason stand in the header
    text = re.sub(r"\s+\*?\s*", " ", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read())
    assert "nbase + ncur <= LH_MAX_KEPT: ONE handle per lane of a wave, and the two lists travel by value" in text
    assert "Longer windows go through lh_kept_merge first" in text


def test_the_tile_hook(native_lib):
    from loghisto_amd import _native
    assert re.search(r"\bint\s+lh_tool_kept_compare_tile\s*\(\s*uint32_t\s*\*\s*bins\s*\)\s*;", _header("loghisto_gpu_tuning.h"))
    assert _native.TUNING_SIGNATURES["lh_tool_kept_compare_tile"][1] == [C.POINTER(C.c_uint32)]
    tile = C.c_uint32(0)
    assert native_lib.lh_tool_kept_compare_tile(None) == _native.EINVAL
    assert native_lib.lh_tool_kept_compare_tile(C.byref(tile)) == 0
    # whole steps of 256 bins; two tiles a row and four rows a workgroup within 64 KiB of LDS
    assert tile.value % 256 == 0 and 256 <= tile.value and 4 * 2 * tile.value * 8 <= 65536


def test_every_early_error_is_decided_on_the_host_in_order(native_lib):
    from loghisto_amd import _native
    L, EINVAL, ERANGE = native_lib, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two = handles(0x1000), handles(0x1000, 0x2000)
    h32, h33 = handles(*[0x1000 * (i + 1) for i in range(32)]), handles(*[0x1000 * (i + 1) for i in range(33)])
    h63, h64 = handles(*[0x1000 * (i + 1) for i in range(63)]), handles(*[0x1000 * (i + 1) for i in range(64)])
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 31 + [None]))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    fields = dict(count_a=np.uint64, count_b=np.uint64, ks=np.float64, key=np.int16, below_a=np.uint64, below_b=np.uint64,
                  w1=np.float64, shift=np.float64)
    arrays = {k: np.full(8, 7, dtype=t) for k, t in fields.items()}
    outs = [a.ctypes.data for a in arrays.values()]
    widths = [a.itemsize for a in arrays.values()]
    ids = np.arange(4, dtype=np.uint32)
    BIG = 1 << 32

    def forms():
        """call(base, nbase, cur, ncur, n, flags, *outs) for the four entry points, the stream NULL"""
        for fn in (L.lh_kept_compare, L.lh_kept_compare_device):
            yield lambda b, nb, c, nc, n, fl, *o, fn=fn: fn(b, nb, c, nc, 0, n, fl, None, *o)
        for fn in (L.lh_kept_compare_ids, L.lh_kept_compare_ids_device):
            yield lambda b, nb, c, nc, n, fl, *o, fn=fn: fn(b, nb, c, nc, ids.ctypes.data, n, fl, None, *o)

    good = ((one, 1, one, 1), (two, 2, one, 1), (h32, 32, h32, 32), (one, 1, h63, 63), (h63, 63, one, 1))
    for fn in forms():
        for n in (1, BIG):                                                    # each cause of LH_EINVAL wins over the early LH_ERANGE
            assert fn(None, 1, one, 1, n, 0, *outs) == EINVAL                 # a NULL list, either side
            assert fn(one, 1, None, 1, n, 0, *outs) == EINVAL
            assert fn(None, 0, None, 0, n, 0, *outs) == EINVAL
            for off in range(1, C.sizeof(VP)):                                # a list off its alignment, either side
                assert fn(C.addressof(odd) + off, 1, one, 1, n, 0, *outs) == EINVAL, off
                assert fn(one, 1, C.addressof(odd) + off, 1, n, 0, *outs) == EINVAL, off
            for h in holes:                                                   # a NULL entry, wherever
                assert fn(h, len(h), one, 1, n, 0, *outs) == EINVAL
                assert fn(one, 1, h, len(h), n, 0, *outs) == EINVAL
            assert fn(one, 0, one, 1, n, 0, *outs) == EINVAL                  # an empty side
            assert fn(one, 1, one, 0, n, 0, *outs) == EINVAL
            assert fn(h33, 33, h32, 32, n, 0, *outs) == EINVAL                # 65 handles in all
            assert fn(h32, 32, h33, 33, n, 0, *outs) == EINVAL
            assert fn(h64, 64, one, 1, n, 0, *outs) == EINVAL
            assert fn(one, 1, h64, 64, n, 0, *outs) == EINVAL
            assert fn(h64, (1 << 64) - 1, one, 2, n, 0, *outs) == EINVAL      # counts whose sum wraps
            assert fn(h64, (1 << 64) - 1, h64, (1 << 64) - 1, n, 0, *outs) == EINVAL
            for b, nb, c, nc in good:
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert fn(b, nb, c, nc, n, flags, *outs) == EINVAL, flags
                assert fn(b, nb, c, nc, n, 0, *[None] * 8) == EINVAL          # all outputs NULL
                for k, width in enumerate(widths):                            # an output off its element's alignment
                    for off in range(1, width):
                        bad = list(outs)
                        bad[k] += off
                        assert fn(b, nb, c, nc, n, 0, *bad) == EINVAL, (k, off)
                        only = [None] * 8
                        only[k] = bad[k]
                        assert fn(b, nb, c, nc, n, 0, *only) == EINVAL, (k, off)
        for b, nb, c, nc in good:
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert fn(b, nb, c, nc, BIG, 0, *outs) == ERANGE
            assert fn(b, nb, c, nc, (1 << 64) - 1, 0, *outs) == ERANGE
            assert fn(b, nb, c, nc, BIG, 0, None, None, None, outs[3], None, None, None, None) == ERANGE
            # an empty call: LH_OK before any handle is looked at (the handles are fakes)
            assert fn(b, nb, c, nc, 0, 0, *outs) == 0
            assert fn(b, nb, c, nc, 0, 0, None, None, outs[2], None, None, None, None, None) == 0
    assert L.lh_kept_compare(one, 1, one, 1, 0xffffffff, BIG, 0, 0x10, *outs) == ERANGE      # whatever first and the stream
    # the id forms' own causes
    for fn in (L.lh_kept_compare_ids, L.lh_kept_compare_ids_device):
        for b, nb, c, nc in good:
            assert fn(b, nb, c, nc, None, 1, 0, None, *outs) == EINVAL        # ids NULL with n > 0
            assert fn(b, nb, c, nc, None, BIG, 0, None, *outs) == EINVAL      # ... wins over the early LH_ERANGE
            assert fn(b, nb, c, nc, None, 0, 0, None, *outs) == 0             # n == 0: no list is needed
            for off in (1, 2, 3):                                             # ids misaligned
                assert fn(b, nb, c, nc, ids.ctypes.data + off, 1, 0, None, *outs) == EINVAL, off
                assert fn(b, nb, c, nc, ids.ctypes.data + off, 0, 0, None, *outs) == EINVAL, off
                assert fn(b, nb, c, nc, ids.ctypes.data + off, BIG, 0, None, *outs) == EINVAL, off
    assert all(np.all(a == 7) for a in arrays.values())                       # nothing was written


def test_python_wrapper_has_compare():
    import loghisto_amd
    sig = inspect.signature(loghisto_amd.Kept.compare)
    assert list(sig.parameters) == ["self", "base", "nmetrics", "first", "earlier", "ids", "stream", "out"]
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default == 0
    assert sig.parameters["earlier"].default == () and sig.parameters["ids"].default is None
    assert sig.parameters["stream"].default is None and sig.parameters["out"].default is None
    # the reader's and the merge's signatures stay as their tests pin them
    assert list(inspect.signature(loghisto_amd.Kept.across).parameters)[:7] == ["self", "earlier", "percentiles", "nmetrics", "first",
                                                                                 "ids", "out"]
    assert list(inspect.signature(loghisto_amd.Kept.merge).parameters) == ["self", "earlier", "nmetrics", "first", "stream"]
