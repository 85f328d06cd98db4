"""CPU tests of lh_kept_merge (kept intervals rolled up into one kept handle): declared, exported, bound, and every error
the host decides before a handle is looked at -- the handle pointers below are fakes that are never dereferenced -- with
*out left as it was."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = 7
SENTINEL = 0x77


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)


def test_the_symbol_is_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = _header()
    decl = re.search(r"\bint\s+lh_kept_merge\s*\((.*?)\)\s*;", src, flags=re.S)
    assert decl, "lh_kept_merge is not declared"
    assert len(decl.group(1).split(",")) == NARGS, decl.group(1)
    assert re.sub(r"\s+", " ", decl.group(1)).strip() == ("lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, "
                                                          "uint32_t flags, void *stream, lh_kept **out")
    assert hasattr(C.CDLL(_native.LIB_PATH), "lh_kept_merge"), "lh_kept_merge is not exported"
    assert "lh_kept_merge" in _native.SIGNATURES and len(_native.SIGNATURES["lh_kept_merge"][1]) == NARGS
    assert native_lib.lh_kept_merge.restype is C.c_int
    # adding a function is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert C.sizeof(_native.LhKeptInfo) == 40


def test_every_early_error_is_decided_on_the_host_and_out_is_untouched(native_lib):
    from loghisto_amd import _native
    fn, EINVAL, ERANGE = native_lib.lh_kept_merge, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p
    out = VP(SENTINEL)

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    def call(h, nkept, nmetrics, flags=0, first=0, out_=None, stream=None):
        return fn(h, nkept, first, nmetrics, flags, stream, C.byref(out) if out_ is None else out_)

    one, two = handles(0x1000), handles(0x1000, 0x2000)
    full = handles(*[0x1000 * (i + 1) for i in range(64)])
    too_many = handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 63 + [None])),
             handles(*([0x1000] * 31 + [None] + [0x1000] * 32))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    BIG = 1 << 32

    for n in (1, BIG):                                                        # each cause of LH_EINVAL wins over the early LH_ERANGE
        assert call(None, 1, n) == EINVAL                                     # NULL list
        assert call(None, 0, n) == EINVAL
        for h in holes:                                                       # a NULL entry, wherever
            assert call(h, len(h), n) == EINVAL
        for off in range(1, C.sizeof(VP)):                                    # the list itself off its alignment
            assert fn(C.addressof(odd) + off, 1, 0, n, 0, None, C.byref(out)) == EINVAL, off
        assert call(one, 0, n) == EINVAL                                      # nkept 0
        assert call(too_many, 65, n) == EINVAL                                # nkept too large
        assert call(full, (1 << 64) - 1, n) == EINVAL
        for s, k in ((one, 1), (two, 2), (full, 64)):
            for flags in (1, 2, 0x80000000):                                  # flags must be 0
                assert call(s, k, n, flags) == EINVAL, flags
            assert fn(s, k, 0, n, 0, None, None) == EINVAL                    # NULL out
    for s, k in ((one, 1), (two, 2), (full, 64)):
        assert call(s, k, 0) == EINVAL                                        # nmetrics == 0, as lh_keep
        assert call(s, k, 0, first=5) == EINVAL
        # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
        assert call(s, k, BIG) == ERANGE
        assert call(s, k, BIG, first=0xffffffff) == ERANGE
        assert call(s, k, (1 << 64) - 1) == ERANGE
        assert call(s, k, BIG, stream=0x10) == ERANGE                         # ... whatever the stream
    assert out.value == SENTINEL                                              # through every failure


def test_python_wrapper_has_merge():
    import loghisto_amd
    sig = inspect.signature(loghisto_amd.Kept.merge)
    assert list(sig.parameters) == ["self", "earlier", "nmetrics", "first", "stream"]
    assert sig.parameters["earlier"].default == ()
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default is None
    assert sig.parameters["stream"].default is None
    # the reader's signature stays as tests/test_kept_abi.py pins it
    assert list(inspect.signature(loghisto_amd.Kept.across).parameters)[:7] == ["self", "earlier", "percentiles", "nmetrics", "first",
                                                                                 "ids", "out"]
