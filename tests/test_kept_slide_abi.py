"""CPU tests of lh_kept_slide (a rolling window of kept intervals advanced exactly): declared, exported, bound, and every
error the host decides before a handle is looked at -- the handle pointers below are fakes that are never dereferenced --
with *out and *why left byte for byte as they were."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = 10
SENTINEL = 0x77


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "loghisto_gpu.h")).read(), flags=re.S)


def test_the_symbol_is_declared_exported_and_bound(native_lib):
    from loghisto_amd import _native
    src = _header()
    decl = re.search(r"\bint\s+lh_kept_slide\s*\((.*?)\)\s*;", src, flags=re.S)
    assert decl, "lh_kept_slide is not declared"
    assert len(decl.group(1).split(",")) == NARGS, decl.group(1)
    assert re.sub(r"\s+", " ", decl.group(1)).strip() == ("lh_kept *const *add, size_t nadd, lh_kept *const *sub, size_t nsub, "
                                                          "uint32_t first, size_t nmetrics, uint32_t flags, void *stream, "
                                                          "lh_kept_under *why, lh_kept **out")
    struct = re.search(r"typedef\s+struct\s+lh_kept_under\s*\{(.*?)\}\s*lh_kept_under\s*;", src, flags=re.S)
    assert struct, "lh_kept_under is not declared"
    assert re.sub(r"\s+", " ", struct.group(1)).strip() == ("uint32_t struct_size; uint32_t row; int16_t key; uint16_t reserved0; "
                                                            "uint32_t reserved1;")
    assert hasattr(C.CDLL(_native.LIB_PATH), "lh_kept_slide"), "lh_kept_slide is not exported"
    assert "lh_kept_slide" in _native.SIGNATURES and len(_native.SIGNATURES["lh_kept_slide"][1]) == NARGS
    assert native_lib.lh_kept_slide.restype is C.c_int
    assert C.sizeof(_native.LhKeptUnder) == 16
    assert [(n, _native.LhKeptUnder.__dict__[n].offset) for n, _ in _native.LhKeptUnder._fields_] == [
        ("struct_size", 0), ("row", 4), ("key", 8), ("reserved0", 10), ("reserved1", 12)]
    # adding a function is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64
    assert C.sizeof(_native.LhKeptInfo) == 40


def test_every_early_error_is_decided_on_the_host_and_out_and_why_are_untouched(native_lib):
    from loghisto_amd import _native
    fn, EINVAL, ERANGE = native_lib.lh_kept_slide, _native.EINVAL, _native.ERANGE
    VP = C.c_void_p
    out = VP(SENTINEL)
    why = _native.LhKeptUnder(struct_size=16, row=0x11223344, key=-77, reserved0=0x5566, reserved1=0x778899aa)
    why_was = bytes(why)
    wrong = [_native.LhKeptUnder(struct_size=s, row=0x11223344, key=-77, reserved0=0x5566, reserved1=0x778899aa)
             for s in (0, 12, 15, 17, 32, 0xffffffff)]
    wrong_was = [bytes(w) for w in wrong]

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    def fake(n, base=0x1000):
        return handles(*[base * (i + 1) for i in range(n)])

    def call(add, nadd, sub, nsub, nmetrics, flags=0, first=0, out_=True, stream=None, why_=why):
        return fn(add, nadd, sub, nsub, first, nmetrics, flags, stream, C.byref(why_) if why_ is not None else None,
                  C.byref(out) if out_ else None)

    one, two, full = fake(1), fake(2), fake(64)
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 63 + [None])),
             handles(*([0x1000] * 31 + [None] + [0x1000] * 32))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment
    BIG = 1 << 32
    HUGE = (1 << 64) - 1
    lists = ((one, 1, None, 0), (one, 1, one, 1), (two, 2, one, 1), (fake(32), 32, fake(32), 32), (full, 64, None, 0),
             (one, 1, fake(63), 63))

    for n in (1, BIG):                                                        # each cause of LH_EINVAL wins over the early LH_ERANGE
        for sub, nsub in ((None, 0), (one, 1)):
            assert call(None, 1, sub, nsub, n) == EINVAL                      # NULL add
            assert call(None, 0, sub, nsub, n) == EINVAL
            assert call(one, 0, sub, nsub, n) == EINVAL                       # nadd 0
            for off in range(1, C.sizeof(VP)):                                # add off its alignment
                assert call(C.addressof(odd) + off, 1, sub, nsub, n) == EINVAL, off
            for h in holes:                                                   # a NULL entry, wherever, in add ...
                assert call(h, len(h), sub, nsub, n) == EINVAL
        assert call(one, 1, None, 1, n) == EINVAL                             # sub NULL with nsub > 0
        assert call(one, 1, None, HUGE, n) == EINVAL
        for off in range(1, C.sizeof(VP)):                                    # sub off its alignment
            assert call(one, 1, C.addressof(odd) + off, 1, n) == EINVAL, off
        for h in holes:                                                       # ... and in sub
            if len(h) < 64:
                assert call(one, 1, h, len(h), n) == EINVAL
        for nadd, nsub in ((1, 64), (64, 1), (33, 32), (65, 0), (64, 64)):    # 65 handles together, however split
            assert call(fake(nadd), nadd, fake(max(nsub, 1)), nsub, n) == EINVAL, (nadd, nsub)
        assert call(one, 1, full, HUGE, n) == EINVAL                          # no overflow in nadd + nsub
        assert call(full, HUGE, one, 1, n) == EINVAL
        assert call(full, HUGE, full, HUGE, n) == EINVAL
        assert call(full, 64, full, HUGE - 63, n) == EINVAL                   # (the sum wraps to 0)
        assert call(two, 2, full, HUGE - 1, n) == EINVAL                      # (... and to 1)
        for add, nadd, sub, nsub in lists:
            for flags in (1, 2, 0x80000000):                                  # flags must be 0
                assert call(add, nadd, sub, nsub, n, flags) == EINVAL, flags
            assert call(add, nadd, sub, nsub, n, out_=False) == EINVAL        # NULL out
            for w in wrong:                                                   # a why of another size
                assert call(add, nadd, sub, nsub, n, why_=w) == EINVAL, w.struct_size
    for add, nadd, sub, nsub in lists:
        for w in (why, None):
            assert call(add, nadd, sub, nsub, 0, why_=w) == EINVAL            # nmetrics == 0, as lh_kept_merge
            assert call(add, nadd, sub, nsub, 0, first=5, why_=w) == EINVAL
            # more rows than any engine can have: LH_ERANGE, decided before a handle is looked at
            assert call(add, nadd, sub, nsub, BIG, why_=w) == ERANGE
            assert call(add, nadd, sub, nsub, BIG, first=0xffffffff, why_=w) == ERANGE
            assert call(add, nadd, sub, nsub, HUGE, why_=w) == ERANGE
            assert call(add, nadd, sub, nsub, BIG, stream=0x10, why_=w) == ERANGE   # ... whatever the stream
    assert out.value == SENTINEL                                              # through every failure
    assert bytes(why) == why_was and [bytes(w) for w in wrong] == wrong_was


def test_python_wrappers():
    import loghisto_amd
    from loghisto_amd import keptfile
    sig = inspect.signature(loghisto_amd.Kept.slide)
    assert list(sig.parameters) == ["self", "add", "sub", "nmetrics", "first", "stream"]
    assert sig.parameters["add"].default == () and sig.parameters["sub"].default == ()
    assert sig.parameters["nmetrics"].default is None and sig.parameters["first"].default is None
    assert sig.parameters["stream"].default is None
    assert loghisto_amd.KeptUnderflow is keptfile.KeptUnderflow
    e = loghisto_amd.KeptUnderflow(7, -3)
    assert (e.row, e.key) == (7, -3)
    assert list(inspect.signature(loghisto_amd.KeptWindow).parameters) == ["size"]
    assert list(inspect.signature(loghisto_amd.KeptWindow.push).parameters) == ["self", "kept"]
    assert list(inspect.signature(loghisto_amd.KeptWindow.close).parameters) == ["self"]
    w = loghisto_amd.KeptWindow(4)
    assert w.total is None and list(w.handles) == [] and w.size == 4
    w.close()
    # merge's signature stays as tests/test_kept_merge_abi.py pins it
    assert list(inspect.signature(loghisto_amd.Kept.merge).parameters) == ["self", "earlier", "nmetrics", "first", "stream"]
