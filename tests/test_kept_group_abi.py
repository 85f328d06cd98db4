"""CPU tests of lh_kept_group / lh_kept_group_device (many kept rows summed into one row, by group): declared, exported, bound with
the header's prototypes, the ABI version unchanged, the three equivalences and the out-of-scope list in the header, and every
refusal the host decides before a handle is looked at -- the handle pointers below are fakes that are never dereferenced -- in the
documented order and with *out left as it was.  What needs a handle (the devices, the host form's members against the blocks) is in
tests/test_gpu_kept_group.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x77
NO_ROW = 0xffffffff
PROTOS = {
    "lh_kept_group": "lh_kept *const *kept, size_t nkept, const uint64_t *goff, const uint32_t *members, size_t nmembers, "
                     "size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out",
    "lh_kept_group_device": "lh_kept *const *kept, size_t nkept, const uint64_t *d_goff, const uint32_t *d_members, size_t nmembers, "
                            "size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out",
}
CTYPES = {"size_t": C.c_size_t, "uint32_t": C.c_uint32}
EQUIVALENCES = (
    "1. With ngroups singleton groups, goff[g] = g and members[g] = src[g]: the bytes are lh_kept_gather's for the list with that one "
    "map repeated for every handle. With members[g] = first + g, they are lh_kept_merge's.",
    "2. A call whose largest group has G members, with nkept x G <= LH_MAX_KEPT: the bytes are lh_kept_gather's for the list in which "
    "every handle stands G times. The copies are G consecutive entries per handle. Copy c is mapped to member c of each group. "
    "LH_KEPT_NO_ROW stands where the group is shorter.",
    "3. Any partition of every group's member list into pieces: the bytes are lh_kept_merge's over the handles that lh_kept_group "
    "gives for each piece.",
)
OUT_OF_SCOPE = ("spreading ONE group over several workgroups", "more than LH_MAX_KEPT handles a call",
                "readers over groups without materialising the handle", "a different member list per handle (gather first, then group)",
                "weights", "retuning the shape switch")


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
    # adding functions is backward compatible: no new version, limit or error code
    assert native_lib.lh_abi_version() == 7 and _native.ABI_VERSION == 7
    assert re.search(r"#define\s+LH_ABI_VERSION\s+7\b", src)
    assert re.search(r"#define\s+LH_MAX_KEPT\s+64\b", src) and _native.MAX_KEPT == 64


def test_the_definition_stands_in_the_header_in_its_own_words():
    text = re.sub(r"\s+\*?\s*", " ", _read("loghisto_gpu.h"))
    at = text.index("lh_kept_group* MANY KEPT ROWS SUMMED INTO ONE ROW, BY GROUP")
    para = text[at:text.index("typedef struct lh_kept lh_kept;", at)]
    for sentence in EQUIVALENCES:
        assert sentence in para, sentence
    scope = para[para.index("OUT OF SCOPE:"):]
    for item in OUT_OF_SCOPE:
        assert item in scope, item
    assert "many-to-one roll-ups of names within one handle" in para[:para.index("THREE EQUIVALENCES")]   # where gather's item went
    assert "contributes nothing for handle i alone" in para and "members may be NULL only with nmembers == 0" in para
    # lh_kept_gather*'s own paragraph is word for word what it was
    assert ("more than LH_MAX_KEPT handles a call (gather in groups, then lh_kept_merge); many-to-one roll-ups of names within one "
            "handle; names inside the blob") in text[:at]


def test_every_early_error_is_decided_on_the_host_and_out_is_untouched(native_lib):
    from loghisto_amd import _native
    EINVAL, ERANGE = _native.EINVAL, _native.ERANGE
    VP = C.c_void_p
    out = VP(SENTINEL)
    BIG = 1 << 32
    NG = 4
    goff = np.array([0, 1, 1, 3, 4] + [4] * 8, dtype=np.uint64)               # a sound CSR of 4 groups over 4 members (and slack)
    members = np.full(16, NO_ROW, dtype=np.uint32)
    gp, mp = goff.ctypes.data, members.ctypes.data

    def handles(*addrs):
        return (VP * len(addrs))(*addrs)

    one, two = handles(0x1000), handles(0x1000, 0x2000)
    full = handles(*[0x1000 * (i + 1) for i in range(64)])
    too_many = handles(*[0x1000 * (i + 1) for i in range(65)])
    holes = [handles(None), handles(None, 0x2000), handles(0x1000, None), handles(*([0x1000] * 63 + [None])),
             handles(*([0x1000] * 31 + [None] + [0x1000] * 32))]
    odd = (C.c_char * 64)()                                                   # for a list of pointers off its alignment

    for fn in (native_lib.lh_kept_group, native_lib.lh_kept_group_device):
        host = fn is native_lib.lh_kept_group

        def call(h, nkept, ngroups=NG, nmembers=4, flags=0, first_out=0, goff_=gp, members_=mp, out_=None, stream=None):
            return fn(h, nkept, goff_, members_, nmembers, ngroups, first_out, flags, stream, C.byref(out) if out_ is None else out_)

        # each cause of LH_EINVAL wins over the early LH_ERANGE (ngroups, first_out + ngroups, nmembers)
        for ng, first_out, nm in ((NG, 0, 4), (BIG, 0, 4), (NG, 0xfffffffd, 4), (NG, 0, BIG)):
            kw = dict(ngroups=ng, first_out=first_out, nmembers=nm)
            assert call(None, 1, **kw) == EINVAL                              # NULL list
            assert call(None, 0, **kw) == EINVAL
            for h in holes:                                                   # a NULL entry, wherever
                assert call(h, len(h), **kw) == EINVAL
            for off in range(1, C.sizeof(VP)):                                # the list itself off its alignment
                assert fn(C.addressof(odd) + off, 1, gp, mp, nm, ng, first_out, 0, None, C.byref(out)) == EINVAL, off
            assert call(one, 0, **kw) == EINVAL                               # nkept 0
            assert call(too_many, 65, **kw) == EINVAL                         # nkept too large
            assert call(full, (1 << 64) - 1, **kw) == EINVAL
            for s, k in ((one, 1), (two, 2), (full, 64)):
                assert call(s, k, goff_=None, **kw) == EINVAL                 # NULL goff
                assert call(s, k, members_=None, **kw) == EINVAL              # NULL members with nmembers > 0
                for off in range(1, 8):                                       # goff off its alignment
                    assert call(s, k, goff_=gp + off, **kw) == EINVAL, off
                for off in (1, 2, 3):                                         # members off its alignment
                    assert call(s, k, members_=mp + off, **kw) == EINVAL, off
                for flags in (1, 2, 0x80000000):                              # flags must be 0
                    assert call(s, k, flags=flags, **kw) == EINVAL, flags
                assert fn(s, k, gp, mp, nm, ng, first_out, 0, None, None) == EINVAL   # NULL out
        for s, k in ((one, 1), (two, 2), (full, 64)):
            assert call(s, k, ngroups=0) == EINVAL                            # ngroups == 0
            assert call(s, k, ngroups=0, first_out=5, nmembers=0, members_=None) == EINVAL
            # more rows than a handle can have, rows that end beyond 2^32, more members than row numbers: LH_ERANGE, decided
            # before a handle is looked at -- and, in the host form, before goff is read (its first entries would refuse these)
            assert call(s, k, ngroups=BIG) == ERANGE
            assert call(s, k, ngroups=(1 << 64) - 1) == ERANGE
            assert call(s, k, ngroups=0xffffffff, first_out=2) == ERANGE
            assert call(s, k, first_out=0xfffffffd) == ERANGE                 # first_out + ngroups == 2^32 + 1
            assert call(s, k, ngroups=2, first_out=0xffffffff) == ERANGE
            assert call(s, k, nmembers=BIG) == ERANGE
            assert call(s, k, nmembers=(1 << 64) - 1) == ERANGE
            assert call(s, k, ngroups=BIG, stream=0x10) == ERANGE             # ... whatever the stream
    assert out.value == SENTINEL                                              # through every failure
    assert np.all(members == NO_ROW) and goff[:5].tolist() == [0, 1, 1, 3, 4]


def test_the_host_form_holds_goff_to_a_csr_before_a_handle_is_looked_at(native_lib):
    from loghisto_amd import _native
    EINVAL = _native.EINVAL
    VP = C.c_void_p
    out = VP(SENTINEL)
    members = np.full(8, NO_ROW, dtype=np.uint32)
    fakes = [(VP * k)(*[0x1000 * (i + 1) for i in range(k)]) for k in (1, 2, 64)]

    def call(h, goff, nmembers, members_=members.ctypes.data, first_out=0):
        g = np.array(goff, dtype=np.uint64)
        return native_lib.lh_kept_group(h, len(h), g.ctypes.data, members_, nmembers, len(goff) - 1, first_out, 0, None, C.byref(out))

    for h in fakes:
        assert call(h, [1, 2, 4], 4) == EINVAL                                # the first entry is not 0
        assert call(h, [1, 1], 1) == EINVAL
        assert call(h, [0, 3, 2, 4], 4) == EINVAL                             # a decrease
        assert call(h, [0, 4, 0, 4], 4) == EINVAL
        assert call(h, [0, 2, 3], 4) == EINVAL                                # the last entry is not nmembers: short,
        assert call(h, [0, 2, 5], 4) == EINVAL                                # long,
        assert call(h, [0, (1 << 64) - 1], 4) == EINVAL                       # far beyond
        assert call(h, [0, 0, 0], 4) == EINVAL
        # members == NULL goes with nmembers == 0 only: non-empty groups over no members are refused by goff's last entry
        assert call(h, [0, 1, 2], 0, members_=None) == EINVAL
        assert call(h, [0, 0, 1], 0, members_=None) == EINVAL
        assert call(h, [0, 2], 2, members_=None) == EINVAL                    # (and NULL members with nmembers > 0 by the first check)
        assert call(h, [0, 2, 3], 4, first_out=0xffffffff) == _native.ERANGE  # the early LH_ERANGE comes before goff is read
    assert out.value == SENTINEL
    assert np.all(members == NO_ROW)


def test_python_wrapper_has_group_and_the_fleet_functions():
    import loghisto_amd
    from loghisto_amd import fleet, keptfile
    sig = inspect.signature(loghisto_amd.Kept.group)
    assert list(sig.parameters) == ["self", "groups", "earlier", "first", "stream"]
    assert sig.parameters["earlier"].default == () and sig.parameters["first"].default == 0 and sig.parameters["stream"].default is None
    assert loghisto_amd.group_names is fleet.group_names and loghisto_amd.roll_up is fleet.roll_up
    assert {"group_names", "roll_up", "union_names", "aggregate"} <= set(loghisto_amd.__all__)
    assert list(inspect.signature(fleet.group_names).parameters) == ["names", "key", "first"]
    assert list(inspect.signature(fleet.roll_up).parameters) == ["kepts", "names", "key", "stream"]
    assert list(inspect.signature(keptfile.group).parameters) == ["blobs", "goff", "members", "first_out", "checked"]
    # gather's signature stays as tests/test_kept_gather_abi.py pins it
    assert list(inspect.signature(loghisto_amd.Kept.gather).parameters) == ["self", "src", "earlier", "first", "stream"]
