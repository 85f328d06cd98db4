"""Snapshot.top / movers / spread / compare / across and Kept.across / compare / count_le / spread: what the wrapper itself
decides about `by`, `arg`, `ids` and `out=` -- every ValueError with its message, raised before the library is entered, the
library call a well-formed `out=` turns into, and what the host form returns and derives.

No GPU and no liblhgpu.so: the Snapshot stands over a stand-in engine and a fake handle, a Kept over a fake handle and a
table, the library is a recorder, and objects with data_ptr / is_cuda / element_size / numel / is_contiguous play the device
tensors."""
import numpy as np
import pytest

from loghisto_amd import _native as N
from loghisto_amd import engine as E

M = 6                                             # nmetrics, always passed


class Tensor:
    """What the wrapper asks of a torch tensor."""

    def __init__(self, width, n, cuda=True, contiguous=True, addr=0x7000):
        self.width, self.n, self.is_cuda, self.contiguous, self.addr = width, n, cuda, contiguous, addr

    def data_ptr(self):
        return self.addr

    def element_size(self):
        return self.width

    def numel(self):
        return self.n

    def is_contiguous(self):
        return self.contiguous


class Recorder:
    """Stands for liblhgpu.so: every function returns LH_OK and leaves its name and arguments in `calls`."""

    def __init__(self):
        self.calls = []
        self.peek = None                          # peek(name, args), called while "the library runs" -> an entry of `peeked`
        self.peeked = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if self.peek is not None:
                self.peeked.append(self.peek(name, args))
            return 0
        return fn


class StandInEngine:
    def num_metrics(self):
        raise AssertionError("nmetrics is passed explicitly")

    def codec_tables(self):
        raise AssertionError("no result is derived in these tests")


@pytest.fixture
def lib(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(N, "lib", lambda: rec)
    return rec


@pytest.fixture
def snap():
    return E.Snapshot(StandInEngine(), 0x1000)


@pytest.fixture
def base():
    return E.Snapshot(StandInEngine(), 0x2000)


def raises(lib, message, f, *args, **kw):
    with pytest.raises(ValueError) as ei:
        f(*args, **kw)
    assert str(ei.value) == message
    assert lib.calls == [], "the library was entered"


def handle(x):
    return getattr(x, "value", x)


# ---- the k leaders: top and movers ---------------------------------------------------------------------------------------
def leaders(snap, base):
    """(call(k, by, arg, out) of the method, its entry dtype, its by names, those that take an arg, its two functions, the
    leading handles)"""
    return [(lambda k, by, arg, out=None: snap.top(k, by, arg, False, M, 0, out), N.TOP_ENTRY,
             ["count", "sum", "percentile", "count_above"], ["percentile", "count_above"], "lh_top", [0x1000], "TOP_ENTRY"),
            (lambda k, by, arg, out=None: snap.movers(base, k, by, arg, False, M, 0, out), N.MOVER_ENTRY,
             ["ks", "w1", "shift", "percentile"], ["percentile"], "lh_movers", [0x2000, 0x1000], "MOVER_ENTRY")]


def test_leaders_by_and_arg(lib, snap, base):
    for call, _, names, with_arg, _, _, _ in leaders(snap, base):
        for by in ("", "Count", "median", None, 0):
            raises(lib, "by is one of " + ", ".join(names), call, 3, by, None)
        for by in with_arg:
            raises(lib, f"by={by!r} takes an arg", call, 3, by, None)
        raises(lib, "by is one of " + ", ".join(names), call, 3, "nope", None, out=(Tensor(1, 0), Tensor(4, 0)))   # by first


def test_leaders_device_pair(lib, snap, base):
    msg = "device form: entries holds k * 32 contiguous bytes and n 4"
    for call, _, names, _, fn, handles, _ in leaders(snap, base):
        k = 5
        for ent, n in ((Tensor(1, k * 32 - 1), Tensor(4, 1)), (Tensor(8, k * 4 - 1), Tensor(4, 1)), (Tensor(1, k * 32), Tensor(1, 3)),
                       (Tensor(1, k * 32), Tensor(4, 0)), (Tensor(1, k * 32, contiguous=False), Tensor(4, 1)),
                       (Tensor(1, k * 32), Tensor(4, 1, contiguous=False))):
            raises(lib, msg, call, k, names[0], None, out=(ent, n))
        pair = (Tensor(8, k * 4, addr=0x7100), Tensor(4, 2, addr=0x7200))                  # larger than needed is fine
        assert call(k, names[1], None, out=pair) is pair
        (name, args), = lib.calls
        assert name == fn + "_device"
        assert [handle(a) for a in args] == handles + [0, M, 1, 0.0, k, 0, 0x7100, 0x7200]
        del lib.calls[:]


def test_leaders_host_out(lib, snap, base):
    for call, dt, names, with_arg, fn, handles, dtname in leaders(snap, base):
        msg = f"out holds at least k contiguous {dtname} elements"
        k = 4
        other = N.MOVER_ENTRY if dt is N.TOP_ENTRY else N.TOP_ENTRY
        for out in (np.zeros(k - 1, dtype=dt), np.zeros(k, dtype=other), np.zeros(k * 32, dtype=np.uint8), np.zeros(2 * k, dtype=dt)[::2],
                    [0] * k, Tensor(32, k, cuda=False)):
            raises(lib, msg, call, k, names[0], None, out=out)
        out = np.zeros(k + 1, dtype=dt)
        got = call(k, with_arg[0], 0.5, out=out)
        assert got.dtype == dt and got.shape == (0,) and got.base is out                    # (the recorder's n_out: 0)
        (name, args), = lib.calls
        assert name == fn
        assert [handle(a) for a in args[:-1]] == handles + [0, M, names.index(with_arg[0]), 0.5, k, 0, out.ctypes.data]
        del lib.calls[:]
        got = call(k, names[0], None)                                                       # the default array
        assert got.dtype == dt and got.shape == (0,) and lib.calls[0][0] == fn
        del lib.calls[:]


def test_leaders_ascending_flag(lib, snap, base):
    snap.top(2, "count", None, True, M)
    snap.movers(base, 2, "ks", None, True, M)
    assert [(name, args[-3]) for name, args in lib.calls] == [("lh_top", N.TOP_ASCENDING), ("lh_movers", N.MOVERS_ASCENDING)]


# ---- a dict of per-name output arrays: spread and compare ---------------------------------------------------------------
SPREAD = (("count", 8, 0), ("sum", 8, 0), ("m2", 8, 0), ("pkeys", 2, 1), ("pvalid", 1, 1), ("count_le", 8, 1), ("sum_le", 8, 1))
COMPARE = (("count_a", 8), ("count_b", 8), ("ks", 8), ("key", 2), ("below_a", 8), ("below_b", 8), ("w1", 8), ("shift", 8))
PCTS = [0.5, 0.9, 0.99]


def dicts(snap, base):
    """(call(out), (key, width, elements) per output, the message for a bad set of keys)"""
    return [(lambda out: snap.spread(PCTS, M, 0, out), [(k, w, M * len(PCTS) if per_p else M) for k, w, per_p in SPREAD],
             "out holds some of count, sum, m2, pkeys, pvalid, count_le, sum_le"),
            (lambda out: snap.compare(base, M, 0, out), [(k, w, M) for k, w in COMPARE],
             "out holds some of count_a, count_b, ks, key, below_a, below_b, w1, shift")]


def test_dict_keys(lib, snap, base):
    for call, outs, msg in dicts(snap, base):
        k0, w0, n0 = outs[0]
        good = np.zeros(n0, dtype=np.uint64)
        for out in ({}, {"nope": good}, {k0: good, "std": good}, {k0: good, "ks_value": good}, {k0.upper(): good}):
            raises(lib, msg, call, out)
    raises(lib, dicts(snap, base)[0][2], snap.spread, PCTS, M, 0, {"key": np.zeros(M, dtype=np.int16)})     # the other's key
    raises(lib, dicts(snap, base)[1][2], snap.compare, base, M, 0, {"count": np.zeros(M, dtype=np.uint64)})


def test_dict_mix_of_device_and_host(lib, snap, base):
    msg = "out holds device tensors or host arrays, not both"
    for call, outs, _ in dicts(snap, base):
        (k0, w0, n0), (k1, w1, n1) = outs[0], outs[3]
        raises(lib, msg, call, {k0: Tensor(w0, n0), k1: np.zeros(n1, dtype=np.int16)})
        raises(lib, msg, call, {k0: np.zeros(n0, dtype=np.uint64), k1: Tensor(w1, n1)})
        raises(lib, msg, call, {k0: Tensor(w0, n0), k1: Tensor(w1, n1, cuda=False)})         # a host tensor is a host array
        raises(lib, msg, call, {k0: Tensor(w0, n0), k1: None})
        raises(lib, msg, call, {k0: Tensor(1, 1), k1: np.zeros(1)})                          # before any array is measured


def test_dict_width_size_contiguity(lib, snap, base):
    np_of = {1: np.uint8, 2: np.int16, 8: np.uint64}
    for call, outs, _ in dicts(snap, base):
        for k, w, n in outs:
            msg = f"out[{k!r}] holds {n} contiguous elements of {w} bytes"
            wrong = 4 if w != 4 else 8
            for cuda in (True, False):
                for t in (Tensor(wrong, n, cuda), Tensor(w, n - 1, cuda), Tensor(w, n + 1, cuda), Tensor(w, n, cuda, contiguous=False)):
                    raises(lib, msg, call, {k: t})
            for a in (np.zeros(n, dtype=np.uint32), np.zeros(n - 1, dtype=np_of[w]), np.zeros(n + 1, dtype=np_of[w]),
                      np.zeros(2 * n, dtype=np_of[w])[::2], [0] * n, bytearray(n * w)):
                raises(lib, msg, call, {k: a})
        # the first bad array, in the order of the outputs, is the one named
        (k0, w0, n0), (k3, w3, n3) = outs[0], outs[3]
        raises(lib, f"out[{k0!r}] holds {n0} contiguous elements of {w0} bytes", call, {k3: Tensor(w3, 1), k0: Tensor(w0, 1)})


def test_spread_without_percentiles_measures_the_moments_only(lib, snap):
    """np == 0: the per-percentile arrays are not measured (they are not computed), the others are."""
    raises(lib, f"out['sum'] holds {M} contiguous elements of 8 bytes", snap.spread, [], M, 0, {"sum": Tensor(8, M - 1), "pkeys": Tensor(4, 99)})
    out = {"count": Tensor(8, M, addr=0x7100), "pkeys": Tensor(4, 99, addr=0x7200)}
    assert snap.spread([], M, 0, out) == out
    (name, args), = lib.calls
    assert name == "lh_spread_device" and list(args[4:]) == [0, 0x7100, 0, 0, 0x7200, 0, 0, 0]


def test_dict_device_form_reaches_the_library(lib, snap, base):
    for (call, outs, _), fn, lead in zip(dicts(snap, base), ("lh_spread_device", "lh_compare_device"), (5, 5)):
        out = {k: Tensor(w, n, addr=0x7000 + 0x100 * i) for i, (k, w, n) in enumerate(outs) if i % 2 == 0}
        got = call(out)
        assert got == out and got is not out
        (name, args), = lib.calls
        assert name == fn
        assert list(args[lead:]) == [0x7000 + 0x100 * i if i % 2 == 0 else 0 for i in range(len(outs))]
        del lib.calls[:]
    snap.spread(PCTS, M, 0, {"m2": Tensor(8, M)})
    snap.compare(base, M, 0, {"w1": Tensor(8, M)})
    (_, spread_args), (_, compare_args) = lib.calls
    assert [handle(a) for a in spread_args[:3]] == [0x1000, 0, M] and spread_args[4] == len(PCTS)
    assert [handle(a) for a in compare_args[:5]] == [0x2000, 0x1000, 0, M, 0]


def test_dict_host_form_reaches_the_library(lib, snap, base):
    out = {"count": np.zeros(M, dtype=np.uint64), "sum_le": np.zeros((M, len(PCTS)))}
    res = snap.spread(PCTS, M, 0, out)
    assert set(res) == {"count", "sum_le"} and res["sum_le"].shape == (M, len(PCTS))
    (name, args), = lib.calls
    assert name == "lh_spread" and list(args[5:]) == [out["count"].ctypes.data, 0, 0, 0, 0, 0, out["sum_le"].ctypes.data]
    del lib.calls[:]
    out = {"w1": np.zeros(M), "below_b": np.zeros(M, dtype=np.uint64)}
    res = snap.compare(base, M, 0, out)
    assert set(res) == {"w1", "below_b"} and res["w1"].shape == (M,)
    (name, args), = lib.calls
    assert name == "lh_compare" and list(args[5:]) == [0, 0, 0, 0, 0, out["below_b"].ctypes.data, out["w1"].ctypes.data, 0]


# ---- the same protocol over a list: across / across_ids / spread_ids of a Snapshot, across / compare / count_le / spread of a Kept --
import ctypes as C  # noqa: E402

ACROSS = (("count", 8, 0), ("sum", 8, 0), ("nbuckets", 4, 0), ("present_bits", 4, 0), ("pkeys", 2, 1), ("pvalid", 1, 1))
KEPT_ACROSS = (("count", 8, 0), ("sum", 8, 0), ("nbuckets", 4, 0), ("present_bits", 8, 0), ("pkeys", 2, 1), ("pvalid", 1, 1))
COUNT_LE = (("cum", 8, 1), ("total", 8, 0))       # (cum: an element per bound)
BOUNDS = [1.0, 10.0, 100.0]                        # as many as PCTS: one `per` for every reader
NP = len(PCTS)
STREAM = 0x5000
IDS = [4, 0, 4, 2, 1, 5]                           # M of them, one repeated
NP_OF = {1: np.uint8, 2: np.int16, 4: np.uint32, 8: np.uint64}
MSG_NO_OUT = "device ids go with an out= of device tensors"
MSG_SIDES = "ids and out are both on the device or both on the host"


class Case:
    """One reader: call(out, nearlier=0, ids=None, pcts=PCTS) calls it; fn: the library call of its host form without ids;
    spec: (key, width, per percentile / bound?) in library order; handles(nearlier): the handle lists the call hands over;
    tail(np): the arguments between the rows and the outputs, addresses left out; ids: the `_ids` form exists."""

    def __init__(self, name, call, fn, spec, handles, tail, lists=1, ids=True, rows=True):
        self.name, self.call, self.fn, self.spec, self.handles, self.tail, self.lists, self.ids, self.rows = \
            name, call, fn, spec, handles, tail, lists, ids, rows

    def outs(self, np_=NP):
        return [(k, w, M * np_ if per else M) for k, w, per in self.spec]

    def some_of(self):
        return "out holds some of " + ", ".join(k for k, _, _ in self.spec)


def kept_handle(lib, h):
    k = E.Kept(C.c_void_p(h), np.arange(N.NKEYS, dtype=np.float64))
    assert [name for name, _ in lib.calls] == ["lh_kept_info_get"] and k.info["first"] == 0 and k.info["nrows"] == 0
    del lib.calls[:]
    return k


@pytest.fixture
def cases(lib, snap):
    earlier = [E.Snapshot(StandInEngine(), 0x1100 + i) for i in range(2)]
    kept = kept_handle(lib, 0x3000)
    kearlier = [kept_handle(lib, 0x3100 + i) for i in range(2)]
    kbase = [kept_handle(lib, 0x3200 + i) for i in range(5)]
    snap.engine._decompress_table = np.arange(N.NKEYS, dtype=np.float64)   # (fetched already: codec_tables is not asked)
    sh = lambda n: [[0x1100 + i for i in range(n)] + [0x1000]]
    kh = lambda n: [[0x3100 + i for i in range(n)] + [0x3000]]
    return [
        Case("Snapshot.across", lambda out, n=0, ids=None, pcts=PCTS: snap.across(earlier[:n], pcts, M, 0, out),
             "lh_across", ACROSS, sh, lambda np_: [np_, 0], ids=False),
        Case("Snapshot.across_ids", lambda out, n=0, ids=IDS, pcts=PCTS: snap.across_ids(ids, earlier[:n], pcts, out),
             "lh_across", ACROSS, sh, lambda np_: [np_, 0], rows=False),
        Case("Snapshot.spread_ids", lambda out, n=0, ids=IDS, pcts=PCTS: snap.spread_ids(ids, pcts, out),
             "lh_spread", SPREAD, lambda n: [], lambda np_: [np_], lists=0, rows=False),
        Case("Kept.across", lambda out, n=0, ids=None, pcts=PCTS: kept.across(kearlier[:n], pcts, M, 0, ids, out, STREAM),
             "lh_kept_across", KEPT_ACROSS, kh, lambda np_: [np_, 0, STREAM]),
        Case("Kept.compare", lambda out, n=0, ids=None, pcts=PCTS: kept.compare(kbase[:2 * n + 1] if n else kbase[0], M, 0, kearlier[:n], ids, STREAM, out),
             "lh_kept_compare", tuple((k, w, 0) for k, w in COMPARE), lambda n: [[0x3200 + i for i in range(2 * n + 1)]] + kh(n),
             lambda np_: [0, STREAM], lists=2),
        Case("Kept.count_le", lambda out, n=0, ids=None, pcts=BOUNDS: kept.count_le(pcts, kearlier[:n], M, 0, ids, out, STREAM),
             "lh_kept_count_le", COUNT_LE, kh, lambda np_: [np_, 0, STREAM]),
        Case("Kept.spread", lambda out, n=0, ids=None, pcts=PCTS: kept.spread(pcts, kearlier[:n], M, 0, ids, out, STREAM),
             "lh_kept_spread", SPREAD, kh, lambda np_: [np_, 0, STREAM]),
    ]


def peek(case, np_=NP):
    """What the addresses among the leading arguments point to WHILE the library runs: the handle lists, the ids, the
    percentiles / bounds."""
    def look(name, args):
        a, seen = list(args), dict(lists=[])
        snapshot_first = case.lists == 0
        if snapshot_first:
            seen["handle"] = handle(a.pop(0))
        for _ in range(case.lists):
            addr, n = a.pop(0), a.pop(0)
            seen["lists"].append([x or 0 for x in (C.c_void_p * n).from_address(addr)])
        if "_ids" in name:
            addr, n = a.pop(0), a.pop(0)
            seen["rows"] = ("ids", addr if "_device" in name else list((C.c_uint32 * n).from_address(addr)), n)
        else:
            seen["rows"] = (a.pop(0), a.pop(0))
        if case.name != "Kept.compare":
            addr = a.pop(0)
            seen["values"] = list((C.c_double * np_).from_address(addr)) if np_ else []
        seen["rest"] = a
        return seen
    return look


def one_call(lib, case, fn, nearlier, ids, np_=NP):
    """The one call the library saw, checked up to its outputs; returns those."""
    (name, _), = lib.calls
    seen, = lib.peeked
    del lib.calls[:], lib.peeked[:]
    assert name == fn
    if case.lists == 0:
        assert seen["handle"] == 0x1000
    assert seen["lists"] == case.handles(nearlier)
    if ids is None:
        assert seen["rows"] == (0, M)
    elif isinstance(ids, Tensor):
        assert seen["rows"] == ("ids", ids.addr, M)
    else:
        assert seen["rows"] == ("ids", IDS, M)
    if case.name != "Kept.compare":
        assert seen["values"] == ([] if not np_ else BOUNDS if case.name == "Kept.count_le" else PCTS)
    tail = case.tail(np_)
    assert seen["rest"][:len(tail)] == tail and len(seen["rest"]) == len(tail) + len(case.spec)
    return seen["rest"][len(tail):]


def forms(case):
    """(ids of the call, the suffix of its library function) for the forms the reader has."""
    return ([(None, "")] if case.rows else []) + ([(IDS, "_ids")] if case.ids else [])


def test_list_dict_keys_and_mix(lib, cases):
    for c in cases:
        (k0, w0, n0), (k1, w1, n1) = c.outs()[0], c.outs()[1]
        good = np.zeros(n0, dtype=NP_OF[w0])
        for out in ({}, {"nope": good}, {k0: good, "avg": good}, {k0: good, "ks_value": good}, {k0.upper(): good}):
            raises(lib, c.some_of(), c.call, out)
        msg = "out holds device tensors or host arrays, not both"
        raises(lib, msg, c.call, {k0: Tensor(w0, n0), k1: np.zeros(n1, dtype=NP_OF[w1])})
        raises(lib, msg, c.call, {k0: np.zeros(n0, dtype=NP_OF[w0]), k1: Tensor(w1, n1)})
        raises(lib, msg, c.call, {k0: Tensor(w0, n0), k1: Tensor(w1, n1, cuda=False)})
        raises(lib, msg, c.call, {k0: Tensor(w0, n0), k1: None})
        raises(lib, msg, c.call, {k0: Tensor(1, 1), k1: np.zeros(1)})                        # before any array is measured
        raises(lib, c.some_of(), c.call, {"nope": Tensor(1, 1), k1: np.zeros(1)})            # the keys before the mix


def test_list_dict_width_size_contiguity(lib, cases):
    for c in cases:
        outs = c.outs()
        for k, w, n in outs:
            msg = f"out[{k!r}] holds {n} contiguous elements of {w} bytes"
            wrong = 4 if w != 4 else 8
            for cuda in (True, False):
                for t in (Tensor(wrong, n, cuda), Tensor(w, n - 1, cuda), Tensor(w, n + 1, cuda), Tensor(w, n, cuda, contiguous=False)):
                    raises(lib, msg, c.call, {k: t})
            for a in (np.zeros(n, dtype=NP_OF[wrong]), np.zeros(n - 1, dtype=NP_OF[w]), np.zeros(n + 1, dtype=NP_OF[w]),
                      np.zeros(2 * n, dtype=NP_OF[w])[::2], [0] * n, bytearray(n * w)):
                raises(lib, msg, c.call, {k: a})
        # the first bad array, in the order of the outputs, is the one named
        (k0, w0, n0), (kl, wl, nl) = outs[0], outs[-1]
        raises(lib, f"out[{k0!r}] holds {n0} contiguous elements of {w0} bytes", c.call, {kl: Tensor(wl, 1), k0: Tensor(w0, 1)})


def test_list_ids_and_out(lib, cases):
    for c in cases:
        if not c.ids:
            continue
        (k0, w0, n0) = c.outs()[0]
        dev_ids = Tensor(4, M, addr=0x7800)
        host = {k0: np.zeros(n0, dtype=NP_OF[w0])}
        raises(lib, MSG_NO_OUT, c.call, None, 0, dev_ids)
        raises(lib, MSG_SIDES, c.call, host, 0, dev_ids)
        raises(lib, MSG_SIDES, c.call, {k0: Tensor(w0, n0)}, 0, IDS)
        raises(lib, MSG_SIDES, c.call, {k0: Tensor(w0, n0)}, 0, np.array(IDS))
        for bad in (Tensor(8, M), Tensor(2, M), Tensor(4, M, contiguous=False)):
            raises(lib, "device ids are contiguous 4-byte elements", c.call, {k0: Tensor(w0, n0)}, 0, bad)
        for bad in ([0.5, 1.0], [-1, 2], [0, 1 << 32], ["a"]):
            raises(lib, "ids are unsigned 32-bit integers", c.call, host, 0, bad)
        # the ids are looked at first, then whether there is an out=, then out= itself, then the sides
        raises(lib, "device ids are contiguous 4-byte elements", c.call, None, 0, Tensor(8, M))
        raises(lib, MSG_NO_OUT, c.call, None, 0, dev_ids)
        raises(lib, c.some_of(), c.call, {"nope": host[k0]}, 0, dev_ids)
        raises(lib, f"out[{k0!r}] holds {n0} contiguous elements of {w0} bytes", c.call, {k0: np.zeros(n0 + 1, dtype=NP_OF[w0])}, 0, dev_ids)


def test_kept_count_le_bounds_are_one_row(lib, cases):
    c, = [c for c in cases if c.name == "Kept.count_le"]
    msg = "bounds over kept intervals are 1-D: one row shared by all names"
    for b in (np.zeros((M, 3)), np.zeros((1, 1, 1))):
        raises(lib, msg, c.call, None, 0, None, b)
        raises(lib, msg, c.call, {"nope": 0}, 0, Tensor(8, M), b)                            # ahead of the ids and of out=


def test_list_device_form_reaches_the_library(lib, cases):
    for c in cases:
        lib.peek = peek(c)
        for nearlier in (0, 2):                                                              # lists of 1 and 3 handles
            for ids, suffix in forms(c):
                if ids is not None:
                    ids = Tensor(4, M, addr=0x7800)
                out = {k: Tensor(w, n, addr=0x7000 + 0x100 * i) for i, (k, w, n) in reversed(list(enumerate(c.outs()))) if i % 2 == 0}
                got = c.call(out, nearlier, ids)
                assert got == out and got is not out and list(got) == list(out)
                ptrs = one_call(lib, c, c.fn + suffix + "_device", nearlier, ids)
                assert ptrs == [0x7000 + 0x100 * i if i % 2 == 0 else 0 for i in range(len(c.spec))]


def test_list_host_form_reaches_the_library(lib, cases):
    for c in cases:
        lib.peek = peek(c)
        for nearlier in (0, 2):
            for ids, suffix in forms(c):
                out = {k: np.zeros((M, NP) if per else M, dtype=NP_OF[w]) for k, w, per in reversed(c.spec[1:])}
                res = c.call(out, nearlier, ids)
                assert list(res)[:len(out)] == list(out)                                     # out's order; derived fields behind
                for k, w, per in c.spec[1:]:
                    assert res[k].shape == ((M, NP) if per else (M,)) and np.shares_memory(res[k], out[k])
                ptrs = one_call(lib, c, c.fn + suffix, nearlier, ids)
                assert ptrs == [0] + [out[k].ctypes.data for k, _, _ in c.spec[1:]]


def test_list_without_percentiles(lib, cases):
    """np == 0: the per-percentile arrays are neither measured nor returned; their addresses are handed over as they are."""
    for c in cases:
        if not any(per for _, _, per in c.spec) or c.name == "Kept.count_le":
            continue
        lib.peek = peek(c, 0)
        (k0, w0, _), (kp, wp, _) = c.spec[0], [s for s in c.spec if s[2]][0]
        ip = [k for k, _, _ in c.spec].index(kp)
        ids, suffix = forms(c)[-1]
        raises(lib, f"out[{k0!r}] holds {M} contiguous elements of {w0} bytes", c.call, {k0: Tensor(w0, M - 1), kp: Tensor(4, 99)}, 0, ids, [])
        out = {k0: Tensor(w0, M, addr=0x7100), kp: Tensor(4, 99, addr=0x7200)}
        assert c.call(out, 0, Tensor(4, M, addr=0x7800) if ids else None, []) == out
        ptrs = one_call(lib, c, c.fn + suffix + "_device", 0, Tensor(4, M, addr=0x7800) if ids else None, 0)
        assert ptrs == [0x7100 if i == 0 else 0x7200 if i == ip else 0 for i in range(len(c.spec))]
        out = {kp: np.zeros(5, dtype=np.float32), k0: np.zeros(M, dtype=NP_OF[w0])}
        res = c.call(out, 0, ids, [])
        assert list(res) == [k0] and res[k0].shape == (M,)
        ptrs = one_call(lib, c, c.fn + suffix, 0, ids, 0)
        assert ptrs == [out[k0].ctypes.data if i == 0 else out[kp].ctypes.data if i == ip else 0 for i in range(len(c.spec))]


def test_list_derived_fields(lib, cases):
    """What the host form derives from the arrays it was given (the recorder leaves them as they are), with decompress(bin) =
    bin for a table: avg / pvals, std / mean_le / upper, ks_value -- behind out's keys, in this order."""
    by = {c.name: c for c in cases}
    keys = np.array([[-32768, -1, 0], [1, 32767, 5]] * 3, dtype=np.int16)
    bins = (keys.astype(np.int64) & 0xffff) ^ 0x8000
    valid = np.array([[1, 0, 1]] * M, dtype=np.uint8)
    count = np.array([0, 1, 2, 3, 4, 5], dtype=np.uint64)
    total = np.arange(M, dtype=np.float64) * 3.0
    with np.errstate(all="ignore"):
        for name in ("Kept.across", "Snapshot.across", "Snapshot.across_ids"):
            res = by[name].call(dict(pvalid=valid, sum=total, pkeys=keys, count=count))
            assert list(res) == ["pvalid", "sum", "pkeys", "count", "avg", "pvals"]
            assert np.array_equal(res["avg"], total / count.astype(np.float64), equal_nan=True)
            assert np.array_equal(res["pvals"], np.where(valid != 0, bins.astype(np.float64), np.nan), equal_nan=True)
            assert list(by[name].call(dict(sum=total, pkeys=keys))) == ["sum", "pkeys"]
        per_p = np.arange(M * NP, dtype=np.float64).reshape(M, NP)
        count_le = np.arange(M * NP, dtype=np.uint64).reshape(M, NP)
        for name in ("Kept.spread", "Snapshot.spread_ids"):
            res = by[name].call(dict(m2=total, count=count, sum_le=per_p, count_le=count_le, pkeys=keys, pvalid=valid))
            assert list(res) == ["m2", "count", "sum_le", "count_le", "pkeys", "pvalid", "std", "mean_le", "upper"]
            assert np.array_equal(res["std"], np.sqrt(total / count.astype(np.float64)), equal_nan=True)
            assert np.array_equal(res["mean_le"], per_p / count_le.astype(np.float64), equal_nan=True)
            assert np.array_equal(res["upper"], np.where(valid != 0, bins.astype(np.float64), np.nan), equal_nan=True)
            assert list(by[name].call(dict(m2=total, sum_le=per_p, pkeys=keys))) == ["m2", "sum_le", "pkeys"]
        ks = np.array([0.0, np.nan, 0.5, np.nan, 1.0, 0.25])
        res = by["Kept.compare"].call(dict(key=keys[:, 0].copy(), ks=ks))
        assert list(res) == ["key", "ks", "ks_value"]
        assert np.array_equal(res["ks_value"], np.where(np.isnan(ks), np.nan, bins[:, 0].astype(np.float64)), equal_nan=True)
        res = by["Kept.compare"].call(dict(key=keys[:, 1].copy()))
        assert list(res) == ["key", "ks_value"] and np.array_equal(res["ks_value"], bins[:, 1].astype(np.float64))
        assert list(by["Kept.count_le"].call(dict(total=count, cum=count_le))) == ["total", "cum"]
