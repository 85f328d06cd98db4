"""Snapshot.top / movers / spread / compare: what the wrapper itself decides about `by`, `arg` and `out=` -- every ValueError
with its message, raised before the library is entered, and the library call a well-formed `out=` turns into.

No GPU and no liblhgpu.so: the Snapshot stands over a stand-in engine and a fake handle, the library is a recorder, and
objects with data_ptr / is_cuda / element_size / numel / is_contiguous play the device tensors."""
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

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
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
