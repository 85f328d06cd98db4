"""lh_spread / lh_spread_device (Snapshot.spread): per name the count, the sum, the centred second moment, and per
percentile the key percentile() selects (metrics.go:406-418) with the count and the sum of the weighted walk
(metrics.go:342-346) up to and including that bucket.

What is required of every result, on engines of 64- and 32-bit cells and under both kernel shapes (lh_tool_spread_switch):
  count, count_le, pkeys, pvalid   integer-exact against oracle.process_dense and the running count over the oracle's rows,
                                   and equal to lh_extract_rows on the same snapshot
  sum, sum_le                      within 1e-12 * sum |terms| of the exact value (the project's _sum rule)
  m2                               within 1e-12 * M2 + 2 * (1e-12 * A)^2 / count of the exact centred moment about the exact
                                   mean, A = sum c |D|: sum c (D - mu')^2 = M2 + count (mu' - mu)^2 and
                                   |mu' - mu| <= 1e-12 A / count by the _sum rule
The exact values are rational arithmetic over oracle.decompress_table(): every double is an integer multiple of 2^-1100, so
the sums are accumulated as Python integers in that unit and compared as fractions.Fraction."""
import contextlib
import ctypes as C
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_count_le import engine, host_arrays, small_stream, stream

pytestmark = pytest.mark.gpu

U64 = np.uint64
SHIFT = 1100
SCALE = 1 << SHIFT
REL = Fraction(1, 10 ** 12)
P_DEFAULT = list(oracle.DEFAULT_PERCENTILES.values())
P_LISTS = {"default": P_DEFAULT, "unsorted_repeat": [0.99, 0.5, 0.999, 0.5, 0.1, 0.75], "ends": [0.0, 1.0],
           "invalid": [1.5, float("nan"), 0.5], "none": []}
SHAPES = {"wave": 1, "block": 1 << 30}
BITS = (64, 32)

_D = {}


def dtable():
    if "f" not in _D:
        d = oracle.decompress_table()
        _D["f"] = d
        _D["i"] = [None] * oracle.NKEYS          # the entries in units of 2^-1100, on demand
    return _D["f"]


def d_int(b):
    dtable()
    if _D["i"][b] is None:
        f = Fraction(float(_D["f"][b])) * SCALE
        assert f.denominator == 1
        _D["i"][b] = f.numerator
    return _D["i"][b]


class Exact:
    """One row {bin: count} in exact arithmetic: running counts, running sums and running sums of |terms| at every occupied
    bin, the total, and the centred second moment sum c D^2 - S^2 / N about the exact mean."""

    def __init__(self, bins, counts):
        self.bins = [int(b) for b in bins]
        self.counts = [int(c) for c in counts]
        assert self.bins == sorted(set(self.bins)) and all(c > 0 for c in self.counts)
        self.at = {b: i for i, b in enumerate(self.bins)}
        self.cum, self.csum, self.cabs = [], [], []
        n = s = a = q = 0
        for b, c in zip(self.bins, self.counts):
            d = d_int(b)
            n += c
            s += c * d
            a += c * abs(d)
            q += c * d * d
            self.cum.append(n)
            self.csum.append(s)
            self.cabs.append(a)
        self.N, self.S, self.A = n, Fraction(s, SCALE), Fraction(a, SCALE)
        self.M2 = Fraction(q * n - s * s, SCALE * SCALE * n) if n else Fraction(0)

    def dense(self):
        row = np.zeros(oracle.NKEYS, dtype=U64)
        row[self.bins] = np.array([c & ((1 << 64) - 1) for c in self.counts], dtype=U64)
        return row


def exact_rows(dense_rows):
    return [Exact(np.nonzero(r)[0], r[np.nonzero(r)[0]]) for r in dense_rows]


def near(got, exact, tol, what):
    got = float(got)
    assert math.isfinite(got), what
    err = abs(Fraction(got) - exact)
    print(f"{what}: got {got!r} error {float(err):.3e} bound {float(tol):.3e}")
    assert err <= tol, (what, got, float(exact), float(err), float(tol))


def check(got, rows, P, extract=None):
    """`got`: Snapshot.spread's dict for the rows `rows` (Exact) at percentiles P; `extract`: Snapshot.extract's for the same."""
    P = list(P)
    D = dtable()
    assert got["count"].dtype == U64 and got["count"].shape == (len(rows),) and got["m2"].shape == (len(rows),)
    for k in ("pkeys", "pvalid", "count_le", "sum_le", "mean_le", "upper"):
        assert got[k].shape == (len(rows), len(P)), k
    for m, r in enumerate(rows):
        ref = oracle.process_dense(r.dense(), P if P else [0.5])
        assert int(got["count"][m]) == r.N % (1 << 64) == ref["count"], m
        near(got["sum"][m], r.S, REL * r.A, f"row {m} sum")
        near(got["m2"][m], r.M2, REL * r.M2 + (2 * (REL * r.A) ** 2 / r.N if r.N else 0), f"row {m} m2")
        if r.N == 0:
            assert got["sum"][m] == 0 and got["m2"][m] == 0 and math.isnan(got["std"][m])
        else:
            assert got["std"][m] == np.sqrt(got["m2"][m] / np.float64(r.N))
        for i, p in enumerate(P):
            ok, key = int(ref["pvalid"][i]), int(ref["pkeys"][i])
            assert int(got["pvalid"][m, i]) == ok and int(got["pkeys"][m, i]) == key, (m, p)
            if not ok:
                assert got["count_le"][m, i] == 0 and got["sum_le"][m, i] == 0 and math.isnan(got["upper"][m, i]), (m, p)
                assert r.N == 0 or not (p <= 1.0)
                continue
            b = int(oracle.key_to_bin(key))
            j = r.at[b]                                            # the selected bucket is occupied
            assert int(got["count_le"][m, i]) == r.cum[j], (m, p)
            near(got["sum_le"][m, i], Fraction(r.csum[j], SCALE), REL * Fraction(r.cabs[j], SCALE), f"row {m} p {p} sum_le")
            assert got["upper"][m, i] == D[b] and got["mean_le"][m, i] == got["sum_le"][m, i] / np.float64(r.cum[j])
    if extract is not None:
        assert np.array_equal(got["count"], extract["count"])
        if P:
            assert np.array_equal(got["pkeys"], extract["pkeys"]) and np.array_equal(got["pvalid"], extract["pvalid"])


@contextlib.contextmanager
def shape(name):
    """Put every call through one kernel shape, whatever the number of rows; the previous value comes back afterwards."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    assert N.lib().lh_tool_spread_switch(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_spread_switch(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


# ---- the mixed stream: 8 names x 50 000 pairs, half lognormal, half +-10^U(-3, 20), names 2 and 7 empty ----------------
M_MIXED = 8
_MIXED = {}


def mixed_reference():
    if not _MIXED:
        ids, v = stream(2024, M_MIXED, M_MIXED * 50_000)
        _MIXED.update(ids=ids, v=v, rows=exact_rows(oracle.histogram_pairs(ids, v, M_MIXED)))
        assert [r.N == 0 for r in _MIXED["rows"]] == [m in (2, M_MIXED - 1) for m in range(M_MIXED)]
    return _MIXED


@pytest.fixture(scope="module", params=BITS)
def mixed(request, native_lib, torch_cuda):
    ref = mixed_reference()
    with engine(M_MIXED, cell_bits=request.param) as e:
        e.submit_pairs(ref["ids"], ref["v"])
        with e.flip() as snap:
            assert snap.device_cells()[2] == request.param // 8
            yield types.SimpleNamespace(e=e, snap=snap, rows=ref["rows"], torch=torch_cuda, bits=request.param)


@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("pname", list(P_LISTS))
def test_mixed_stream(mixed, kind, pname):
    P = P_LISTS[pname]
    with shape(kind):
        got = mixed.snap.spread(P, M_MIXED)
    check(got, mixed.rows, P, mixed.snap.extract(P if P else [0.5], M_MIXED))
    if pname == "invalid":
        assert got["pvalid"].tolist() == [[0, 0, int(r.N > 0)] for r in mixed.rows]


@pytest.mark.parametrize("kind", list(SHAPES))
def test_sub_range(mixed, kind):
    with shape(kind):
        got = mixed.snap.spread(P_DEFAULT, 4, 3)
    check(got, mixed.rows[3:7], P_DEFAULT, mixed.snap.extract(P_DEFAULT, 4, 3))


@pytest.mark.parametrize("kind", list(SHAPES))
def test_device_form(mixed, kind):
    """Torch device tensors, read after the snapshot's stream has been waited for; equal to the host form bit for bit."""
    torch = mixed.torch
    P = P_DEFAULT
    kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8,
                 count_le=torch.int64, sum_le=torch.float64)
    out = {k: torch.full((M_MIXED,) if k in ("count", "sum", "m2") else (M_MIXED, len(P)), 77, dtype=t, device="cuda")
           for k, t in kinds.items()}
    torch.cuda.synchronize()
    with shape(kind):
        back = mixed.snap.spread(P, M_MIXED, out=out)
        host = mixed.snap.spread(P, M_MIXED)
    torch.cuda.ExternalStream(mixed.snap.stream()).synchronize()
    assert all(back[k] is out[k] for k in kinds)
    for k in kinds:
        assert np.array_equal(out[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(host[k]).view(np.uint8)), k
    # moments only, some outputs left out
    some = {k: torch.full((M_MIXED,), 77, dtype=kinds[k], device="cuda") for k in ("count", "m2")}
    torch.cuda.synchronize()
    with shape(kind):
        mixed.snap.spread([], M_MIXED, out=some)
    torch.cuda.ExternalStream(mixed.snap.stream()).synchronize()
    assert np.array_equal(some["count"].cpu().numpy().view(U64), host["count"])
    assert np.array_equal(some["m2"].cpu().numpy().view(U64), host["m2"].view(U64))
    check(host, mixed.rows, P)


@pytest.mark.parametrize("kind", list(SHAPES))
def test_read_only(mixed, kind):
    """lh_buckets_all returns the same before and after, and the cells keep their store and their width."""
    snap = mixed.snap
    cells = snap.device_cells()
    widenings = mixed.e.counters()["widenings"]
    before = [x.copy() for x in snap.buckets_all(M_MIXED)]
    with shape(kind):
        snap.spread(P_DEFAULT, M_MIXED)
        snap.spread([], 4, 3)
    after = snap.buckets_all(M_MIXED)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    assert snap.device_cells() == cells and cells[2] == mixed.bits // 8
    assert mixed.e.counters()["widenings"] == widenings


def test_range_errors_and_the_empty_call(mixed):
    import loghisto_amd
    snap, M = mixed.snap, M_MIXED
    for first, k in ((0, M + 1), (M, 1), (M + 1, 0), (7, 2)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            snap.spread([0.5], k, first)
        assert ei.value.code == N.ERANGE, (first, k)
    out = np.full(4, 7, dtype=U64)
    p = np.array([0.5])
    for first, k in ((1, (1 << 32) - 1), (0xffffffff, 1), (1, (1 << 64) - 1)):                   # sums that wrap
        assert N.lib().lh_spread(snap._h, first, k, p.ctypes.data, 1, out.ctypes.data, 0, 0, 0, 0, 0, 0) == N.ERANGE
    for first in (0, M):                                                                         # nmetrics == 0
        assert N.lib().lh_spread(snap._h, first, 0, p.ctypes.data, 1, out.ctypes.data, 0, 0, 0, 0, 0, 0) == 0
    assert np.all(out == 7)
    # plain (pageable) numpy arrays take the library's pinned block; outputs left out are not written
    count, sle, keys = np.zeros(M, dtype=U64), np.zeros((M, 2), dtype=np.float64), np.zeros((M, 2), dtype=np.int16)
    got = snap.spread([0.5, 1.0], M, out=dict(count=count, sum_le=sle, pkeys=keys))
    want = snap.spread([0.5, 1.0], M)
    assert sorted(got) == ["count", "pkeys", "sum_le"]
    assert np.array_equal(count, want["count"]) and np.array_equal(keys, want["pkeys"])
    assert np.array_equal(sle.view(U64), want["sum_le"].view(U64))


# ---- crafted rows, imported through add_buckets ------------------------------------------------------------------------
STEP_LO = 40001                                  # not a multiple of 4; the walks' steps start at 40 000: one ends at 40 255
def kb(key):
    return int(oracle.key_to_bin(key))


CRAFTED = [
    {kb(1234): 7},                                                # one cell
    {0: 3, 65535: 5},                                                            # keys -32768 and 32767: a full span
    {STEP_LO: 10, 40255: 10, 40256: 10, 40300: 10},                              # thresholds either side of a step boundary
    {kb(500): (1 << 53) + 1, kb(700): 1},          # float64(count) rounds
    {kb(-250): 17, kb(900): (1 << 33) + 5},        # a cell beyond 32 bits
    {},
    {kb(3000): 123_456_789},                                      # one bucket, many samples
    {b: 1 + b % 3 for b in range(33000, 33000 + 1500, 7)},                       # several steps, sparse
]
P_CRAFTED = [0.25, 0.5, 0.51, 0.75, 0.0, 1.0, 0.999]


@pytest.fixture(scope="module", params=BITS)
def crafted(request, native_lib, torch_cuda):
    rows = [Exact(sorted(int(b) for b in r), [r[b] for b in sorted(r)]) for r in CRAFTED]
    ids = np.concatenate([np.full(len(r.bins), m, dtype=np.uint32) for m, r in enumerate(rows)])
    keys = np.concatenate([oracle.bin_to_key(np.array(r.bins, dtype=np.int64)).astype(np.int16) for r in rows if r.bins])
    counts = np.concatenate([np.array(r.counts, dtype=U64) for r in rows if r.bins])
    with engine(len(rows), cell_bits=request.param) as e:
        with e.flip() as snap:
            assert snap.device_cells()[2] == request.param // 8
            snap.add_buckets(ids, keys, counts)
            assert snap.device_cells()[2] == 8                   # (an import moves a narrow snapshot to its wide store)
            yield types.SimpleNamespace(e=e, snap=snap, rows=rows)


@pytest.mark.parametrize("kind", list(SHAPES))
def test_crafted_rows(crafted, kind):
    M = len(crafted.rows)
    with shape(kind):
        got = crafted.snap.spread(P_CRAFTED, M)
        moments = crafted.snap.spread([], M)
    check(got, crafted.rows, P_CRAFTED, crafted.snap.extract(P_CRAFTED, M))
    check(moments, crafted.rows, [])
    # the step boundary: 0.5 ends on the last bin of one step, 0.51 and 0.75 on the first bin of the next
    assert [int(oracle.key_to_bin(int(k))) for k in got["pkeys"][2][:4]] == [STEP_LO, 40255, 40256, 40256]
    assert got["count_le"][2][:4].tolist() == [10, 20, 30, 30]
    assert got["count"][3] == (1 << 53) + 2 and got["count_le"][3][1] == (1 << 53) + 1
    assert got["count"][4] == (1 << 33) + 22 and got["count_le"][4].tolist()[:2] == [(1 << 33) + 22] * 2


@pytest.mark.parametrize("kind", list(SHAPES))
def test_one_bucket_names_have_no_spread(crafted, kind):
    """All samples in one bucket: mean' = (D c) / c is D to two roundings, so m2 is far inside the bound, which here is
    1e-12 * 0 + 2 * (1e-12 c |D|)^2 / c = 2e-24 c D^2."""
    with shape(kind):
        got = crafted.snap.spread([], len(crafted.rows))
    for m in (0, 6):
        r = crafted.rows[m]
        assert r.M2 == 0 and len(r.bins) == 1
        bound = 2e-24 * r.N * float(dtable()[r.bins[0]]) ** 2
        print(f"row {m}: m2 {got['m2'][m]!r} bound {bound!r}")
        assert 0 <= got["m2"][m] <= bound and got["std"][m] <= 1.5e-12 * abs(float(dtable()[r.bins[0]]))


# ---- the table is the engine's ------------------------------------------------------------------------------------------
def test_single_samples_return_the_engines_table_bit_for_bit(native_lib, torch_cuda):
    """One sample in one cell per name: sum is D[bin] * 1.0 and nothing else, so it shows the unit's own decompress table,
    which has to be the D[] of lh_codec_tables bit for bit."""
    bins = np.unique(np.concatenate([np.arange(0, 65536, 97), [1, 2, 3, 32767, 32768, 32769, 65534, 65535]]))
    M = bins.size
    with engine(M) as e:
        D = e.codec_tables()[1]
        with e.flip() as snap:
            snap.add_buckets(np.arange(M, dtype=np.uint32), oracle.bin_to_key(bins).astype(np.int16), np.ones(M, dtype=U64))
            for kind in SHAPES:
                with shape(kind):
                    got = snap.spread([0.5], M)
                assert np.array_equal(got["sum"].view(U64), D[bins].view(U64)), kind
                assert np.array_equal(got["sum_le"][:, 0].view(U64), D[bins].view(U64)), kind
                assert np.array_equal(got["upper"][:, 0].view(U64), D[bins].view(U64)) and not got["m2"].any()


# ---- crafted rows in the NARROW store ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(native_lib, torch_cuda):
    """The rows of tests/_cells32_rows.py written straight into uint32 cells (add_buckets would widen the snapshot): every
    lo % 4, spans around 1 024 bins, the ends of the key space, full-range rows, totals beyond 2^32 from 32-bit cells.
    Checked: the ingested row, the filler rows before the special ones, every special row and twelve rows behind them."""
    from tests import _cells32_rows as R
    from tests.test_gpu_cells32_readers import M, _engine, write_rows
    rows = R.make_rows(M)
    last = max(m for m, r in enumerate(rows) if m and not r.kind.startswith("f_"))       # the last special row
    exact = [Exact(r.bins, r.counts) for r in rows[:last + 13]]                          # ... and twelve filler rows more
    with _engine(M) as e:
        snap = write_rows(torch_cuda, e, rows)
        try:
            yield types.SimpleNamespace(e=e, snap=snap, rows=exact, cells=snap.device_cells())
        finally:
            snap.release()


@pytest.mark.parametrize("kind", list(SHAPES))
def test_crafted_rows_in_32_bit_cells(narrow, kind):
    M = len(narrow.rows)
    with shape(kind):
        got = narrow.snap.spread(P_DEFAULT, M)
    assert narrow.snap.device_cells() == narrow.cells and narrow.cells[2] == 4           # still narrow
    check(got, narrow.rows, P_DEFAULT, narrow.snap.extract(P_DEFAULT, M))


# ---- the host form's two ways back -------------------------------------------------------------------------------------
SPREAD_OUT = dict(count=U64, sum=np.float64, m2=np.float64, pkeys=np.int16, pvalid=np.uint8, count_le=U64, sum_le=np.float64)


def test_pinned_and_pageable_outputs_receive_the_same_results(native_lib, torch_cuda):
    """lh_spread with caller-supplied arrays: pinned (one copy per array, straight in) and pageable (through the unit's
    pinned block) -- the same bits, and the oracle's.  All seven outputs, then four of them: the block's 8-byte-aligned
    layout with arrays left out."""
    M = 5
    ids, v = small_stream()
    rows = exact_rows(oracle.histogram_pairs(ids, v, M))
    assert [r.N for r in rows][2:4] == [0, 1]
    P = [0.5, 0.9, 1.0]

    def arrays(pinned, names):
        return {k: host_arrays(torch_cuda, pinned, (M,) if k in ("count", "sum", "m2") else (M, len(P)), SPREAD_OUT[k]) for k in names}

    with engine(M) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            full = [(arrays(pinned, SPREAD_OUT), pinned) for pinned in (True, False)]
            got = [snap.spread(P, M, out=a) for a, _ in full]
            some = [arrays(pinned, ("sum", "pkeys", "pvalid", "sum_le")) for pinned in (True, False)]
            for a in some:
                snap.spread(P, M, out=a)
    for g in got:
        check(g, rows, P)
    for a in [a for a, _ in full[1:]] + some:
        for k in a:
            assert a[k].tobytes() == full[0][0][k].tobytes(), k
