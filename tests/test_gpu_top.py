"""lh_top / lh_top_device (Snapshot.top): the k names of a range that lead by count, by sum, by the bucket a percentile
falls into or by the samples above a value.

The expected list is computed in numpy from what the library already returns for the same snapshot: count and pkey from
lh_extract_rows, above = count - lh_count_le at the value, the sum as the exact rational sum of D[b] * c[b] over lh_buckets_all
(tests/test_gpu_spread.py's arithmetic).  Candidates (count != 0) are sorted by (score, id) and the first k taken.  ids, count,
pkey and above must be EQUAL; each returned sum lies within 1e-12 * sum |terms| of the exact value (the project's _sum rule,
test_gpu_spread.REL).  By sum the order itself is required: the test data keeps neighbouring sums either exactly equal
(identical cells: id order) or further apart than 1e-10 of their terms, which assert_sums_are_apart checks of the data."""
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_count_le import engine, host_arrays, stream
from tests.test_gpu_spread import REL, SCALE, d_int, kb

pytestmark = pytest.mark.gpu

U64 = np.uint64
BITS = (64, 32)
INF = float("inf")
PCTS = [0.0, 0.5, 0.99, 1.0]
ABOVE = [250.0, oracle.decompress(700), -5.0, INF, -INF, 1e200]
BYS = [("count", None)] + [("sum", None)] + [("percentile", p) for p in PCTS] + [("count_above", a) for a in ABOVE]
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2500)
KS = (1, 2, 64, 65, 1000, 1024)
M_BIG = 2500


# ---- the expected side: everything from the library's other calls on the same snapshot --------------------------------
class Ref:
    """Per row of the snapshot: count, the bin of every percentile of PCTS, the count above every value of ABOVE, and the
    exact sum with the sum of its |terms|; `srank` ranks the exact sums (equal sums share a rank)."""

    def __init__(self, snap, M):
        self.M = M
        ex = snap.extract(PCTS, M)
        self.count = [int(c) for c in ex["count"]]
        self.pkey = ex["pkeys"].astype(np.int64)
        assert np.array_equal(ex["pvalid"] != 0, np.repeat(ex["count"][:, None] != 0, len(PCTS), axis=1))
        self.pbin = oracle.key_to_bin(self.pkey).astype(np.int64)
        cum = np.stack([snap.count_le(np.array([a]), M)["cum"][:, 0] for a in ABOVE], axis=1)      # (a call per bound: unsorted)
        assert np.array_equal(snap.count_le(np.array([INF]), M)["total"], ex["count"])
        self.above = [[(self.count[m] - int(cum[m, j])) % (1 << 64) for j in range(len(ABOVE))] for m in range(M)]
        off, keys, counts = snap.buckets_all(M)
        self.S, self.A = [], []
        for m in range(M):
            s = a = 0
            for key, c in zip(keys[int(off[m]):int(off[m + 1])], counts[int(off[m]):int(off[m + 1])]):
                d = d_int(kb(int(key)))
                s += int(c) * d
                a += int(c) * abs(d)
            self.S.append(s)                                         # in units of 2^-1100
            self.A.append(a)
        order = sorted(set(self.S))
        rank = {s: i for i, s in enumerate(order)}
        self.srank = [rank[s] for s in self.S]

    def score(self, m, by, arg):
        if by == "count":
            return self.count[m]
        if by == "sum":
            return self.srank[m]
        if by == "percentile":
            return int(self.pbin[m, PCTS.index(arg)])
        return self.above[m][ABOVE.index(arg)]

    def expected(self, by, arg, k, ascending, first=0, nmetrics=None):
        nmetrics = self.M - first if nmetrics is None else nmetrics
        cand = [m for m in range(first, first + nmetrics) if self.count[m] != 0]
        sign = 1 if ascending else -1
        return sorted(cand, key=lambda m: (sign * self.score(m, by, arg), m))[:k]

    def assert_sums_are_apart(self):
        """Of the data: two candidates' sums are exactly equal or differ by more than 1e-10 of their terms -- a hundred times
        the tolerance of one sum -- so the order by the returned float64 sums is the order by the exact ones."""
        cand = sorted((m for m in range(self.M) if self.count[m]), key=lambda m: self.S[m])
        for a, b in zip(cand, cand[1:]):
            assert self.S[a] == self.S[b] or (self.S[b] - self.S[a]) * 10 ** 10 > max(self.A[a], self.A[b]), (a, b)


def check(got, ref, by, arg, k, ascending, first=0, nmetrics=None):
    want = ref.expected(by, arg, k, ascending, first, nmetrics)
    what = (by, arg, k, ascending, first, nmetrics)
    assert got.dtype == N.TOP_ENTRY and got.shape == (len(want),), what
    assert got["id"].tolist() == want, what
    assert not got["reserved"].any(), what
    for e, m in zip(got, want):
        assert int(e["count"]) == ref.count[m] != 0, (what, m)
        assert int(e["pkey"]) == (int(ref.pkey[m, PCTS.index(arg)]) if by == "percentile" else 0), (what, m)
        assert int(e["above"]) == (ref.above[m][ABOVE.index(arg)] if by == "count_above" else 0), (what, m)
        err = abs(Fraction(float(e["sum"])) - Fraction(ref.S[m], SCALE))
        assert np.isfinite(e["sum"]) and err <= REL * Fraction(ref.A[m], SCALE), (what, m, float(e["sum"]), float(err))
    return want


def run(snap, ref, by, arg, k, ascending=False, first=0, nmetrics=None):
    n = ref.M - first if nmetrics is None else nmetrics
    return check(snap.top(k, by, arg, ascending, n, first), ref, by, arg, k, ascending, first, n)


# ---- crafted rows, imported through add_buckets ------------------------------------------------------------------------
X = 0x00123456789abc
Y = (1 << 32) | 0x5500
SPECIAL = [
    {kb(1234): 7},
    {},
    # counts that differ only in the top byte -- one of them beyond 2^63
    {kb(100): (0x01 << 56) | X}, {kb(100): (0x02 << 56) | X}, {kb(100): (0x80 << 56) | X}, {kb(100): (0x7f << 56) | X},
    # ... only in the low byte, beyond 2^32: seven bytes shared
    {kb(200): Y | 1}, {kb(200): Y | 3}, {kb(200): Y | 2}, {kb(201): Y | 2},
    # ... only in a middle byte
    {kb(300): 0xaa0011 | (5 << 8)}, {kb(300): 0xaa0011 | (4 << 8)}, {kb(300): 0xaa0011 | (6 << 8)},
    # sums of both signs, 5e-4 .. 1e142; cancellation down to 1e-3
    {kb(1): 10, kb(-2): 5}, {kb(1): 181, kb(-2): 90}, {kb(1): 1}, {kb(-1): 1}, {kb(-1): 12, kb(2): 5},
    {kb(32236): 1}, {kb(-32236): 1}, {kb(32767): 3}, {kb(-32768): 2}, {kb(20000): 1 << 40}, {kb(-20000): (1 << 40) + 1},
    {kb(0): 5},                                   # samples at value 0: a zero sum
    {kb(77): 4, kb(-77): 4},                      # ... and one from cancellation
    {kb(555): 9, kb(-40): 2}, {kb(555): 9, kb(-40): 2},   # identical cells: equal bits, id order
    {0: 3, 65535: 5},                             # keys -32768 and 32767: bins 0 .. 65 535
    {0: 1, 30000: 1, 65535: 1},
    {40001: 10, 40255: 10, 40256: 10, 40300: 10},  # a span from a bin that is no multiple of 4; a cell either side of a step
    {40001: 1, 40255: 49, 40256: 50},
    {kb(-900): 30, kb(-100): 30, kb(50): 1},      # percentiles at negative keys
]


def crafted_rows(M):
    """The special rows, then filler: every seventh row empty, else one to four cells at keys of both signs with small
    counts (many equal counts and equal percentile buckets: ties everywhere)."""
    rng = np.random.default_rng(5)
    rows = [dict(r) for r in SPECIAL]
    while len(rows) < M:
        m = len(rows)
        if m % 7 == 3:
            rows.append({})
            continue
        keys = rng.choice(np.concatenate([np.arange(-3000, -2000), np.arange(1, 6000)]), int(rng.integers(1, 5)), replace=False)
        rows.append({kb(int(k)): int(rng.integers(1, 40)) for k in keys})
    return rows


def import_rows(snap, rows, first=0):
    ids = np.concatenate([np.full(len(r), first + m, dtype=np.uint32) for m, r in enumerate(rows)])
    bins = np.concatenate([np.array(sorted(r), dtype=np.int64) for r in rows])
    counts = np.concatenate([np.array([r[b] for b in sorted(r)], dtype=U64) for r in rows])
    snap.add_buckets(ids, oracle.bin_to_key(bins).astype(np.int16), counts)


@pytest.fixture(scope="module", params=BITS)
def crafted(request, native_lib, torch_cuda):
    with engine(M_BIG, cell_bits=request.param) as e:
        with e.flip() as snap:
            assert snap.device_cells()[2] == request.param // 8
            import_rows(snap, crafted_rows(M_BIG))
            assert snap.device_cells()[2] == 8       # (an import moves a narrow snapshot to its wide store: `narrow` below
            ref = Ref(snap, M_BIG)                   # holds these rows in 32-bit cells)
            ref.assert_sums_are_apart()
            yield types.SimpleNamespace(e=e, snap=snap, ref=ref, torch=torch_cuda)


@pytest.mark.parametrize("nmetrics", SIZES)
def test_sizes(crafted, nmetrics):
    """Every nmetrics x k, every score, both directions."""
    for k in KS:
        for by, arg in BYS:
            for asc in (False, True):
                run(crafted.snap, crafted.ref, by, arg, k, asc, 0, nmetrics)


def test_the_special_rows_rank_as_designed(crafted):
    snap, ref = crafted.snap, crafted.ref
    n = len(SPECIAL)
    top = run(snap, ref, "count", None, 8, nmetrics=n)
    assert top[:6] == [4, 5, 3, 2, 23, 22] and top[6:] == [7, 8]           # the top byte decides, then 2^40, then the low byte
    assert run(snap, ref, "count", None, 3, True, nmetrics=n) == [15, 16, 18]       # count 1: lowest ids first
    by_sum = run(snap, ref, "sum", None, n, nmetrics=n)
    assert by_sum[:3] == [20, 28, 18] and by_sum[-3:] == [19, 29, 21]
    zero = [m for m in by_sum if ref.S[m] == 0]
    assert zero == [24, 25] and ref.S[26] == ref.S[27] and by_sum.index(27) == by_sum.index(26) + 1
    assert ref.S[13] < 0 < ref.S[14] and abs(Fraction(ref.S[14], SCALE)) < Fraction(1, 900)
    full = run(snap, ref, "percentile", 1.0, 4, nmetrics=n)
    assert full[:3] == [20, 28, 29]                                                  # bin 65 535, lowest ids first
    assert run(snap, ref, "percentile", 0.0, 3, True, nmetrics=n)[:3] == [21, 28, 29]  # bin 0
    got = snap.top(n, "percentile", 0.5, False, n)
    at = {int(e["id"]): int(oracle.key_to_bin(int(e["pkey"]))) for e in got}
    assert (at[30], at[31], at[28], at[29]) == (40255, 40255, 65535, 30000)
    got = snap.top(n, "percentile", 0.99, False, n)
    at = {int(e["id"]): int(oracle.key_to_bin(int(e["pkey"]))) for e in got}
    assert (at[30], at[31], at[32]) == (40300, 40256, kb(50))
    above = snap.top(n, "count_above", -5.0, False, n)
    assert {int(e["id"]): int(e["above"]) for e in above}[32] == 31                  # the cells at keys -100 and 50


def test_more_wanted_than_there_are(crafted):
    ref = crafted.ref
    for first, n in ((0, 63), (0, 1023), (2000, 500)):
        have = sum(1 for m in range(first, first + n) if ref.count[m])
        assert have < n and have < 1024
        for by, arg in BYS:
            assert len(run(crafted.snap, ref, by, arg, 1024, False, first, n)) == have


def test_sub_ranges_return_absolute_ids(crafted):
    for first, n, k in ((1, 1, 5), (3, 1, 1), (2, 62, 7), (777, 1025, 65), (M_BIG - 1, 1, 2), (1500, 1000, 1000)):
        for by, arg in BYS[:2] + [("percentile", 0.5), ("count_above", 250.0)]:
            for asc in (False, True):
                want = run(crafted.snap, crafted.ref, by, arg, k, asc, first, n)
                assert all(first <= m < first + n for m in want)
    assert run(crafted.snap, crafted.ref, "count", None, 5, False, 1, 1) == []      # row 1 is empty: no candidate
    assert run(crafted.snap, crafted.ref, "count", None, 5, False, 0, 2) == [0]     # one candidate


def test_device_form_equals_host_form(crafted):
    torch, snap = crafted.torch, crafted.snap
    for (by, arg), k, asc, first, n in ((BYS[0], 64, False, 0, M_BIG), (BYS[1], 1024, True, 5, 2000), (BYS[4], 1000, False, 0, 1025),
                                        (BYS[6], 65, False, 100, 63), (BYS[0], 7, False, 1, 1)):
        ent = torch.full((k * 32,), 0x77, dtype=torch.uint8, device="cuda")
        cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert snap.top(k, by, arg, asc, n, first, out=(ent, cnt)) == (ent, cnt)
        host = snap.top(k, by, arg, asc, n, first)
        torch.cuda.ExternalStream(snap.stream()).synchronize()
        nout = cnt.cpu().numpy()
        raw = ent.cpu().numpy()
        assert nout.tolist() == [host.size, -1]
        assert raw[:host.size * 32].tobytes() == host.tobytes() and np.all(raw[host.size * 32:] == 0x77)
        check(host, crafted.ref, by, arg, k, asc, first, n)


def test_pinned_and_pageable_out_receive_the_same_bytes(crafted):
    """Entries at and beyond n_out keep what they held."""
    torch, snap = crafted.torch, crafted.snap
    for (by, arg), k, n in ((BYS[0], 64, M_BIG), (BYS[1], 100, 63), (BYS[3], 1024, 700)):
        outs = [host_arrays(torch, pinned, (k,), N.TOP_ENTRY) for pinned in (True, False)]
        got = [snap.top(k, by, arg, False, n, out=o) for o in outs]
        want = check(got[0], crafted.ref, by, arg, k, False, 0, n)
        assert outs[0].tobytes() == outs[1].tobytes() and got[1].tobytes() == got[0].tobytes()
        assert np.all(outs[0].view(np.uint8)[len(want) * 32:] == 0x77)


def test_read_only(crafted):
    from loghisto_amd import merge
    torch, snap = crafted.torch, crafted.snap

    def state():
        torch.cuda.ExternalStream(snap.stream()).synchronize()
        ranges = torch.as_tensor(merge._DeviceArray(snap.device_ranges(), (2 * M_BIG,), "<i4"), device="cuda").cpu().numpy().copy()
        return [x.copy() for x in snap.buckets_all(M_BIG)], ranges, snap.device_cells(), crafted.e.counters()["widenings"]
    before = state()
    for by, arg in BYS:
        snap.top(100, by, arg, False, M_BIG)
        snap.top(1024, by, arg, True, 1000, 37)
    after = state()
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert before[2:] == after[2:]


def test_range_errors_and_the_empty_call(crafted):
    import ctypes as C
    import loghisto_amd
    snap, M = crafted.snap, M_BIG
    for first, n in ((0, M + 1), (M, 1), (M + 1, 0), (M - 1, 2)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            snap.top(3, "count", None, False, n, first)
        assert ei.value.code == N.ERANGE, (first, n)
    out = np.zeros(4, dtype=N.TOP_ENTRY)
    n_out = C.c_size_t(99)
    for first, n in ((1, (1 << 32) - 1), (0xffffffff, 1)):                               # sums that wrap
        assert N.lib().lh_top(snap._h, first, n, 0, 0.0, 4, 0, out.ctypes.data, C.addressof(n_out)) == N.ERANGE
    assert n_out.value == 99 and not out.view(np.uint8).any()
    for first in (0, M):                                                                 # nmetrics == 0: LH_OK, n_out = 0
        n_out.value = 99
        assert N.lib().lh_top(snap._h, first, 0, 0, 0.0, 4, 0, out.ctypes.data, C.addressof(n_out)) == 0 and n_out.value == 0
    assert not out.view(np.uint8).any()
    torch = crafted.torch
    cnt = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    ent = torch.zeros((128,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert N.lib().lh_top_device(snap._h, 0, 0, 0, 0.0, 4, 0, ent.data_ptr(), cnt.data_ptr()) == 0
    torch.cuda.ExternalStream(snap.stream()).synchronize()
    assert int(cnt.cpu()[0]) == 0


def test_the_timing_hook_runs_both_passes(crafted):
    import ctypes as C
    snap = crafted.snap
    before = snap.top(20, "sum", None, False, M_BIG).copy()
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    assert N.lib().lh_tool_top_passes_ms(snap._h, 0, M_BIG, N.TOP_BY_SUM, 0.0, 20, 0, C.byref(a), C.byref(b)) == 0
    assert a.value > 0 and b.value > 0
    run(snap, crafted.ref, "sum", None, 20)                                              # the unit's blocks are as they were
    assert snap.top(20, "sum", None, False, M_BIG).tobytes() == before.tobytes()


# ---- ties across the cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_a_tie_group_that_straddles_the_cut(native_lib, torch_cuda, bits):
    """2 500 rows whose counts take three values: whatever k, the cut falls inside a group of some 833 equal scores, and the
    winners of that group are its lowest ids -- in both directions."""
    values = (5, 9, 7)
    rows = [{kb(100 + m % 11): values[m % 3]} for m in range(M_BIG)]
    with engine(M_BIG, cell_bits=bits) as e:
        with e.flip() as snap:
            import_rows(snap, rows)
            assert snap.device_cells()[2] == 8       # (the engine of 32-bit cells: a snapshot an import has widened)
            ref = Ref(snap, M_BIG)
            for k in (1, 2, 64, 833, 834, 835, 1000, 1024):
                desc = run(snap, ref, "count", None, k)
                nines = [m for m in range(M_BIG) if m % 3 == 1]
                sevens = [m for m in range(M_BIG) if m % 3 == 2]
                assert desc == (nines + sevens)[:k]
                asc = run(snap, ref, "count", None, k, True)
                assert asc == ([m for m in range(M_BIG) if m % 3 == 0] + sevens)[:k]
                run(snap, ref, "count_above", 250.0, k)                               # every score 0: ids 0 .. k - 1
                run(snap, ref, "percentile", 0.5, k, True)
            for n in (1023, 1025):
                run(snap, ref, "count", None, 1000, False, 3, n)


@pytest.mark.parametrize("bits", BITS)
def test_all_rows_empty(native_lib, torch_cuda, bits):
    with engine(M_BIG, cell_bits=bits) as e:
        with e.flip() as snap:
            assert snap.device_cells()[2] == bits // 8                               # empty rows in cells of either width
            for by, arg in BYS:
                for n in (1, 64, 1025, M_BIG):
                    got = snap.top(1024, by, arg, False, n)
                    assert got.dtype == N.TOP_ENTRY and got.size == 0
            import_rows(snap, [{kb(-300): 2}], first=1999)                           # one candidate, far into the range
            for by, arg in BYS:
                for asc in (False, True):
                    got = snap.top(1024, by, arg, asc, M_BIG)
                    assert got["id"].tolist() == [1999] and int(got["count"][0]) == 2
                    assert snap.top(3, by, arg, asc, 1999).size == 0 and snap.top(3, by, arg, asc, 1, 1999)["id"].tolist() == [1999]


# ---- an ingested mixed stream: the cells stay as narrow as the engine keeps them -------------------------------------------
M_MIXED = 600


@pytest.fixture(scope="module", params=BITS)
def mixed(request, native_lib, torch_cuda):
    ids, v = stream(2026, M_MIXED, M_MIXED * 300)
    with engine(M_MIXED, cell_bits=request.param) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            assert snap.device_cells()[2] == request.param // 8
            yield types.SimpleNamespace(e=e, snap=snap, ref=Ref(snap, M_MIXED), bits=request.param)


def test_mixed_stream(mixed):
    assert mixed.ref.count[2] == 0 and mixed.ref.count[M_MIXED - 1] == 0
    for by, arg in BYS:
        for asc in (False, True):
            for k, first, n in ((20, 0, M_MIXED), (1024, 0, M_MIXED), (100, 17, 301)):
                run(mixed.snap, mixed.ref, by, arg, k, asc, first, n)
    assert mixed.snap.device_cells()[2] == mixed.bits // 8                           # a snapshot of 32-bit cells stays one


def test_count_le_is_what_it_was(mixed):
    """le_take moved into the shared header: lh_count_le's answers against the oracle's bound-to-key rule and a running
    sum over lh_buckets_all."""
    from tests.test_gpu_count_le import take_of
    bounds = np.array(sorted([-INF, -1e200, -1e150, -250.0, -5.0, -0.0, 0.0, 1e-9, 250.0, oracle.decompress(700), 1e25, 1e150,
                              1e200, INF]))
    E = take_of(bounds)
    off, keys, counts = mixed.snap.buckets_all(M_MIXED)
    got = mixed.snap.count_le(bounds, M_MIXED)
    for m in range(M_MIXED):
        b = oracle.key_to_bin(keys[int(off[m]):int(off[m + 1])].astype(np.int64))
        c = counts[int(off[m]):int(off[m + 1])]
        assert got["cum"][m].tolist() == [int(c[b < e].sum()) for e in E], m
        assert int(got["total"][m]) == int(c.sum())


def test_a_widened_snapshot(native_lib, torch_cuda):
    """32-bit cells, then one cell beyond 2^32 imported: the snapshot moves to its wide store and ranks as before."""
    ids, v = stream(11, 300, 300 * 200)
    with engine(300, cell_bits=32) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            assert snap.device_cells()[2] == 4
            before = Ref(snap, 300)
            for by, arg in BYS:
                run(snap, before, by, arg, 50)
            narrow = snap.top(50, "count", None, False, 300)
            assert snap.device_cells()[2] == 4
            snap.add_buckets(np.array([123], dtype=np.uint32), np.array([77], dtype=np.int16), np.array([(1 << 32) + 9], dtype=U64))
            assert snap.device_cells()[2] == 8
            ref = Ref(snap, 300)
            for by, arg in BYS:
                run(snap, ref, by, arg, 50)
            wide = snap.top(50, "count", None, False, 300)
            assert wide["id"][0] == 123 and int(wide["count"][0]) > 1 << 32
            assert [m for m in narrow["id"].tolist() if m != 123][:49] == wide["id"].tolist()[1:]


# ---- the crafted rows in the NARROW store ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def narrow(native_lib, torch_cuda):
    """crafted_rows written straight into uint32 cells (add_buckets would widen the snapshot), counts capped at 2^32 - 1: the
    full-span rows, the rows either side of the step boundary 40 255 / 40 256, the negative keys and the sums of both signs
    under k_top_score<uint32_t>.  Row 0 is ingested, as tests/test_gpu_cells32_readers.write_rows has it."""
    from tests import _cells32_rows as R
    from tests.test_gpu_cells32_readers import _engine, write_rows
    h0 = oracle.histogram_dense(R.ROW0_SAMPLES)
    cells = [{int(b): int(h0[b]) for b in np.nonzero(h0)[0]}]
    cells += [{b: min(c, R.U32) for b, c in r.items()} for r in crafted_rows(M_BIG)[1:]]
    rows = [R.Row("crafted", c) for c in cells]
    with _engine(M_BIG) as e:
        snap = write_rows(torch_cuda, e, rows)
        try:
            assert snap.device_cells()[2] == 4
            ref = Ref(snap, M_BIG)
            ref.assert_sums_are_apart()
            yield types.SimpleNamespace(e=e, snap=snap, ref=ref, rows=cells)
        finally:
            snap.release()


def test_crafted_rows_in_32_bit_cells(narrow):
    snap, ref = narrow.snap, narrow.ref
    for m in (28, 29, 30, 31, 32):                                                   # the library's other readers saw these cells
        assert ref.count[m] == sum(narrow.rows[m].values())
    for by, arg in BYS:
        for asc in (False, True):
            for k, first, n in ((1, 0, M_BIG), (64, 0, M_BIG), (1024, 0, M_BIG), (1000, 0, 1025), (65, 20, 63), (5, 28, 5)):
                run(snap, ref, by, arg, k, asc, first, n)
    got = snap.top(5, "percentile", 0.5, False, 5, 28)
    at = {int(e["id"]): int(oracle.key_to_bin(int(e["pkey"]))) for e in got}
    assert (at[28], at[29], at[30], at[31]) == (65535, 30000, 40255, 40255)
    got = snap.top(5, "percentile", 0.99, False, 5, 28)
    at = {int(e["id"]): int(oracle.key_to_bin(int(e["pkey"]))) for e in got}
    assert (at[30], at[31], at[32]) == (40300, 40256, kb(50))
    assert snap.device_cells()[2] == 4                                               # a snapshot of 32-bit cells stays one


# ---- two engines on one device: two streams, one records block -------------------------------------------------------------
def test_the_records_block_regrows_behind_a_pending_device_form_call(native_lib, torch_cuda):
    """A device-form call on a snapshot of 300 names, then -- nothing waited for -- a host-form call on another engine's
    snapshot of 4 100 names: just past the records block's floor of 4 096, so the block the first call's passes may still be
    using is freed and allocated again (in a process whose calls so far stayed below the floor: every test above does).
    Both results are what the same calls return afterwards, with nothing in flight."""
    torch, k = torch_cuda, 50
    with engine(300) as e1, engine(4100) as e2:
        e1.submit_pairs(*stream(31, 300, 30_000))
        e2.submit_pairs(*stream(32, 4100, 40_000))
        with e1.flip() as s1, e2.flip() as s2:
            assert s1.stream() != s2.stream()
            ent = torch.full((k * 32,), 0x77, dtype=torch.uint8, device="cuda")
            cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            s1.top(k, "sum", None, False, 300, out=(ent, cnt))
            large = s2.top(k, "sum", None, False, 4100).copy()
            torch.cuda.ExternalStream(s1.stream()).synchronize()
            small = ent.cpu().numpy().view(N.TOP_ENTRY)[:int(cnt.cpu()[0])]
            torch.cuda.synchronize()
            assert small.size == large.size == k
            assert small.tobytes() == s1.top(k, "sum", None, False, 300).tobytes()
            assert large.tobytes() == s2.top(k, "sum", None, False, 4100).tobytes()


# ---- more records than one tile of the select pass ---------------------------------------------------------------------
# ON PURPOSE above the 3 000 names the other engines here keep to: k_top_select takes 4 096 records per tile, and below that
# its loops over the records run once.  9 000 names are three tiles, the last one partial; 30 samples per name keep the
# reference's Python loops short (the test takes about a second on the MI355X).
M_TILES = 9000


def test_more_names_than_one_tile_of_the_select_pass(native_lib, torch_cuda):
    """The engines above stay below 3 000 names, where the select pass's loops over the records run once.  9 000 names (in
    32-bit cells, ingested) take three tiles: the histogram passes add up over tiles, the winners' prefix counts carry from
    tile to tile, tie groups spread over all of them (by count above +Inf every score is 0: the k lowest ids) and the
    loop ends early once the winners are complete."""
    ids, v = stream(77, M_TILES, M_TILES * 30)
    with engine(M_TILES, cell_bits=32) as e:
        e.submit_pairs(ids, v)
        with e.flip() as snap:
            assert snap.device_cells()[2] == 4
            ref = Ref(snap, M_TILES)
            for by, arg in BYS:
                for asc in (False, True):
                    for k, first, n in ((1, 0, M_TILES), (100, 0, M_TILES), (1024, 0, M_TILES), (1024, 100, 8193), (65, 4000, 4097)):
                        run(snap, ref, by, arg, k, asc, first, n)
            late = run(snap, ref, "count", None, 1024, False, 4096, M_TILES - 4096)       # every winner beyond the first tile
            assert min(late) >= 4096 and max(late) >= 8192
            assert snap.device_cells()[2] == 4
