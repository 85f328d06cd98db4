"""lh_movers / lh_movers_device (Snapshot.movers): the k names of a range whose distribution moved most between two
snapshots, by lh_compare's ks, w1 or shift or by how many buckets the bucket of a percentile moved.

The expected list is computed in numpy from what the library already returns for the same two snapshots:
  ks, w1, shift   cur.compare(base) with lh_tool_compare_switch on the wave shape; the rows with both counts non-zero sorted
                  by (-+score as float64 with -0.0 folded to +0.0, id), the first k taken.  ids, count_a, count_b and key must be
                  EQUAL and score BIT-EQUAL to the compare array's entry.  Independently of lh_compare, on the crafted pairs
                  every w1 and shift score lies within tests/test_gpu_compare.check's bound, 4 n 2^-53 (1 + w1), of model()'s
                  exact Fraction, and every ks is bit-equal to the model's.
  percentile      extract([p]) of both snapshots: score = key_to_bin(pkey of cur) - key_to_bin(pkey of base), compared exactly;
                  key / key_base are the two pkeys."""
import ctypes as C
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_compare import BIG, EPS, _import, _write_narrow, crafted_models, crafted_pairs, model, rows_of, shape
from tests.test_gpu_count_le import engine, host_arrays

pytestmark = pytest.mark.gpu

U64 = np.uint64
PCTS = [0.0, 0.5, 0.99, 1.0]
BYS = [("ks", None), ("w1", None), ("shift", None)] + [("percentile", p) for p in PCTS]
KS = (1, 2, 64, 65, 1000, 1024)
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097)              # 4 097 crosses one tile of the select pass


# ---- the expected side: everything from the library's other calls on the same two snapshots ----------------------------
class Ref:
    """Rows [0, M) of the pair (base, cur): compare's arrays from its wave-per-row kernel and both snapshots' percentile
    buckets.  A call over fewer rows is a slice: each row's walk is its own."""

    def __init__(self, base, cur, M):
        self.M = M
        with shape("wave"):
            self.cmp = cur.compare(base, M)
        self.cand = (self.cmp["count_a"] != 0) & (self.cmp["count_b"] != 0)
        assert np.array_equal(self.cand, ~np.isnan(self.cmp["ks"]))
        self.pkey = [snap.extract(PCTS, M)["pkeys"].astype(np.int64).reshape(M, len(PCTS)) for snap in (base, cur)]
        self.pbin = [oracle.key_to_bin(k).astype(np.int64) for k in self.pkey]

    def score(self, by, arg):
        if by == "percentile":
            j = PCTS.index(arg)
            return (self.pbin[1][:, j] - self.pbin[0][:, j]).astype(np.float64)
        return self.cmp[by]

    def expected(self, by, arg, k, ascending, first=0, nmetrics=None):
        nmetrics = self.M - first if nmetrics is None else nmetrics
        ids = np.arange(first, first + nmetrics)
        ids = ids[self.cand[ids]]
        s = self.score(by, arg)[ids] + 0.0                    # -0.0 -> +0.0
        assert not np.isnan(s).any()
        return ids[np.lexsort((ids, s if ascending else -s))][:k].tolist()


def check(got, ref, by, arg, k, ascending, first=0, nmetrics=None):
    want = ref.expected(by, arg, k, ascending, first, nmetrics)
    what = (by, arg, k, ascending, first, nmetrics)
    assert got.dtype == N.MOVER_ENTRY and got.shape == (len(want),), what
    assert got["id"].tolist() == want, what
    w = np.array(want, dtype=np.int64)
    assert np.array_equal(got["count_a"], ref.cmp["count_a"][w]) and np.array_equal(got["count_b"], ref.cmp["count_b"][w]), what
    assert got["count_a"].all() and got["count_b"].all(), what
    if by == "percentile":
        j = PCTS.index(arg)
        assert np.array_equal(got["key"], ref.pkey[1][w, j]) and np.array_equal(got["key_base"], ref.pkey[0][w, j]), what
        assert np.array_equal(got["score"], ref.score(by, arg)[w]), what                   # exact integers
    else:
        assert np.array_equal(got["key"], ref.cmp["key"][w] if by == "ks" else np.zeros(len(w), dtype=np.int16)), what
        assert not got["key_base"].any(), what
        assert got["score"].tobytes() == np.ascontiguousarray(ref.cmp[by][w]).tobytes(), what
    return want


def run(base, cur, ref, by, arg, k, ascending=False, first=0, nmetrics=None):
    n = ref.M - first if nmetrics is None else nmetrics
    return check(cur.movers(base, k, by, arg, ascending, n, first), ref, by, arg, k, ascending, first, n)


def state(torch, e, snaps, M):
    from loghisto_amd import merge
    for s in snaps:
        torch.cuda.ExternalStream(s.stream()).synchronize()
    return ([s.device_cells() for s in snaps], [merge.snapshot_ranges(s, M).cpu().numpy().copy() for s in snaps],
            [[x.copy() for x in s.buckets_all(M)] for s in snaps], e.counters()["widenings"])


def same_state(a, b):
    return (a[0] == b[0] and a[3] == b[3] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and
            all(np.array_equal(x, y) for sa, sb in zip(a[2], b[2]) for x, y in zip(sa, sb)))


# ---- the crafted pairs of tests/test_gpu_compare.py ----------------------------------------------------------------------
@pytest.fixture(scope="module", params=["wide64", "wide32", "narrow32", "narrow_against_widened"])
def crafted(request, native_lib, torch_cuda):
    """The crafted pairs in two snapshots of one engine: imported (uint64 cells), written into the narrow store of a 32-bit
    engine (4-byte cells on both sides), or base narrow and cur imported (which widens cur only)."""
    kind = request.param
    big = kind in ("wide64", "wide32")
    pairs = crafted_pairs() + ([(k, a, b, "tight", "tight") for k, a, b in BIG] if big else [])
    rows = [[{k: v for k, v in p[i].items() if v} for p in pairs] for i in (1, 2)]
    spans = [[p[i] if p[i - 2] or p[i] != "tight" else None for p in pairs] for i in (3, 4)]   # tight over no cell: unmarked
    M = len(pairs)
    with engine(M, cell_bits=64 if kind == "wide64" else 32, num_buffers=3) as e:
        with e.flip() as base, e.flip() as cur:
            narrow = (kind.startswith("narrow"), kind == "narrow32")
            for snap, r, s, nar in ((base, rows[0], spans[0], narrow[0]), (cur, rows[1], spans[1], narrow[1])):
                if nar:
                    _write_narrow(torch_cuda, snap, r, s)
                else:
                    _import(snap, r, s)
            widths = (base.device_cells()[2], cur.device_cells()[2])
            assert widths == tuple(4 if nar else 8 for nar in narrow)
            assert rows_of(base, M) == rows[0] and rows_of(cur, M) == rows[1]
            yield types.SimpleNamespace(e=e, base=base, cur=cur, pairs=pairs, kinds=[p[0] for p in pairs], M=M,
                                        ref=Ref(base, cur, M), want=crafted_models(pairs, big), torch=torch_cuda)
            assert (base.device_cells()[2], cur.device_cells()[2]) == widths


def test_crafted_pairs(crafted):
    """Every score, both directions, every k; rows empty on one or both sides and rows never marked do not appear."""
    c = crafted
    ncand = sum(1 for w in c.want if w["w1"] is not None)
    assert int(c.ref.cand.sum()) == ncand and 0 < ncand < c.M
    for by, arg in BYS:
        for asc in (False, True):
            for k in KS:
                want = run(c.base, c.cur, c.ref, by, arg, k, asc)
                assert len(want) == min(k, ncand)
                assert all(c.want[m]["w1"] is not None for m in want)
    at = {k: m for m, k in enumerate(c.kinds)}
    # exact zeros: identical normalised distributions score 0 by every distance, and go in id order
    zeros = [at[k] for k in ("identical", "identical_scaled", "identical_loose_span", "one_bin_same", "span_1/20000", "span_1/20002")]
    for by in ("ks", "w1"):
        got = c.cur.movers(c.base, len(zeros), by, None, True, c.M)
        assert got["id"].tolist() == sorted(zeros) and not got["score"].any() and not got["key"].any()
    up = c.cur.movers(c.base, 1, "shift", None, False, c.M)
    down = c.cur.movers(c.base, 1, "shift", None, True, c.M)
    assert up["score"][0] > 0 > down["score"][0]
    if "argmax_by_one_in_2^122" in at:
        got = c.cur.movers(c.base, 1024, "ks", None, False, c.M)
        key = {int(e["id"]): int(e["key"]) for e in got}
        assert [int(oracle.key_to_bin(key[at[k]])) for k in ("argmax_by_one_in_2^122", "argmax_by_one_mirrored")] == [200, 200]
    # a sub-range returns absolute ids; the same snapshot twice scores 0 everywhere: the lowest candidates' ids
    for by, arg in BYS:
        want = run(c.base, c.cur, c.ref, by, arg, 5, False, 3, c.M - 7)
        assert all(3 <= m < c.M - 4 for m in want)
        for snap, col in ((c.base, "count_a"), (c.cur, "count_b")):
            same = snap.movers(snap, 7, by, arg, by == "w1", c.M)
            assert same["id"].tolist() == np.nonzero(c.ref.cmp[col])[0][:7].tolist() and not same["score"].any()


def test_crafted_scores_against_the_exact_model(crafted):
    """Independently of lh_compare: ks bit-equal to the model's, w1 and shift within 4 n 2^-53 (1 + w1) of the exact value."""
    c = crafted
    for by in ("ks", "w1", "shift"):
        got = c.cur.movers(c.base, 1024, by, None, False, c.M)
        assert sorted(got["id"].tolist()) == [m for m, w in enumerate(c.want) if w["w1"] is not None]
        for e in got:
            w = c.want[int(e["id"])]
            assert (int(e["count_a"]), int(e["count_b"])) == (w["count_a"], w["count_b"])
            if by == "ks":
                assert np.float64(e["score"]).tobytes() == np.float64(w["ks"]).tobytes(), (c.kinds[int(e["id"])], e["score"], w["ks"])
                assert int(e["key"]) == (0 if w["bin"] is None else int(oracle.bin_to_key(w["bin"])))
            else:
                tol = 4 * w["n"] * EPS * (1 + w["w1"])
                err = abs(Fraction(float(e["score"])) - w[by])
                print(f"{c.kinds[int(e['id'])]} {by}: got {e['score']!r} error {float(err):.3e} bound {float(tol):.3e}")
                assert np.isfinite(e["score"]) and err <= tol, (c.kinds[int(e["id"])], by, float(e["score"]), float(err), float(tol))


def test_crafted_percentile_buckets(crafted):
    """Of the data: the selected buckets are the ones the pairs were built around."""
    c = crafted
    at = {k: m for m, k in enumerate(c.kinds)}
    got = {int(e["id"]): e for e in c.cur.movers(c.base, 1024, "percentile", 1.0, False, c.M)}
    for kind, ba, bb in (("disjoint", 1010, 2500), ("one_bin_each_far", 65000, 3), ("both_ends", 65535, 65535), ("tie", 30, 40)):
        e = got[at[kind]]
        assert (int(oracle.key_to_bin(int(e["key_base"]))), int(oracle.key_to_bin(int(e["key"])))) == (ba, bb), kind
        assert e["score"] == bb - ba
    got = {int(e["id"]): e for e in c.cur.movers(c.base, 1024, "percentile", 0.0, True, c.M)}
    assert got[at["one_bin_each_far"]]["score"] == 3 - 65000 and got[at["both_ends_one_inside"]]["score"] == 1


def test_crafted_read_only(crafted):
    """Nothing of either snapshot moves, and lh_top / lh_compare (whose select pass and pair helpers this unit shares) give
    the same bytes before and after."""
    c, torch = crafted, crafted.torch
    snaps = (c.base, c.cur)
    before = state(torch, c.e, snaps, c.M)

    def others():
        with shape("wave"):
            w = c.cur.compare(c.base, c.M)
        with shape("block"):
            b = c.cur.compare(c.base, c.M)
        tops = [c.cur.top(k, by, arg, asc, c.M).tobytes() for by, arg in (("count", None), ("sum", None), ("percentile", 0.5),
                                                                         ("count_above", 250.0)) for k, asc in ((5, False), (1024, True))]
        return [w[k].tobytes() for k in sorted(w)] + [b[k].tobytes() for k in sorted(b)] + tops
    ref = others()
    ent = torch.zeros((1024 * 32,), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    for by, arg in BYS:
        for asc in (False, True):
            c.cur.movers(c.base, 1024, by, arg, asc, c.M)
            c.base.movers(c.cur, 3, by, arg, asc, c.M - 5, 2)
            c.cur.movers(c.base, 64, by, arg, asc, c.M, out=(ent, cnt))
    assert same_state(before, state(torch, c.e, snaps, c.M))
    assert others() == ref


# ---- row counts either side of the select pass's sizes: a dozen distinct pairs, repeated ---------------------------------
M_ROWS = 4097
DOZEN = [  # (base, cur), at most 3 cells each
    ({30000: 1}, {30000: 1}),                                  # identical: 0
    ({30000: 2, 30010: 2}, {30005: 1, 30020: 3}),              # moved up
    ({30005: 1, 30020: 3}, {30000: 2, 30010: 2}),              # moved down
    ({30000: 5}, {}),                                          # empty in cur: never a candidate
    ({}, {31000: 2}),                                          # empty in base
    ({}, {}),                                                  # never marked
    ({29000: 1, 29300: 1}, {29000: 1, 29300: 3}),              # two steps of the walk
    ({100: 4, 40000: 4}, {100: 4, 40001: 4}),                  # a wide span
    ({30000: 3, 30001: 1}, {30001: 4}),
    ({32000: 1, 32100: 1, 32200: 2}, {32050: 2, 32150: 2}),
    ({30000: 1 << 33}, {30000: 1, 30002: 1}),                  # a count beyond 2^32
    ({30002: 7}, {30000: 7}),                                  # two buckets down: ks 1, w1 2, shift -2
]
NONE_FROM, NONE_TO = 2000, 2100                                # rows without a candidate
ALL_FROM, ALL_TO = 3000, 3100                                  # rows that are all candidates, all alike


def dozen_rows():
    pairs = [DOZEN[m % len(DOZEN)] for m in range(M_ROWS)]
    for m in range(NONE_FROM, NONE_TO):
        pairs[m] = DOZEN[3 + m % 3]
    for m in range(ALL_FROM, ALL_TO):
        pairs[m] = DOZEN[1]
    return [dict(p[0]) for p in pairs], [dict(p[1]) for p in pairs]


@pytest.fixture(scope="module")
def tiled(native_lib, torch_cuda):
    ra, rb = dozen_rows()
    with engine(M_ROWS, cell_bits=64, num_buffers=3) as e:
        with e.flip() as base, e.flip() as cur:
            _import(base, ra, ["tight"] * M_ROWS)
            _import(cur, rb, ["tight"] * M_ROWS)
            ref = Ref(base, cur, M_ROWS)
            assert int(ref.cand.sum()) > 3000 and not ref.cand[NONE_FROM:NONE_TO].any() and ref.cand[ALL_FROM:ALL_TO].all()
            w = model(*DOZEN[11])
            assert (w["ks"], w["w1"], w["shift"]) == (1.0, 2, -2)
            assert (ref.cmp["ks"][11], ref.cmp["w1"][11], ref.cmp["shift"][11]) == (1.0, 2.0, -2.0)
            yield types.SimpleNamespace(e=e, base=base, cur=cur, ref=ref, torch=torch_cuda)


@pytest.mark.parametrize("nmetrics", SIZES)
def test_sizes(tiled, nmetrics):
    """Every nmetrics x k, every score, both directions: most scores tie exactly, and the id rule decides."""
    t = tiled
    for k in KS:
        for by, arg in BYS:
            for asc in (False, True):
                run(t.base, t.cur, t.ref, by, arg, k, asc, 0, nmetrics)


def test_ties_at_the_cut_go_to_the_lowest_ids(tiled):
    """The leading score is shared by some 300 rows, far more than k leaves room for: its lowest ids win, in both directions."""
    t = tiled
    ids = np.nonzero(t.ref.cand)[0]
    for by, arg in (("ks", None), ("w1", None), ("shift", None), ("percentile", 0.5), ("percentile", 1.0)):
        s = t.ref.score(by, arg)[ids] + 0.0
        for asc in (False, True):
            group = ids[s == (s.min() if asc else s.max())].tolist()
            assert len(group) > 250, (by, asc)
            for k in (1, 64, 65, 250):
                assert run(t.base, t.cur, t.ref, by, arg, k, asc) == group[:k], (by, asc, k)
    assert t.ref.cmp["shift"][ids].min() < 0 < t.ref.cmp["shift"][ids].max()              # names that moved down and up


def test_fewer_candidates_than_k_and_none_at_all(tiled):
    t, torch = tiled, tiled.torch
    for first, n in ((0, 63), (0, 1023), (NONE_FROM - 20, 150), (NONE_TO - 1, 2)):
        have = int(t.ref.cand[first:first + n].sum())
        assert 0 < have < n
        for by, arg in BYS:
            assert len(run(t.base, t.cur, t.ref, by, arg, 1024, False, first, n)) == have
    for by, arg in BYS:
        for first, n in ((NONE_FROM, NONE_TO - NONE_FROM), (NONE_FROM + 3, 1), (3, 1), (4, 2)):
            out = host_arrays(torch, False, (8,), N.MOVER_ENTRY)
            got = t.cur.movers(t.base, 8, by, arg, False, n, first, out=out)
            assert got.size == 0 and np.all(out.view(np.uint8) == 0x77), (by, first, n)     # n_out == 0, out untouched


def test_sub_ranges_return_absolute_ids(tiled):
    t = tiled
    for first, n, k in ((1, 1, 5), (2, 62, 7), (777, 1025, 65), (M_ROWS - 1, 1, 2), (1500, 2597, 1000), (4090, 7, 1024)):
        for by, arg in BYS:
            for asc in (False, True):
                want = run(t.base, t.cur, t.ref, by, arg, k, asc, first, n)
                assert all(first <= m < first + n for m in want)


def test_the_same_snapshot_twice(tiled):
    """base is cur: every candidate scores 0 and the lowest ids win, in both directions."""
    t = tiled
    for by, arg in BYS:
        for asc in (False, True):
            for k in (1, 64, 100):
                got = t.cur.movers(t.cur, k, by, arg, asc, ALL_TO - ALL_FROM, ALL_FROM)
                assert got["id"].tolist() == list(range(ALL_FROM, ALL_FROM + k)) and not got["score"].any()
                assert np.array_equal(got["count_a"], got["count_b"]) and got["count_a"].all()
            got = t.base.movers(t.base, 1024, by, arg, asc, 1025)
            assert got["id"].tolist() == np.nonzero(t.ref.cmp["count_a"][:1025])[0].tolist()[:1024] and not got["score"].any()


def test_device_form_equals_host_form(tiled):
    t, torch = tiled, tiled.torch
    for (by, arg), k, asc, first, n in ((BYS[0], 64, False, 0, M_ROWS), (BYS[1], 1024, True, 5, 2000), (BYS[2], 1000, False, 0, 1025),
                                        (BYS[4], 65, True, 100, 63), (BYS[6], 1024, False, NONE_FROM - 10, 120),
                                        (BYS[0], 7, False, NONE_FROM, 50)):
        ent = torch.full((k * 32,), 0x77, dtype=torch.uint8, device="cuda")
        cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert t.cur.movers(t.base, k, by, arg, asc, n, first, out=(ent, cnt)) == (ent, cnt)
        host = t.cur.movers(t.base, k, by, arg, asc, n, first)
        torch.cuda.ExternalStream(t.cur.stream()).synchronize()
        nout, raw = cnt.cpu().numpy(), ent.cpu().numpy()
        assert nout.tolist() == [host.size, -1]
        assert raw[:host.size * 32].tobytes() == host.tobytes() and np.all(raw[host.size * 32:] == 0x77)   # the sentinel stays
        check(host, t.ref, by, arg, k, asc, first, n)
    for pinned in (True, False):                                   # the host form into the caller's array, either kind
        out = host_arrays(torch, pinned, (100,), N.MOVER_ENTRY)
        got = t.cur.movers(t.base, 100, "w1", None, False, 90, 0, out=out)
        want = check(got, t.ref, "w1", None, 100, False, 0, 90)
        assert len(want) < 90 and np.all(out.view(np.uint8)[len(want) * 32:] == 0x77)


def test_range_errors_and_the_empty_call(tiled):
    import loghisto_amd
    t, M, torch = tiled, M_ROWS, tiled.torch
    for first, n in ((0, M + 1), (M, 1), (M + 1, 0), (M - 1, 2)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            t.cur.movers(t.base, 3, "ks", None, False, n, first)
        assert ei.value.code == N.ERANGE, (first, n)
    out = np.zeros(4, dtype=N.MOVER_ENTRY)
    n_out = C.c_size_t(99)
    L = N.lib()
    for first, n in ((1, (1 << 32) - 1), (0xffffffff, 1)):                               # sums that wrap
        assert L.lh_movers(t.base._h, t.cur._h, first, n, 0, 0.0, 4, 0, out.ctypes.data, C.addressof(n_out)) == N.ERANGE
    assert n_out.value == 99 and not out.view(np.uint8).any()
    for first in (0, M):                                                                 # nmetrics == 0: LH_OK, n_out = 0
        n_out.value = 99
        assert L.lh_movers(t.base._h, t.cur._h, first, 0, 0, 0.0, 4, 0, out.ctypes.data, C.addressof(n_out)) == 0
        assert n_out.value == 0
    assert not out.view(np.uint8).any()
    cnt = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    ent = torch.zeros((128,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.lh_movers_device(t.base._h, t.cur._h, 0, 0, 0, 0.0, 4, 0, ent.data_ptr(), cnt.data_ptr()) == 0
    torch.cuda.ExternalStream(t.cur.stream()).synchronize()
    assert int(cnt.cpu()[0]) == 0 and not ent.cpu().numpy().any()


def test_the_timing_hook_runs_both_passes(tiled):
    t = tiled
    a, b = C.c_float(-1.0), C.c_float(-1.0)
    assert N.lib().lh_tool_movers_passes_ms(t.base._h, t.cur._h, 0, M_ROWS, 1, 0.0, 20, 0, C.byref(a), C.byref(b)) == 0
    assert a.value > 0 and b.value > 0
    run(t.base, t.cur, t.ref, "w1", None, 20)                                            # the unit's blocks are as they were


# ---- two engines on one device: two streams ------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_two_engines(native_lib, torch_cuda, bits):
    """A snapshot of an engine of 300 names against one of an engine of 200 (its stream is another one: the unit orders the
    two), in both argument orders: results as for one engine; rows beyond either engine's are LH_ERANGE."""
    import loghisto_amd
    rng = np.random.default_rng(bits)
    sets = []
    for M, mu in ((300, 3.0), (200, 3.4)):
        ids = rng.integers(0, M - 3, 30_000).astype(np.uint32)                           # the last three names stay empty
        sets.append((ids, rng.lognormal(mu + 0.002 * (ids % 50), 0.8, ids.size)))
    with engine(300, cell_bits=bits, num_buffers=3) as e1, engine(200, cell_bits=bits, num_buffers=3) as e2:
        e1.submit_pairs(*sets[0])
        e2.submit_pairs(*sets[1])
        with e1.flip() as s1, e2.flip() as s2:
            assert s1.stream() != s2.stream() and s1.device_cells()[2] == s2.device_cells()[2] == bits // 8
            for base, cur in ((s1, s2), (s2, s1)):
                ref = Ref(base, cur, 200)
                assert int(ref.cand.sum()) == 197
                for by, arg in BYS:
                    for asc in (False, True):
                        for k, first, n in ((20, 0, 200), (1024, 0, 200), (64, 50, 150)):
                            run(base, cur, ref, by, arg, k, asc, first, n)
                ent = torch_cuda.full((20 * 32,), 0x77, dtype=torch_cuda.uint8, device="cuda")
                cnt = torch_cuda.full((1,), -1, dtype=torch_cuda.int32, device="cuda")
                torch_cuda.cuda.synchronize()
                cur.movers(base, 20, "w1", None, False, 200, out=(ent, cnt))
                torch_cuda.cuda.ExternalStream(cur.stream()).synchronize()
                assert int(cnt.cpu()[0]) == 20
                assert ent.cpu().numpy().tobytes() == cur.movers(base, 20, "w1", None, False, 200).tobytes()
                for first, n in ((0, 250), (50, 200), (200, 1)):
                    with pytest.raises(loghisto_amd.LhError) as ei:
                        cur.movers(base, 5, "ks", None, False, n, first)
                    assert ei.value.code == N.ERANGE, (first, n)
            assert s1.device_cells()[2] == s2.device_cells()[2] == bits // 8
