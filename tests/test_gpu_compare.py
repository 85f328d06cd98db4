"""lh_compare / lh_compare_device (Snapshot.compare): per name, how the distribution in one snapshot differs from the one in
another -- the totals, the Kolmogorov-Smirnov distance with the bin it is reached at (chosen in exact integers, the lowest
among equals), and the earth mover's distance in buckets with its signed form.

The expected values are Python integers and fractions.Fraction over Snapshot.buckets_all of both snapshots (a path the
other tests hold to the oracle).  On engines of 64- and 32-bit cells and under both kernel shapes (lh_tool_compare_switch):
  count_a, count_b, key, below_a, below_b   equal to the model
  ks                                        bit-equal to fabs(float64(A) / float64(na) - float64(B) / float64(nb)) in numpy
  w1, shift                                 |got - exact| <= 4 n 2^-53 (1 + exact w1), n = the bins from the lowest to the
                                            highest occupied cell of the two rows (a subset of the union span: outside it
                                            every term is an exact zero).  Each term carries at most three roundings of
                                            values <= 1; a sum of n terms adds at most n 2^-53 relative to the sum of |terms|.
No test here can put the two snapshots on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib
import ctypes as C
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests import _cells32_rows as R
from tests.test_gpu_count_le import engine, host_arrays

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
SHAPES = {"wave": 1, "block": 1 << 30}
BITS = (64, 32)
EPS = Fraction(1, 1 << 53)
FIELDS = dict(count_a=U64, count_b=U64, ks=np.float64, key=np.int16, below_a=U64, below_b=U64, w1=np.float64, shift=np.float64)


@contextlib.contextmanager
def shape(name):
    """Put every call through one kernel shape, whatever the number of rows; the previous value comes back afterwards."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    assert N.lib().lh_tool_compare_switch(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_compare_switch(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


# ---- the model -----------------------------------------------------------------------------------------------------------
def model(a, b):
    """a, b: {bin: count} of base and cur.  X changes at occupied bins only, so the lowest bin of its maximum is an occupied
    one, and a run of bins up to the next occupied one adds its length times the term."""
    na, nb = sum(a.values()), sum(b.values())
    assert na < 1 << 64 and nb < 1 << 64
    out = dict(count_a=na, count_b=nb, ks=math.nan, bin=None, below_a=0, below_b=0, w1=None, shift=None, n=0)
    if na == 0 or nb == 0:
        return out
    bins = sorted(set(a) | set(b))
    best, A, B, w1, shift = 0, 0, 0, 0, 0                    # the sums in units of 1 / (na nb)
    for i, j in enumerate(bins):
        A += a.get(j, 0)
        B += b.get(j, 0)
        d = A * nb - B * na
        if abs(d) > best:
            best = abs(d)
            out.update(bin=j, below_a=A, below_b=B)
        run = (bins[i + 1] if i + 1 < len(bins) else j + 1) - j
        w1 += abs(d) * run
        shift += d * run
    with np.errstate(all="raise"):
        out["ks"] = 0.0 if best == 0 else float(np.abs(np.float64(out["below_a"]) / np.float64(na) -
                                                       np.float64(out["below_b"]) / np.float64(nb)))
    out.update(w1=Fraction(w1, na * nb), shift=Fraction(shift, na * nb), n=bins[-1] - bins[0] + 1, x=best)
    return out


def rows_of(snap, M, first=0):
    off, keys, counts = snap.buckets_all(M, first)
    bins = (keys.astype(np.int64) & 0xffff) ^ 0x8000
    return [{int(j): int(c) for j, c in zip(bins[int(off[m]):int(off[m + 1])], counts[int(off[m]):int(off[m + 1])])}
            for m in range(M)]


def check(got, want, what=""):
    """got: Snapshot.compare's dict; want: the models of the same rows."""
    assert all(got[k].dtype == t and got[k].shape == (len(want),) for k, t in FIELDS.items())
    for m, w in enumerate(want):
        at = (what, m)
        assert int(got["count_a"][m]) == w["count_a"] and int(got["count_b"][m]) == w["count_b"], at
        if w["w1"] is None:                                        # one side is empty
            assert math.isnan(got["ks"][m]) and math.isnan(got["w1"][m]) and math.isnan(got["shift"][m]), at
            assert math.isnan(got["ks_value"][m]), at
            assert got["key"][m] == 0 and got["below_a"][m] == 0 and got["below_b"][m] == 0, at
            continue
        key = 0 if w["bin"] is None else int(oracle.bin_to_key(w["bin"]))
        assert int(got["key"][m]) == key, (at, int(oracle.key_to_bin(int(got["key"][m]))), w["bin"])
        assert int(got["below_a"][m]) == w["below_a"] and int(got["below_b"][m]) == w["below_b"], at
        assert np.float64(got["ks"][m]).tobytes() == np.float64(w["ks"]).tobytes(), (at, got["ks"][m], w["ks"])
        assert got["ks_value"][m] == oracle.decompress(key), at
        tol = 4 * w["n"] * EPS * (1 + w["w1"])
        for f in ("w1", "shift"):
            err = abs(Fraction(float(got[f][m])) - w[f])
            print(f"{what} row {m} {f}: got {got[f][m]!r} error {float(err):.3e} bound {float(tol):.3e}")
            assert math.isfinite(got[f][m]) and err <= tol, (at, f, got[f][m], float(w[f]), float(err), float(tol))
        assert abs(got["shift"][m]) <= got["w1"][m] * (1 + 2.0 ** -40), at
        if w["bin"] is None:                                       # identical normalised distributions: exactly 0
            assert got["ks"][m] == 0 and got["w1"][m] == 0 and got["shift"][m] == 0, at


# ---- crafted pairs of rows -----------------------------------------------------------------------------------------------
def _full(step):
    return {b: 1 + b % 3 for b in range(0, NK, step)}


def crafted_pairs():
    """(kind, a, b, span_a, span_b): span 'tight', None (never marked) or (lo, hi) marked besides the cells."""
    P = []

    def add(kind, a, b, sa="tight", sb="tight"):
        P.append((kind, a, b, sa, sb))

    add("identical", {100: 3, 200: 5}, {100: 3, 200: 5})
    add("identical_scaled", {100: 1, 200: 2, 777: 4}, {100: 3, 200: 6, 777: 12})
    add("identical_loose_span", {1000: 3, 1100: 5}, {1000: 3, 1100: 5}, (900, 1300), "tight")
    add("disjoint", {1000: 2, 1010: 3}, {2000: 1, 2500: 4})                    # ks 1 at 1 010, w1 = 4 + 990 + 400
    add("disjoint_swapped", {2000: 1, 2500: 4}, {1000: 2, 1010: 3})
    add("tie", {10: 1, 30: 1}, {20: 1, 40: 1})                                  # X = 2 at bins 10 and 30: bin 10
    add("tie_same_lane", {8: 1, 10: 1}, {9: 1, 11: 1})
    add("tie_lanes_of_one_step", {1000: 1, 1100: 1}, {1050: 1, 1150: 1})
    add("tie_two_steps", {5010: 1, 5310: 1}, {5160: 1, 5510: 1})               # steps start at 5 008: 5 010 and 5 310 differ
    add("tie_many_steps", {6001: 1, 9001: 1}, {7501: 1, 12001: 1})
    add("tie_same_wave_of_a_workgroup", {6001: 1, 10097: 1}, {8000: 1, 12000: 1})       # chunks 0 and 16; then 0 and 32
    add("tie_chunks_0_32", {6001: 1, 14233: 1}, {9000: 1, 15000: 1})
    # the span starts at 400: bin 600 is lane 50 of step 0, bin 664 lane 2 of step 1 -- the higher lane holds the lower bin
    add("tie_higher_lane_holds_the_lower_bin", {600: 1, 664: 1}, {630: 1, 690: 1}, (400, 700), "tight")
    add("one_bin_same", {500: 7}, {500: 3})
    add("one_bin_each", {500: 7}, {501: 3})
    add("one_bin_each_far", {65000: 7}, {3: 3})
    for w in (1, 255, 256, 257, 1025):                                          # the union span's width in bins
        for lo in (20000, 20002):
            if w == 1:
                add(f"span_{w}/{lo}", {lo: 1}, {lo: 5})
            else:
                add(f"span_{w}/{lo}", {lo: 2, lo + w // 2: 1}, {lo + w // 3: 1, lo + w - 1: 3})
    for r in range(4):                                                          # every lo % 4 and (hi - lo) % 4
        for g in range(4):
            lo, w = 4000 + 64 * (4 * r + g) + r, 9 + g
            add(f"lo{r}_w{g}", {lo: 1, lo + 3: 2}, {lo + 1: 1, lo + w - 1: 2})
            add(f"lo{r}_w{g}_b_inside", {lo: 1, lo + w - 1: 2}, {lo + 2: 1, lo + 5: 2})
    add("both_ends", {0: 1, NK - 1: 2}, {0: 2, NK - 1: 1})
    add("both_ends_one_inside", {0: 1, NK - 1: 2}, {1: 2, NK - 2: 1})
    add("full_span_row", _full(1), {30000: 5, 40000: 1})
    add("full_span_row_cur", {123: 1}, _full(1))
    add("sparse_full_both", _full(97), _full(101))
    add("a_empty", {}, {100: 1})
    add("b_empty", {100: 1, 5000: 2}, {})
    add("both_empty", {}, {})
    add("never_marked", {}, {}, None, None)
    add("never_marked_a", {}, {4321: 2}, None, "tight")
    add("marked_zero_both", {}, {}, (700, 1200), (30000, 30001))
    add("marked_zero_a", {}, {800: 1}, (700, 1200), "tight")
    add("marked_zero_wide_b", {800: 1, 900: 1}, {}, "tight", (0, NK - 1))
    add("loose_spans", {40001: 2, 40100: 1}, {40050: 3}, (39000, 42000), (0, NK - 1))
    return P


BIG = [  # wide cells only: A nb needs more than 64 bits
    ("cells_2^40_2^62", {100: 1 << 40, 200: 1 << 62, 300: (1 << 53) + 1}, {150: 1 << 61, 250: (1 << 62) + 12345, 400: 1 << 41}),
    ("three_of_2^62", {7: 1 << 62, 8: 1 << 62, 60000: 1 << 62}, {7: 1 << 40, 9: (1 << 62) - 1, 65535: 1 << 50}),
    # X(100) = 2^61 nb, X(200) = X(100) + 1 (nb = na + 1: (A + 1) nb - 1 na = A nb + 1), everything later is smaller: the
    # larger X sits at the HIGHER bin, and float64 cannot tell the two apart
    ("argmax_by_one_in_2^122", {100: 1 << 61, 200: 1, 300: 1 << 40}, {150: 1, 250: (1 << 61) + (1 << 40) + 1}),
    ("argmax_by_one_mirrored", {150: 1, 250: (1 << 61) + (1 << 40) + 1}, {100: 1 << 61, 200: 1, 300: 1 << 40}),
]


def test_the_argmax_pair_is_what_it_claims():
    for kind, a, b in BIG[2:]:
        if kind.endswith("mirrored"):
            a, b = b, a
        na, nb = sum(a.values()), sum(b.values())
        x100, x200 = (1 << 61) * nb, ((1 << 61) + 1) * nb - na
        assert nb == na + 1 and x200 == x100 + 1 and float(x100) == float(x200) and x100 > 1 << 100
        w = model(a, b)
        assert w["bin"] == 200 and w["x"] == x200


def _import(snap, rows, spans):
    ids = np.concatenate([np.full(len(r), m, dtype=np.uint32) for m, r in enumerate(rows)])
    bins = np.concatenate([np.array(sorted(r), dtype=np.int64) for r in rows])
    counts = np.concatenate([np.array([r[b] for b in sorted(r)], dtype=U64) for r in rows])
    snap.add_buckets(ids, oracle.bin_to_key(bins).astype(np.int16), counts)
    for m, s in enumerate(spans):
        if isinstance(s, tuple):
            snap.mark_dirty(m, 1, s[0], s[1])


def _write_narrow(torch, snap, rows, spans):
    """Straight into the uint32 cells (an import would widen the snapshot), as tests/test_gpu_cells32_readers.py does."""
    from tests.test_gpu_cells32_readers import _row_view
    ptr, nrows, cb = snap.device_cells()
    assert cb == 4 and nrows >= len(rows)
    stride = snap.row_stride()
    for m, (cells, s) in enumerate(zip(rows, spans)):
        cells = {b: c for b, c in cells.items() if c}
        if s is None:
            assert not cells
            continue
        row = R.Row(f"row{m}", cells, s)
        if row.bins.size:
            lo, hi = row.span
            _row_view(torch, ptr, m, stride)[lo:hi + 1] = torch.from_numpy(row.window().view(np.int32)).cuda()
    torch.cuda.synchronize()
    for m, (cells, s) in enumerate(zip(rows, spans)):
        if s is not None:
            keys = [b for b, c in cells.items() if c]
            lo, hi = (min(keys), max(keys)) if s == "tight" else s
            snap.mark_dirty(m, 1, lo, hi)


_WANT = {}


def crafted_models(pairs, tag):
    if tag not in _WANT:
        _WANT[tag] = [model({k: v for k, v in a.items() if v}, {k: v for k, v in b.items() if v}) for _, a, b, *_ in pairs]
    return _WANT[tag]


@pytest.fixture(scope="module", params=["wide64", "wide32", "narrow32"])
def crafted(request, native_lib, torch_cuda):
    """The crafted pairs in two snapshots of one engine: imported (uint64 cells; on the 32-bit engine the import widens both
    snapshots) or written into the narrow store of a 32-bit engine (4-byte cells on both sides)."""
    pairs = crafted_pairs() + ([(k, a, b, "tight", "tight") for k, a, b in BIG] if request.param != "narrow32" else [])
    rows = [[{k: v for k, v in p[i].items() if v} for p in pairs] for i in (1, 2)]
    spans = [[p[i] if p[i - 2] or p[i] != "tight" else None for p in pairs] for i in (3, 4)]   # tight over no cell: unmarked
    with engine(len(pairs), cell_bits=64 if request.param == "wide64" else 32, num_buffers=3) as e:
        with e.flip() as base, e.flip() as cur:
            for snap, r, s in ((base, rows[0], spans[0]), (cur, rows[1], spans[1])):
                if request.param == "narrow32":
                    _write_narrow(torch_cuda, snap, r, s)
                else:
                    _import(snap, r, s)
            width = 4 if request.param == "narrow32" else 8
            assert base.device_cells()[2] == width and cur.device_cells()[2] == width
            # buckets_all returns what was put in: the model below is the model of the snapshots
            assert rows_of(base, len(pairs)) == rows[0] and rows_of(cur, len(pairs)) == rows[1]
            yield types.SimpleNamespace(e=e, base=base, cur=cur, pairs=pairs, kinds=[p[0] for p in pairs], width=width,
                                        want=crafted_models(pairs, request.param != "narrow32"), torch=torch_cuda)
            assert base.device_cells()[2] == width and cur.device_cells()[2] == width


@pytest.mark.parametrize("kind", list(SHAPES))
def test_crafted_pairs(crafted, kind):
    c = crafted
    M = len(c.pairs)
    with shape(kind):
        got = c.cur.compare(c.base, M)
    check(got, c.want, kind)
    at = {k: m for m, k in enumerate(c.kinds)}

    def bin_of(k):
        return int(oracle.key_to_bin(int(got["key"][at[k]])))

    for k in ("identical", "identical_scaled", "identical_loose_span", "one_bin_same", "span_1/20000", "span_1/20002"):
        m = at[k]
        assert got["ks"][m] == 0 and got["w1"][m] == 0 and got["shift"][m] == 0 and got["key"][m] == 0, k
        assert got["below_a"][m] == 0 and got["below_b"][m] == 0, k
    m = at["disjoint"]
    assert got["ks"][m] == 1.0 and bin_of("disjoint") == 1010 and (got["below_a"][m], got["below_b"][m]) == (5, 0)
    assert abs(got["w1"][m] - 1394.0) <= 1e-9 and abs(got["shift"][m] - 1394.0) <= 1e-9
    m = at["disjoint_swapped"]
    assert got["ks"][m] == 1.0 and bin_of("disjoint_swapped") == 1010 and abs(got["shift"][m] + 1394.0) <= 1e-9
    assert [bin_of(k) for k in ("tie", "tie_same_lane", "tie_lanes_of_one_step", "tie_two_steps", "tie_many_steps",
                                "tie_same_wave_of_a_workgroup", "tie_chunks_0_32",
                                "tie_higher_lane_holds_the_lower_bin")] == [10, 8, 1000, 5010, 6001, 6001, 6001, 600]
    assert bin_of("one_bin_each") == 500 and got["ks"][at["one_bin_each"]] == 1.0
    assert bin_of("one_bin_each_far") == 3 and got["shift"][at["one_bin_each_far"]] < 0
    if "argmax_by_one_in_2^122" in at:
        assert bin_of("argmax_by_one_in_2^122") == 200 and bin_of("argmax_by_one_mirrored") == 200
    # a sub-range and the same snapshot twice
    f, n = 3, M - 7
    with shape(kind):
        part = c.cur.compare(c.base, n, f)
        same = c.base.compare(c.base, M)
    for k in FIELDS:
        assert part[k].tobytes() == got[k][f:f + n].tobytes(), k
    for m, w in enumerate(c.want):
        if w["count_a"]:
            assert same["ks"][m] == 0 and same["w1"][m] == 0 and same["shift"][m] == 0 and same["key"][m] == 0, m
            assert same["count_a"][m] == same["count_b"][m] == w["count_a"]
        else:
            assert math.isnan(same["ks"][m]) and math.isnan(same["w1"][m]) and math.isnan(same["shift"][m]), m


# ---- a mixed ingested stream: two intervals ------------------------------------------------------------------------------
M_MIXED = 300


def interval(seed, mu, sigma, absent):
    rng = np.random.default_rng(seed)
    n = 60_000
    ids = rng.integers(0, M_MIXED, n).astype(np.uint32)
    v = rng.lognormal(mu, sigma, n) * np.exp(0.01 * (ids % 7))
    v[rng.random(n) < 0.05] *= -1.0
    keep = ~np.isin(ids, absent)
    return ids[keep], v[keep]


@pytest.fixture(scope="module", params=BITS)
def mixed(request, native_lib, torch_cuda):
    """Interval 1 (base) and interval 2 (cur) of one engine; names 5 and 17 are missing from the first, 17 and 40 from the
    second.  On the 32-bit engine both snapshots keep 4-byte cells."""
    with engine(M_MIXED, cell_bits=request.param, num_buffers=3) as e:
        e.submit_pairs(*interval(11, 3.0, 0.7, [5, 17]))
        with e.flip() as base:
            e.submit_pairs(*interval(12, 3.2, 0.9, [17, 40]))
            with e.flip() as cur:
                e.sync()
                assert base.device_cells()[2] == cur.device_cells()[2] == request.param // 8
                ra, rb = rows_of(base, M_MIXED), rows_of(cur, M_MIXED)
                assert not ra[5] and not ra[17] and not rb[17] and not rb[40] and ra[40] and rb[5]
                yield types.SimpleNamespace(e=e, base=base, cur=cur, ra=ra, rb=rb, torch=torch_cuda, bits=request.param,
                                            want=[model(a, b) for a, b in zip(ra, rb)])


@pytest.mark.parametrize("kind", list(SHAPES))
def test_mixed_stream(mixed, kind):
    c = mixed
    with shape(kind):
        got = c.cur.compare(c.base, M_MIXED)
        back = c.base.compare(c.cur, M_MIXED)
        same = c.cur.compare(c.cur, M_MIXED)
    check(got, c.want, kind)
    assert np.nanmax(got["ks"]) > 0.05 and np.nanmedian(got["shift"]) > 0       # the second interval sits higher
    ok = ~np.isnan(got["ks"])
    assert ok.sum() == M_MIXED - 3 and not ok[[5, 17, 40]].any()
    assert np.all(same["ks"][ok] == 0) and np.all(same["w1"][ok] == 0) and np.all(same["shift"][ok] == 0)
    # base and cur swapped: X is the same integer, so the bin, ks and every |term| are; shift changes its sign
    assert np.array_equal(back["key"], got["key"]) and back["ks"].tobytes() == got["ks"].tobytes()
    assert back["w1"].tobytes() == got["w1"].tobytes()
    assert np.array_equal(back["below_a"], got["below_b"]) and np.array_equal(back["count_b"], got["count_a"])
    for m, w in enumerate(c.want):
        if w["w1"] is not None:
            assert abs(Fraction(float(back["shift"][m])) + w["shift"]) <= 4 * w["n"] * EPS * (1 + w["w1"]), m


def _device_form(torch, cur, base, n, first=0, names=tuple(FIELDS)):
    kinds = dict(count_a=torch.int64, count_b=torch.int64, ks=torch.float64, key=torch.int16, below_a=torch.int64,
                 below_b=torch.int64, w1=torch.float64, shift=torch.float64)
    out = {k: torch.full((n,), 77, dtype=kinds[k], device="cuda") for k in names}
    torch.cuda.synchronize()
    back = cur.compare(base, n, first, out=out)
    torch.cuda.ExternalStream(cur.stream()).synchronize()
    assert all(back[k] is out[k] for k in names)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("kind", list(SHAPES))
def test_forms_and_read_only(mixed, kind):
    """Device form == host form byte for byte, pinned == pageable, sub-ranges, outputs left out, and nothing moves."""
    from loghisto_amd import merge
    c, torch, M = mixed, mixed.torch, M_MIXED
    snaps = (c.base, c.cur)
    cells = [s.device_cells() for s in snaps]
    widenings = c.e.counters()["widenings"]
    ranges = [merge.snapshot_ranges(s, M).cpu().numpy().copy() for s in snaps]
    before = [[x.copy() for x in s.buckets_all(M)] for s in snaps]
    with shape(kind):
        host = c.cur.compare(c.base, M)
        dev = _device_form(torch, c.cur, c.base, M)
        for k in FIELDS:
            assert dev[k].tobytes() == host[k].tobytes(), k
        f, n = 37, 201                                                            # first > 0, both forms
        part, dpart = c.cur.compare(c.base, n, f), _device_form(torch, c.cur, c.base, n, f)
        for k in FIELDS:
            assert part[k].tobytes() == host[k][f:f + n].tobytes() == dpart[k].tobytes(), k
        for pinned in (True, False):                                              # the host form's two ways back
            out = {k: host_arrays(torch, pinned, (M,), t) for k, t in FIELDS.items()}
            c.cur.compare(c.base, M, out=out)
            for k in FIELDS:
                assert out[k].tobytes() == host[k].tobytes(), (pinned, k)
        for names in (("key",), ("ks", "key"), ("count_b", "w1"), ("count_a", "below_a", "below_b", "shift"),
                      tuple(k for k in FIELDS if k != "key")):                    # NULL for the others
            d = _device_form(torch, c.cur, c.base, M, names=names)
            for pinned in (True, False):
                out = {k: host_arrays(torch, pinned, (M,), FIELDS[k]) for k in names}
                got = c.cur.compare(c.base, M, out=out)
                assert set(got) - {"ks_value"} == set(names)
                for k in names:
                    assert out[k].tobytes() == host[k].tobytes() == d[k].tobytes(), (names, pinned, k)
        # through ctypes: outputs that are NULL are not touched, and neither is anything on an empty call
        guard = np.full(M, 7, dtype=U64)
        ks = np.zeros(M)
        L = N.lib()
        assert L.lh_compare(c.base._h, c.cur._h, 0, M, 0, 0, 0, ks.ctypes.data, 0, 0, 0, 0, 0) == 0
        assert ks.tobytes() == host["ks"].tobytes()
        for first in (0, M):
            assert L.lh_compare(c.base._h, c.cur._h, first, 0, 0, guard.ctypes.data, 0, 0, 0, 0, 0, 0, 0) == 0
        assert np.all(guard == 7)
    after = [s.buckets_all(M) for s in snaps]
    for b, a in zip(before, after):
        assert len(b) == len(a) and all(np.array_equal(x, y) for x, y in zip(b, a))
    assert [s.device_cells() for s in snaps] == cells and cells[0][2] == cells[1][2] == c.bits // 8
    assert all(np.array_equal(merge.snapshot_ranges(s, M).cpu().numpy(), r) for s, r in zip(snaps, ranges))
    assert c.e.counters()["widenings"] == widenings


def test_range_errors(mixed):
    import loghisto_amd
    c, M = mixed, M_MIXED
    for first, k in ((0, M + 1), (M, 1), (M + 1, 0), (M - 1, 2)):
        with pytest.raises(loghisto_amd.LhError) as ei:
            c.cur.compare(c.base, k, first)
        assert ei.value.code == N.ERANGE, (first, k)
    out = np.full(4, 7, dtype=U64)
    for first, k in ((1, (1 << 32) - 1), (0xffffffff, 1), (1, (1 << 64) - 1)):    # sums that wrap
        assert N.lib().lh_compare(c.base._h, c.cur._h, first, k, 0, out.ctypes.data, 0, 0, 0, 0, 0, 0, 0) == N.ERANGE
    assert N.lib().lh_compare(c.base._h, c.cur._h, 0, 1, 4, out.ctypes.data, 0, 0, 0, 0, 0, 0, 0) == N.EINVAL
    assert np.all(out == 7)


# ---- all four combinations of cell widths --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
def test_narrow_against_widened(native_lib, torch_cuda, kind):
    """On an engine of 32-bit cells: an ingested snapshot (4-byte cells) against an imported one (the import widened it to
    8-byte cells), in both argument orders; neither changes its width."""
    M = 40
    rng = np.random.default_rng(5)
    ids = rng.integers(0, M - 2, 20_000).astype(np.uint32)                       # names 38 and 39 stay empty there
    v = rng.lognormal(2.0, 1.0, ids.size)
    stored = [{int(b): int(c) for b, c in zip(20000 + 50 * m + np.arange(0, 600, 7), rng.integers(1, 1 << 34, 86))}
              for m in range(M - 1)] + [{}]                                      # a stored baseline; name 39 empty in both
    with engine(M, cell_bits=32, num_buffers=3) as e:
        e.submit_pairs(ids, v)
        with e.flip() as narrow, e.flip() as wide:
            e.sync()
            _import(wide, stored, ["tight"] * M)
            assert narrow.device_cells()[2] == 4 and wide.device_cells()[2] == 8
            cells, widenings = (narrow.device_cells(), wide.device_cells()), e.counters()["widenings"]
            rn, rw = rows_of(narrow, M), rows_of(wide, M)
            assert rw == stored and not rn[38] and not rn[39] and rn[0]
            with shape(kind):
                nw, wn = wide.compare(narrow, M), narrow.compare(wide, M)
            check(nw, [model(a, b) for a, b in zip(rn, rw)], "base narrow")
            check(wn, [model(a, b) for a, b in zip(rw, rn)], "base wide")
            assert (narrow.device_cells(), wide.device_cells()) == cells
            assert e.counters()["widenings"] == widenings


# ---- two engines on one device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("bits", BITS)
def test_two_engines(native_lib, torch_cuda, kind, bits):
    """A snapshot of an engine of 300 names against one of an engine of 200 (its stream is another one: the unit orders the
    two): rows beyond either engine's are LH_ERANGE."""
    import loghisto_amd
    rng = np.random.default_rng(bits)
    sets = []
    for M, mu in ((300, 3.0), (200, 3.4)):
        ids = rng.integers(0, M, 30_000).astype(np.uint32)
        sets.append((ids, rng.lognormal(mu, 0.8, ids.size)))
    with engine(300, cell_bits=bits, num_buffers=3) as e1, engine(200, cell_bits=bits, num_buffers=3) as e2:
        e1.submit_pairs(*sets[0])
        e2.submit_pairs(*sets[1])
        with e1.flip() as s1, e2.flip() as s2:
            r1, r2 = rows_of(s1, 200), rows_of(s2, 200)
            with shape(kind):
                check(s2.compare(s1, 200), [model(a, b) for a, b in zip(r1, r2)], "cur of 200 names")
                check(s1.compare(s2, 150, 50), [model(a, b) for a, b in zip(r2[50:], r1[50:])], "cur of 300 names")
                dev = _device_form(torch_cuda, s1, s2, 200)
                host = s1.compare(s2, 200)
                for k in FIELDS:
                    assert dev[k].tobytes() == host[k].tobytes(), k
                for cur, base in ((s1, s2), (s2, s1)):
                    for first, n in ((0, 250), (50, 200), (200, 1)):
                        with pytest.raises(loghisto_amd.LhError) as ei:
                            cur.compare(base, n, first)
                        assert ei.value.code == N.ERANGE, (first, n)
