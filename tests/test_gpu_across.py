"""lh_across / lh_across_device (Snapshot.across): count, sum, nbuckets, present_bits and the percentile buckets of a name
over SEVERAL snapshots at once -- the cells added up in 64 bits, then what lh_extract_rows does for one snapshot.

The model is Python integers over Snapshot.buckets_all of each snapshot of the list (a path the other tests hold to the
oracle): C = the sum of the dicts; count, nbuckets and present_bits exact; keys and valid from oracle.process_dense on the
summed dense row; |sum - exact| <= 1e-12 x sum of |D[b] C[b]| with exact a fractions.Fraction (the project's _sum parity).
The cross-check on the device: the same snapshots' buckets_all imported into a spare empty snapshot and lh_extract_rows on
it -- count, nbuckets, keys, valid and values equal, sum within the same bound.  Every case runs under both kernel shapes
(lh_tool_across_switch), on engines of 64- and of 32-bit cells.
No test here can put the snapshots on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib
import ctypes as C
import math
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_compare import _import, _write_narrow, rows_of
from tests.test_gpu_count_le import engine, host_arrays

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
U32MAX = (1 << 32) - 1
SHAPES = {"wave": 1, "block": 1 << 30}
NAN = float("nan")
P_MAIN = [0.99, 0.0, 1.0, 0.5, 0.5, 1.0000000000000002, NAN, 0.9]            # unsorted, repeated, 0, 1, > 1, NaN
FIELDS = dict(count=U64, sum=np.float64, nbuckets=np.uint32, present_bits=np.uint32, pkeys=np.int16, pvalid=np.uint8)
PER_P = ("pkeys", "pvalid")
K = 16


@contextlib.contextmanager
def shape(name):
    """Put every call through one kernel shape, whatever the number of rows; the previous value comes back afterwards."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    assert N.lib().lh_tool_across_switch(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_across_switch(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


# ---- the model -----------------------------------------------------------------------------------------------------------
_D = []


def table():
    if not _D:
        _D.append(oracle.decompress_table())
    return _D[0]


def model(rows, P):
    """rows: {bin: count} of one name in every snapshot of the list, in list order."""
    D = table()
    c = {}
    for r in rows:
        for b, n in r.items():
            c[b] = c.get(b, 0) + n
    total = sum(c.values())
    out = dict(count=total % (1 << 64), wrapped=total >= 1 << 64, nbuckets=len(c),
               present=sum(1 << i for i, r in enumerate(rows) if r))
    if out["wrapped"]:
        return out
    assert all(n < 1 << 64 for n in c.values())
    out["exact"] = sum((Fraction(float(D[b])) * n for b, n in c.items()), Fraction(0))
    out["mag"] = sum((abs(Fraction(float(D[b]))) * n for b, n in c.items()), Fraction(0))
    dense = np.zeros(NK, dtype=U64)
    if c:
        dense[np.array(list(c), dtype=np.int64)] = np.array(list(c.values()), dtype=U64)
    ref = oracle.process_dense(dense, np.array(P, dtype=np.float64))
    assert ref["count"] == total and ref["nbuckets"] == len(c)
    out.update(pkeys=ref["pkeys"], pvalid=ref["pvalid"])
    return out


def check(got, want, P, what=""):
    """got: Snapshot.across's dict; want: the models of the same rows."""
    M, D = len(want), table()
    for k, t in FIELDS.items():
        if k in got:
            assert got[k].dtype == t and got[k].shape == ((M, len(P)) if k in PER_P else (M,)), k
    for m, w in enumerate(want):
        at = (what, m)
        assert int(got["count"][m]) == w["count"], at
        if w["wrapped"]:
            continue
        assert int(got["nbuckets"][m]) == w["nbuckets"], at
        assert int(got["present_bits"][m]) == w["present"], (at, bin(int(got["present_bits"][m])), bin(w["present"]))
        err, tol = abs(Fraction(float(got["sum"][m])) - w["exact"]), Fraction(1, 10 ** 12) * w["mag"]
        assert math.isfinite(got["sum"][m]) and err <= tol, (at, got["sum"][m], float(w["exact"]), float(err), float(tol))
        if w["count"] == 0:
            assert got["sum"][m] == 0 and math.isnan(got["avg"][m]), at
        else:
            assert got["avg"][m] == got["sum"][m] / np.float64(w["count"]), at
        if not len(P):
            continue
        ok = w["pvalid"] != 0
        assert np.array_equal(got["pvalid"][m] != 0, ok) and set(np.unique(got["pvalid"][m])) <= {0, 1}, (at, got["pvalid"][m], ok)
        bins_got = [int(oracle.key_to_bin(int(k))) for k in got["pkeys"][m]]
        bins_want = [int(oracle.key_to_bin(int(k))) for k in w["pkeys"]]
        assert np.array_equal(got["pkeys"][m][ok], w["pkeys"][ok]), (at, bins_got, bins_want)
        assert not got["pkeys"][m][~ok].any(), at
        vals = D[(got["pkeys"][m].astype(np.int64) & 0xffff) ^ 0x8000]
        assert np.array_equal(got["pvals"][m][ok], vals[ok]) and np.all(np.isnan(got["pvals"][m][~ok])), at


def cross_check(spare_engine, snaps, got, want, P, M, what):
    """The same snapshots' cells imported into a spare empty snapshot, then lh_extract_rows there."""
    with spare_engine.flip() as spare:
        for s in snaps:
            spare.add_buckets_csr(*s.buckets_all(M))
        ex = spare.extract(P, M)
    for m, w in enumerate(want):
        at = (what, m)
        assert not w["wrapped"]
        assert int(ex["count"][m]) == int(got["count"][m]) and int(ex["nbuckets"][m]) == int(got["nbuckets"][m]), at
        assert np.array_equal(ex["pvalid"][m], got["pvalid"][m]) and np.array_equal(ex["pkeys"][m], got["pkeys"][m]), at
        ok = ex["pvalid"][m] != 0
        assert np.array_equal(ex["pvals"][m][ok], got["pvals"][m][ok]), at
        err = abs(Fraction(float(got["sum"][m])) - Fraction(float(ex["sum"][m])))
        assert err <= Fraction(1, 10 ** 12) * w["mag"], (at, got["sum"][m], ex["sum"][m], float(err))


# ---- crafted names: per name {snapshot index: (cells, span)}; a snapshot not named never marks the row -----------------------
def crafted_names(wide):
    """span: 'tight', or (lo, hi) marked beside the cells.  The lists of the tests: [0, 1, 2], all 16, and shorter ones."""
    names = []

    def add(kind, per_snap):
        names.append((kind, {i: (v if isinstance(v, tuple) else (v, "tight")) for i, v in per_snap.items()}))

    add("plain", {0: {100: 3, 200: 5}, 1: {150: 2}, 2: {100: 1, 300: 7}, 7: {90: 1}, 15: {310: 2}})
    add("only_in_0", {0: {4321: 2, 4400: 1}})
    add("only_in_2", {2: {777: 5, 901: 1}})
    add("only_in_15", {15: {33: 1}})
    add("never", {})
    add("marked_zero", {0: ({}, (700, 1200)), 1: ({}, (30000, 30001))})
    add("marked_zero_and_one_cell", {0: ({}, (0, NK - 1)), 2: {800: 1}})
    add("disjoint", {0: {1000: 2, 1010: 3}, 1: {2000: 1, 2500: 4}, 9: {3000: 20}})     # every percentile bucket in one snapshot only
    add("loose", {0: ({40001: 2, 40100: 1}, (39000, 42000)), 1: ({40050: 3}, (0, NK - 1)), 2: ({40002: 1}, (40001, 40003))})
    for w in (1, 255, 256, 257, 1025, NK):                                              # the union span's width in bins
        for lo in ((0,) if w == NK else (20000, 20002)):                                # 20 002: not a multiple of 4
            per = {0: {lo: 2}, 2: {lo + w - 1: 3}}
            if w > 2:
                per[1] = {lo + w // 2: 1}
            add(f"union_{w}/{lo}", per)
    add("hi_65535", {0: {64990: 2}, 1: {65535: 4, 65000: 1}})
    add("far_apart", {0: {10001: 1}, 1: {40001: 1}})                                    # the union exists only because of both
    # thresholds: span from 8 000 (a multiple of 4); total 11, p = 0.5 -> T = 6 = the prefix at X, and only because of the
    # LAST snapshot's 3 there (without them: total 8, T = 4, prefix 3 at X -> bin 13 000).  X: the last bin of a lane's group
    # and one later; of a 256-bin step; of the 16 chunks the waves of a workgroup take first
    for x in (8003, 8004, 8255, 8256, 8000 + 16 * 256 - 1, 8000 + 16 * 256):
        add(f"threshold_at_{x}", {0: {8000: 1}, 1: {x: 2, 13000: 5}, 2: {x: 3}})
    # the same cell at 2^32 - 1 in two snapshots: 0x1fffffffe, and p = 0.5 picks bin 500 only because of it (a 32-bit wrap
    # would leave 2^32 - 2 there and pick 600)
    add("two_cells_of_2^32-1", {0: {500: U32MAX}, 1: {500: U32MAX}, 2: {600: U32MAX}})
    add("dense_full", {4: {b: 1 + b % 3 for b in range(NK)}, 0: {5: 1}})
    add("widened_later", {0: {700: U32MAX, 650: 5}, 3: {640: 9}})                       # (snapshot 3 is the one an import widens)
    if wide:
        add("total_2^64-1", {0: {100: 1 << 63}, 1: {200: (1 << 63) - 1}})
        add("total_2^64-1_three", {0: {100: 1 << 62}, 1: {100: 1 << 62, 50: 1 << 62}, 2: {60000: (1 << 62) - 1}})
        add("wrapped_total", {0: {100: 1 << 63}, 1: {200: 1 << 63}, 2: {300: 7}})          # the LAST name: the spare leaves it out
    return names


LISTS = [[0], [2], [0, 0], [0, 1], [1, 0], [0, 1, 2], [1, 0, 1], [2, 2, 2], [3, 0], [0, 3, 1], list(range(16)), list(range(15, -1, -1))]
_WANT = {}


@pytest.fixture(scope="module", params=["wide64", "narrow32"])
def crafted(request, native_lib, torch_cuda):
    """16 snapshots, 15 of one engine and one of a second, holding the crafted names: imported (uint64 cells) or written into the narrow store of an
    engine of 32-bit cells, where snapshot 3 is then widened by the import of one cell of 2^33."""
    wide = request.param == "wide64"
    names = crafted_names(wide)
    M = len(names)
    assert 5 <= M <= 40
    rows = [[dict(per.get(i, ({}, None))[0]) for _, per in names] for i in range(K)]
    spans = [[per.get(i, ({}, None))[1] for _, per in names] for i in range(K)]
    spans = [[None if (s == "tight" and not r) else s for r, s in zip(rs, ss)] for rs, ss in zip(rows, spans)]
    bits = 64 if wide else 32
    # (an engine has at most 16 buffers, so it keeps at most 15 snapshots alive: the 16th is another engine's, on its own stream)
    with engine(M, cell_bits=bits, num_buffers=K) as e, engine(M, cell_bits=bits, num_buffers=2) as e2, \
            engine(M, cell_bits=64, num_buffers=2) as spare:
        with contextlib.ExitStack() as stack:
            snaps = [stack.enter_context(e.flip()) for _ in range(K - 1)] + [stack.enter_context(e2.flip())]
            assert snaps[-1].stream() != snaps[0].stream()
            for s, r, sp in zip(snaps, rows, spans):
                if wide:
                    if any(r):
                        _import(s, r, sp)
                    else:
                        for m, x in enumerate(sp):
                            if isinstance(x, tuple):
                                s.mark_dirty(m, 1, x[0], x[1])
                else:
                    _write_narrow(torch_cuda, s, r, sp)
            at = {k: m for m, (k, _) in enumerate(names)}
            if not wide:
                m = at["widened_later"]
                snaps[3].add_buckets(np.array([m], dtype=np.uint32), oracle.bin_to_key(np.array([700])).astype(np.int16),
                                     np.array([1 << 33], dtype=U64))
                rows[3][m][700] = 1 << 33
            widths = [s.device_cells()[2] for s in snaps]
            assert widths == ([8] * K if wide else [4, 4, 4, 8] + [4] * (K - 4))
            for s, r in zip(snaps, rows):                          # buckets_all returns what was put in
                assert rows_of(s, M) == r

            def want(lst, P=P_MAIN, first=0, n=M):
                key = (request.param, tuple(lst), tuple(repr(p) for p in P))
                if key not in _WANT:
                    _WANT[key] = [model([rows[i][m] for i in lst], P) for m in range(M)]
                return _WANT[key][first:first + n]

            yield types.SimpleNamespace(e=e, spare=spare, snaps=snaps, rows=rows, names=names, at=at, M=M, wide=wide,
                                        widths=widths, want=want, torch=torch_cuda)
            assert [s.device_cells()[2] for s in snaps] == widths


def call(c, lst, P=P_MAIN, nmetrics=None, first=0, out=None):
    return c.snaps[lst[-1]].across([c.snaps[i] for i in lst[:-1]], P, c.M if nmetrics is None else nmetrics, first, out=out)


@pytest.mark.parametrize("kind", list(SHAPES))
def test_crafted_lists(crafted, kind):
    c = crafted
    got = {}
    with shape(kind):
        for lst in LISTS:
            got[tuple(lst)] = call(c, lst)
    for lst in LISTS:
        check(got[tuple(lst)], c.want(lst), P_MAIN, (kind, lst))
    # K = 1 is extract() of that snapshot
    for i in (0, 2):
        ex, g = c.snaps[i].extract(P_MAIN, c.M), got[(i,)]
        assert np.array_equal(ex["count"], g["count"]) and np.array_equal(ex["nbuckets"], g["nbuckets"])
        assert np.array_equal(ex["pkeys"], g["pkeys"]) and np.array_equal(ex["pvalid"], g["pvalid"])
    # [s, s] doubles every count of [s] and keeps every key
    one, two = got[(0,)], got[(0, 0)]
    fits = np.array([not w["wrapped"] for w in c.want([0, 0])])                 # (a cell of 2^63 taken twice wraps)
    assert np.array_equal(two["count"], 2 * one["count"]) and np.array_equal(two["nbuckets"][fits], one["nbuckets"][fits])
    assert np.array_equal(two["pkeys"][fits], one["pkeys"][fits]) and np.array_equal(two["pvalid"][fits], one["pvalid"][fits])
    assert np.array_equal(two["present_bits"][fits], 3 * one["present_bits"][fits])
    # the order of the list moves present_bits only
    a, b = got[tuple(range(16))], got[tuple(range(15, -1, -1))]
    for k in ("count", "nbuckets", "pkeys", "pvalid"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(got[(0, 1)]["sum"], got[(1, 0)]["sum"])              # integer cell sums: the same bits
    # what the names were made for
    t3, half = got[(0, 1, 2)], P_MAIN.index(0.5)

    def bin_of(g, name, i=half):
        return int(oracle.key_to_bin(int(g["pkeys"][c.at[name], i])))

    for x in (8003, 8004, 8255, 8256, 8000 + 16 * 256 - 1, 8000 + 16 * 256):
        assert bin_of(t3, f"threshold_at_{x}") == x and bin_of(got[(0, 1)], f"threshold_at_{x}") == 13000, x
    m = c.at["two_cells_of_2^32-1"]
    assert int(got[(0, 1)]["count"][m]) == 0x1fffffffe and int(t3["count"][m]) == 3 * U32MAX
    assert bin_of(t3, "two_cells_of_2^32-1") == 500
    assert bin_of(got[(0, 1)], "far_apart") == 10001 and bin_of(got[(0, 1)], "far_apart", P_MAIN.index(1.0)) == 40001
    assert t3["present_bits"][c.at["only_in_2"]] == 4 and t3["present_bits"][c.at["never"]] == 0
    assert t3["present_bits"][c.at["marked_zero"]] == 0 and a["present_bits"][c.at["only_in_15"]] == 1 << 15
    assert b["present_bits"][c.at["only_in_15"]] == 1
    if c.wide:
        assert int(got[(0, 1)]["count"][c.at["total_2^64-1"]]) == (1 << 64) - 1
        assert int(t3["count"][c.at["wrapped_total"]]) == 7                     # count wraps, and the call returned LH_OK
    else:
        m = c.at["widened_later"]
        assert int(got[(3, 0)]["count"][m]) == int(got[(0, 3, 1)]["count"][m]) == (1 << 33) + U32MAX + 5 + 9
    # the import cross-check (not for the total that wraps)
    mx = c.M - 1 if c.wide else c.M
    assert all(not w["wrapped"] for lst in ([0, 1, 2], list(range(16))) for w in c.want(lst)[:mx])
    for lst in ([0, 1, 2], list(range(16))):
        cross_check(c.spare, [c.snaps[i] for i in lst], got[tuple(lst)], c.want(lst)[:mx], P_MAIN, mx, (kind, lst))


@pytest.mark.parametrize("kind", list(SHAPES))
def test_percentile_counts_and_ranges(crafted, kind):
    """np = 0 and np = 32; first > 0 with nmetrics in {1, 3, 4, 5} (the wave form packs 4 rows per workgroup)."""
    c, lst = crafted, [0, 1, 2]
    p32 = [((7 * i) % 32) / 31.0 for i in range(32)]
    with shape(kind):
        full = call(c, lst)
        none = call(c, lst, [])
        many = call(c, lst, p32)
        assert set(none) == {"count", "sum", "avg", "nbuckets", "present_bits", "pkeys", "pvalid", "pvals"}
        assert none["pkeys"].shape == (c.M, 0) and none["pvals"].shape == (c.M, 0)
        check(none, c.want(lst, []), [], (kind, "np=0"))
        check(many, c.want(lst, p32), p32, (kind, "np=32"))
        for k in ("count", "sum", "nbuckets", "present_bits"):
            assert none[k].tobytes() == full[k].tobytes() == many[k].tobytes(), k
        for first, n in ((1, 1), (2, 3), (3, 4), (c.M - 5, 5), (0, 5), (7, 1)):
            part = call(c, lst, nmetrics=n, first=first)
            for k in FIELDS:
                assert part[k].tobytes() == full[k][first:first + n].tobytes(), (first, n, k)


def _device_form(torch, c, lst, P, n, first=0, names=tuple(FIELDS)):
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int32, pkeys=torch.int16,
                 pvalid=torch.uint8)
    out = {k: torch.full((n, len(P)) if k in PER_P else (n,), 77, dtype=kinds[k], device="cuda") for k in names}
    torch.cuda.synchronize()
    back = call(c, lst, P, n, first, out=out)
    torch.cuda.ExternalStream(c.snaps[lst[-1]].stream()).synchronize()
    assert all(back[k] is out[k] for k in names)
    return {k: v.cpu().numpy().view(FIELDS[k]) for k, v in out.items()}


@pytest.mark.parametrize("kind", list(SHAPES))
def test_forms_and_read_only(crafted, kind):
    """Device form == host form byte for byte, pinned == pageable, outputs left out, and nothing moves in any snapshot."""
    from loghisto_amd import merge
    c, torch, M = crafted, crafted.torch, crafted.M
    cells = [s.device_cells() for s in c.snaps]
    ranges = [merge.snapshot_ranges(s, M).cpu().numpy().copy() for s in c.snaps]
    before = [[x.copy() for x in s.buckets_all(M)] for s in c.snaps]
    widenings = c.e.counters()["widenings"]
    with shape(kind):
        for lst in ([0, 1, 2], [0, 3, 1], list(range(16))):
            host = call(c, lst)
            dev = _device_form(torch, c, lst, P_MAIN, M)
            for k in FIELDS:
                assert dev[k].tobytes() == host[k].tobytes(), (lst, k)
        lst = [0, 3, 1]
        host = call(c, lst)
        f, n = 2, M - 5
        dpart = _device_form(torch, c, lst, P_MAIN, n, f)
        for k in FIELDS:
            assert dpart[k].tobytes() == host[k][f:f + n].tobytes(), k
        for pinned in (True, False):                                              # the host form's two ways back
            out = {k: host_arrays(torch, pinned, (M, len(P_MAIN)) if k in PER_P else (M,), t) for k, t in FIELDS.items()}
            call(c, lst, out=out)
            for k in FIELDS:
                assert out[k].tobytes() == host[k].tobytes(), (pinned, k)
        for names in (("count",), ("pkeys",), ("pvalid", "present_bits"), ("sum", "nbuckets"), ("count", "pkeys", "pvalid"),
                      tuple(k for k in FIELDS if k != "count")):                  # NULL for the others
            d = _device_form(torch, c, lst, P_MAIN, M, names=names)
            for pinned in (True, False):
                out = {k: host_arrays(torch, pinned, (M, len(P_MAIN)) if k in PER_P else (M,), FIELDS[k]) for k in names}
                got = call(c, lst, out=out)
                assert set(got) - {"avg", "pvals"} == set(names)
                for k in names:
                    assert out[k].tobytes() == host[k].tobytes() == d[k].tobytes(), (names, pinned, k)
        # through ctypes: an empty call writes nothing, first beyond the rows is LH_ERANGE, a flag is LH_EINVAL
        L = N.lib()
        hs = (C.c_void_p * 3)(*[c.snaps[i]._h.value for i in lst])
        guard = np.full(M, 7, dtype=U64)
        pp = np.array(P_MAIN)
        for first in (0, M):
            assert L.lh_across(hs, 3, first, 0, pp.ctypes.data, pp.size, 0, guard.ctypes.data, 0, 0, 0, 0, 0) == 0
        assert L.lh_across(hs, 3, M + 1, 0, pp.ctypes.data, pp.size, 0, guard.ctypes.data, 0, 0, 0, 0, 0) == N.ERANGE
        assert L.lh_across(hs, 3, 1, M, pp.ctypes.data, pp.size, 0, guard.ctypes.data, 0, 0, 0, 0, 0) == N.ERANGE
        assert L.lh_across(hs, 3, 0, M, pp.ctypes.data, pp.size, 1, guard.ctypes.data, 0, 0, 0, 0, 0) == N.EINVAL
        assert np.all(guard == 7)
        assert L.lh_across(hs, 3, 0, M, None, 0, 0, guard.ctypes.data, 0, 0, 0, 0, 0) == 0
        assert guard.tobytes() == host["count"].tobytes()
    after = [s.buckets_all(M) for s in c.snaps]
    for b, a in zip(before, after):
        assert len(b) == len(a) and all(np.array_equal(x, y) for x, y in zip(b, a))
    assert [s.device_cells() for s in c.snaps] == cells
    assert all(np.array_equal(merge.snapshot_ranges(s, M).cpu().numpy(), r) for s, r in zip(c.snaps, ranges))
    assert c.e.counters()["widenings"] == widenings


# ---- two engines on one device: other streams, other widths, other numbers of rows -------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
def test_two_engines(native_lib, torch_cuda, kind):
    """Snapshots of an engine of 40 names with 64-bit cells and of one of 25 names with 32-bit cells in one list: rows
    beyond the smaller engine's are LH_ERANGE."""
    import loghisto_amd
    rng = np.random.default_rng(77)
    sets = []
    for M in (40, 25, 40, 25):
        ids = rng.integers(0, M - 2, 20_000).astype(np.uint32)                   # the last two names stay empty
        sets.append((ids, rng.lognormal(2.0 + 0.2 * len(sets), 0.8, ids.size)))
    with engine(40, cell_bits=64, num_buffers=3) as e1, engine(25, cell_bits=32, num_buffers=3) as e2, \
            engine(25, cell_bits=64, num_buffers=2) as spare:
        e1.submit_pairs(*sets[0])
        e2.submit_pairs(*sets[1])
        with e1.flip() as a1, e2.flip() as b1:
            e1.submit_pairs(*sets[2])
            e2.submit_pairs(*sets[3])
            with e1.flip() as a2, e2.flip() as b2:
                e1.sync()
                e2.sync()
                assert [s.device_cells()[2] for s in (a1, a2, b1, b2)] == [8, 8, 4, 4]
                r = {s: rows_of(s, 25) for s in (a1, a2, b1, b2)}
                with shape(kind):
                    for lst in ([a1, b1, a2, b2], [b2, a1], [b1, b2, a2]):
                        want = [model([r[s][m] for s in lst], P_MAIN) for m in range(25)]
                        got = lst[-1].across(lst[:-1], P_MAIN, 25)
                        check(got, want, P_MAIN, (kind, "two engines"))
                        cross_check(spare, lst, got, want, P_MAIN, 25, (kind, "two engines"))
                    part = a2.across([b1], P_MAIN, 5, 20)
                    check(part, [model([r[b1][m], r[a2][m]], P_MAIN) for m in range(20, 25)], P_MAIN, (kind, "first = 20"))
                    for lst in ([a1, b1], [b1, a1], [a1, a2, b2, a1]):
                        for first, n in ((0, 26), (20, 6), (25, 1), (0, 40)):
                            with pytest.raises(loghisto_amd.LhError) as ei:
                                lst[-1].across(lst[:-1], P_MAIN, n, first)
                            assert ei.value.code == N.ERANGE, (first, n)
                    assert a2.across([a1], P_MAIN, 40)["count"].shape == (40,)      # both of 40 names: fine


# ---- intervals of real ingest ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_five_intervals_of_a_zipf_stream(native_lib, torch_cuda, bits):
    """K = 5 intervals of 2e5 (Zipf name, lognormal value) pairs on 40 names, against the model and the import cross-check,
    in both shapes."""
    M, k, n = 40, 5, 200_000
    rng = np.random.default_rng(2024)
    w = 1.0 / np.arange(1, M + 1)
    with engine(M, cell_bits=bits, num_buffers=k + 1) as e, engine(M, cell_bits=64, num_buffers=2) as spare:
        with contextlib.ExitStack() as stack:
            snaps = []
            for i in range(k):
                ids = rng.choice(M, n, p=w / w.sum()).astype(np.uint32)
                v = rng.lognormal(3.0 + 0.1 * i, 1.0, n)
                v[rng.random(n) < 0.02] *= -1.0
                keep = ids != (7 + i)                                             # a name missing from each interval
                e.submit_pairs(ids[keep], v[keep])
                snaps.append(stack.enter_context(e.flip()))
            e.sync()
            assert all(s.device_cells()[2] == bits // 8 for s in snaps)
            rows = [rows_of(s, M) for s in snaps]
            P = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]
            want = [model([r[m] for r in rows], P) for m in range(M)]
            assert sum(x["count"] for x in want) == sum(sum(sum(r.values()) for r in rs) for rs in rows) > 0.9 * k * n
            res = {}
            for kind in SHAPES:
                with shape(kind):
                    res[kind] = snaps[-1].across(snaps[:-1], P, M)
                check(res[kind], want, P, kind)
                cross_check(spare, snaps, res[kind], want, P, M, kind)
            for f in ("count", "nbuckets", "present_bits", "pkeys", "pvalid"):
                assert res["wave"][f].tobytes() == res["block"][f].tobytes(), f
            assert res["wave"]["present_bits"][7] == 0b11110 and res["wave"]["present_bits"][11] == 0b01111
