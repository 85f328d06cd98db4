"""lh_kept_compare* (Kept.compare): lh_compare's outputs between two LISTS of kept intervals -- a[j] the sum over the base
list of the name's cell j, b[j] the same over the cur list -- with no dense buffer alive.

The model and the check are those of tests/test_gpu_compare.py: Python integers and fractions.Fraction over the summed
{bin: count} of each side; counts, key and both prefixes exact, ks bit-equal, w1 and shift within that file's derived bound
4 n 2^-53 (1 + w1), n = the bins from the lowest to the highest occupied one.  The bound holds here as it stands: the bins
that no tile covers are taken g at a time as one product and one add, two roundings for g bins where the dense walk has g.
Every case runs under both kernel shapes (lh_tool_kept_switch), on ONE two-buffer engine per cell width (64- and 32-bit
cells: on the latter the rows are written into the narrow store); the two tiles' width comes from lh_tool_kept_compare_tile.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_compare import BIG, FIELDS, _import, _write_narrow, check, crafted_pairs, model, rows_of
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import same_listing, shape

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
KINDS = ("wave", "block")
INTS = ("count_a", "count_b", "key", "below_a", "below_b")


def tile():
    t = C.c_uint32(0)
    assert N.lib().lh_tool_kept_compare_tile(C.byref(t)) == 0 and t.value % 256 == 0 and 256 <= t.value <= 1024
    return int(t.value)


def tile_pairs(T):
    """(kind, a, b) aimed at the edges of the tiles and at the stretches between them; `expect`: kind -> the bin of ks"""
    P, expect = [], {}

    def add(kind, a, b, bin_=None):
        P.append((kind, a, b))
        if bin_ is not None:
            expect[kind] = bin_

    add("tile_0_T-1_vs_T_2T-1", {0: 1, T - 1: 2}, {T: 3, 2 * T - 1: 4}, T - 1)
    for r in range(4):                                                          # every t % 4: where the second tile starts
        t = 8000 + 4 * T * r + r
        add(f"edge{r}_one_side", {t: 1, t + T - 1: 2, t + T: 3, t + T + 1: 4}, {t + 2: 5, t + T + 2: 1})
        add(f"edge{r}_split", {t: 1, t + T: 2}, {t + T - 1: 1, t + T + 1: 3})
    add("stretch_3T_one_side", {1000: 1, 1000 + 3 * T + 77: 2}, {1001: 3})
    add("stretch_3T_both", {2000: 1, 2000 + 3 * T + 77: 2}, {2003: 1, 2000 + 3 * T + 80: 5})
    add("stretch_ends_at_Tk-1", {5: 1, 4 * T: 2}, {6: 1, 4 * T + 3: 1})          # the next occupied bin is T k
    add("stretch_ends_at_Tk", {5: 1, 4 * T + 1: 2}, {6: 1, 4 * T + 2: 1})
    add("stretch_ends_behind_the_tile", {4: 1, T + 4: 2}, {5: 1, T + 9: 1})      # the second tile starts where the first ends
    add("stretch_of_4", {4: 1, T + 8: 2}, {5: 1, T + 13: 1})
    add("bins_0_vs_65535", {0: 3}, {NK - 1: 5}, 0)
    add("bins_65535_vs_0", {NK - 1: 5}, {0: 3}, 0)
    # X = 2 at bin 10 and again at 10 + 2 T, in another tile: the lowest bin wins
    add("tie_in_another_tile", {10: 1, 10 + 2 * T: 1}, {20: 1, 20 + 2 * T: 1}, 10)
    # X = 3 first at T - 1, the last bin of the first tile, constant over [T, 5 T), 0 at 5 T and 3 again at 5 T + 1
    add("tie_before_a_stretch", {0: 1, T - 1: 1, 5 * T + 1: 1}, {0: 1, 5 * T: 1, 5 * T + 2: 1}, T - 1)
    add("dense_over_tiles", {b: 1 + b % 5 for b in range(30000, 30000 + 3 * T, 3)}, {b: 2 for b in range(30100, 30100 + 2 * T, 7)})
    return P, expect


def deal(rows, k, only=None):
    """rows dealt over k handles with every row's sums kept: a cell of 2 or more is split over two handles, so that the same
    bin stands in several.  only: the rows that are dealt at all (the others stay empty in every handle)."""
    parts = [[{} for _ in rows] for _ in range(k)]
    for m, r in enumerate(rows):
        if only is not None and m not in only:
            continue
        for j, b in enumerate(sorted(r)):
            c, i = r[b], (j + m) % k
            if c >= 2 and k > 1:
                parts[i][m][b] = c // 2
                parts[(i + 1) % k][m][b] = c - c // 2
            else:
                parts[i][m][b] = c
    return parts


def summed(handles):
    out = []
    for m in range(len(handles[0].rows)):
        cells = {}
        for h in handles:
            for b, c in h.rows[m].items():
                cells[b] = cells.get(b, 0) + c
        out.append(cells)
    return out


_MODEL = {}


def models(c, LA, LB):
    """the models of every row for base list LA and cur list LB, None where a side's total passes 2^64 (unspecified)"""
    sa, sb = summed(LA), summed(LB)
    out = []
    for m, (a, b) in enumerate(zip(sa, sb)):
        if sum(a.values()) >= 1 << 64 or sum(b.values()) >= 1 << 64:
            out.append(None)
            continue
        plain = a == c.rows_a[m] and b == c.rows_b[m]
        key = (c.wide, m)
        if plain and key in _MODEL:
            out.append(_MODEL[key])
            continue
        w = model(a, b)
        if plain:
            _MODEL[key] = w
        out.append(w)
    return out


def check_rows(got, want, what):
    """test_gpu_compare.check over the rows that have a model"""
    keep = [m for m, w in enumerate(want) if w is not None]
    check({k: v[keep] for k, v in got.items()}, [want[m] for m in keep], what)


def call(LA, LB, **kw):
    return LB[-1].k.compare([h.k for h in LA], earlier=[h.k for h in LB[:-1]], **kw)


def same_bits(x, y, what, rows=None):
    for f in FIELDS:
        a, b = (x[f], y[f]) if rows is None else (x[f][rows], y[f][rows])
        assert a.tobytes() == b.tobytes(), (what, f)


@pytest.fixture(scope="module", params=["wide64", "narrow32"])
def kept(request, native_lib, torch_cuda):
    """Every handle of this file, taken from successive snapshots of ONE two-buffer engine, each released right after its
    keep: the two sides of every pair in one handle each (A, B), dealt over 2 and 3 handles, a few rows dealt over 32, and
    sub-blocks of A and B with different `first`."""
    wide = request.param == "wide64"
    T = tile()
    tiles, expect = tile_pairs(T)
    pairs = [(k, a, b) for k, a, b, *_ in crafted_pairs()] + tiles + ([(k, a, b) for k, a, b in BIG] if wide else [])
    M = len(pairs)
    assert M < 200
    at = {k: m for m, (k, _, _) in enumerate(pairs)}
    rows_a = [{b: c for b, c in p[1].items() if c} for p in pairs]
    rows_b = [{b: c for b, c in p[2].items() if c} for p in pairs]
    made = []

    with engine(M, cell_bits=64 if wide else 32, num_buffers=2) as e:
        def handle(rows, subs=()):
            spans = ["tight" if r else None for r in rows]
            with e.flip() as s:
                if wide and any(rows):
                    _import(s, rows, spans)
                elif not wide:
                    _write_narrow(torch_cuda, s, rows, spans)
                assert s.device_cells()[2] == (8 if wide else 4)
                h = types.SimpleNamespace(k=s.keep(M), rows=rows, rec=[x.copy() for x in s.buckets_all(M)], first=0)
                made.append(h)
                out = [h]
                for first, n in subs:
                    sub = [r if first <= m < first + n else {} for m, r in enumerate(rows)]
                    out.append(types.SimpleNamespace(k=s.keep(n, first), rows=sub, rec=[x.copy() for x in s.buckets_all(n, first)],
                                                     first=first))
                    made.append(out[-1])
            return out if subs else h

        A, A_sub = handle(rows_a, [(10, 20)])
        B, B_sub = handle(rows_b, [(5, 25)])
        assert rows_of(types.SimpleNamespace(buckets_all=lambda M_, first, r=A.rec: r), M) == rows_a
        few = {at[k] for k, _, _ in tiles} | {at["tie"], at["disjoint"], at["sparse_full_both"], at["a_empty"]}
        lists = {1: ([A], [B])}
        for k in (2, 3):
            lists[k] = ([handle(r) for r in deal(rows_a, k)], [handle(r) for r in deal(rows_b, k)])
        lists[32] = ([handle(r) for r in deal(rows_a, 32, few)], [handle(r) for r in deal(rows_b, 32, few)])
        e.flip().release()                                                      # (both buffers have been cleared since)
        e.flip().release()
        yield types.SimpleNamespace(e=e, A=A, B=B, A_sub=A_sub, B_sub=B_sub, lists=lists, few=sorted(few), pairs=pairs, at=at, M=M,
                                    T=T, wide=wide, rows_a=rows_a, rows_b=rows_b, expect=expect, torch=torch_cuda)
    # the engine is gone; every handle still holds, byte for byte, what it was made from -- after every case
    for h in made:
        same_listing(h.k, h.rec, "at teardown")
        h.k.close()


# ---- 1. crafted pairs and tile cases, both shapes ------------------------------------------------------------------------------
def test_crafted_pairs_and_tile_cases(kept):
    c = kept
    want = models(c, [c.A], [c.B])
    got = {}
    for kind in KINDS:
        with shape(kind):
            got[kind] = call([c.A], [c.B], nmetrics=c.M)
        check_rows(got[kind], want, kind)
    same_bits(got["wave"], got["block"], "the two shapes")
    g = got["wave"]

    def bin_of(k):
        return int(oracle.key_to_bin(int(g["key"][c.at[k]])))

    for k, b in c.expect.items():
        assert bin_of(k) == b, (k, bin_of(k), b)
    assert [bin_of(k) for k in ("tie", "tie_same_lane", "tie_lanes_of_one_step", "tie_two_steps", "tie_many_steps",
                                "tie_same_wave_of_a_workgroup", "tie_chunks_0_32",
                                "tie_higher_lane_holds_the_lower_bin")] == [10, 8, 1000, 5010, 6001, 6001, 6001, 600]
    for k in ("identical", "identical_scaled", "identical_loose_span", "one_bin_same"):
        m = c.at[k]
        assert g["ks"][m] == 0 and g["w1"][m] == 0 and g["shift"][m] == 0 and g["key"][m] == 0 and g["below_a"][m] == 0, k
    m = c.at["disjoint"]
    assert g["ks"][m] == 1.0 and abs(g["w1"][m] - 1394.0) <= 1e-9 and abs(g["shift"][m] - 1394.0) <= 1e-9
    m = c.at["bins_0_vs_65535"]                                                  # one stretch of 65 535 bins at X = na nb
    assert g["ks"][m] == 1.0 and g["w1"][m] == NK - 1 and g["shift"][m] == NK - 1
    assert g["shift"][c.at["bins_65535_vs_0"]] == -(NK - 1.0)
    # a name empty on one side: NaN and the counts
    for k, na, nb in (("a_empty", 0, 1), ("b_empty", 3, 0), ("both_empty", 0, 0)):
        m = c.at[k]
        assert (int(g["count_a"][m]), int(g["count_b"][m])) == (na, nb), k
        assert math.isnan(g["ks"][m]) and math.isnan(g["w1"][m]) and math.isnan(g["shift"][m]) and math.isnan(g["ks_value"][m]), k
        assert g["key"][m] == 0 and g["below_a"][m] == 0 and g["below_b"][m] == 0, k
    if c.wide:
        assert bin_of("argmax_by_one_in_2^122") == 200 and bin_of("argmax_by_one_mirrored") == 200


# ---- 2. lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lists_equal_the_merged_handles_and_the_model(kept, kind):
    import loghisto_amd
    c = kept
    with shape(kind):
        one = call([c.A], [c.B], nmetrics=c.M)
        cases = [(f"{k} + {k}", LA, LB) for k, (LA, LB) in c.lists.items()]
        LA, LB = c.lists[3]
        cases.append(("a handle listed twice", LA + [LA[1]], [LB[2]] + LB))
        cases.append(("1 + 3", [c.A], LB))
        assert len(c.lists[32][0]) + len(c.lists[32][1]) == 64                  # 32 + 32 handles are accepted
        for what, LA, LB in cases:
            got = call(LA, LB, nmetrics=c.M)
            want = models(c, LA, LB)
            check_rows(got, want, (kind, what))
            ok = [m for m, w in enumerate(want) if w is not None]                # (a total past 2^64 is unspecified)
            assert len(ok) >= c.M - 4
            with LA[-1].k.merge([h.k for h in LA[:-1]]) as ma, LB[-1].k.merge([h.k for h in LB[:-1]]) as mb:
                merged = mb.compare(ma, c.M)
            same_bits(got, merged, (kind, what, "the merged handles"), ok)
            if what in ("2 + 2", "3 + 3", "1 + 3"):                              # the same sums as the one handle per side
                same_bits(got, one, (kind, what, "one handle per side"))
            if what == "32 + 32":
                same_bits(got, one, (kind, what, "one handle per side"), c.few)
                rest = [m for m in range(c.M) if m not in c.few]
                assert not got["count_a"][rest].any() and np.isnan(got["ks"][rest]).all()
        for LA, LB in (([c.A] * 33, [c.B] * 32), ([c.A] * 32, [c.B] * 33), ([c.A] * 64, [c.B])):
            with pytest.raises(loghisto_amd.LhError) as ei:
                call(LA, LB, nmetrics=c.M)
            assert ei.value.code == N.EINVAL


# ---- 3. agreement with lh_compare on the live snapshots -------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (64, 32))
def test_agrees_with_compare_on_the_live_snapshots(native_lib, torch_cuda, bits):
    M, n = 40, 30_000
    rng = np.random.default_rng(70 + bits)
    with engine(M, cell_bits=bits, num_buffers=3) as e:
        e.submit_pairs(rng.integers(0, M - 2, n).astype(np.uint32), rng.lognormal(3.0, 0.7, n))
        with e.flip() as base:
            e.submit_pairs(rng.integers(1, M - 1, n).astype(np.uint32), rng.lognormal(3.2, 0.9, n))
            with e.flip() as cur:
                e.sync()
                want = [model(a, b) for a, b in zip(rows_of(base, M), rows_of(cur, M))]
                live = cur.compare(base, M)
                with base.keep(M) as ka, cur.keep(M) as kb:
                    for kind in KINDS:
                        with shape(kind):
                            got = kb.compare(ka, M)
                        check(got, want, (kind, bits))
                        for f in INTS + ("ks",):
                            assert got[f].tobytes() == live[f].tobytes(), (kind, f)
                check(live, want, "lh_compare")                                  # both within the bound of the exact model
    assert sum(w["w1"] is not None for w in want) == M - 3


# ---- 4. edge entries, blocks and ids ---------------------------------------------------------------------------------------------
def _device_out(torch, n, names=tuple(FIELDS)):
    kinds = dict(count_a=torch.int64, count_b=torch.int64, ks=torch.float64, key=torch.int16, below_a=torch.int64,
                 below_b=torch.int64, w1=torch.float64, shift=torch.float64)
    return {k: torch.full((n,), 77, dtype=kinds[k], device="cuda") for k in names}


def _back(out):
    return {k: v.cpu().numpy().view(FIELDS[k]) for k, v in out.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_identical_lists_blocks_and_ids(kept, kind):
    import loghisto_amd
    c, torch, M = kept, kept.torch, kept.M
    with shape(kind):
        full = call([c.A], [c.B], nmetrics=M)
        # identical lists, and a handle present in both lists: exact zeros for every non-empty name
        for LA, LB in (([c.B], [c.B]), ([c.A, c.B], [c.A, c.B]), ([c.A, c.B], [c.B, c.A])):
            same = call(LA, LB, nmetrics=M)
            for m, cells in enumerate(summed(LA)):
                total = sum(cells.values())
                if total >= 1 << 64:
                    continue
                assert int(same["count_a"][m]) == int(same["count_b"][m]) == total, m
                if total:
                    assert same["ks"][m] == 0 and same["w1"][m] == 0 and same["shift"][m] == 0 and same["key"][m] == 0, m
                    assert same["below_a"][m] == 0 and same["below_b"][m] == 0, m
                else:
                    assert math.isnan(same["ks"][m]) and math.isnan(same["w1"][m]) and math.isnan(same["shift"][m]), m
        # sub-block handles of rows [10, 30) and [5, 30): absolute first and ids, inside both blocks
        for first, n in ((10, 20), (12, 10), (29, 1)):
            part = call([c.A_sub], [c.B_sub], nmetrics=n, first=first)
            same_bits(part, {f: v[first:first + n] for f, v in full.items()}, (kind, first, n))
        assert call([c.A_sub], [c.B_sub], first=10)["ks"].shape == (20,)         # nmetrics=None: to the end of cur's block
        for LA, LB, first, n in (([c.A_sub], [c.B_sub], 9, 2), ([c.A_sub], [c.B_sub], 10, 21), ([c.A_sub], [c.B_sub], 5, 5),
                                 ([c.A], [c.B_sub], 4, 2), ([c.A_sub], [c.B], 0, M), ([c.A], [c.B], 1, M), ([c.A], [c.B], M, 1)):
            with pytest.raises(loghisto_amd.LhError) as ei:
                call(LA, LB, nmetrics=n, first=first)
            assert ei.value.code == N.ERANGE, (first, n)
        # the ids form over a permutation with repeats equals the gathered block form
        rng = np.random.default_rng(3)
        ids = np.concatenate([rng.permutation(M), rng.integers(0, M, 9)]).astype(np.uint32)
        by_id = call([c.A], [c.B], ids=ids)
        same_bits(by_id, {f: v[ids] for f, v in full.items()}, (kind, "ids"))
        sub_ids = np.array([29, 10, 17, 10, 12], dtype=np.uint32)
        same_bits(call([c.A_sub], [c.B_sub], ids=sub_ids), {f: v[sub_ids] for f, v in full.items()}, (kind, "ids of sub-blocks"))
        assert call([c.A], [c.B], ids=[])["ks"].shape == (0,)
        # a host id outside some handle's block: LH_ERANGE and the outputs stay as they were
        for LA, LB, bad in (([c.A], [c.B], [0, M, 1]), ([c.A_sub], [c.B_sub], [12, 9]), ([c.A], [c.B_sub], [30]),
                            ([c.A_sub], [c.B], [11, 0xffffffff])):
            out = {k: np.full(len(bad), 7, dtype=t) for k, t in FIELDS.items()}
            with pytest.raises(loghisto_amd.LhError) as ei:
                call(LA, LB, ids=bad, out=out)
            assert ei.value.code == N.ERANGE, bad
            assert all(np.all(v == 7) for v in out.values()), bad
        # a device id outside some handle's block: the entry of two empty sides; the others are unaffected
        st = torch.cuda.Stream()
        dids = [12, 9, 29, 30, 0xffffffff - (1 << 32), 10, 4]
        with torch.cuda.stream(st):
            d_ids = torch.tensor(dids, dtype=torch.int32, device="cuda")
            out = _device_out(torch, len(dids))
        st.synchronize()
        assert call([c.A_sub], [c.B_sub], ids=d_ids, out=out, stream=st)["ks"] is out["ks"]
        st.synchronize()
        dev = _back(out)
        for j, i in enumerate(dids):
            if 10 <= i < 30:
                for f in FIELDS:
                    assert dev[f][j].tobytes() == full[f][i].tobytes(), (j, f)
            else:
                assert dev["count_a"][j] == 0 and dev["count_b"][j] == 0 and dev["key"][j] == 0, j
                assert dev["below_a"][j] == 0 and dev["below_b"][j] == 0, j
                assert math.isnan(dev["ks"][j]) and math.isnan(dev["w1"][j]) and math.isnan(dev["shift"][j]), j


# ---- 5. forms and lifetime ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_forms_and_lifetime(kept, kind):
    c, torch, M = kept, kept.torch, kept.M
    st = torch.cuda.Stream()
    LA, LB = c.lists[3]
    with shape(kind):
        host = call(LA, LB, nmetrics=M)
        out = _device_out(torch, M)
        torch.cuda.synchronize()
        back = call(LA, LB, nmetrics=M, out=out, stream=st)
        st.synchronize()
        assert all(back[k] is out[k] for k in FIELDS)
        same_bits(_back(out), host, (kind, "device form"))
        f0, n = 3, M - 7
        out = _device_out(torch, n)
        torch.cuda.synchronize()
        call(LA, LB, nmetrics=n, first=f0, out=out)                              # the null stream
        torch.cuda.synchronize()
        same_bits(_back(out), {f: v[f0:f0 + n] for f, v in host.items()}, (kind, "device form of a sub-range"))
        for names in (("key",), ("ks", "key"), ("count_b", "w1"), tuple(k for k in FIELDS if k != "key")):   # NULL for the others
            d = _device_out(torch, M, names)
            torch.cuda.synchronize()
            call(LA, LB, nmetrics=M, out=d, stream=st)
            st.synchronize()
            pageable = {k: np.full(M, 7, dtype=FIELDS[k]) for k in names}
            got = call(LA, LB, nmetrics=M, out=pageable)
            assert set(got) - {"ks_value"} == set(names)
            for k, v in _back(d).items():
                assert v.tobytes() == host[k].tobytes() == pageable[k].tobytes(), (names, k)
        # close() right after a device-form call waits for it, whichever list the handle stands in
        fa, fb = [h.k.merge() for h in LA], [h.k.merge() for h in LB]           # copies, to be closed at once
        out, junk = _device_out(torch, M), _device_out(torch, M)
        torch.cuda.synchronize()
        for _ in range(20):                                                      # work ahead of the call on the same stream
            fb[-1].compare(fa, M, earlier=fb[:-1], out=junk, stream=st)
        fb[-1].compare(fa, M, earlier=fb[:-1], out=out, stream=st)
        for k in fa + fb:
            k.close()                                                            # waits for the enqueued kernels
        st.synchronize()
        same_bits(_back(out), host, (kind, "closed right after the call"))
    for h in LA + LB + [c.A, c.B, c.A_sub, c.B_sub]:                              # only read
        same_listing(h.k, h.rec, "after the readers")
