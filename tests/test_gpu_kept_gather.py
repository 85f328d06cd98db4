"""lh_kept_gather* (Kept.gather, loghisto_amd.fleet): kept rows re-mapped PER HANDLE and summed into one kept handle -- exactly what
lh_keep would return for a snapshot whose row first_out + j has cells C[b] = the sum over i of cell b of row src[i][j] of kept[i].

The inputs are the crafted handles of tests/test_gpu_kept.py (70 rows, 6 handles, engines of 64- and of 32-bit cells: cells either
side of every tile edge, eight tiles, bins 0 and 65 535, a cell that wraps to 0 when its handle is listed twice, more rows than a
workgroup has waves).  The references are lh_kept_merge (identity maps), Python integers over the fixture's rows, and
loghisto_amd.keptfile.gather over the saved blobs; every comparison is byte for byte and every check runs under both kernel shapes
(lh_tool_kept_switch).  One handle goes the direct route by default: the forced tile route and the transposed map
(lh_tool_kept_gather_route) must give the same bytes.
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from loghisto_amd import _native as N
from loghisto_amd import fleet, keptfile
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import BIG, LISTS, arrays_of, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_merge import listing

pytestmark = pytest.mark.gpu

U64 = np.uint64
WRAP = 1 << 64
NO = N.KEPT_NO_ROW
KINDS = ("wave", "block")
SENTINEL = 0x77
INFO = ("first", "nrows", "cells", "samples", "bytes")
_BLOBS = {}


@contextlib.contextmanager
def route(value):
    prev, now = C.c_uint32(0), C.c_uint32(0)
    assert N.lib().lh_tool_kept_gather_route(value, C.byref(prev)) == 0
    try:
        yield
    finally:
        assert N.lib().lh_tool_kept_gather_route(prev.value, C.byref(now)) == 0 and now.value == value


def gather(handles, src, **kw):
    return handles[-1].gather(src, handles[:-1], **kw)


def blob_of(c, i):
    """handle i's saved bytes, once per fixture"""
    key = (c.wide, i)
    if key not in _BLOBS:
        _BLOBS[key] = c.kept[i].to_bytes()
    return _BLOBS[key]


def model(c, lst, src):
    """Python integers: per output row {bin: the sum mod 2^64, zeros dropped}, and the sum mod 2^64 of the source rows' totals"""
    rows, rcs = [], []
    for j in range(len(src[0])):
        cells, rc = {}, 0
        for i, line in zip(lst, src):
            if line[j] != NO:
                for b, x in c.rows[i][line[j]].items():
                    cells[b] = (cells.get(b, 0) + x) % WRAP
                    rc = (rc + x) % WRAP
        rows.append({b: x for b, x in cells.items() if x})
        rcs.append(rc)
    return rows, rcs


def held_to_both(c, k, lst, src, first_out, rows, rcs, blob, what):
    """the handle k against the Python-integer model (rows, rcs) and against keptfile.gather of the saved source handles (blob)"""
    want = listing(rows)
    off, keys, counts, row_count = arrays_of(k)
    assert np.array_equal(off, want[0]) and np.array_equal(keys, want[1]) and np.array_equal(counts, want[2]), what
    assert [int(x) for x in row_count] == rcs, what
    cells = len(want[1])
    assert {f: k.info[f] for f in INFO} == dict(first=first_out, nrows=len(rows), cells=cells, samples=sum(rcs) % WRAP,
                                               bytes=keptfile.block_bytes(len(rows), cells)), what
    assert k.to_bytes() == blob, what
    assert {f: k.info[f] for f in INFO} == {f: keptfile.unpack(blob)[f] for f in INFO}, what


def cases(c):
    """(name, handles of the fixture, map, first_out) of check 2"""
    M = c.M
    rng = np.random.default_rng(20)
    three = [[int(x) for x in rng.permutation(M)] for _ in range(3)]
    for line in three:
        for j in rng.choice(M, 9, replace=False):
            line[int(j)] = NO
    three[0][7] = three[1][7] = three[2][7] = NO                              # an output row nobody feeds
    rev = list(range(M - 1, -1, -1))
    return [
        ("reversed", [2], [rev], 0),
        ("reversed, the handle of the large cells", [BIG], [rev], 5),
        ("every row twice", [0], [[m // 2 for m in range(2 * M)]], 0),
        ("one row", [2], [[c.at["edges_in_one"]]], 0),
        ("one row, the last there is", [1], [[c.at["dense300"]]], WRAP // (1 << 32) - 1),
        ("nothing at all", [0], [[NO] * 5], 0),
        ("three handles, a permutation each", [0, BIG, 4], three, 0),
        ("three handles, at the end of the row space", [0, BIG, 4], three, (1 << 32) - M),
        ("the same handle twice with the same map: half_of_2^64 wraps to 0", [BIG, BIG], [rev, rev], 5),
        ("one handle three times with different maps", [1, 1, 1], three, 0),
    ]


# ---- 1. identity maps: the merge -----------------------------------------------------------------------------------------------
def test_identity_maps_give_the_merge(crafted):
    c = crafted
    ident = np.arange(c.M, dtype=np.uint32)
    got = {}
    for kind in KINDS:
        with shape(kind):
            for lst in LISTS:
                hs = [c.kept[i] for i in lst]
                with gather(hs, np.tile(ident, (len(hs), 1))) as g, hs[-1].merge(hs[:-1]) as m:
                    assert [a.tobytes() for a in arrays_of(g)] == [a.tobytes() for a in arrays_of(m)], (kind, lst[:8], len(lst))
                    assert g.info == m.info, (kind, lst[:8])
                    got[kind, tuple(lst)] = g.to_bytes()
                # a sub-block, written where it came from
                with gather(hs, np.tile(ident[3:8], (len(hs), 1)), first=3) as g, hs[-1].merge(hs[:-1], 5, 3) as m:
                    assert g.to_bytes() == m.to_bytes(), (kind, lst[:8])
    for lst in LISTS:
        assert got["wave", tuple(lst)] == got["block", tuple(lst)], lst[:8]


# ---- 2. against the two models ---------------------------------------------------------------------------------------------------
def test_against_python_integers_and_keptfile_gather(crafted):
    c = crafted
    for name, lst, src, first_out in cases(c):
        rows, rcs = model(c, lst, src)                                        # the references, once per case
        blob = keptfile.gather([blob_of(c, i) for i in lst], src, first_out)
        for kind in KINDS:
            with shape(kind), gather([c.kept[i] for i in lst], np.array(src, dtype=np.uint32), first=first_out) as k:
                held_to_both(c, k, lst, src, first_out, rows, rcs, blob, (name, kind))
    # what the cases were made for
    with gather([c.kept[0]], [NO] * 5) as k:
        assert k.info["cells"] == 0 and k.info["samples"] == 0 and k.info["nrows"] == 5 and keptfile.check(k.to_bytes()) is None
    rev = list(range(c.M - 1, -1, -1))
    with gather([c.kept[BIG], c.kept[BIG]], [rev, rev]) as k:
        off = arrays_of(k)[0]
        j = c.M - 1 - c.at["half_of_2^64"]
        bins = (arrays_of(k)[1][int(off[j]):int(off[j + 1])].astype(np.int64) & 0xffff) ^ 0x8000
        assert list(bins) == [300] and int(arrays_of(k)[3][j]) == 14            # bin 100 wrapped to 0 and is not listed


# ---- 3. the routes ---------------------------------------------------------------------------------------------------------------
def test_the_routes_give_identical_bytes(crafted):
    c = crafted
    for name, lst, src, first_out in cases(c):
        hs, a = [c.kept[i] for i in lst], np.array(src, dtype=np.uint32)
        got = {}
        for kind in KINDS:
            for r in (N.GATHER_DEFAULT, N.GATHER_DIRECT, N.GATHER_TILE, N.GATHER_TRANSPOSED):
                with shape(kind), route(r), gather(hs, a, first=first_out) as k:
                    got[kind, r] = k.to_bytes()
        assert len(set(got.values())) == 1, (name, [key for key, v in got.items() if v != got["wave", N.GATHER_DEFAULT]])


# ---- 4. the readers see what they should -----------------------------------------------------------------------------------------
def test_across_over_a_gathered_handle_is_across_by_ids_over_its_source(crafted):
    c = crafted
    P = [0.5, 0.99, 1.0]
    src = np.random.default_rng(21).permutation(c.M).astype(np.uint32)
    for kind in KINDS:
        for i in (1, BIG):
            with shape(kind), gather([c.kept[i]], src) as g:
                got, want = g.across([], P, c.M), c.kept[i].across([], P, ids=src)
                assert set(got) == set(want)
                for f in got:
                    assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), (kind, i, f)


# ---- 5. the device form ------------------------------------------------------------------------------------------------------------
def test_device_rows_outside_a_block_count_as_no_row_and_the_host_form_refuses_them(crafted):
    c = crafted
    torch = c.torch
    sub = c.extra["sub"][0]                                                   # rows 3 .. 7 of handle 0
    assert (sub.info["first"], sub.info["nrows"]) == (3, 5)
    wild = np.array([[0, 3, 69, 7, 2, 70, 4], [2, 7, 5, 0xfffffffe, 3, 70, 4]], dtype=np.uint32)
    tame = wild.copy()
    tame[0, 5] = NO                                                           # handle 0 holds rows 0 .. 69
    tame[1, [0, 3, 5]] = NO                                                   # rows 2, 0xfffffffe and 70 are outside [3, 8)
    hs = [c.kept[0], sub]
    d_wild = torch.from_numpy(wild.view(np.int32)).cuda()
    for kind in KINDS:
        with shape(kind), gather(hs, d_wild, first=9) as dev, gather(hs, tame, first=9) as host:
            assert dev.to_bytes() == host.to_bytes() and dev.info == host.info, kind
            assert dev.to_bytes() == keptfile.gather([blob_of(c, 0), sub.to_bytes()], tame, 9), kind
        with shape(kind), gather([sub], torch.from_numpy(wild[1].view(np.int32).copy()).cuda()) as dev, gather([sub], tame[1]) as host:
            assert dev.to_bytes() == host.to_bytes(), kind                    # one handle: the direct route guards its rows too
    # the host form with the same array: LH_ERANGE, *out as it was
    handles = (C.c_void_p * 2)(hs[0]._h.value, hs[1]._h.value)
    out = C.c_void_p(SENTINEL)
    assert N.lib().lh_kept_gather(handles, 2, wild.ctypes.data, wild.shape[1], 9, 0, None, C.byref(out)) == N.ERANGE
    assert out.value == SENTINEL
    import loghisto_amd
    with pytest.raises(loghisto_amd.LhError) as e:
        gather(hs, wild, first=9)
    assert e.value.code == N.ERANGE
    for bad in ([[0, 1]], [[0, 1], [3, 4], [3, 4]], np.zeros((2, 2, 2), dtype=np.uint32)):   # not a line per handle
        with pytest.raises(ValueError):
            gather(hs, bad)


# ---- 6. a fleet, end to end --------------------------------------------------------------------------------------------------------
def test_two_processes_with_their_own_name_orders_add_up_to_one(native_lib, torch_cuda):
    rng = np.random.default_rng(22)
    names = ["rpc.latency", "db.query", "größe", "cache.hit", "queue.depth", "gc.pause", "disk.io"]
    mine = [[names[i] for i in (4, 0, 2, 6, 1)], [names[i] for i in (3, 1, 5, 0)]]      # overlapping sets, other orders
    n = 600
    who = rng.integers(0, len(names), n)
    v = rng.lognormal(2.0, 1.5, n)
    share = [[j for j in range(n) if names[who[j]] in mine[0] and (names[who[j]] not in mine[1] or j % 2)], None]
    share[1] = [j for j in range(n) if j not in set(share[0])]
    assert all(names[who[j]] in mine[1] for j in share[1]) and len(share[0]) > 100 and len(share[1]) > 100

    def interval(order, take):
        """an engine that interns `order`, takes samples `take` -> (its kept interval, the sidecar of its rows' names)"""
        with engine(len(order)) as e:
            ids = {name: e.intern(name) for name in order}
            e.submit_pairs(np.array([ids[names[who[j]]] for j in take], dtype=np.uint32), v[take])
            with e.flip() as s:
                k = s.keep(len(order))
            return k, keptfile.pack_names([e.metric_name(m) for m in range(len(order))], k.info["first"])

    parts = [interval(order, take) for order, take in zip(mine, share)]
    lists = [keptfile.unpack_names(sidecar) for _, sidecar in parts]
    assert lists == mine
    union, src = fleet.union_names(lists)
    assert sorted(union) == sorted(names) and union[:5] == mine[0]
    whole, sidecar = interval(union, list(range(n)))
    assert keptfile.unpack_names(sidecar) == union
    for kind in KINDS:
        with shape(kind):
            total, got_union = fleet.aggregate([k for k, _ in parts], lists)
            with total:
                assert got_union == union and total.info == whole.info and total.info["samples"] == n
                assert total.to_bytes() == whole.to_bytes(), kind
    for k in [whole] + [k for k, _ in parts]:
        k.close()


# ---- 7. the new handle depends on none of its sources ----------------------------------------------------------------------------------
def test_the_sources_may_go_right_after_the_call(native_lib, torch_cuda):
    from loghisto_amd import Kept
    rows = [{100: 3, 5000: 1}, {}, {0: 2, 65535: 9}, {40000 + b: 1 + b for b in range(300)}]
    blobs = []
    for shift in (0, 1):
        off = np.cumsum([0] + [len(r) for r in rows]).astype(U64)
        bins = np.array([b for r in rows for b in sorted(r)], dtype=np.int64)
        counts = np.array([r[b] + shift for r in rows for b in sorted(r)], dtype=U64)
        blobs.append(keptfile.pack(off, (bins ^ 0x8000).astype(np.uint16).view(np.int16), counts, first=2 * shift))
    src = np.array([[3, 0, NO, 2, 3], [2, NO, 5, 4, 3]], dtype=np.uint32)
    want = keptfile.gather(blobs, src, 1)
    hs = [Kept.from_bytes(b) for b in blobs]
    g = gather(hs, src, first=1)
    for h in hs:
        h.close()
    torch_cuda.cuda.synchronize()
    junk = torch_cuda.full((1 << 16,), -1, dtype=torch_cuda.int64, device="cuda")   # whatever takes the freed blocks' place
    assert g.to_bytes() == want
    with Kept.from_bytes(g.to_bytes()) as back:
        assert back.to_bytes() == want and back.info == g.info
    assert [int(x) for x in g.across([], [0.5], 5, 1)["count"]] == keptfile.unpack(want)["row_count"].tolist()
    del junk
    g.close()
