"""lh_kept_group* (Kept.group, loghisto_amd.fleet.roll_up): many kept rows summed into ONE row, by group -- exactly what lh_keep
would return for a snapshot whose row first_out + g has cells C[b] = the sum over the handles i and over the members r of group g
of cell b of row r of kept[i].  The three equivalences of the header are the definition and the tests: singleton groups are the
gather (identity members: the merge), small groups are the gather of the list in which every handle stands G times, and any
partition of the member lists is the merge of the pieces' groups.

The inputs are the crafted handles of tests/test_gpu_kept.py (70 rows, 6 handles, engines of 64- and of 32-bit cells: cells either
side of every tile edge, eight tiles, bins 0 and 65 535, a cell that wraps to 0 when counted twice, a row of 2^64 - 1 samples, a row
that never saw one).  Beyond 64 sources a group goes in chunks of 64 sources: the sizes either side of a chunk's edge are here, with
the eight-tile row and the rows of the tile edges in the first chunk, in the last, and either side of source 63 / 64.  Every
comparison is byte for byte -- the four arrays, info, to_bytes() -- and every check runs under both kernel shapes
(lh_tool_kept_switch).  No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import ctypes as C

import numpy as np
import pytest

from loghisto_amd import _native as N
from loghisto_amd import fleet, keptfile
from tests.test_gpu_kept import BIG, K, LISTS, arrays_of, crafted, shape  # noqa: F401  (crafted: the fixture)
from tests.test_gpu_kept_merge import listing

pytestmark = pytest.mark.gpu

WRAP = 1 << 64
NO = N.KEPT_NO_ROW
KINDS = ("wave", "block")
SENTINEL = 0x77
INFO = ("first", "nrows", "cells", "samples", "bytes")
_BLOBS = {}


def csr(groups):
    return np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64), np.array([r for g in groups for r in g], dtype=np.uint32)


def group(handles, groups, **kw):
    return handles[-1].group(groups, handles[:-1], **kw)


def gather(handles, src, **kw):
    return handles[-1].gather(src, handles[:-1], **kw)


def blob_of(c, i):
    """handle i's saved bytes, once per fixture"""
    key = (c.wide, i)
    if key not in _BLOBS:
        _BLOBS[key] = c.kept[i].to_bytes()
    return _BLOBS[key]


def model(c, lst, groups, blocks=None):
    """Python integers: per group {bin: the sum mod 2^64, zeros dropped}, and the sum mod 2^64 of the source rows' totals.  blocks
    (the device form): per handle of the list the rows [lo, end) it holds -- a member outside counts as nothing for that handle."""
    rows, rcs = [], []
    for g in groups:
        cells, rc = {}, 0
        for n, i in enumerate(lst):
            for r in g:
                if r == NO or (blocks and not blocks[n][0] <= r < blocks[n][1]):
                    continue
                for b, x in c.rows[i][r].items():
                    cells[b] = (cells.get(b, 0) + x) % WRAP
                    rc = (rc + x) % WRAP
        rows.append({b: x for b, x in cells.items() if x})
        rcs.append(rc)
    return rows, rcs


def same(a, b, what):
    """two handles, byte for byte: the four arrays, info, the saved bytes"""
    assert [x.tobytes() for x in arrays_of(a)] == [x.tobytes() for x in arrays_of(b)], what
    assert a.info == b.info, what
    assert a.to_bytes() == b.to_bytes(), what


def held_to_model(k, first_out, rows, rcs, what, blob=None):
    """the handle k against the Python-integer model (rows, rcs) and, if given, keptfile.group of the saved source handles"""
    want = listing(rows)
    off, keys, counts, row_count = arrays_of(k)
    assert np.array_equal(off, want[0]) and np.array_equal(keys, want[1]) and np.array_equal(counts, want[2]), what
    assert [int(x) for x in row_count] == rcs, what
    cells = len(want[1])
    assert {f: k.info[f] for f in INFO} == dict(first=first_out, nrows=len(rows), cells=cells, samples=sum(rcs) % WRAP,
                                               bytes=keptfile.block_bytes(len(rows), cells)), what
    saved = k.to_bytes()
    assert keptfile.check(saved) is None, what
    if blob is not None:
        assert saved == blob, what
        assert {f: k.info[f] for f in INFO} == {f: keptfile.unpack(blob)[f] for f in INFO}, what


# ---- 1. singleton groups: the merge, the gather ------------------------------------------------------------------------------------
def test_singleton_groups_give_the_merge_and_the_gather(crafted):
    c = crafted
    ident = [[m] for m in range(c.M)]
    rng = np.random.default_rng(30)
    perm = [int(x) for x in rng.permutation(c.M)]
    for j in rng.choice(c.M, 9, replace=False):
        perm[int(j)] = NO
    got = {}
    for kind in KINDS:
        with shape(kind):
            for lst in LISTS:
                hs = [c.kept[i] for i in lst]
                with group(hs, ident) as g, hs[-1].merge(hs[:-1]) as m:
                    same(g, m, (kind, lst[:8], len(lst)))
                    got[kind, tuple(lst)] = g.to_bytes()
                with group(hs, ident[3:8], first=3) as g, hs[-1].merge(hs[:-1], 5, 3) as m:   # a sub-block, written where it came from
                    same(g, m, (kind, lst[:8], "sub-block"))
                # a permutation with holes: the gather with that one map for every handle
                with group(hs, [[r] for r in perm], first=11) as g, gather(hs, np.tile(np.array(perm, dtype=np.uint32), (len(hs), 1)), first=11) as m:
                    same(g, m, (kind, lst[:8], "permutation"))
    for lst in LISTS:
        assert got["wave", tuple(lst)] == got["block", tuple(lst)], lst[:8]


# ---- 2. small groups: the gather of the list in which every handle stands G times -------------------------------------------------
def small_cases(c):
    rng = np.random.default_rng(31)

    def groups_of(sizes):
        gs = [[int(x) for x in rng.integers(0, c.M, n)] for n in sizes]
        for g in gs:
            if len(g) >= 3:
                g[len(g) // 2] = NO                                           # nothing, in the middle of a group
        gs[0][0], gs[1][-1] = c.at["eight_tiles"], c.at["edges_in_one"]
        return gs

    ten = [1, 10, 2, 9, 3, 8, 4, 7, 5, 6, 10, 1]
    return [("1 handle, groups of 1 .. 10", [2], groups_of(ten)),
            ("2 handles, groups of 1 .. 10", [0, BIG], groups_of(ten)),
            ("3 handles, groups of 1 .. 10", [1, 2, 4], groups_of(ten)),
            ("6 handles, groups of 1 .. 10: 60 sources", list(range(K)), groups_of(ten)),
            ("1 handle x 64 members: exactly 64 sources", [2], groups_of([64, 3, 64, 1, 63])),
            ("2 handles x 32 members: exactly 64 sources", [BIG, 5], groups_of([32, 31, 1, 32])),
            ("the same handle twice x 32", [BIG, BIG], groups_of([32, 2, 17]))]


def repeated(hs, groups):
    """the gather equivalence 2 names: every handle G times in a row, copy c mapped to member c of each group"""
    G = max(len(g) for g in groups)
    maps = [[g[k] if k < len(g) else NO for g in groups] for k in range(G)]
    return [h for h in hs for _ in range(G)], np.array(maps * len(hs), dtype=np.uint32)


def test_small_groups_are_the_gather_of_the_repeated_list(crafted):
    c = crafted
    for name, lst, groups in small_cases(c):
        hs = [c.kept[i] for i in lst]
        many, src = repeated(hs, groups)
        assert len(many) <= N.MAX_KEPT
        rows, rcs = model(c, lst, groups)
        for kind in KINDS:
            with shape(kind), group(hs, groups, first=4) as g, gather(many, src, first=4) as m:
                same(g, m, (name, kind))
                held_to_model(g, 4, rows, rcs, (name, kind))


# ---- 3. the chunk edge -------------------------------------------------------------------------------------------------------------
def placed(c, rng, n):
    """n members drawn from all rows with repeats; the eight-tile row and the rows with cells at tile edges in the first chunk, in
    the last, and either side of source 63 / 64"""
    g = [int(x) for x in rng.integers(0, c.M, n)]
    wide, edge, other, dense = c.at["eight_tiles"], c.at["edges_in_one"], c.at["edges"], c.at["dense_over_an_edge"]
    for pos, r in ((0, wide), (1, edge), (2, NO), (62, other), (63, edge), (64, wide), (65, dense), (n - 2, edge), (n - 1, wide)):
        if 0 <= pos < n:
            g[pos] = r
    return g


def chunk_cases(c):
    rng = np.random.default_rng(32)
    every = list(range(c.M))
    return [("1 handle, groups of 63, 64, 65, 128 and 129", [2], [placed(c, rng, n) for n in (63, 64, 65, 128, 129)], 0),
            ("6 handles x all 70 rows: 420 sources", list(range(K)), [every], 9),
            ("a member, nothing and 129 members in one call", [2], [[c.at["edges_in_one"]], [], placed(c, rng, 129)], 0),
            ("2 handles x 33 members: 66 sources, the second handle starts in chunk 0", [0, BIG], [placed(c, rng, 33), [5], every], 1)]


def test_groups_of_more_than_64_sources_go_in_chunks(crafted):
    c = crafted
    for name, lst, groups, first_out in chunk_cases(c):
        rows, rcs = model(c, lst, groups)                                     # the references, once per case
        blob = keptfile.group([blob_of(c, i) for i in lst], *csr(groups), first_out)
        got = {}
        for kind in KINDS:
            with shape(kind), group([c.kept[i] for i in lst], groups, first=first_out) as k:
                held_to_model(k, first_out, rows, rcs, (name, kind), blob)
                got[kind] = k.to_bytes()
        assert got["wave"] == got["block"], name
    assert len(rows[-1]) > 8 * c.T // (97 * K)                                # (the rows of eight tiles were summed)


# ---- 4. wraps ----------------------------------------------------------------------------------------------------------------------
def test_cells_and_row_counts_wrap(crafted):
    c = crafted
    half, total, never = c.at["half_of_2^64"], c.at["total_2^64-1"], c.at["never"]
    far = [never if j % 2 else NO for j in range(70)]
    far[3] = far[67] = half                                                   # the two copies in different chunks
    for kind in KINDS:
        for groups in ([[half, half]], [far]):
            with shape(kind), group([c.kept[BIG]], groups) as k:
                off, keys, counts, row_count = arrays_of(k)
                bins = (keys.astype(np.int64) & 0xffff) ^ 0x8000
                assert list(bins) == [300] and [int(x) for x in counts] == [14], kind   # bin 100: 2^63 + 2^63 wrapped to 0, not listed
                assert [int(x) for x in row_count] == [14] and k.info["samples"] == 14 and k.info["cells"] == 1, kind
        # 2^64 - 1 samples and one more: row_count wraps to 0 with cells present
        one = c.at["far_apart"]
        assert sum(c.rows[0][one].values()) == 1 and not c.rows[BIG][one] and not c.rows[0][total]
        with shape(kind), group([c.kept[BIG], c.kept[0]], [[total, one]]) as k:
            rows, rcs = model(c, [BIG, 0], [[total, one]])
            assert rcs == [0] and len(rows[0]) == 3
            held_to_model(k, 0, rows, rcs, kind)
            assert k.info["samples"] == 0 and k.info["cells"] == 3, kind


# ---- 5. any partition of the member lists: the merge of the pieces --------------------------------------------------------------------
def test_a_group_is_the_merge_of_the_groups_of_its_pieces(crafted):
    c = crafted
    hs = [c.kept[i] for i in range(K)]
    every = list(range(c.M))
    for kind in KINDS:
        with shape(kind), group(hs, [every]) as whole:
            with group(hs, [every[:35]]) as a, group(hs, [every[35:]]) as b, b.merge([a]) as m:
                same(whole, m, (kind, "halves"))
            with group(hs, [every[0::3]]) as a, group(hs, [every[1::3]]) as b, group(hs, [every[2::3]]) as d, d.merge([a, b]) as m:
                same(whole, m, (kind, "thirds"))
            # a roll-up, rolled up again: seven groups of ten rows, then the seven
            with group(hs, [every[10 * j:10 * j + 10] for j in range(7)], first=100) as tens, group([tens], [list(range(100, 107))]) as again:
                same(whole, again, (kind, "a group of a grouped handle"))


# ---- 6. nothing at all --------------------------------------------------------------------------------------------------------------
def test_calls_in_which_no_cell_survives_give_a_valid_handle(crafted):
    c = crafted
    never = c.at["never"]
    for kind in KINDS:
        for groups in ([[NO, NO, NO], [NO]], [[], [], []], [[never], [never] * 70, [never, NO]]):
            for lst in ([0], [0, BIG, 4]):
                for first_out in (0, (1 << 32) - len(groups)):
                    with shape(kind), group([c.kept[i] for i in lst], groups, first=first_out) as k:
                        assert k.info == dict(k.info, first=first_out, nrows=len(groups), cells=0, samples=0,
                                              bytes=keptfile.block_bytes(len(groups), 0)), (kind, groups[0][:2])
                        blob = k.to_bytes()
                        assert blob == keptfile.group([blob_of(c, i) for i in lst], *csr(groups), first_out), kind
                        assert keptfile.check(blob) is None and not np.any(arrays_of(k)[0]) and not np.any(arrays_of(k)[3])
    import loghisto_amd
    with pytest.raises(loghisto_amd.LhError) as e:                            # one row beyond the last there is
        group([c.kept[0]], [[], []], first=(1 << 32) - 1)
    assert e.value.code == N.ERANGE


# ---- 7. the device form --------------------------------------------------------------------------------------------------------------
def test_the_device_form_clamps_and_the_host_form_refuses(crafted):
    c = crafted
    torch = c.torch
    sub = c.extra["sub"][0]                                                   # rows 3 .. 7 of handle 0
    assert (sub.info["first"], sub.info["nrows"]) == (3, 5)
    hs, lst, blocks = [c.kept[2], sub], [2, 0], [(0, c.M), (3, 8)]
    handles = (C.c_void_p * 2)(hs[0]._h.value, hs[1]._h.value)
    out = C.c_void_p(SENTINEL)

    def on_device(goff, members, pad=16):
        """the arrays in the middle of allocations filled with a sentinel that would be a wild row / a wild offset"""
        g = np.full(len(goff) + 2 * pad, 0x7777777777777777, dtype=np.uint64)
        m = np.full(len(members) + 2 * pad, 0x77777777, dtype=np.uint32)
        g[pad:pad + len(goff)], m[pad:pad + len(members)] = goff, members
        dg, dm = torch.from_numpy(g.view(np.int64)).cuda(), torch.from_numpy(m.view(np.int32)).cuda()
        return (dg[pad:pad + len(goff)], dm[pad:pad + len(members)]), (dg, dm, g, m)

    def untouched(whole):
        dg, dm, g, m = whole
        assert np.array_equal(dg.cpu().numpy().view(np.uint64), g) and np.array_equal(dm.cpu().numpy().view(np.uint32), m)

    # members outside a handle's block: nothing for THAT handle, whatever they are for the other
    wild = [[0, 3, 69, 7, 2], [70, 4, 0xfffffffe], [5] + list(range(c.M)) + [70, 5], [1 << 31, 70]]
    goff, members = csr(wild)
    rows, rcs = model(c, lst, wild, blocks)
    assert rows[1] == model(c, lst, [[4]])[0][0] and not rows[3] and rows[0] != model(c, [2], wild, blocks[:1])[0][0]
    view, whole = on_device(goff, members)
    for kind in KINDS:
        with shape(kind), group(hs, view, first=9) as k:
            held_to_model(k, 9, rows, rcs, (kind, "members outside a block"))
    untouched(whole)
    assert N.lib().lh_kept_group(handles, 2, goff.ctypes.data, members.ctypes.data, members.size, len(wild), 9, 0, None, C.byref(out)) == N.ERANGE
    assert N.lib().lh_kept_group(handles, 2, goff.ctypes.data, members.ctypes.data, 5, 1, 9, 0, None, C.byref(out)) == N.ERANGE   # row 2: sub lacks it
    # a goff that decreases, and one that runs past nmembers: a = min(goff[g], nmembers), b = min(goff[g + 1], nmembers), none if b <= a
    members = np.array([3 + (7 * j) % 5 for j in range(70)], dtype=np.uint32)
    assert all(3 <= int(r) < 8 for r in members)                              # (every member is inside both blocks)
    nm = members.size
    for goff, clamped in (([0, 4, 2, 9, 5, 70], [(0, 4), (4, 2), (2, 9), (9, 5), (5, 70)]),          # decreases twice
                          ([0, 66, 200, 1 << 40, 3, 71], [(0, 66), (66, 70), (70, 70), (70, 3), (3, 70)]),   # past nmembers
                          ([90, 80, 5, (1 << 64) - 1], [(70, 70), (70, 5), (5, 70)])):               # (the first entry is not 0)
        groups = [[int(r) for r in members[a:b]] if b > a else [] for a, b in clamped]
        rows, rcs = model(c, lst, groups)
        view, whole = on_device(np.array(goff, dtype=np.uint64), members)
        for kind in KINDS:
            with shape(kind), group(hs, view) as k:
                held_to_model(k, 0, rows, rcs, (kind, goff))
        untouched(whole)
        g = np.array(goff, dtype=np.uint64)
        assert N.lib().lh_kept_group(handles, 2, g.ctypes.data, members.ctypes.data, nm, len(goff) - 1, 0, 0, None, C.byref(out)) == N.EINVAL
    assert out.value == SENTINEL                                              # through every refusal
    torch.cuda.synchronize()                                                  # (nothing was enqueued: nothing to wait for, nothing failed)
    # the sound call over the same members is taken, by both forms alike
    sound = [0, 4, 4, 9, 9, 70]
    view, _ = on_device(np.array(sound, dtype=np.uint64), members)
    with group(hs, view) as dev, group(hs, (np.array(sound, dtype=np.uint64), members)) as host:
        same(dev, host, "the two forms")
    import loghisto_amd
    for bad, code in ((([0, 4, 2, 70], members), N.EINVAL), (([0, 2], np.array([3, 70], dtype=np.uint32)), N.ERANGE)):
        with pytest.raises(loghisto_amd.LhError) as e:
            group(hs, (np.array(bad[0], dtype=np.uint64), bad[1]))
        assert e.value.code == code
    for bad in ([[-1]], [[1 << 32]], (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32)), []):
        with pytest.raises(ValueError):
            group(hs, bad)


# ---- 8. a reader on the result --------------------------------------------------------------------------------------------------------
def test_across_over_a_grouped_handle_is_across_over_the_equivalent_gather(crafted):
    c = crafted
    P = [0.5, 0.99, 1.0]
    name, lst, groups = small_cases(c)[3]
    hs = [c.kept[i] for i in lst]
    many, src = repeated(hs, groups)
    for kind in KINDS:
        with shape(kind), group(hs, groups) as g, gather(many, src) as m:
            got, want = g.across([], P, len(groups)), m.across([], P, len(groups))
            for f in ("count", "sum", "pkeys", "pvalid"):
                assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), (kind, f)
            assert [int(x) for x in got["count"]] == model(c, lst, groups)[1], kind


# ---- 9. by label, end to end ------------------------------------------------------------------------------------------------------------
def test_roll_up_by_label(crafted):
    c = crafted
    names = [kind for kind, _ in c.names]

    def key(name):
        if name == "never":
            return None
        return ("random", "all") if name.startswith("random") else (name.split("_")[0], "all")

    labels, goff, members = fleet.group_names(names, key)
    assert labels[:3] == ["plain", "all", "marked"] and "random" in labels and "never" not in labels
    groups = [[int(r) for r in members[int(a):int(b)]] for a, b in zip(goff[:-1], goff[1:])]
    assert groups[labels.index("all")] == [m for m in range(c.M) if m != c.at["never"]]
    hs = [c.kept[0], c.kept[BIG]]
    rows, rcs = model(c, [0, BIG], groups)
    for kind in KINDS:
        with shape(kind):
            k, got = fleet.roll_up(hs, names, key)
            with k:
                assert got == labels
                held_to_model(k, 0, rows, rcs, kind)
