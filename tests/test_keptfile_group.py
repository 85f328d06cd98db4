"""loghisto_amd.keptfile.group -- lh_kept_group stated on blobs, the reference the device is held to -- against hand-written
dict-of-rows models and against keptfile.gather / keptfile.combine (the equivalences that define it); loghisto_amd.fleet.group_names.
No GPU, no library."""
import numpy as np
import pytest

from loghisto_amd import fleet, keptfile

NO = keptfile.NO_ROW
M64 = (1 << 64) - 1
NK = 65536


def blob_of(rows, first=0):
    """[{bin: count}] -> the blob of rows [first, first + len(rows))"""
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    bins = np.array([b for r in rows for b in sorted(r)], dtype=np.int64)
    keys = ((bins ^ 0x8000).astype(np.uint16)).view(np.int16)
    counts = np.array([r[b] for r in rows for b in sorted(r)], dtype=np.uint64)
    blob = keptfile.pack(off, keys, counts, first=first)
    assert keptfile.check(blob) is None
    return blob


def rows_of(blob):
    """-> (first, [{bin: count}], row_count, samples) of a sound blob"""
    assert keptfile.check(blob) is None
    u = keptfile.unpack(blob)
    bins = (u["keys"].view("<u2") ^ np.uint16(0x8000)).tolist()
    counts = u["counts"].tolist()
    rows = []
    for a, b in zip(u["offsets"][:-1].tolist(), u["offsets"][1:].tolist()):
        assert bins[a:b] == sorted(set(bins[a:b]))                            # ascending, each once
        rows.append(dict(zip(bins[a:b], counts[a:b])))
    return u["first"], rows, u["row_count"].tolist(), u["samples"]


def csr(groups):
    return np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64), np.array([r for g in groups for r in g], dtype=np.uint32)


def added(*rows):
    out = {}
    for r in rows:
        for b, c in r.items():
            out[b] = (out.get(b, 0) + c) & M64
    return {b: c for b, c in out.items() if c}


def total(*rows):
    return sum(sum(r.values()) for r in rows) & M64


A = [{0: 1, 100: 3}, {}, {NK - 1: 7, 5: 2}, {100: 1 << 63}, {1023: 1, 1024: 2}]   # rows 10 .. 14
B = [{100: 4, 200: 5}, {100: 1 << 63, 7: 9}, {NK - 1: 1}, {3: M64}, {3: 1}]        # rows 10 .. 14
BA, BB = blob_of(A, first=10), blob_of(B, first=10)


def test_singleton_groups_are_the_gather_with_one_map_for_every_blob():
    for src in ([10, 11, 12, 13, 14], [14, NO, 10, 10, 12, NO], [NO], [13]):
        goff, members = csr([[r] for r in src])
        for blobs in ([BA], [BA, BB], [BB, BA, BA]):
            for first_out in (0, 7):
                assert keptfile.group(blobs, goff, members, first_out) == keptfile.gather(blobs, [src] * len(blobs), first_out)
    # identity members: the combine (the merge)
    goff, members = csr([[10 + g] for g in range(5)])
    assert keptfile.group([BA, BB], goff, members, 10) == keptfile.combine([BA, BB])
    goff, members = csr([[11], [12]])
    assert keptfile.group([BA, BB, BB], goff, members, 11) == keptfile.combine([BA, BB, BB], first=11, nrows=2)


def test_small_groups_are_the_gather_of_the_repeated_list():
    groups = [[10, 12, 14], [], [13], [11, NO, 10], [12, 12]]
    G = max(len(g) for g in groups)
    for blobs in ([BA], [BA, BB]):
        maps = [[g[c] if c < len(g) else NO for g in groups] for c in range(G)]
        want = keptfile.gather([b for b in blobs for _ in range(G)], maps * len(blobs), 3)
        assert keptfile.group(blobs, *csr(groups), 3) == want


def test_against_the_model_rows_in_two_groups_twice_in_one_no_row_and_an_empty_group():
    groups = [[10, 12], [10, 11, 12, 13, 14], [], [12, 12, 12], [NO, 14, NO], [NO]]
    first, rows, rc, samples = rows_of(keptfile.group([BA], *csr(groups), 100))
    want = [added(A[0], A[2]), added(*A), {}, {NK - 1: 21, 5: 6}, A[4], {}]
    assert first == 100 and rows == want
    assert rc == [total(A[0], A[2]), total(*A), 0, 27, 3, 0] and samples == sum(rc) & M64
    # two blobs, one listed twice: every source counts as often as it is named
    first, rows, rc, _ = rows_of(keptfile.group([BA, BB, BA], *csr([[10, 10], [14]])))
    assert rows == [added(A[0], A[0], B[0], B[0], A[0], A[0]), added(A[4], B[4], A[4])] and rc == [34, 7]
    # nothing at all: a sound blob without a cell
    for groups in ([[NO, NO], [NO]], [[], [], []], [[11]]):
        blob = keptfile.group([BA], *csr(groups))
        assert rows_of(blob) == (0, [{}] * len(groups), [0] * len(groups), 0) and keptfile.unpack(blob)["cells"] == 0
        assert len(blob) == keptfile.HEADER + keptfile.block_bytes(len(groups), 0)
    n = 2
    assert rows_of(keptfile.group([BB], *csr([[11], []]), (1 << 32) - n))[0] == (1 << 32) - n


def test_a_cell_that_wraps_to_zero_is_dropped_and_row_count_wraps():
    first, rows, rc, samples = rows_of(keptfile.group([BA], *csr([[13, 13], [13, 10, 13]])))
    assert rows == [{}, A[0]] and rc == [0, 4] and samples == 4               # 2^63 + 2^63: no cell, and row_count 0 with it
    first, rows, rc, samples = rows_of(keptfile.group([BA, BB], *csr([[13], [11, 13]])))
    assert rows == [{100: 1 << 63, 3: M64}, {7: 9, 3: M64}]                   # across blobs: A13 + B11 lose bin 100
    assert rc == [((1 << 63) + M64) & M64, (9 + M64) & M64]
    # row_count wraps to 0 with cells present: 2^64 - 1 and one more sample, in another bin and in the same
    first, rows, rc, samples = rows_of(keptfile.group([BB], *csr([[13, 10], [13, 14]])))
    assert rows == [{3: M64, 100: 4, 200: 5}, {}] and rc == [8, 0] and samples == 8
    first, rows, rc, _ = rows_of(keptfile.group([BB], *csr([[13, 12]])))
    assert rows == [{3: M64, NK - 1: 1}] and rc == [0]


def test_any_partition_of_the_member_lists_is_the_combine_of_the_pieces():
    groups = [[10, 11, 12, 13, 14, 13, 10], [12], [], [14, NO, 14, 11]]
    for blobs in ([BA], [BA, BB]):
        whole = keptfile.group(blobs, *csr(groups), 5)
        for cut in (0, 1, 2, 3, 7):
            pieces = [keptfile.group(blobs, *csr([g[:cut] for g in groups]), 5), keptfile.group(blobs, *csr([g[cut:] for g in groups]), 5)]
            assert keptfile.combine(pieces) == whole, cut
        thirds = [keptfile.group(blobs, *csr([g[k::3] for g in groups]), 5) for k in range(3)]
        assert keptfile.combine(thirds) == whole
        # a roll-up of a roll-up: groups of the grouped rows
        again = keptfile.group([whole], *csr([[5, 6], [8, 7, 5]]))
        assert again == keptfile.group(blobs, *csr([groups[0] + groups[1], groups[3] + groups[2] + groups[0]]))


def test_what_group_refuses():
    ok = csr([[10, 11], [12]])
    assert keptfile.check(keptfile.group([BA], *ok)) is None
    bad = [([1, 2, 3], [10, 11, 12]),                                         # the first entry is not 0
           ([0, 2, 1, 3], [10, 11, 12]),                                      # a decrease
           ([0, 2], [10, 11, 12]), ([0, 4], [10, 11, 12]),                    # the last entry is not len(members)
           ([0], []), ([], []),                                               # no group
           ([0, 1], [9]), ([0, 1], [15]), ([0, 2], [10, 0xfffffffe])]         # a member outside the block
    for goff, members in bad:
        with pytest.raises(ValueError):
            keptfile.group([BA], goff, members)
    short = blob_of(A[:3], first=10)                                          # rows 10 .. 12: row 13 is inside BA's block alone
    assert keptfile.check(keptfile.group([BA], [0, 1], [13])) is None
    for blobs in ([BA, short], [short, BA], [short]):
        with pytest.raises(ValueError):
            keptfile.group(blobs, [0, 1], [13])
    with pytest.raises(ValueError):
        keptfile.group([], *ok)
    with pytest.raises(ValueError):
        keptfile.group([BA[:-1]], *ok)
    assert keptfile.group([BA[:-1] + b"\0"], *ok, checked=False)              # (trusted: not looked at)
    with pytest.raises(ValueError):
        keptfile.group([BA], *ok, first_out=(1 << 32) - 1)
    with pytest.raises(ValueError):
        keptfile.group([BA], *ok, first_out=-1)


def test_group_names():
    names = ["api.get./a", "db.read", "api.get./b", "cache.hit", "api.post./a", "db.write"]
    labels, goff, members = fleet.group_names(names, lambda n: n.split(".")[0])
    assert labels == ["api", "db", "cache"]                                   # first appearance
    assert goff.dtype == np.uint64 and members.dtype == np.uint32
    assert goff.tolist() == [0, 3, 5, 6] and members.tolist() == [0, 2, 4, 1, 5, 3]   # members in row order
    # None drops a name; `first` makes the rows absolute
    labels, goff, members = fleet.group_names(names, lambda n: None if n.startswith("cache") else n.split(".")[0], first=100)
    assert labels == ["api", "db"] and goff.tolist() == [0, 3, 5] and members.tolist() == [100, 102, 104, 101, 105]
    # several labels per name: its service, its verb, and everything
    def key(n):
        part = n.split(".")
        return (part[0], "all") if part[0] != "api" else [part[0], part[0] + "." + part[1], "all"]
    labels, goff, members = fleet.group_names(names, key, first=7)
    assert labels == ["api", "api.get", "all", "db", "cache", "api.post"]
    got = {lb: members[int(a):int(b)].tolist() for lb, a, b in zip(labels, goff[:-1], goff[1:])}
    assert got == {"api": [7, 9, 11], "api.get": [7, 9], "all": [7, 8, 9, 10, 11, 12], "db": [8, 12], "cache": [10], "api.post": [11]}
    labels, goff, members = fleet.group_names(names, lambda n: None)
    assert labels == [] and goff.tolist() == [0] and members.size == 0
    labels, goff, members = fleet.group_names(["x"], lambda n: ("t", "t"), first=0xfffffffe)
    assert labels == ["t"] and members.tolist() == [0xfffffffe] * 2           # a label given twice counts twice
    with pytest.raises(ValueError):
        fleet.group_names(["x"], lambda n: n, first=0xffffffff)
    # the CSR is what group takes: blob A's rows by label
    labels, goff, members = fleet.group_names(["s.a", "t.a", "s.b", "drop", "t.b"], lambda n: None if n == "drop" else (n[0], "*"), first=10)
    first, rows, _, _ = rows_of(keptfile.group([BA], goff, members))
    assert labels == ["s", "*", "t"] and rows == [added(A[0], A[2]), added(A[0], A[1], A[2], A[4]), added(A[1], A[4])]
