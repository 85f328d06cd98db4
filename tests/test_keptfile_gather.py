"""loghisto_amd.keptfile.gather -- lh_kept_gather stated on blobs, the reference the device is held to -- against hand-written
dict-of-rows models; the names sidecar (pack_names / unpack_names); loghisto_amd.fleet.union_names.  No GPU, no library."""
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


A = [{0: 1, 100: 3}, {}, {NK - 1: 7, 5: 2}, {100: 1 << 63}]                    # rows 0 .. 3
B = [{100: 4, 200: 5}, {100: 1 << 63, 7: 9}, {NK - 1: 1}]                      # rows 10 .. 12
BA, BB = blob_of(A), blob_of(B, first=10)


def total(r):
    return sum(r.values()) & M64


def test_a_permutation_a_duplication_and_a_row_of_nothing():
    first, rows, rc, samples = rows_of(keptfile.gather([BA], [3, 2, 1, 0]))
    assert (first, rows) == (0, A[::-1]) and rc == [total(r) for r in A[::-1]] and samples == sum(rc) & M64
    # every row twice, then a selection, into rows that start at 5; a 2-D map of one line is the same thing
    first, rows, rc, _ = rows_of(keptfile.gather([BA], [[0, 0, 1, 1, 2, 2, 3, 3]], first_out=5))
    assert first == 5 and rows == [A[0], A[0], A[1], A[1], A[2], A[2], A[3], A[3]] and rc == [total(r) for r in rows]
    first, rows, rc, _ = rows_of(keptfile.gather([BB], np.array([12, 10], dtype=np.uint32)))
    assert (first, rows, rc) == (0, [B[2], B[0]], [1, 9])
    # an output row no blob feeds, and a map of nothing at all: a sound blob without a cell
    first, rows, rc, samples = rows_of(keptfile.gather([BA, BB], [[0, NO, 2], [10, NO, NO]]))
    assert rows == [{0: 1, 100: 7, 200: 5}, {}, A[2]] and rc == [13, 0, 9] and samples == 22
    # one blob is done in whole arrays, several cell by cell: the same bytes
    for b, m in ((BA, [3, NO, 0, 0, 2, 1]), (BB, [12, 12, NO, 10]), (BA, [NO, NO])):
        assert keptfile.gather([b], m, 9) == keptfile.gather([b, b], [m, [NO] * len(m)], 9) == keptfile.gather([b], m, 9, checked=False)
    blob = keptfile.gather([BA, BB], [[NO, NO], [NO, NO]])
    assert rows_of(blob) == (0, [{}, {}], [0, 0], 0) and keptfile.unpack(blob)["cells"] == 0
    assert len(blob) == keptfile.HEADER + keptfile.block_bytes(2, 0)


def test_two_blobs_with_different_maps_and_a_blob_listed_twice():
    got = keptfile.gather([BA, BB, BA], [[2, 0, NO, 3], [12, 11, 10, NO], [0, 0, 3, NO]])
    first, rows, rc, samples = rows_of(got)
    want = [{NK - 1: 8, 5: 2, 0: 1, 100: 3},                                  # A2 + B12 + A0
            {0: 2, 100: (6 + (1 << 63)) & M64, 7: 9},                         # A0 + B11 + A0
            {100: (4 + (1 << 63)) & M64, 200: 5},                             # B10 + A3
            {100: 1 << 63}]                                                   # A3
    assert rows == want and rc == [total(r) for r in want] and samples == sum(rc) & M64
    # the gather of a list is the combine (the merge) of the one-blob gathers
    singles = [keptfile.gather([b], m) for b, m in zip((BA, BB, BA), ([2, 0, NO, 3], [12, 11, 10, NO], [0, 0, 3, NO]))]
    assert keptfile.combine(singles) == got


def test_a_sum_that_wraps_to_zero_is_not_listed():
    got = keptfile.gather([BA, BB], [[3, 3], [11, NO]])
    first, rows, rc, samples = rows_of(got)
    assert rows == [{7: 9}, {100: 1 << 63}]                                   # 2^63 + 2^63 wraps to 0: no cell of bin 100 in row 0
    assert rc == [9, 1 << 63] and samples == (9 + (1 << 63)) & M64
    # the same blob twice with the same map: the whole row goes, its row_count wraps with it
    first, rows, rc, samples = rows_of(keptfile.gather([BA, BA], [[3, 0], [3, 0]]))
    assert rows == [{}, {0: 2, 100: 6}] and rc == [0, 8] and samples == 8


def test_the_last_rows_there_are():
    n = 3
    got = keptfile.gather([BB], [11, NO, 10], first_out=(1 << 32) - n)
    first, rows, rc, _ = rows_of(got)
    assert first == (1 << 32) - n and rows == [B[1], {}, B[0]]
    with pytest.raises(ValueError):
        keptfile.gather([BB], [11, NO, 10], first_out=(1 << 32) - n + 1)


def test_identity_maps_are_the_combine():
    C_ = [{100: 2}, {3: 3}, {}, {100: 1 << 63, 65535: 1}]
    BC = blob_of(C_)
    ident = np.arange(4, dtype=np.uint32)
    for blobs in ([BA], [BA, BC], [BC, BA, BA], [BA, BC, BC]):
        assert keptfile.gather(blobs, np.tile(ident, (len(blobs), 1))) == keptfile.combine(blobs)
    # a sub-block: rows 1 .. 2 of both, written as rows 1 .. 2
    assert keptfile.gather([BA, BC], [[1, 2], [1, 2]], first_out=1) == keptfile.combine([BA, BC], first=1, nrows=2)


def test_what_gather_refuses():
    for bad_map in ([[0, 1]], [[0], [10], [0]], [[], []], [4, 0], [[0, 1], [9, 10]], [[0, 1], [10, 13]]):
        with pytest.raises(ValueError):
            keptfile.gather([BA, BB], bad_map)
    with pytest.raises(ValueError):
        keptfile.gather([], [[0]])
    with pytest.raises(ValueError):
        keptfile.gather([BA[:-1]], [0])


def test_names_round_trip():
    for names, first in (([], 0), ([""], 0), (["a", "", "b"], 7), (["rpc.latency", "größe", "延迟/毫秒", "\U0001f600 x", "a" * 1000], 3),
                         (["x"], 0xffffffff)):
        blob = keptfile.pack_names(names, first)
        assert keptfile.unpack_names(blob) == names
        assert keptfile.unpack_names(blob, with_first=True) == (names, first)
        assert blob[:8] == keptfile.NAMES_MAGIC and len(blob) == 24 + sum(4 + len(s.encode()) for s in names)
    blob = keptfile.pack_names(["alpha", "beta"], 1)
    for bad in (b"", blob[:23], b"LHKEPT\x1a\n" + blob[8:], b"lhnames\n" + blob[8:], blob[:-1], blob[:24], blob[:30], blob + b"\0",
                blob[:8] + (2).to_bytes(4, "little") + blob[12:], blob[:20] + (1).to_bytes(4, "little") + blob[24:],
                blob[:16] + (3).to_bytes(4, "little") + blob[20:], blob[:28] + b"\xff\xfe" + blob[30:]):
        with pytest.raises(ValueError):
            keptfile.unpack_names(bad)
    with pytest.raises(ValueError):
        keptfile.pack_names(["a", "b"], 0xffffffff)


def test_union_names():
    a, b, c = ["x", "y", "z"], ["z", "w", "x"], ["q"]
    union, src = fleet.union_names([a, b, c])
    assert union == ["x", "y", "z", "w", "q"]                                 # first appearance, list by list
    assert src.dtype == np.uint32 and src.shape == (3, 5)
    assert src.tolist() == [[0, 1, 2, NO, NO], [2, NO, 0, 1, NO], [NO, NO, NO, NO, 0]]
    union2, src2 = fleet.union_names([a, b, c], firsts=[0, 100, 0xfffffffe])   # absolute rows
    assert union2 == union and src2.tolist() == [[0, 1, 2, NO, NO], [102, NO, 100, 101, NO], [NO, NO, NO, NO, 0xfffffffe]]
    assert fleet.union_names([[], ["k"]])[1].tolist() == [[NO], [0]]
    u, s = fleet.union_names([])
    assert u == [] and s.shape == (0, 0)
    for bad in (lambda: fleet.union_names([["x", "x"]]), lambda: fleet.union_names([a], firsts=[0, 1]),
                lambda: fleet.union_names([c], firsts=[0xffffffff])):
        with pytest.raises(ValueError):
            bad()
    # the map is what gather takes: two blobs whose rows carry the names in different orders, summed per NAME
    first, rows, _, _ = rows_of(keptfile.gather([BA, BB], fleet.union_names([["p", "q", "r", "s"], ["s", "t", "p"]], firsts=[0, 10])[1]))
    assert rows == [{0: 1, 100: 3, NK - 1: 1}, {}, A[2], {100: ((1 << 63) + 4) & M64, 200: 5}, B[1]]
