"""keptfile.combine (the pure-NumPy statement of lh_kept_slide, the reference the device is held to) against a model in Python
integers, on small hand-made blobs: per row and bin the add side's sum mod 2^64 minus the sub side's, zero differences
dropped, an underflow reported for the lowest row and in it the lowest bin.  No GPU, no library."""
import numpy as np
import pytest

from loghisto_amd import keptfile as kf

M64 = (1 << 64) - 1
NK = kf.NKEYS


def key_of(b):
    return (b ^ 0x8000) - (NK if (b ^ 0x8000) >= 0x8000 else 0)


def blob(rows, first=0):
    """rows: per row {bin: count}"""
    off, keys, counts = [0], [], []
    for r in rows:
        for b in sorted(r):
            keys.append(key_of(b))
            counts.append(r[b])
        off.append(len(keys))
    out = kf.pack(off, np.array(keys, dtype=np.int16), np.array(counts, dtype=np.uint64), first=first)
    assert kf.check(out) is None
    return out


def rows_of(b):
    u = kf.unpack(b)
    bins = (u["keys"].view("<u2") ^ np.uint16(0x8000)).tolist()
    cnt = u["counts"].tolist()
    return [{bins[j]: cnt[j] for j in range(int(a), int(e))} for a, e in zip(u["offsets"][:-1], u["offsets"][1:])]


def model(add, sub, first, nrows):
    """add, sub: lists of (first, rows) -> the rows of the result, or ("under", row, bin)"""
    def side(lst, m):
        s = {}
        for f, rows in lst:
            for b, c in rows[first + m - f].items():
                s[b] = (s.get(b, 0) + c) & M64
        return s
    out = []
    for m in range(nrows):
        A, S = side(add, m), side(sub, m)
        under = sorted(b for b, c in S.items() if c > A.get(b, 0))
        if under:
            return ("under", first + m, under[0])
        out.append({b: A[b] - S.get(b, 0) for b in sorted(A) if A[b] - S.get(b, 0)})
    return out


def run(add, sub=(), first=None, nrows=None):
    """combine() of the blobs of add / sub -- lists of (first, rows) -- checked against the model; -> the result's rows"""
    f = add[0][0] if first is None else first
    n = add[0][0] + len(add[0][1]) - f if nrows is None else nrows
    want = model(add, list(sub), f, n)
    got = kf.combine([blob(r, fi) for fi, r in add], [blob(r, fi) for fi, r in sub], first, nrows)
    assert kf.check(got) is None                                     # row_count and samples are consistent with the cells
    u = kf.unpack(got)
    assert (u["first"], u["nrows"]) == (f, n) and rows_of(got) == want
    assert len(got) == kf.HEADER + kf.block_bytes(n, sum(len(r) for r in want))
    assert list(u["keys"]) == [key_of(b) for r in want for b in sorted(r)]        # ascending by bin within a row
    return want


A0 = [{100: 3, 200: 5}, {}, {7: 1}, {0: 2, NK - 1: 9}]
A1 = [{150: 2, 200: 1}, {40000: 4}, {}, {0: 1}]
A2 = [{100: 1}, {}, {7: 1, 8: 1}, {NK - 1: 1}]


def test_union_of_bins_and_plain_sum_without_sub():
    got = run([(0, A0), (0, A1), (0, A2)])
    assert got[0] == {100: 4, 150: 2, 200: 6} and got[1] == {40000: 4} and got[3] == {0: 3, NK - 1: 10}
    assert kf.combine([blob(A0), blob(A1)]) == kf.combine([blob(A0), blob(A1)], ())
    one = blob(A0)
    assert kf.combine([one]) == one                                  # a copy, byte for byte
    assert run([(0, A0), (0, A0)])[0] == {100: 6, 200: 10}           # listed twice: counts twice


def test_cancellation_drops_the_cell_and_the_row():
    got = run([(0, A0), (0, A1), (0, A2)], [(0, A1)])
    assert got == model([(0, A0), (0, A2)], [], 0, 4)
    got = run([(0, A0), (0, A2)], [(0, A2)])
    assert got == [{b: c for b, c in r.items()} for r in A0]
    got = run([(0, A0)], [(0, A0)])
    assert got == [{}, {}, {}, {}]
    res = kf.combine([blob(A0)], [blob(A0)])
    u = kf.unpack(res)
    assert u["cells"] == 0 and u["samples"] == 0 and u["bytes"] == 8 * (2 * 4 + 1) and list(u["row_count"]) == [0] * 4
    got = run([(0, A0), (0, A1)], [(0, [{200: 6}, {40000: 4}, {7: 1}, {0: 3}])])     # whole rows 1 and 2 go, cells of 0 and 3
    assert got == [{100: 3, 150: 2}, {}, {}, {NK - 1: 9}]
    assert run([(0, A0), (0, A0)], [(0, A0)]) == A0                  # on both sides: it cancels once


def test_sub_block():
    wide = [{b: 1 + m} for m, b in enumerate(range(10, 18))]          # rows 0 .. 7
    part = [{13: 1, 99: 5}, {14: 5}, {15: 2}]                         # rows 3 .. 5
    assert run([(0, wide), (3, part)], first=3, nrows=3) == [{13: 5, 99: 5}, {14: 10}, {15: 8}]
    assert run([(3, part), (0, wide)], [(3, part)], first=4, nrows=2) == [{14: 5}, {15: 6}]
    assert run([(3, part)]) == part                                   # first=None, nrows=None: the first add blob's block
    assert kf.unpack(kf.combine([blob(part, 3)]))["first"] == 3
    for first, nrows in ((2, 2), (3, 4), (0, 8), (5, 0)):
        with pytest.raises(ValueError):
            kf.combine([blob(wide), blob(part, 3)], (), first, nrows)
    with pytest.raises(ValueError):
        kf.combine([blob(wide)], [blob(part, 3)])                     # the default block is the first add blob's: rows 0 .. 7
    with pytest.raises(ValueError):
        kf.combine([])
    with pytest.raises(ValueError):
        kf.combine([blob(wide)[:-1]])


def test_underflow_names_the_lowest_row_then_the_lowest_bin():
    add = [{100: 3, 200: 5}, {50: 1}, {7: 2, 9: 2}]
    sub = [{100: 3}, {50: 2}, {9: 3, 7: 3}]                           # rows 1 and 2 violate, row 2 in two bins
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob(add)], [blob(sub)])
    assert (e.value.row, e.value.key) == (1, key_of(50)) and model([(0, add)], [(0, sub)], 0, 3) == ("under", 1, 50)
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob(add)], [blob(sub)], first=2, nrows=1)
    assert (e.value.row, e.value.key) == (2, key_of(7))                # the lowest BIN, not the first listed
    assert kf.unpack(kf.combine([blob(add)], [blob(sub)], first=0, nrows=1))["cells"] == 1       # the rows asked for alone
    # a row that is an ABSOLUTE metric id
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob(add, 1000)], [blob(sub, 1000)])
    assert e.value.row == 1001
    # a bin the add side does not hold counts as 0 there
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob([{100: 3}])], [blob([{100: 3, 101: 1}])])
    assert (e.value.row, e.value.key) == (0, key_of(101))
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob([{}, {5: 1}])], [blob([{0: 1}, {5: 1}])])     # an add row without a cell
    assert (e.value.row, e.value.key) == (0, key_of(0))
    # bins below 32 768 have NEGATIVE keys: the order is by bin
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob([{0x8001: 1, 0x7fff: 1}])], [blob([{0x8001: 2, 0x7fff: 2}])])
    assert e.value.key == key_of(0x7fff) == -1


def test_bins_0_and_65535_and_counts_at_the_top_of_64_bits():
    top = [{0: M64, NK - 1: M64}]
    assert run([(0, top)], [(0, top)]) == [{}]
    assert run([(0, top)], [(0, [{0: 1}])]) == [{0: M64 - 1, NK - 1: M64}]
    assert run([(0, top)], [(0, [{NK - 1: M64}])]) == [{0: M64}]
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob([{0: 5, NK - 1: M64 - 1}])], [blob(top)])
    assert (e.value.row, e.value.key) == (0, key_of(0)) and key_of(0) == -32768
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob([{0: M64, NK - 1: M64 - 1}])], [blob(top)])
    assert (e.value.row, e.value.key) == (0, key_of(NK - 1)) and key_of(NK - 1) == 32767
    # sums are taken mod 2^64 on each side: 2^63 + 2^63 wraps to 0 and the cell is gone; minus anything it is an underflow
    half = [{300: 1 << 63, 301: 7}]
    assert run([(0, half), (0, half)]) == [{301: 14}]
    with pytest.raises(kf.KeptUnderflow) as e:
        kf.combine([blob(half), blob(half)], [blob([{300: 1}])])       # the wrap corner is refused like any other
    assert (e.value.row, e.value.key) == (0, key_of(300))
    assert run([(0, half), (0, half)], [(0, half), (0, half)]) == [{}]            # both sides wrap alike
    # row_count wraps with the cells: (2^64 - 1) + 2 = 1 (mod 2^64), minus 1
    res = kf.combine([blob([{5: M64}]), blob([{6: 2}])], [blob([{6: 1}])])
    u = kf.unpack(res)
    assert kf.check(res) is None and list(u["row_count"]) == [0] and u["samples"] == 0 and rows_of(res) == [{5: M64, 6: 1}]
