"""A merged snapshot followed past the merge: the store it leaves, every reader on it, its release and the reuse of its buffer
and of the engine's plan arrays (run as a subprocess by tests/test_gpu_after_merge.py; the scenarios themselves are checked
without a GPU by tests/test_after_merge_rows.py).

tests/_merge_edges_driver.py makes one engine per rank, merges ONE interval, reads the owned rows through buckets_all and
extract and closes.  Here the engines live on, in tests/_merge_edges_driver.py's harness (N engines on the one GPU as N ranks,
a thread each, tests/cpp/rccl_stub.cc as RCCL, LH_TEST_CELL_BITS=32 for engines of 32-bit cells):

  life     3 ranks, ONE engine each (72 names, two epoch buffers) over five merged intervals and three unmerged flips:
             I1  buffer 0  uint32 wire, all 72 rows, the three classes (A_COUNTS[3]'s boundary counts among them), every merged
                           window made by different ranks, widths either side of the 4-cell word at every lo % 4; a row only
                           rank 2 holds, one rank 1 lacks, two nobody holds, windows at bin 0 and at bin 65 535
             I2  buffer 1  nrows = 40 < 72: every row below 40 in ANOTHER class than in I1, in a narrower window somewhere
                           else; rows 40 .. 71 hold the rank's own cells and must keep them and their own spans
             I3  buffer 0  nobody submits: the merge returns where the plan's total is 0; the whole store is zero
             I4  buffer 1  uint64 wire (rank 0's sample count unknown: lh_snapshot_mark_dirty on a cell it holds); rank 1 is
                           empty and its snapshot is judged clean BEFORE the merge; one merged cell is 2^32 + 5
             --  buffer 0  flipped, judged clean, released (so that I5 comes back to buffer 1)
             I5  buffer 1  a small merge on the uint32 wire: engines of 32-bit cells are back on their narrow store
             --  buffers 0 and 1 once more, judged clean: what the releases after I4's spare flip and after I5 left
           The cell of 2^32 + 5: rank 0 ingests 5 pairs of one (row, value), rank 2 IMPORTS 2^32 into the same cell
           (lh_snapshot_add_buckets).  The import is the cheapest route that lands an exact cell: 2^32 pairs through an ingest
           route are seconds of device time per rank, the import is one entry.  It also widens rank 2's narrow snapshot before
           the merge, while ranks 0 and 1 are widened BY the merge.
  rs_wave  2 ranks, 4 200 names: 4 197 rows of one 6-cell window at 8 bits and three rows of 1 027 cells.  The reduce-scatter's
           owner blocks are [0, 2 100) and [2 100, 4 200): both at or above the 2 048 rows from which k_unpack_rows runs a
           wave per row, so the wave shape runs with first_row != 0 and kblock != 0.  (Two of the wide rows lie in block 1 --
           one inside it and the very last row -- at 8 bits, 257 words each; block 0's one travels at 16 bits, 514 words:
           that balance is what puts the cut at 2 100.  With all three at 8 bits the cut is 2 164 | 2 036.)  The same engines
           then merge the same rows by all-reduce, the shape's control.

After every merge, on every rank:
  (a) tests/_span_contract.check_store over all M rows and assert_contract: no padding cell, no cell outside its span, no
      malformed range -- owned rows, rows of other owners, rows at and beyond nrows alike;
  (b) the ranges are (min lo, max hi) over the ranks below nrows and the rank's own from nrows on;
  (c) every owned row and every row from nrows on, all 65 536 bins read from the store as it is, equals the model;
  (d) rows of OTHER owners under reduce-scatter: include/loghisto_gpu.h says which rows hold merged data ("first_owned /
      last_owned receive the [first, last) rows holding merged data on this rank") and nothing about the others.  They are
      UNSPECIFIED: (a) alone is asserted of them -- and that they hold no other row's words: every nonzero cell lies where the
      merged row has one and does not exceed it (true of the rank's own cells, of the merged cells and of anything between);
  (e) every reader family over the owned rows against a model of the merged rows: extract, spread, count_le, top (by count,
      k = 5), keep + Kept.across on the one handle, serialize;
  (f) device_cells()[2] == 4 exactly when the engine is narrow and the wire was uint32;
  (g) merge_info's packed_cells, packed_words, rows_8bit, rows_16bit, cell_bytes, occupied_rows (and padded_words, widest_row)
      equal the model's: a plan left over from the merge before shows here.
Nothing expected comes from the library or from loghisto_amd.merge: a rank's cells are oracle.histogram_pairs on its own pairs
(plus the one imported entry), sums, ranges, classes, words and owner blocks are numpy on those.  Integers compare with ==; the
float sums under tests/test_gpu_serialize.py's bound 1e-12 x sum |value| x count (spread and top: tests/test_gpu_spread.py's
REL, the same bound in exact arithmetic).

usage: python tests/_after_merge_driver.py CASE PLAN        (LH_TEST_CELL_BITS=32: engines of 32-bit cells)
       CASE life | rs_wave; PLAN allreduce | reduce_scatter (rs_wave: reduce_scatter, its all-reduce control included)
"""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import threading
import time
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _merge_edges_driver as d  # noqa: E402  (Scenario, the bins that round-trip, A_COUNTS, B_BIG)

NKEYS, EMPTY = d.NKEYS, d.EMPTY
U64 = np.uint64
U32MAX = 0xffffffff
CASES = ("life", "rs_wave")
P = [0.0, 0.5, 0.99, 1.0]
PCT = {"%s_p0": 0.0, "%s_50": 0.5, "%s_99": 0.99, "%s_max": 1.0}
WIRE = dict(prefix="lh.", sep=" ", suffix=" 1411104988\n", underscore_to_dot=False)
CHUNK = 256                               # rows per pass of the oracle: one dense temporary of 128 MiB

LIFE_RANKS, LIFE_M, I2_ROWS = 3, 72, 40
W1 = (2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027)      # I1's widths (rows below 40: I2 halves them)
SINGLE, LACKS1, NOBODY, TOP, BOTTOM, ONE = 10, 20, (7, 30), 44, 45, 46
HOT_ROW, HOT_BIN, HOT_OWN, HOT_IMPORT = 33, 35555, 5, 1 << 32
LIFE_SEQUENCE = ("I1", "I2", "I3", "I4", "spare", "I5", "end0", "end1")

WAVE_RANKS, WAVE_M, WAVE_MIN_BLOCK = 2, 4200, 2048
WAVE_SMALL, WAVE_WIDE = 6, 1027
WAVE_WIDE_ROWS = {1000: (16, 1), 3000: (8, 2), WAVE_M - 1: (8, 3)}                 # row -> (class, lo % 4)


class Interval(d.Scenario):
    """tests/_merge_edges_driver.Scenario plus: nrows (the merge's), imports[r] = [(row, bin, count)] added to rank r's snapshot
    through lh_snapshot_add_buckets, merged (False: flipped, judged clean and released without a merge)."""

    def __init__(self, name, nranks, M, nrows=None, dirty=False, merged=True):
        super().__init__(name, nranks, M, dirty=dirty)
        self.nrows = M if nrows is None else nrows
        self.imports = [[] for _ in range(nranks)]
        self.merged = merged

    def holds_nothing(self, rank):
        return not self.cells[rank] and not self.imports[rank]


# ---- the rows ----------------------------------------------------------------------------------------------------------
def _window(sc, D, row, lo, w, cls, lo_rank, hi_rank, rest):
    """One merged window [lo, lo + w): lo on one rank, hi on another, a few interior cells on `rest`; the largest per-rank
    cell (B_BIG[cls]) stands at the window's last cell in even rows and at its first in odd ones."""
    hi = lo + w - 1
    big_at_hi = row % 2 == 0
    sc.put(lo_rank, row, D[lo], 1 if big_at_hi else d.B_BIG[cls])
    sc.put(hi_rank, row, D[hi], d.B_BIG[cls] if big_at_hi else 1)
    for pos in sorted({1, 2, 3, 4, 5, w // 2, w - 6, w - 5, w - 4, w - 3, w - 2}):
        if 0 < pos < w - 1:
            c = 1 + pos % 5                                # distinct small counts: a field in the wrong place shows
            for k, r in enumerate(rest):
                sc.put(r, row, D[lo + pos], (c + len(rest) - 1 - k) // len(rest))
    sc.bins[(row, "lo")], sc.bins[(row, "hi")], sc.bins[(row, "cls")] = lo, hi, cls


def _cls1(row):
    return (8, 16, 8, 16, 32)[row % 5]


def _cls2(cls_in_i1, row):
    """another class than I1's, row by row (a row nobody held in I1 has none: 16)"""
    return {None: 16, 8: 16, 16: 32 if row % 4 == 1 else 8, 32: 8}[cls_in_i1]


def life_i1(D):
    nr, M = LIFE_RANKS, LIFE_M
    sc = Interval("I1", nr, M)
    idx = 0
    for row in range(M):
        if row in NOBODY:
            continue
        if row < 4:                                        # nranks x c = 255 | 258 | 65 535 | 65 538, the hot cell in field `row`
            c = d.A_COUNTS[nr][row]
            lo = 33000 + 60 * row + (row + 1) % 4
            hot = lo + 4 + row
            sc.put(0, row, D[lo], 1)
            for r in range(nr):
                sc.put(r, row, D[hot], c)
            others = [lo + 4 + q for q in range(4) if q != row]
            sc.put(row % nr, row, D[others[0]], 1)
            sc.put(nr - 1, row, D[others[2]], 2)
            sc.put(1, row, D[lo + 9], 1)
            sc.bins[(row, "lo")], sc.bins[(row, "hi")], sc.bins[(row, "cls")] = lo, lo + 9, d.A_CLASS[nr][row]
            sc.bins[(row, "hot")] = hot
        elif row == SINGLE:                                # only rank 2 holds it
            _window(sc, D, row, 33000 + 60 * row + 1, 9, _cls1(row), 2, 2, [2])
        elif row == LACKS1:                                # rank 1's span goes from (65 536, 0) to a real window
            _window(sc, D, row, 33000 + 60 * row + 3, 65, _cls1(row), 0, 2, [0])
        elif row == TOP:                                   # ends at bin 65 535: the padding cells come next
            _window(sc, D, row, NKEYS - 6, 6, _cls1(row), 0, 1, [2])
        elif row == BOTTOM:                                # starts at bin 0
            _window(sc, D, row, 0, 7, _cls1(row), 1, 2, [0])
        else:
            w = 1 if row == ONE else W1[idx % len(W1)]
            lo_rank, hi_rank = idx % nr, (idx + 1) % nr
            _window(sc, D, row, 33000 + 60 * row + idx % 4, w, _cls1(row), lo_rank, hi_rank,
                    [r for r in range(nr) if r not in (lo_rank, hi_rank)])
            idx += 1
    return sc


def life_i2(D, i1):
    nr, M = LIFE_RANKS, LIFE_M
    sc = Interval("I2", nr, M, nrows=I2_ROWS)
    for row in range(I2_ROWS):                             # narrower than I1's window, elsewhere, in another class
        w1 = i1.bins[(row, "hi")] - i1.bins[(row, "lo")] + 1 if (row, "lo") in i1.bins else 0
        w = max(1, w1 // 2) if w1 else 3
        _window(sc, D, row, 38000 + 12 * row + (row + 2) % 4, w, _cls2(i1.bins.get((row, "cls")), row),
                (row + 1) % nr, (row + 2) % nr, [row % nr])
    for row in range(I2_ROWS, M):                          # beyond nrows: every rank its own window (or none)
        for r in range(nr):
            if (row + r) % 11 == 0:
                continue
            lo, w = 34000 + 40 * row + 5 * r + row % 4, 2 + (row + r) % 6
            sc.put(r, row, D[lo], 1 + r)
            sc.put(r, row, D[lo + w // 2], 3 + row % 7)
            sc.put(r, row, D[lo + w - 1], 2)
            sc.bins[(row, "own", r)] = (lo, lo + w - 1)
    return sc


def life_i4(D):
    nr, M = LIFE_RANKS, LIFE_M
    sc = Interval("I4", nr, M, dirty=True)                 # rank 1 holds nothing
    for k, row in enumerate(range(2, M, 5)):
        assert row != HOT_ROW
        w = W1[3 * k % len(W1)]
        lo = 34000 + 55 * row + k % 4
        sc.put(0, row, D[lo], 2)
        sc.put(2, row, D[lo + w - 1], 3)
        for j, pos in enumerate(sorted({1, w // 2, w - 2})):
            if 0 < pos < w - 1:
                sc.put((0, 2)[j % 2], row, D[lo + pos], 1 + j)
        sc.bins[(row, "lo")], sc.bins[(row, "hi")] = lo, lo + w - 1
    sc.put(0, HOT_ROW, D[HOT_BIN], HOT_OWN)                # 5 here, 2^32 imported on rank 2: one merged cell of 2^32 + 5
    sc.put(0, HOT_ROW, D[HOT_BIN - 3], 1)
    sc.put(2, HOT_ROW, D[HOT_BIN + 6], 2)
    sc.imports[2].append((HOT_ROW, HOT_BIN, HOT_IMPORT))
    sc.bins[(HOT_ROW, "lo")], sc.bins[(HOT_ROW, "hi")] = HOT_BIN - 3, HOT_BIN + 6
    return sc


def life_i5(D):
    nr, M = LIFE_RANKS, LIFE_M
    sc = Interval("I5", nr, M)
    for k, row in enumerate(range(1, M, 4)):
        w = (1, 2, 3, 5, 8, 9)[k % 6]
        cls = 32 if k in (2, 11) else (8, 16)[k % 2]
        lo_rank, hi_rank = k % nr, (k + 1) % nr
        _window(sc, D, row, 36000 + 30 * row + k % 4, w, cls, lo_rank, hi_rank, [r for r in range(nr) if r not in (lo_rank, hi_rank)])
    return sc


_BUILT = {}


def life_intervals():
    """name -> Interval, in LIFE_SEQUENCE's order"""
    if "life" not in _BUILT:
        D = d._values()
        i1 = life_i1(D)
        empty = lambda name, merged: Interval(name, LIFE_RANKS, LIFE_M, merged=merged)  # noqa: E731
        _BUILT["life"] = {"I1": i1, "I2": life_i2(D, i1), "I3": empty("I3", True), "I4": life_i4(D), "spare": empty("spare", False),
                          "I5": life_i5(D), "end0": empty("end0", False), "end1": empty("end1", False)}
        assert tuple(_BUILT["life"]) == LIFE_SEQUENCE
    return _BUILT["life"]


def wave_interval():
    if "wave" not in _BUILT:
        D = d._values()
        sc = Interval("rs_wave", WAVE_RANKS, WAVE_M)
        for row in range(WAVE_M):
            a, b = row % 2, 1 - row % 2                    # lo on one rank, hi on the other
            if row in WAVE_WIDE_ROWS:
                cls, lo4 = WAVE_WIDE_ROWS[row]
                lo, w = 36000 + 4 * (row % 100) + lo4, WAVE_WIDE
                sc.put(a, row, D[lo], {8: 1, 16: 200}[cls])  # (2 ranks x 200 = 400: past 8 bits)
                sc.put(b, row, D[lo + w - 1], 2)
                for j, pos in enumerate((1, 2, 3, 4, 5, 511, 512, 513, 1021, 1022, 1023, 1024, 1025)):
                    sc.put((a, b)[j % 2], row, D[lo + pos], 1 + j % 4)
            else:
                lo, w, cls = 33000 + 7 * (row % 500), WAVE_SMALL, 8
                sc.put(a, row, D[lo], 1)
                sc.put(a, row, D[lo + 2 + row % 2], 1 + row % 2)
                sc.put(b, row, D[lo + 1 + 3 * (row % 2)], 1)
                sc.put(b, row, D[lo + w - 1], 1 + (row % 3 == 0))
            sc.bins[(row, "lo")], sc.bins[(row, "hi")], sc.bins[(row, "cls")] = lo, lo + w - 1, cls
        _BUILT["wave"] = sc
    return _BUILT["wave"]


# ---- what the engines must hold: the oracle's cells and numpy ---------------------------------------------------------------
class Cells:
    """Sparse cells (row, bin) -> count, sorted by row then bin; entries of one cell add up."""

    def __init__(self, rows, bins, counts):
        key = (np.asarray(rows, dtype=np.int64) << 16) | np.asarray(bins, dtype=np.int64)
        self.key, inv = np.unique(key, return_inverse=True)
        self.count = np.zeros(self.key.size, dtype=U64)
        np.add.at(self.count, inv.ravel(), np.asarray(counts, dtype=U64))
        assert self.count.all()
        self.rows, self.bins = self.key >> 16, self.key & 0xffff

    def span(self, first, last):
        a, b = np.searchsorted(self.key, [first << 16, last << 16])
        return slice(int(a), int(b))

    def below(self, nrows):
        s = self.span(0, nrows)
        return self.rows[s], self.bins[s], self.count[s]

    def dense(self, first, last):
        """uint64[last - first, 65 536]"""
        out = np.zeros((last - first, NKEYS), dtype=U64)
        s = self.span(first, last)
        out[self.rows[s] - first, self.bins[s]] = self.count[s]
        return out

    def ranges(self, M):
        out = np.tile(np.array(EMPTY, dtype=np.int64), (M, 1))
        np.minimum.at(out[:, 0], self.rows, self.bins)
        np.maximum.at(out[:, 1], self.rows, self.bins)
        return out


def cells_of_pairs(ids, v, M):
    """oracle.histogram_pairs on the pairs, CHUNK rows at a time, as (rows, bins, counts) of the nonzero cells"""
    import oracle
    ids = np.asarray(ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    ids, v = ids[order], np.asarray(v, dtype=np.float64)[order]
    cut = np.searchsorted(ids, np.arange(0, M + CHUNK, CHUNK))
    buf = np.zeros((CHUNK, NKEYS), dtype=U64)
    out = [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=U64))]
    for c in range(cut.size - 1):
        a, b = int(cut[c]), int(cut[c + 1])
        if a == b:
            continue
        oracle.histogram_pairs((ids[a:b] - c * CHUNK).astype(np.uint32), v[a:b], CHUNK, buf)
        cols = np.flatnonzero(np.bitwise_or.reduce(buf, axis=0))     # (the occupied bins first: a scan of all cells is 0.1 s)
        rr, cc = np.nonzero(buf[:, cols])
        bb = cols[cc]
        out.append((rr + c * CHUNK, bb, buf[rr, bb]))
        buf[rr, bb] = 0
    assert ids.size == 0 or int(ids[-1]) < M
    return tuple(np.concatenate(x) for x in zip(*out))


class Model:
    pass


_MODELS = {}


def model(iv, plan):
    """What interval `iv` must leave on every rank (plan: the owner blocks and padded_words only)."""
    if (iv.name, plan) in _MODELS:
        return _MODELS[(iv.name, plan)]
    nranks, M, nrows = iv.nranks, iv.M, iv.nrows
    X = Model()
    base = _MODELS.get((iv.name, "cells"))
    if base is None:
        own = []
        for r in range(nranks):
            rows, bins, counts = cells_of_pairs(*iv.pairs(r), M)
            for row, b, c in iv.imports[r]:
                rows, bins, counts = np.append(rows, row), np.append(bins, b), np.append(counts, U64(c))
            own.append(Cells(rows, bins, counts))
        merged = Cells(*(np.concatenate(x) for x in zip(*[c.below(nrows) for c in own])))
        base = _MODELS[(iv.name, "cells")] = (own, merged)
    X.own, X.merged = base
    X.own_ranges = [c.ranges(M) for c in X.own]
    X.merged_ranges = X.merged.ranges(M)
    X.final_ranges = [np.concatenate([X.merged_ranges[:nrows], rg[nrows:]]) for rg in X.own_ranges]
    rowmax = np.zeros(nrows, dtype=np.int64)
    for c in X.own:                                        # the largest cell any rank holds in the row, clipped as the wire's word is
        rows, _, counts = c.below(nrows)
        np.maximum.at(rowmax, rows, np.minimum(counts, U64(U32MAX)).astype(np.int64))
    X.rowmax = rowmax
    lo, hi = X.merged_ranges[:nrows, 0], X.merged_ranges[:nrows, 1]
    X.width = np.where(lo <= hi, hi - lo + 1, 0)
    X.largest = max(iv.samples(r) for r in range(nranks))
    X.words32 = not iv.dirty and X.largest < U32MAX and nranks * X.largest < (1 << 32)
    bound = nranks * rowmax
    X.cls = np.where(bound <= 255, 8, np.where(bound <= 65535, 16, 32))
    X.words = (X.width * X.cls + 31) // 32 if X.words32 else X.width.copy()
    X.P = np.concatenate(([0], np.cumsum(X.words)))
    X.total = int(X.P[-1])
    nb = nranks if plan == "reduce_scatter" else 1
    # owner blocks: block k starts at the first row whose prefix reaches its share of the wire words
    X.brow = [0] + [int(np.searchsorted(X.P, X.total // nb * k + X.total % nb * k // nb, side="left")) for k in range(1, nb)] + [nrows]
    bmax = max(int(X.P[X.brow[k + 1]] - X.P[X.brow[k]]) for k in range(nb))
    X.owned = [(X.brow[r], X.brow[r + 1]) if plan == "reduce_scatter" else (0, nrows) for r in range(nranks)]
    occ = X.width > 0
    X.info = dict(packed_cells=int(X.width.sum()), packed_words=X.total, cell_bytes=4 if X.words32 else 8,
                  rows_8bit=int((occ & (X.cls == 8)).sum()) if X.words32 else 0,
                  rows_16bit=int((occ & (X.cls == 16)).sum()) if X.words32 else 0, occupied_rows=int(occ.sum()),
                  widest_row=int(X.width.max()), padded_words=nranks * bmax if plan == "reduce_scatter" else X.total)
    _MODELS[(iv.name, plan)] = X
    return X


def merged_store(X, nrows, stride=NKEYS + 8):
    """The model's merged rows as a host store [nrows, stride] with its ranges, for tests/_span_contract.check_planted."""
    store = np.zeros((nrows, stride), dtype=U64)
    store[:, :NKEYS] = X.merged.dense(0, nrows)
    return store, X.merged_ranges[:nrows].copy()


# ---- the scenarios are what they claim (numpy on the oracle's cells: no GPU, no library) ---------------------------------------
def self_check_life():
    ivs = life_intervals()
    X = {k: model(iv, "allreduce") for k, iv in ivs.items()}
    i1, i2, x1, x2 = ivs["I1"], ivs["I2"], X["I1"], X["I2"]
    assert i1.nrows == LIFE_M == 72 and i2.nrows == I2_ROWS == 40 and all(iv.nranks == 3 for iv in ivs.values())
    for iv, x in ((i1, x1), (i2, x2), (ivs["I5"], X["I5"])):     # every aimed window is the merged one, at the aimed class
        for row in range(iv.nrows):
            want = (iv.bins[(row, "lo")], iv.bins[(row, "hi")]) if (row, "lo") in iv.bins else EMPTY
            assert tuple(x.merged_ranges[row]) == want, (iv.name, row, x.merged_ranges[row], want)
            if (row, "cls") in iv.bins:
                assert int(x.cls[row]) == iv.bins[(row, "cls")], (iv.name, row, x.cls[row])
        assert x.words32 and x.info["cell_bytes"] == 4 and x.info["rows_8bit"] and x.info["rows_16bit"]
        assert x.info["occupied_rows"] > x.info["rows_8bit"] + x.info["rows_16bit"]          # ... and rows at 32 bits
    # I1: the boundary counts, the special rows, the geometry
    for row, c in enumerate(d.A_COUNTS[3]):
        hot = i1.bins[(row, "hot")]
        assert [int(o.dense(row, row + 1)[0, hot]) for o in x1.own] == [c] * 3 and int(x1.rowmax[row]) == c
        assert int(x1.merged.dense(row, row + 1)[0, hot]) == 3 * c and (hot - x1.merged_ranges[row, 0]) % 4 == row
    assert {3 * c for c in d.A_COUNTS[3]} == {255, 258, 65535, 65538}
    held = lambda x, row: [tuple(rg[row]) != EMPTY for rg in x.own_ranges]  # noqa: E731
    assert held(x1, SINGLE) == [False, False, True]
    assert held(x1, LACKS1) == [True, False, True] and x1.width[LACKS1] > 1
    assert all(held(x1, row) == [False] * 3 and x1.width[row] == 0 for row in NOBODY)
    assert x1.merged_ranges[TOP, 1] == NKEYS - 1 and x1.merged_ranges[BOTTOM, 0] == 0
    assert all(sum(held(x1, row)) >= 2 for row in (TOP, BOTTOM)) and x1.width[ONE] == 1
    seen = {}
    for row in range(LIFE_M):
        if x1.width[row] > 1 and row not in (SINGLE,):           # the merged window is one no rank has
            assert all(tuple(rg[row]) != tuple(x1.merged_ranges[row]) for rg in x1.own_ranges), row
        if x1.width[row]:
            seen.setdefault(int(x1.cls[row]), set()).add((int(x1.width[row]), int(x1.merged_ranges[row, 0]) % 4))
    for c in (8, 16, 32):
        assert {m for _, m in seen[c]} == {0, 1, 2, 3}, (c, seen[c])
    widths = {w for s in seen.values() for w, _ in s}
    assert widths >= set(W1) | {1, 6, 10} and {w % 4 for w in widths} == {0, 1, 2, 3}
    # I2: below nrows another class, a narrower window, elsewhere; from nrows on the ranks' own windows
    for row in range(I2_ROWS):
        assert int(x2.cls[row]) != int(x1.cls[row]), (row, x1.cls[row])
        assert 0 < x2.width[row] and (x2.width[row] < x1.width[row] or x1.width[row] == 0), (row, x1.width[row], x2.width[row])
        assert x2.merged_ranges[row, 0] > x1.merged_ranges[row, 1] or x1.width[row] == 0, row
    assert {(int(a), int(b)) for a, b in zip(x1.cls[:I2_ROWS], x2.cls[:I2_ROWS]) if a != b} >= {(32, 8), (8, 16), (16, 32), (16, 8)}
    assert {int(x2.merged_ranges[row, 0]) % 4 for row in range(I2_ROWS)} == {0, 1, 2, 3}
    assert x2.merged.rows.max() < I2_ROWS
    for r in range(3):
        rg = x2.own_ranges[r][I2_ROWS:]
        nothing = [(row + r) % 11 == 0 for row in range(I2_ROWS, LIFE_M)]
        assert [tuple(x) == EMPTY for x in rg] == nothing and any(nothing)
        assert np.array_equal(x2.final_ranges[r][I2_ROWS:], rg) and np.array_equal(x2.final_ranges[r][:I2_ROWS], x2.merged_ranges[:I2_ROWS])
    assert len({tuple(x2.own_ranges[r][50]) for r in range(3)}) == 3          # the ranks' windows differ
    # I3 and the unmerged flips: nobody submits
    for k in ("I3", "spare", "end0", "end1"):
        assert all(ivs[k].holds_nothing(r) for r in range(3)) and X[k].total == 0 and X[k].info["occupied_rows"] == 0
    assert X["I3"].owned == [(0, LIFE_M)] * 3 and model(ivs["I3"], "reduce_scatter").owned == [(0, 0), (0, 0), (0, LIFE_M)]
    # I4: the uint64 wire, rank 1 empty, one merged cell of 2^32 + 5 out of 5 ingested and 2^32 imported
    i4, x4 = ivs["I4"], X["I4"]
    assert i4.dirty and not x4.words32 and x4.info["cell_bytes"] == 8 and x4.info["packed_words"] == x4.info["packed_cells"]
    assert i4.holds_nothing(1) and not i4.holds_nothing(0) and not i4.holds_nothing(2)
    hot = [int(o.dense(HOT_ROW, HOT_ROW + 1)[0, HOT_BIN]) for o in x4.own]
    assert hot == [HOT_OWN, 0, HOT_IMPORT] and int(x4.merged.dense(HOT_ROW, HOT_ROW + 1)[0, HOT_BIN]) == (1 << 32) + 5
    assert int(x4.merged.count.max()) == (1 << 32) + 5 and int(np.sort(x4.merged.count)[-2]) < 1 << 16
    for row in range(LIFE_M):
        want = (i4.bins[(row, "lo")], i4.bins[(row, "hi")]) if (row, "lo") in i4.bins else EMPTY
        assert tuple(x4.merged_ranges[row]) == want, (row, x4.merged_ranges[row], want)
    row0, value0, _ = i4.cells[0][0]                             # the cell lh_snapshot_mark_dirty names is one rank 0 holds
    import oracle
    assert int(x4.own[0].dense(row0, row0 + 1)[0, int(oracle.key_to_bin(oracle.compress(value0)))]) > 0
    # a stale plan would show: the merges' plans differ from one to the next
    infos = [tuple(sorted(X[k].info.items())) for k in ("I1", "I2", "I3", "I4", "I5")]
    assert len(set(infos)) == 5
    return X


def self_check_wave():
    sc = wave_interval()
    X = model(sc, "reduce_scatter")
    assert sc.nranks == 2 and sc.M == WAVE_M == 4200 and X.words32
    small = [row for row in range(WAVE_M) if row not in WAVE_WIDE_ROWS]
    assert set(X.width[small]) == {WAVE_SMALL} and set(X.cls[small]) == {8} and set(X.words[small]) == {2}
    for row, (cls, lo4) in WAVE_WIDE_ROWS.items():
        assert X.width[row] == WAVE_WIDE and X.cls[row] == cls and X.merged_ranges[row, 0] % 4 == lo4, row
    for row in range(WAVE_M):
        assert tuple(X.merged_ranges[row]) == (sc.bins[(row, "lo")], sc.bins[(row, "hi")])
        assert all(tuple(rg[row]) != tuple(X.merged_ranges[row]) for rg in X.own_ranges), row
    assert {int(x) % 4 for x in X.merged_ranges[small, 0]} == {0, 1, 2, 3}
    blocks = [b - a for a, b in X.owned]
    assert min(blocks) >= WAVE_MIN_BLOCK and X.owned == [(0, 2100), (2100, 4200)], X.owned
    inside = [[row for row in WAVE_WIDE_ROWS if a <= row < b] for a, b in X.owned]
    assert [len(x) for x in inside] == [1, 2] and WAVE_M - 1 in inside[1]
    assert max(sc.samples(r) for r in range(2)) < 20000
    return X


# ---- the merge and what follows it --------------------------------------------------------------------------------------------
def feed(iv, engines):
    for r, e in enumerate(engines):
        ids, v = iv.pairs(r)
        if ids.size:
            e.submit_pairs(ids, v)


def merge_all(snaps, comms, iv, plan):
    nranks = iv.nranks
    results, errors = [None] * nranks, []

    def rank_main(r):
        try:
            results[r] = snaps[r].merge_rccl(comms[r], nranks, r, iv.nrows, plan=plan)
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank never left the collective"
    return results


class Refs:
    """The merged rows of one interval as the readers' models take them, computed once and shared by the ranks."""

    def __init__(self, X, nrows, names):
        import oracle
        self.X, self.nrows, self.names = X, nrows, names
        self.D = oracle.decompress_table()
        self.count = np.zeros(nrows, dtype=U64)
        self.nbuckets = np.zeros(nrows, dtype=np.int64)
        self.sum, self.mag = np.zeros(nrows), np.zeros(nrows)
        self.pkeys, self.pvalid = np.zeros((nrows, len(P)), dtype=np.int16), np.zeros((nrows, len(P)), dtype=np.uint8)
        for first in range(0, nrows, CHUNK):
            dense = X.merged.dense(first, min(nrows, first + CHUNK))
            for j, row in enumerate(dense):
                m = first + j
                ref = oracle.process_dense(row, P)
                self.count[m], self.nbuckets[m], self.sum[m] = ref["count"], ref["nbuckets"], ref["sum"]
                self.pkeys[m], self.pvalid[m] = ref["pkeys"], ref["pvalid"]
        # sum |value| x count per row: what the bound on a float sum is relative to (tests/test_gpu_serialize.py)
        rows, bins, counts = X.merged.below(nrows)
        np.add.at(self.mag, rows, np.abs(self.D[bins]) * counts.astype(np.float64))
        self._exact = {}

    def cells(self, m):
        s = self.X.merged.span(m, m + 1)
        return [int(b) for b in self.X.merged.bins[s]], [int(c) for c in self.X.merged.count[s]]

    def exact(self, m):
        from tests.test_gpu_spread import Exact
        if m not in self._exact:
            self._exact[m] = Exact(*self.cells(m))
        return self._exact[m]


def check_extract(snap, R, first, last, what):
    st = snap.extract(P, last - first, first=first)
    sel = slice(first, last)
    assert np.array_equal(np.asarray(st["count"]).astype(U64), R.count[sel]), (what, "extract count")
    assert np.array_equal(np.asarray(st["nbuckets"]).astype(np.int64), R.nbuckets[sel]), (what, "extract nbuckets")
    assert np.array_equal(np.asarray(st["pvalid"]) != 0, R.pvalid[sel] != 0), (what, "extract pvalid")
    ok = R.pvalid[sel] != 0
    bad = np.argwhere((np.asarray(st["pkeys"]) != R.pkeys[sel]) & ok)
    assert bad.size == 0, (what, "extract pkeys", first + int(bad[0][0]), st["pkeys"][bad[0][0]], R.pkeys[first + bad[0][0]])
    err = np.abs(np.asarray(st["sum"], dtype=np.float64) - R.sum[sel])
    bad = np.nonzero(~(err <= 1e-12 * R.mag[sel]))[0]
    assert bad.size == 0, (what, "extract sum", first + int(bad[0]), float(st["sum"][bad[0]]), float(R.sum[first + bad[0]]))
    return st


def check_readers(snap, R, first, last, what):
    """(e): spread, count_le, top, keep + Kept.across, serialize over rows [first, last) (extract: check_extract)"""
    import oracle
    from tests.test_gpu_across import model as across_model
    from tests.test_gpu_count_le import take_of
    from tests.test_gpu_kept import check64
    from tests.test_gpu_spread import REL, check as check_spread
    from loghisto_amd import _native as N
    n = last - first
    st = check_extract(snap, R, first, last, what)
    exact = [R.exact(m) for m in range(first, last)]
    with contextlib.redirect_stdout(io.StringIO()):           # (the check prints every figure it compares)
        check_spread(snap.spread(P, n, first), exact, P, extract=st)
    # count_le at the ends of the key space, at the ends of a few merged windows and between them
    occupied = [m for m in range(first, last) if R.count[m]][:6]
    at = sorted({0, 1, 33000, HOT_BIN - 1, HOT_BIN, 38000, NKEYS - 2, NKEYS - 1}
                | {int(b) for m in occupied for b in (R.X.merged_ranges[m, 0], R.X.merged_ranges[m, 1], max(0, R.X.merged_ranges[m, 1] - 1))})
    bounds = np.concatenate(([-np.inf], R.D[at], [np.inf]))
    E = take_of(bounds)
    dense = R.X.merged.dense(first, last)
    pre = np.zeros((n, NKEYS + 1), dtype=U64)
    np.cumsum(dense, axis=1, dtype=U64, out=pre[:, 1:])
    got = snap.count_le(bounds, n, first)
    assert np.array_equal(got["cum"], pre[:, E]) and np.array_equal(got["total"], pre[:, NKEYS]), (what, "count_le")
    # top by count, k = 5: descending count, equal counts lowest id first
    want = sorted((m for m in range(first, last) if R.count[m]), key=lambda m: (-int(R.count[m]), m))[:5]
    top = snap.top(5, "count", nmetrics=n, first=first)
    assert top.dtype == N.TOP_ENTRY and top["id"].tolist() == want, (what, "top ids", top["id"].tolist(), want)
    assert [int(c) for c in top["count"]] == [int(R.count[m]) for m in want], (what, "top counts")
    assert not top["reserved"].any() and not top["pkey"].any() and not top["above"].any(), (what, "top")
    for e, m in zip(top, want):
        ex = R.exact(m)
        assert abs(Fraction(float(e["sum"])) - ex.S) <= REL * ex.A, (what, "top sum", m, float(e["sum"]))
    # keep, then Kept.across on the one handle
    with snap.keep(n, first) as kept:
        assert kept.info["first"] == first and kept.info["nrows"] == n and kept.info["cells"] == int(R.nbuckets[first:last].sum())
        got = kept.across([], P, n, first)
    check64(got, [across_model([dict(zip(*R.cells(m)))], P) for m in range(first, last)], P, what)
    # serialize: the owned rows' lines, byte for byte with the engine's own float64 sums (held to their bound above)
    text = snap.serialize(PCT, nmetrics=n, first=first, **WIRE)
    lines = oracle.wire_lines(R.names[first:last], list(dense), PCT, sums=np.asarray(st["sum"]), **WIRE)
    got_lines = text.decode().split("\n")
    assert got_lines[-1] == "" and got_lines[:-1] == [w.rstrip("\n") for w in lines], (what, "serialize")
    return len(lines)


def rows_on_device(snap, M, first, last, cells, torch, what, at_most=False):
    """Many rows at once: rows [first, last) of the store as it is (4- or 8-byte cells, all 65 536 bins) against `cells`, on the
    device, 512 rows at a time -- equal cell by cell, or (at_most) nowhere above it; the first offending cells are named.  The
    counts here stay far below 2^63: the signed comparison is the unsigned one."""
    from tests import _span_contract as SC
    store, _, cb = SC.store_view(snap, M, torch)
    for a in range(first, last, 512):
        b = min(last, a + 512)
        got = store[a:b, :NKEYS]
        got = (got.to(torch.int64) & U32MAX) if cb == 4 else got
        s = cells.span(a, b)
        want = torch.zeros((b - a, NKEYS), dtype=torch.int64, device="cuda")
        want[torch.from_numpy(cells.rows[s] - a).cuda(), torch.from_numpy(cells.bins[s]).cuda()] = \
            torch.from_numpy(cells.count[s].view(np.int64)).cuda()
        bad = ((got > want) | (got < 0) if at_most else got != want).nonzero()
        if bad.numel():
            named = [(a + int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:8].cpu().numpy()]
            raise AssertionError(f"{what}: {int(bad.shape[0])} cells of rows [{a}, {b}) are not what they must be, "
                                 f"(row, bin, got, want): {named}")


def judge(iv, X, r, snap, result, narrow_engine, torch, R, full):
    """(a) .. (g) on rank r after the merge of `iv`.  full: every reader family (else extract only) and raw_rows of every row."""
    from tests import _span_contract as SC
    M, nrows = iv.M, iv.nrows
    what = f"{iv.name} rank {r}"
    first, last = result
    assert (first, last) == X.owned[r], (what, result, X.owned)
    rec = SC.check_store(snap, M, torch)                               # (a)
    try:
        SC.assert_contract(rec)
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from None
    bad = np.nonzero((rec.ranges != X.final_ranges[r]).any(axis=1))[0]  # (b)
    assert bad.size == 0, (what, "ranges", int(bad[0]), rec.ranges[bad[0]].tolist(), X.final_ranges[r][bad[0]].tolist())
    width = snap.device_cells()[2]                                      # (f)
    assert width == (4 if narrow_engine and X.words32 else 8), (what, "cell bytes", width)
    info = snap.merge_info()                                            # (g)
    for k, v in X.info.items():
        assert info[k] == v, (what, "merge_info", k, info[k], v)
    # (c) owned rows, and the rows from nrows on (the rank's own), cell by cell
    if full:
        for a, b, cells, which in ((first, last, X.merged, "owned"), (nrows, M, X.own[r], "beyond nrows")):
            if b > a:
                got, want = SC.raw_rows(snap, range(a, b), torch), cells.dense(a, b)
                diff = np.argwhere(got != want)
                assert diff.size == 0, (what, which, len(diff), [(a + int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in diff[:8]])
    else:
        rows_on_device(snap, M, first, last, X.merged, torch, what + " owned")
        rows_on_device(snap, M, nrows, M, X.own[r], torch, what + " beyond nrows")
        probe = sorted({first, last - 1} | {m for m in WAVE_WIDE_ROWS if first <= m < last})
        assert np.array_equal(SC.raw_rows(snap, probe, torch), np.concatenate([X.merged.dense(m, m + 1) for m in probe])), (what, probe)
    # the store's totals: every owned row's sum is the merged row's (over the padding cells too)
    assert np.array_equal(rec.total[first:last], R.count[first:last]) and not rec.npad.any(), (what, "row sums")
    # (d) rows of other owners: unspecified by the header; nothing there but what the merged row has, at most as much
    for a, b in ((0, first), (last, nrows)):
        if b > a and full:
            got, want = SC.raw_rows(snap, range(a, b), torch), X.merged.dense(a, b)
            over = np.argwhere(got > want)
            assert over.size == 0, (what, "a row of another owner holds what its merged row does not",
                                    [(a + int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in over[:8]])
        elif b > a:
            rows_on_device(snap, M, a, b, X.merged, torch, what + " rows of another owner", at_most=True)
    lines = 0
    if last > first:                                                    # (e)
        if full:
            lines = check_readers(snap, R, first, last, what)
        else:
            check_extract(snap, R, first, last, what)
    return dict(owned=[first, last], cell_bytes=width, violations=len(rec.violations) + int(rec.npad.sum()) + int(rec.nstray.sum()),
                nonzero_cells=int(rec.nnz.sum()), lines=lines)


def judge_clean(snap, M, torch, what):
    from tests import _span_contract as SC
    try:
        SC.assert_clean(SC.check_store(snap, M, torch))
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from None


def make_engines(nranks, M, names=False):
    import loghisto_amd
    engines = [loghisto_amd.Engine(max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16) for _ in range(nranks)]
    labels = [f"svc_{i}.lat" for i in range(M)]
    if names:
        for e in engines:
            assert [e.intern(nm) for nm in labels] == list(range(M))
    return engines, labels


def run_life(plan, stub):
    import torch
    import oracle
    t_start = time.perf_counter()
    ivs = life_intervals()
    self_check_life()
    nranks, M = LIFE_RANKS, LIFE_M
    narrow_engine = os.environ.get("LH_TEST_CELL_BITS", "0") == "32"
    comms = (C.c_void_p * nranks)()
    assert stub.stub_comm_create(nranks, comms) == 0
    engines, names = make_engines(nranks, M, names=True)
    out, buffers, merges = [], [], [0] * nranks
    for name in LIFE_SEQUENCE:
        iv = ivs[name]
        t0 = time.perf_counter()
        feed(iv, engines)
        snaps = [e.flip() for e in engines]
        buffers.append(snaps[0].device_ranges())
        # a rank that submitted nothing: the buffer is what the release before left -- judged before anything else touches it
        judged = [r for r in range(nranks) if iv.holds_nothing(r)]
        for r in judged:
            judge_clean(snaps[r], M, torch, f"{name} rank {r} before the merge")
            assert snaps[r].device_cells()[2] == (4 if narrow_engine else 8), (name, r)
        rec = dict(name=name, merged=iv.merged, clean_before=judged)
        if iv.merged:
            X = model(iv, plan)
            for r in range(nranks):
                for row, b, c in iv.imports[r]:
                    snaps[r].add_buckets(np.array([row], dtype=np.uint32), oracle.bin_to_key(np.array([b])), np.array([c], dtype=U64))
            if iv.dirty:                                       # (a cell rank 0 already holds: its ranges stay as they are)
                row, value, _ = iv.cells[0][0]
                b = int(oracle.key_to_bin(oracle.compress(value)))
                snaps[0].mark_dirty(row, 1, b, b)
            results = merge_all(snaps, comms, iv, plan)
            R = Refs(X, iv.nrows, names)
            covered = []
            ranks = []
            for r in range(nranks):
                ranks.append(judge(iv, X, r, snaps[r], results[r], narrow_engine, torch, R, full=True))
                covered.extend(range(*results[r]))
                merges[r] += 1
            assert sorted(covered) == sorted(list(range(iv.nrows)) * (nranks if plan == "allreduce" else 1)), name
            if X.total == 0:                                   # I3: the whole raw store is zero behind the merge as well
                for r in range(nranks):
                    judge_clean(snaps[r], M, torch, f"{name} rank {r} after the merge")
            rec.update(nrows=iv.nrows, wire_bytes=X.info["cell_bytes"], ranks=ranks, clean_after=X.total == 0,
                       **{k: X.info[k] for k in ("packed_cells", "packed_words", "rows_8bit", "rows_16bit", "occupied_rows")})
        for s in snaps:
            s.release()
        rec["s"] = round(time.perf_counter() - t0, 3)
        out.append(rec)
    assert buffers[0] != buffers[1] and buffers == [buffers[0], buffers[1]] * 4, buffers     # I1 I3 spare end0 | I2 I4 I5 end1
    for e in engines:
        e.close()
    stub.stub_comm_destroy(nranks, comms)
    return dict(intervals=out, merges_per_rank=merges, buffer_of=dict(zip(LIFE_SEQUENCE, [0, 1] * 4)),
                samples_per_rank={k: [iv.samples(r) for r in range(nranks)] for k, iv in ivs.items() if iv.merged},
                total_s=round(time.perf_counter() - t_start, 3))


def run_wave(stub):
    import torch
    t_start = time.perf_counter()
    iv = wave_interval()
    self_check_wave()
    nranks, M = WAVE_RANKS, WAVE_M
    narrow_engine = os.environ.get("LH_TEST_CELL_BITS", "0") == "32"
    comms = (C.c_void_p * nranks)()
    assert stub.stub_comm_create(nranks, comms) == 0
    engines, names = make_engines(nranks, M)
    R = Refs(model(iv, "reduce_scatter"), M, names)
    out = []
    for plan in ("reduce_scatter", "allreduce"):               # the same engines: buffer 0, then buffer 1
        t0 = time.perf_counter()
        X = model(iv, plan)
        feed(iv, engines)
        snaps = [e.flip() for e in engines]
        results = merge_all(snaps, comms, iv, plan)
        for r, (first, last) in enumerate(results):
            # a condition of the test: below 2 048 rows k_unpack_rows runs a workgroup per row and nothing here is new
            assert last - first >= WAVE_MIN_BLOCK, f"rank {r} owns [{first}, {last}): {last - first} rows < {WAVE_MIN_BLOCK}, the wave shape does not run"
        ranks = [judge(iv, X, r, snaps[r], results[r], narrow_engine, torch, R, full=False) for r in range(nranks)]
        for s in snaps:
            s.release()
        out.append(dict(plan=plan, owned=[list(x) for x in results], owned_rows=[b - a for a, b in results], ranks=ranks,
                        packed_words=X.total, s=round(time.perf_counter() - t0, 3)))
    for e in engines:                                          # both buffers once more: what the two releases left
        for k in range(2):
            with e.flip() as snap:
                judge_clean(snap, M, torch, f"after the releases, flip {k}")
    for e in engines:
        e.close()
    stub.stub_comm_destroy(nranks, comms)
    return dict(merges=out, samples_per_rank=[iv.samples(r) for r in range(nranks)], total_s=round(time.perf_counter() - t_start, 3))


def main():
    case, plan = sys.argv[1], sys.argv[2]
    assert case in CASES and plan in ("allreduce", "reduce_scatter") and (case != "rs_wave" or plan == "reduce_scatter"), sys.argv
    from loghisto_amd import _native as N
    stub_path = os.path.join(ROOT, "loghisto_amd", "build", "librccl_stub.so")
    N.check(N.lib().lh_set_rccl_library(stub_path.encode()), "lh_set_rccl_library")
    stub = C.CDLL(stub_path)
    res = run_life(plan, stub) if case == "life" else run_wave(stub)
    print(json.dumps(dict(ok=True, case=case, plan=plan, cell_bits=os.environ.get("LH_TEST_CELL_BITS", "0"), **res)))


if __name__ == "__main__":
    main()
