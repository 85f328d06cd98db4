"""Crafted sparse rows for the readers of a snapshot of 32-bit cells (tests/test_gpu_cells32_readers.py writes them into
the narrow store; tests/test_cells32_rows.py checks, without a GPU, that every code path below has a row).

What the rows aim at (loghisto_amd/csrc/lh_kernels.hip, k_extract_wave<uint32_t>):
  * the four cells of a lane are ONE 16-byte load from row + lo + 4 j: 4-byte aligned only, whenever lo % 4 != 0;
  * a span stays in registers as 32-bit cells while hi - lo < 1 024 and every cell is below 2^22 (route "reg": the prefix
    scan then runs in uint32 and the largest total it may see is 1 024 x (2^22 - 1) = 2^32 - 1 024); anything else takes
    the two-pass loop (route "loop");
  * a 4-bin group that straddles hi is read whole: the cells behind hi must be zero, and the group that STARTS at hi
    (hi - lo a multiple of 4) must still be read;
  * _sum goes through uint64(float64) as Go compiles it for amd64: five branches.

A row is {bin: count} with every count in 1 .. 2^32 - 1, kept as sorted arrays; `span` is what lh_snapshot_mark_dirty is
called with: the tight [min bin, max bin], a span over nothing but zeros, or None for a row that is never marked."""
import numpy as np

import oracle

NKEYS = 65536
EW_REG = 1024            # bins k_extract_wave holds in registers
REG_CELL = 1 << 22       # ... while every cell is below this
U32 = (1 << 32) - 1
FIRST_SPECIAL = 100      # the special rows start here: inside [100, 1600), which both extract kernels read
ROW0_SAMPLES = np.array([1.0, 2.0, 2.0, 300.0, -7.5, 0.0, 1e9])   # row 0 is ingested: an interval has to hold something
TWO63, TWO64 = 2.0 ** 63, 2.0 ** 64


class Row:
    __slots__ = ("kind", "bins", "counts", "span")

    def __init__(self, kind, cells, span="tight"):
        items = sorted((int(b), int(c)) for b, c in cells.items() if int(c))
        self.kind = kind
        self.bins = np.array([b for b, _ in items], dtype=np.int64)
        self.counts = np.array([c for _, c in items], dtype=np.uint64)
        assert all(0 <= b < NKEYS for b, _ in items) and all(0 < c <= U32 for _, c in items), kind
        if span == "tight":
            span = (int(self.bins[0]), int(self.bins[-1])) if items else None
        assert span is None or (0 <= span[0] <= span[1] < NKEYS and (not items or (span[0] <= items[0][0] and items[-1][0] <= span[1])))
        self.span = span

    def total(self) -> int:
        return int(self.counts.sum(dtype=np.uint64))

    def dense(self) -> np.ndarray:
        """The row as the oracle takes it: uint64[65536].  Built on demand, one at a time."""
        d = np.zeros(NKEYS, dtype=np.uint64)
        d[self.bins] = self.counts
        return d

    def window(self) -> np.ndarray:
        """uint32 cells of [span lo, span hi]."""
        lo, hi = self.span
        w = np.zeros(hi - lo + 1, dtype=np.uint32)
        w[self.bins - lo] = self.counts.astype(np.uint32)
        return w

    def magnitude(self, D) -> float:
        """sum |D[b]| * float64(c): what the bound on _sum is relative to."""
        return float(np.sum(np.abs(D[self.bins]) * self.counts.astype(np.float64)))


# ---- the model: which path a row takes ---------------------------------------------------------------------------------
def route(row):
    """'reg' (one read, 32-bit registers), 'loop' (two passes, 64-bit counts) or None (never marked: lo > hi)."""
    if row.span is None:
        return None
    lo, hi = row.span
    return "reg" if hi - lo < EW_REG and (row.counts.size == 0 or int(row.counts.max()) < REG_CELL) else "loop"


def last_group(row):
    """(hi - lo) % 4: 0 -- the last 4-bin group STARTS at hi --, 1 or 2 -- it straddles hi --, 3 -- it ends there."""
    lo, hi = row.span
    return (hi - lo) % 4


def conversion_branch(s: float) -> str:
    """The branch uint64(float64) takes (d_f64_to_u64_amd64 / lh_expand_compact's host twin)."""
    if s != s:
        return "nan"
    if s >= TWO64:
        return "ge_2_64"
    if s >= TWO63:
        return "2_63_to_2_64"
    if s <= -TWO63:
        return "le_minus_2_63"
    return "negative" if s < 0 else "0_to_2_63"


def f64_to_u64_model(s: float) -> int:
    """The conversion restated: CVTTSD2SQ's 'integer indefinite' 2^63 outside int64, truncation inside, and Go's
    subtract-2^63-and-flip-the-top-bit for f >= 2^63."""
    br = conversion_branch(s)
    if br in ("nan", "le_minus_2_63"):
        return 1 << 63
    if br == "ge_2_64":
        return 0                                          # (indefinite 2^63) ^ 2^63
    if br == "2_63_to_2_64":
        return int(s - TWO63) ^ (1 << 63)
    return int(s) & ((1 << 64) - 1)                       # truncates towards zero; two's complement below zero


# ---- the rows ----------------------------------------------------------------------------------------------------------
def _lo(rng, r, room):
    """A first bin with lo % 4 == r and `room` bins behind it."""
    return 4 * int(rng.integers(1, (NKEYS - room - 8) // 4)) + r


def _dense(rng, lo, w, top):
    """w consecutive bins with counts 0 .. top - 1, both ends occupied."""
    c = rng.integers(0, top, w)
    c[0], c[-1] = max(1, c[0]), max(1, c[-1])
    return {lo + i: int(c[i]) for i in range(w) if c[i]}


def _specials(rng, D):
    out = []

    def add(kind, cells, span="tight"):
        out.append(Row(kind, cells, span))

    for r in range(4):                                     # ---- every lo % 4
        # a handful of cells, total 1 .. 10: every percentile of P_A lands on or beside a quotient k / total
        for _ in range(2):
            lo = _lo(rng, r, 64)
            k = int(rng.integers(1, 6))
            bins = [lo] + sorted(int(b) for b in rng.choice(np.arange(lo + 1, lo + 40), size=k - 1, replace=False))
            add(f"handful/{r}", {b: int(rng.integers(1, 3)) for b in bins})
        add(f"one_sample/{r}", {_lo(rng, r, 8): 1})
        for c in (10, 100, 1000):                          # ten equal cells
            lo, step = _lo(rng, r, 1000), int(rng.integers(1, 100))
            add(f"ten_equal_{c}/{r}", {lo + i * step: c for i in range(10)})
        # one cell either side of the boundary between the registers and the two-pass loop
        for c in (1, REG_CELL - 1, REG_CELL, 1 << 31, U32):
            add(f"one_cell_{c}/{r}", {_lo(rng, r, 8): c})
        # exactly 1 024 bins of 2^22 - 1: total 2^32 - 1 024, the largest the uint32 scan may see; it must not wrap
        lo = _lo(rng, r, 1100)
        add(f"reg_max_total/{r}", {lo + i: REG_CELL - 1 for i in range(EW_REG)})
        cells = {lo + i: REG_CELL - 1 for i in range(EW_REG)}
        cells[lo + int(rng.integers(0, EW_REG))] = REG_CELL
        add(f"reg_max_total_one_cell_up/{r}", cells)       # one cell at 2^22: the loop
        # cells of 2^22 .. 2^23 - 1 whose total passes 2^32: a uint32 scan that took them would wrap (to 0 for 1 024 x 2^22)
        add(f"span_1024_of_2^22/{r}", {lo + i: REG_CELL for i in range(EW_REG)})
        add(f"span_1024_below_2^23/{r}", {lo + i: int(c) for i, c in enumerate(rng.integers(REG_CELL, 2 * REG_CELL, EW_REG))})
        for w in range(1021, 1028):                        # spans around 1 024 bins, occupied at both ends and the middle
            lo = _lo(rng, r, 1100)
            add(f"span_{w}/{r}", {lo: 3, lo + w // 2: 1, lo + w - 1: 5})
        for g in range(4):                                 # dense windows, every (lo % 4, (hi - lo) % 4)
            w = 4 * int(rng.integers(1, 250)) + g + 1
            add(f"dense_narrow/{r}{g}", _dense(rng, _lo(rng, r, 1100), w, 4))
            w = 4 * int(rng.integers(257, 1250)) + g + 1
            add(f"dense_wide/{r}{g}", _dense(rng, _lo(rng, r, 5100), w, 3))
        # windows that end at bin 65 535: the last lanes' groups reach into the padding behind the row
        w = 4 * int(rng.integers(1, 250)) - r
        add(f"top_narrow/{r}", _dense(rng, NKEYS - w, w, 50))
        w = 4 * int(rng.integers(300, 1200)) - r
        add(f"top_wide/{r}", _dense(rng, NKEYS - w, w, 50))
        # many 1s and one dominant cell: the prefix jumps over several thresholds at once
        lo, w = _lo(rng, r, 1100), int(rng.integers(10, 1000))
        cells = {lo + i: 1 for i in range(0, w, 7)}
        cells[lo + 7 * (w // 21)] = REG_CELL - 1
        add(f"dominant_reg/{r}", cells)
        cells = dict(cells)
        cells[lo + 7 * (w // 21)] = 10 ** 9
        add(f"dominant_loop/{r}", cells)
        # totals at or above 2^32 from cells below 2^32 (what a caller's own reduction on the cell view can leave)
        lo = _lo(rng, r, 1100)
        add(f"five_cells_of_2^32-1/{r}", {int(b): U32 for b in lo + np.sort(rng.choice(1000, 5, replace=False))})
    lo = _lo(rng, 1, 3600)
    add("3000_cells_of_2^21", {int(b): 1 << 21 for b in lo + rng.choice(3500, 3000, replace=False)})
    add("only_bin_65535", {NKEYS - 1: 7})
    add("only_bin_0", {0: 9})
    add("bottom_narrow", _dense(rng, 0, 603, 50))          # 0 .. k
    add("bottom_wide", _dense(rng, 0, 2601, 50))
    add("both_ends", {0: 2, NKEYS - 1: 3})
    add("full_range_small", {b: int(c) for b, c in enumerate(rng.integers(1, 4, NKEYS))})
    add("full_range_large", {b: int(c) for b, c in enumerate(rng.integers(1, 1 << 32, NKEYS))})
    add("never_marked", {})
    lo = _lo(rng, 2, 600)
    add("marked_zero_narrow", {}, span=(lo, lo + 500))     # marked dirty over nothing but zeros
    lo = _lo(rng, 3, 3000)
    add("marked_zero_wide", {}, span=(lo, lo + 2500))

    # ---- _sum in every branch of uint64(float64): one cell of 2^32 - 1 at a bin whose value puts the product there, and
    # the same total spread over three neighbouring cells (so that the kernels' own additions take part)
    def first_bin(x):                                       # the first bin whose value x (2^32 - 1) reaches x
        return int(np.nonzero(D * float(U32) >= x)[0][0])

    def last_bin(x):                                        # the last bin whose value x (2^32 - 1) is at or below x
        return int(np.nonzero(D * float(U32) <= x)[0][-1])

    for name, b in (("2_63_to_2_64", first_bin(1.3 * TWO63)), ("ge_2_64", first_bin(1.02 * TWO64)),
                    ("below_2_63", first_bin(0.9 * TWO63)), ("le_minus_2_63", last_bin(-1.02 * TWO63)),
                    ("above_minus_2_63", last_bin(-0.9 * TWO63))):
        add(f"sum_{name}/1", {b: U32})
        add(f"sum_{name}/3", {b - 1: U32 // 3, b: U32 // 3, b + 1: U32 // 3 + U32 % 3})
    add("sum_ge_2_64/top", {NKEYS - 1: 1})
    add("sum_le_minus_2_63/bottom", {0: 1})
    minus5 = int(oracle.key_to_bin(oracle.compress(-5.0)))
    add("sum_small_negative", {minus5: 3})
    add("sum_small_negative/mixed", {minus5 - 30: 2, minus5: 3, int(oracle.key_to_bin(oracle.compress(4.0))): 1})
    return out


def _filler(rng, i):
    """Ordinary rows of every shape, cells up to 2^32 - 1 (what tests/test_gpu_extract_thresholds.py draws, capped)."""
    kind = i % 12
    lo = int(rng.integers(0, NKEYS - 1100))
    if kind == 0:
        k = int(rng.integers(1, 6))
        bins = np.sort(rng.choice(np.arange(lo, lo + 40), size=k, replace=False))
        return Row("f_handful", {int(b): int(rng.integers(1, 3)) for b in bins})
    if kind == 1:
        step = int(rng.integers(1, 100))
        return Row("f_ten_equal", {lo + i * step: 10 ** int(rng.integers(1, 4)) for i in range(10)})
    if kind == 2:
        return Row("f_one_cell", {lo: int(rng.integers(1, 1 << 32))})
    if kind == 3:
        return Row("f_dense_narrow", _dense(rng, lo, int(rng.integers(2, 1024)), 4))
    if kind == 4:
        lo = int(rng.integers(0, NKEYS - 5100))
        return Row("f_dense_wide", _dense(rng, lo, int(rng.integers(1025, 5000)), 3))
    if kind == 5:
        w = int(rng.integers(1, 700))
        return Row("f_top", _dense(rng, NKEYS - w, w, 50))
    if kind == 6:
        return Row("f_bottom", _dense(rng, 0, int(rng.integers(1, 700)), 50))
    if kind == 7:
        w = 1024 + i // 12 % 2
        return Row("f_span_1024_1025", {lo: 3, lo + w - 1: 5, lo + w // 2: 1})
    if kind == 8:
        w = int(rng.integers(10, 1000))
        cells = {lo + j: 1 for j in range(0, w, 7)}
        cells[lo + 7 * (w // 21)] = 10 ** 9 if i // 12 % 2 else 10 ** 6
        return Row("f_dominant", cells)
    if kind == 9:                                           # lognormal counts either side of 2^22, up to 2^32 - 1
        w = int(rng.integers(50, 1000))
        c = np.minimum(rng.lognormal(10, 4, w), float(U32)).astype(np.uint64)
        return Row("f_lognormal", {lo + j: int(c[j]) for j in range(w) if c[j]})
    if kind == 10:                                          # a wide span of few, large cells
        lo = int(rng.integers(0, NKEYS - 9100))
        k = int(rng.integers(2, 40))
        bins = lo + np.sort(rng.choice(int(rng.integers(1100, 9000)), size=k, replace=False))
        return Row("f_wide_sparse", {int(b): int(rng.integers(1, 1 << 32)) for b in bins})
    return Row("f_empty", {})


_CACHE = {}


def make_rows(M, seed=32):
    """M rows, seeded: row 0 = the ingested samples, [FIRST_SPECIAL, ...) the special rows, the rest filler."""
    if (M, seed) in _CACHE:
        return _CACHE[(M, seed)]
    rng = np.random.default_rng(seed)
    D = oracle.decompress_table()
    special = _specials(rng, D)
    assert M >= FIRST_SPECIAL + len(special) + 12, (M, len(special))
    h0 = oracle.histogram_dense(ROW0_SAMPLES)
    rows = [Row("ingested", {int(b): int(h0[b]) for b in np.nonzero(h0)[0]})]
    for m in range(1, M):
        k = m - FIRST_SPECIAL
        rows.append(special[k] if 0 <= k < len(special) else _filler(rng, m))
    _CACHE[(M, seed)] = rows
    return rows
