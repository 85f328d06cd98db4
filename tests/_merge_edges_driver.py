"""Crafted rows for lh_snapshot_merge's wire (run as a subprocess by tests/test_gpu_merge_edges.py; the rows themselves are
checked without a GPU by tests/test_merge_gloo.py).

K4 packs a row's cells into 8-, 16- or 32-bit fields of uint32 wire words, or into whole uint64 words, and the collective
adds the words as plain integers.  Two inequalities keep that exact (k_merge_widths, lh_snapshot_merge):
  * a row travels at 8 / 16 bits iff nranks x (the largest cell any rank holds in it) <= 0xff / 0xffff;
  * the wire word is uint32 iff the largest per-rank sample count < 0xffffffff and nranks x it < 2^32.
One off and a field's sum carries into the next cell of the word, or wraps to 0 -- only when a merged cell REACHES the bound,
which no random stream does.  Here every rank's cells are crafted: c pairs of one (id, value) leave exactly c in one cell.

  A        class boundaries: every rank holds c in the same cell, nranks x c = 255 | 256 (258) | 65 535 (65 532) | 65 536
           (65 538), the hot cell in every field of its word beside cells of 1, 0 and 2; rows whose bound comes from ONE rank
           (the last, the first); a row that one rank does not hold at all.
  B_small  window geometry: merged widths 1 .. 1 027 at every class and every lo % 4, the window made by different ranks
  B_large  (lo on one, hi on another, a few interior cells on the rest) -- below 2 048 rows (a workgroup walks a row) and at
           2 050 rows (a wave does), rows on both sides of the 1 024-row seam of the plan kernels and the last row; then the
           same rows on the uint64 wire (one rank's sample count unknown: lh_snapshot_mark_dirty).
  C1 C2 C3 the wire-word boundary, 4 ranks fed from ONE 2^24-pair device buffer: 2^30 - 1 pairs per rank (uint32 words, the
           hot merged cell 2^32 - 4), 2^30 per rank (uint64 words, the hot cell exactly 2^32), 2^30 on the LAST rank only.

Nothing expected comes from the library or from loghisto_amd.merge: a rank's rows are oracle.histogram_pairs on its own
pairs (C: the oracle's bin of each distinct pair times the count submitted), classes, words and owner blocks are numpy on
those rows.  loghisto_amd.merge.row_bits / plan_windows are then held against the same numbers.

usage: python tests/_merge_edges_driver.py CASE PLAN        (LH_TEST_CELL_BITS=32: engines of 32-bit cells)
"""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NKEYS = 65536
EMPTY = (NKEYS, 0)                       # the range of a row nobody holds
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027)
A_COUNTS = {3: (85, 86, 21845, 21846), 4: (63, 64, 16383, 16384)}          # nranks -> c; nranks x c either side of 2^8, 2^16
A_CLASS = {3: (8, 16, 16, 32), 4: (8, 16, 16, 32)}                         # ... and the class the issue's table gives it
A_MAX_ONLY = {3: 86, 4: 64}              # held by ONE rank: nranks x c is 258 / 256 although the merged cell is c
B_BIG = {8: 1, 16: 100, 32: 22000}       # the largest per-rank cell of a class' rows: 3 x and 4 x it lie inside the class
LARGE_M = 2050
LARGE_IDS = ([0, 1023, 1024, 2047, LARGE_M - 1] + list(range(300, 316)) + list(range(1010, 1023)) + list(range(1025, 1031))
             + list(range(1600, 1614)))
C_BUF = 1 << 24                          # pairs of the device buffer every Case C rank submits over and over
C_PAIRS = {"C1": (1 << 30) - 1, "C2": 1 << 30, "C3": 1 << 30}
C_CELL_BYTES = {"C1": 4, "C2": 8, "C3": 8}
C_HOT = (2, 1234.5)                      # (row, value) of the hot cell
C_ROWS = 5
CASES = ("A", "B_small", "B_large", "C1", "C2", "C3")


class Scenario:
    """cells[r] = [(row, value, count)]: rank r submits `count` pairs (row, value).  dirty: rank 0's sample count is made
    unknown after the flip.  expand: the pairs are few enough to write out (host submit, the oracle buckets every one)."""

    def __init__(self, name, nranks, M, expand=True, dirty=False):
        self.name, self.nranks, self.M, self.expand, self.dirty = name, nranks, M, expand, dirty
        self.cells = [[] for _ in range(nranks)]
        self.bins = {}                   # (row, what) -> bin: what the builder AIMED at, for the self-checks only

    def put(self, rank, row, value, count):
        if count:
            self.cells[rank].append((int(row), float(value), int(count)))

    def samples(self, rank):
        return sum(c for _, _, c in self.cells[rank])

    def pairs(self, rank):
        rows = np.array([r for r, _, _ in self.cells[rank]], dtype=np.uint32)
        vals = np.array([v for _, v, _ in self.cells[rank]], dtype=np.float64)
        cnt = np.array([c for _, _, c in self.cells[rank]], dtype=np.int64)
        return np.repeat(rows, cnt), np.repeat(vals, cnt)


# ---- the rows ----------------------------------------------------------------------------------------------------------
def _values():
    """value of every bin, and a check that the bins used below come back as themselves"""
    import oracle
    D = oracle.decompress_table()
    b = np.arange(33000, 40000)
    assert np.array_equal(oracle.key_to_bin(oracle.compress_many(D[b])), b)
    return D


def case_a(nranks):
    D = _values()
    cs = A_COUNTS[nranks]
    M = 4 * len(cs) + 4
    sc = Scenario(f"A/{nranks}", nranks, M)
    for p in range(4):                                     # the hot cell's field: (bin - lo) % 4
        for ci, c in enumerate(cs):
            row = p * len(cs) + ci                         # neighbouring rows differ in class
            lo = 33000 + 40 * row + (p + ci) % 4
            sc.put(0, row, D[lo], 1)                       # the window starts a word before the hot one
            hot = lo + 4 + p
            for r in range(nranks):
                sc.put(r, row, D[hot], c)
            others = [lo + 4 + q for q in range(4) if q != p]
            sc.put(p % nranks, row, D[others[0]], 1)       # 1, 0 and 2 in the other fields of the 4-cell word
            sc.put(nranks - 1, row, D[others[2]], 2)
            sc.put(1, row, D[lo + 9], 1)                   # ... and ends in the middle of a later one
            sc.bins[(row, "hot")] = hot
            sc.bins[(row, "lo")] = lo
    base = 4 * len(cs)
    for k, holder in enumerate((nranks - 1, 0)):           # the class follows the MAX over the ranks, not the sum
        row, lo = base + k, 36000 + 40 * k + 1 + k
        sc.put(holder, row, D[lo + 2], A_MAX_ONLY[nranks])
        sc.put((holder + 1) % nranks, row, D[lo], 1)
        sc.put((holder + 1) % nranks, row, D[lo + 3], 2)
        sc.put((holder + 2) % nranks, row, D[lo + 6], 1)
        sc.bins[(row, "hot")] = lo + 2
    # base + 2 stays empty on every rank; base + 3 is empty on rank 1 (lo > hi there) and occupied on the others
    for r in range(nranks):
        if r != 1:
            sc.put(r, base + 3, D[36200 + 3 * r], 1 + r)
    return sc


def _b_rows():
    """(width, class, lo % 4) of the 54 geometry rows: every width and every lo % 4 at every class, dealt out so that
    neighbouring rows differ in class and wide windows stand between narrow ones (19 is coprime to 54;
    with it an owner block of both shapes' reduce-scatter starts directly before a narrow row and one directly behind one)"""
    rows = [(w, cls, (wi + ci) % 4) for wi, w in enumerate(WIDTHS) for ci, cls in enumerate((8, 16, 32))]
    return [rows[19 * i % len(rows)] for i in range(len(rows))]


def case_b(shape, dirty):
    D = _values()
    rows = _b_rows()
    if shape == "small":
        nranks, M = 3, len(rows) + 2
        ids = [i for i in range(M) if i not in (7, 30)]    # two rows nobody holds
    else:
        nranks, M = 4, LARGE_M
        ids = sorted(LARGE_IDS)
    assert len(ids) == len(rows) and len(set(ids)) == len(ids) and M - 1 in ids and 0 in ids
    sc = Scenario(f"B_{shape}/{'uint64' if dirty else 'uint32'}", nranks, M, dirty=dirty)
    for idx, ((w, cls, lo4), row) in enumerate(zip(rows, ids)):
        lo = 33000 + 4 * idx + lo4
        hi = lo + w - 1
        lo_rank, hi_rank = idx % nranks, (idx + 1) % nranks
        rest = [r for r in range(nranks) if r not in (lo_rank, hi_rank)]
        big_at_hi = idx % 2 == 0                           # the cell that sets the class: the last field or the first
        sc.put(lo_rank, row, D[lo], 1 if big_at_hi else B_BIG[cls])
        sc.put(hi_rank, row, D[hi], B_BIG[cls] if big_at_hi else 1)
        for pos in sorted({1, 2, 3, 4, 5, w // 2, w - 6, w - 5, w - 4, w - 3, w - 2}):
            if 0 < pos < w - 1:
                c = 1 + pos % 5                            # distinct small counts: a field in the wrong place shows
                for k, r in enumerate(rest):
                    sc.put(r, row, D[lo + pos], (c + len(rest) - 1 - k) // len(rest))
        sc.bins[(row, "lo")], sc.bins[(row, "hi")], sc.bins[(row, "cls")] = lo, hi, cls
    return sc


def case_c(sub):
    nranks, n = 4, C_PAIRS[sub]
    sc = Scenario(sub, nranks, C_ROWS, expand=False)
    if sub == "C3":                                        # the bound comes from the largest rank, and that is not rank 0
        sc.put(nranks - 1, *C_HOT, n)
        sc.put(0, C_HOT[0], 1250.0, 1)                     # the cell beside the hot one
        sc.put(1, 0, -3.5, 1)
        sc.put(2, *C_HOT, 1)
    else:
        for r in range(nranks):
            sc.put(r, *C_HOT, n)
    return sc


def scenarios(case):
    if case == "A":
        return [case_a(3), case_a(4)]
    if case in ("B_small", "B_large"):
        return [case_b(case[2:], False), case_b(case[2:], True)]
    return [case_c(case)]


# ---- what the merge must give: the oracle's rows and numpy ---------------------------------------------------------------
def expected(sc, plan):
    import oracle
    nranks, M = sc.nranks, sc.M
    used = np.array(sorted({row for cells in sc.cells for row, _, _ in cells}), dtype=np.int64)
    K = used.size
    per_rank = []
    for r in range(nranks):
        if sc.expand:
            ids, v = sc.pairs(r)
            per_rank.append(oracle.histogram_pairs(np.searchsorted(used, ids), v, K))
        else:                                              # the oracle's bin of each distinct pair x the count submitted
            h = np.zeros((K, NKEYS), dtype=np.uint64)
            for row, value, count in sc.cells[r]:
                h += oracle.histogram_pairs([np.searchsorted(used, row)], [value], K) * np.uint64(count)
            per_rank.append(h)
    merged = per_rank[0].copy()
    for h in per_rank[1:]:
        merged += h

    def ranges_of(h):
        out = np.empty((K, 2), dtype=np.int64)
        for k in range(K):
            nz = np.nonzero(h[k])[0]
            out[k] = (nz[0], nz[-1]) if nz.size else EMPTY
        return out

    ranges = np.tile(np.array(EMPTY, dtype=np.int64), (M, 1))
    ranges[used] = ranges_of(merged)
    rowmax = np.zeros(M, dtype=np.int64)
    rowmax[used] = np.max([h.max(axis=1) for h in per_rank], axis=0).astype(np.int64)
    width = np.where(ranges[:, 0] <= ranges[:, 1], ranges[:, 1] - ranges[:, 0] + 1, 0)
    largest = max(sc.samples(r) for r in range(nranks))
    words32 = not sc.dirty and largest < 0xffffffff and nranks * largest < (1 << 32)
    bound = nranks * rowmax
    cls = np.where(bound <= 255, 8, np.where(bound <= 65535, 16, 32))
    words = (width * cls + 31) // 32 if words32 else width.copy()
    P = np.concatenate(([0], np.cumsum(words)))
    total = int(P[-1])
    nb = nranks if plan == "reduce_scatter" else 1
    # owner blocks: block k starts at the first row whose prefix reaches its share of the wire words
    brow = [0] + [int(np.searchsorted(P, total // nb * k + total % nb * k // nb, side="left")) for k in range(1, nb)] + [M]
    bmax = max(int(P[brow[k + 1]] - P[brow[k]]) for k in range(nb))
    rr, bb = np.nonzero(merged)
    return dict(used=used, per_rank=per_rank, per_rank_ranges=[ranges_of(h) for h in per_rank], merged=merged,
                cell_rows=used[rr], cell_bins=bb, cell_counts=merged[rr, bb], ranges=ranges, rowmax=rowmax, width=width,
                largest=largest, words32=words32, cls=cls, words=words, P=P, total=total, brow=brow, bmax=bmax,
                occupied=width > 0, rows_8bit=int(((width > 0) & (cls == 8)).sum()) if words32 else 0,
                rows_16bit=int(((width > 0) & (cls == 16)).sum()) if words32 else 0,
                packed_cells=int(width.sum()), cell_bytes=4 if words32 else 8,
                padded_words=nranks * bmax if plan == "reduce_scatter" else total)


def self_check(case, sc, X):
    """The rows are what the case says they are (numpy on the oracle's rows; no GPU, no library)."""
    nranks, cls, width, ranges = sc.nranks, X["cls"], X["width"], X["ranges"]
    row_of = {int(u): k for k, u in enumerate(X["used"])}
    if case == "A":
        n = len(A_COUNTS[nranks])
        fields = set()
        for p in range(4):
            for ci, c in enumerate(A_COUNTS[nranks]):
                row = p * n + ci
                hot, k = sc.bins[(row, "hot")], row_of[row]
                assert ranges[row, 0] == sc.bins[(row, "lo")] and width[row] == 10
                assert all(int(h[k, hot]) == c for h in X["per_rank"]) and int(X["merged"][k, hot]) == nranks * c
                assert int(X["rowmax"][row]) == c and int(cls[row]) == A_CLASS[nranks][ci], (row, c, cls[row])
                f = (hot - ranges[row, 0]) % 4
                fields.add((ci, f))
                word = hot - f                             # the other fields of the hot cell's 4-cell word: 1, 0 and 2
                assert sorted(int(X["merged"][k, word + q]) for q in range(4) if q != f) == [0, 1, 2]
        assert fields == {(ci, f) for ci in range(n) for f in range(4)}
        assert {nranks * c for c in A_COUNTS[nranks]} & {255, 256, 65535, 65536} and len(set(cls[:4 * n])) == 3
        for k, holder in enumerate((nranks - 1, 0)):
            row = 4 * n + k
            hot = sc.bins[(row, "hot")]
            held = [int(h[row_of[row], hot]) for h in X["per_rank"]]
            assert held[holder] == A_MAX_ONLY[nranks] and sum(held) == held[holder] <= 255 and int(cls[row]) == 16
        assert width[4 * n + 2] == 0
        pr = X["per_rank_ranges"]
        k = row_of[4 * n + 3]
        assert [tuple(pr[r][k]) == EMPTY for r in range(nranks)] == [r == 1 for r in range(nranks)]
        return
    if case.startswith("B"):
        seen = {}
        for row, k in row_of.items():
            lo, hi, c = sc.bins[(row, "lo")], sc.bins[(row, "hi")], sc.bins[(row, "cls")]
            assert tuple(ranges[row]) == (lo, hi) and int(cls[row]) == c, (row, ranges[row], lo, hi, cls[row], c)
            if hi > lo:                                    # the merged window is one no rank has
                assert all(tuple(rg[k]) != (lo, hi) for rg in X["per_rank_ranges"]), row
            seen.setdefault(c, set()).add((int(width[row]), lo % 4))
        for c in (8, 16, 32):
            assert {w for w, _ in seen[c]} == set(WIDTHS) and {m for _, m in seen[c]} == {0, 1, 2, 3}, (c, seen[c])
        assert X["words32"] != sc.dirty
        if sc.M >= 2048:
            assert all(width[r] > 0 for r in (0, 1023, 1024, 2047, sc.M - 1)) and int(X["occupied"].sum()) == len(_b_rows())
        else:
            assert sc.M < 2048
        return
    sub = case
    assert sc.nranks == 4 and X["largest"] == C_PAIRS[sub] and X["cell_bytes"] == C_CELL_BYTES[sub]
    assert [sc.samples(r) for r in range(4)] == ([C_PAIRS[sub]] * 4 if sub != "C3" else [1, 1, 1, C_PAIRS[sub]])
    hot = int(X["merged"][row_of[C_HOT[0]]].max())
    assert hot == {"C1": (1 << 32) - 4, "C2": 1 << 32, "C3": (1 << 30) + 1}[sub]


def boundary_check(sc, X):
    """reduce-scatter: an owner block starts directly before a crafted narrow row, and one directly after such a row"""
    narrow = X["occupied"] & (X["cls"] < 32) & X["words32"]
    inner = X["brow"][1:-1]
    assert any(0 < b < sc.M and narrow[b] for b in inner), (sc.name, X["brow"])
    assert any(0 < b <= sc.M and narrow[b - 1] for b in inner), (sc.name, X["brow"])


# ---- the merge itself ------------------------------------------------------------------------------------------------------
def feed(sc, engines, torch):
    """every rank's pairs into its engine; returns the seconds the device-fed form took (0 for host submits)"""
    if sc.expand:
        for r, e in enumerate(engines):
            ids, v = sc.pairs(r)
            if ids.size:
                e.submit_pairs(ids, v)
        return 0.0
    # Case C: ONE device buffer of 2^24 constant pairs, submitted until the rank has its count; the few other pairs go in
    # small buffers of their own
    d_ids = torch.full((C_BUF,), C_HOT[0], dtype=torch.int32, device="cuda")
    d_v = torch.full((C_BUF,), C_HOT[1], dtype=torch.float64, device="cuda")
    keep = []                                              # (the small buffers live until the device is done with them)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r, e in enumerate(engines):
        for row, value, count in sc.cells[r]:
            if (row, value) == C_HOT:
                left = count
                while left:
                    n = min(left, C_BUF)
                    e.submit_pairs_device(d_ids, d_v, n=n)
                    left -= n
            else:
                assert count == 1
                keep.append((torch.tensor([row], dtype=torch.int32, device="cuda"),
                             torch.tensor([value], dtype=torch.float64, device="cuda")))
                e.submit_pairs_device(*keep[-1])
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(case, sc, plan, stub):
    import torch
    import loghisto_amd
    import oracle
    from loghisto_amd import merge
    nranks, M = sc.nranks, sc.M
    t_start = time.perf_counter()
    X = expected(sc, plan)
    self_check(case, sc, X)
    if plan == "reduce_scatter" and case.startswith("B") and not sc.dirty:
        boundary_check(sc, X)
    narrow_engine = os.environ.get("LH_TEST_CELL_BITS", "0") == "32"

    # the torch front end's restatement of the same rules gives the same classes, words and owner blocks
    bits = merge.row_bits(torch.from_numpy(X["rowmax"]), nranks, 0xffffffff if sc.dirty else X["largest"]).numpy()
    assert np.array_equal(bits, X["cls"] if X["words32"] else np.full(M, 64)), (bits, X["cls"])
    W = merge.plan_windows(torch.from_numpy(X["ranges"].astype(np.int32)), nranks, plan, torch.from_numpy(bits))
    assert np.array_equal(W["words"].numpy(), X["words"]) and W["total"] == X["total"] and W["bmax"] == X["bmax"]
    if plan == "reduce_scatter":
        assert [int(b) for b in W["brow"]] == X["brow"], (W["brow"], X["brow"])

    comms = (C.c_void_p * nranks)()
    assert stub.stub_comm_create(nranks, comms) == 0
    engines = [loghisto_amd.Engine(max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16) for _ in range(nranks)]
    feed_s = feed(sc, engines, torch)
    snaps = [e.flip() for e in engines]
    if sc.dirty:   # (a cell rank 0 already holds: its ranges stay as they are)
        row, value, _ = sc.cells[0][0]
        b = int(oracle.key_to_bin(oracle.compress(value)))
        snaps[0].mark_dirty(row, 1, b, b)
    results, errors = [None] * nranks, []

    def rank_main(r):
        try:
            results[r] = snaps[r].merge_rccl(comms[r], nranks, r, M, plan=plan)
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))

    t0 = time.perf_counter()
    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errors, errors
    assert all(not t.is_alive() for t in th), "a rank never left the collective"
    merge_s = time.perf_counter() - t0

    covered = []
    for r in range(nranks):
        first, last = results[r]
        want_own = (X["brow"][r], X["brow"][r + 1]) if plan == "reduce_scatter" else (0, M)
        assert (first, last) == want_own, (sc.name, r, results, X["brow"])
        covered.extend(range(first, last))
        snap = snaps[r]
        info = snap.merge_info()
        for k in ("packed_cells", "cell_bytes", "rows_8bit", "rows_16bit", "padded_words"):
            assert info[k] == X[k], (sc.name, r, k, info, X[k])
        assert info["packed_words"] == X["total"], (sc.name, r, info, X["total"])
        assert info["occupied_rows"] == int(X["occupied"].sum()) and info["widest_row"] == int(X["width"].max()), info
        assert info["send_bytes"] == X["cell_bytes"] * (X["padded_words"] if plan == "reduce_scatter" else X["total"]), info
        # a narrow store holds the merged cells while the wire word is uint32; on the uint64 wire it has moved to uint64 cells
        assert snap.device_cells()[2] == (4 if narrow_engine and X["words32"] else 8), (sc.name, snap.device_cells())
        torch.cuda.synchronize()
        got_ranges = merge.snapshot_ranges(snap, M).cpu().numpy().view(np.uint32)
        assert np.array_equal(got_ranges.astype(np.int64), X["ranges"]), (sc.name, r)
        if last > first:
            # every cell of every owned row
            off, keys, counts = snap.buckets_all(last - first, first=first)
            rows = first + np.repeat(np.arange(last - first), np.diff(off.astype(np.int64)))
            bins = oracle.key_to_bin(keys)
            order = np.lexsort((bins, rows))
            sel = (X["cell_rows"] >= first) & (X["cell_rows"] < last)
            got = np.stack([rows[order], bins[order], counts[order].astype(np.int64)], axis=1)
            want = np.stack([X["cell_rows"][sel], X["cell_bins"][sel], X["cell_counts"][sel].astype(np.int64)], axis=1)
            if got.shape != want.shape or not np.array_equal(got, want):
                gs, ws = {tuple(x) for x in got.tolist()}, {tuple(x) for x in want.tolist()}
                raise AssertionError(f"{sc.name} rank {r}: merged cells (row, bin, count) differ: "
                                     f"got only {sorted(gs - ws)[:12]}, want only {sorted(ws - gs)[:12]}")
            st = snap.extract([0.0, 0.5, 1.0], last - first, first=first)
            want_count = np.zeros(M, dtype=np.uint64)
            want_count[X["used"]] = X["merged"].sum(axis=1)
            assert np.array_equal(np.asarray(st["count"]).astype(np.uint64), want_count[first:last]), (sc.name, r)
            for k, m in enumerate(X["used"]):
                if first <= m < last:
                    ref = oracle.process_dense(X["merged"][k], [0.0, 0.5, 1.0])
                    assert np.array_equal(st["pkeys"][m - first], ref["pkeys"]), (sc.name, r, int(m))
    # the owned blocks tile [0, M): no row goes unchecked
    assert sorted(covered) == sorted(list(range(M)) * (nranks if plan == "allreduce" else 1)), sc.name
    for s in snaps:
        s.release()
    for e in engines:
        e.close()
    stub.stub_comm_destroy(nranks, comms)
    return dict(name=sc.name, nranks=nranks, rows=M, cell_bytes=X["cell_bytes"], rows_8bit=X["rows_8bit"],
                rows_16bit=X["rows_16bit"], packed_cells=X["packed_cells"], packed_words=X["total"], brow=X["brow"],
                feed_s=round(feed_s, 3), merge_s=round(merge_s, 3), total_s=round(time.perf_counter() - t_start, 3))


def main():
    case, plan = sys.argv[1], sys.argv[2]
    assert case in CASES and plan in ("allreduce", "reduce_scatter"), sys.argv
    from loghisto_amd import _native as N
    stub_path = os.path.join(ROOT, "loghisto_amd", "build", "librccl_stub.so")
    N.check(N.lib().lh_set_rccl_library(stub_path.encode()), "lh_set_rccl_library")
    stub = C.CDLL(stub_path)
    out = [run(case, sc, plan, stub) for sc in scenarios(case)]
    print(json.dumps({"ok": True, "case": case, "plan": plan, "cell_bits": os.environ.get("LH_TEST_CELL_BITS", "0"),
                      "merges": out}))


if __name__ == "__main__":
    main()
