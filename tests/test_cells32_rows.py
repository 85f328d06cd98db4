"""The crafted rows of tests/test_gpu_cells32_readers.py (tests/_cells32_rows.py) reach every path they are meant for.

No GPU: the routing predicate of k_extract_wave<uint32_t> (lh_kernels.hip: a span stays in registers as 32-bit cells iff
hi - lo < 1 024 and every cell is below 2^22; the two-pass loop otherwise) and the branches of uint64(float64)
(d_f64_to_u64_amd64, lh_expand_compact) are restated in _cells32_rows.py, and this file asserts that the generator's
output holds a row for each combination a reader can get wrong -- so that a change of the generator cannot quietly drop
one."""
import numpy as np
import pytest

import oracle
from tests import _cells32_rows as R

M = 2400


@pytest.fixture(scope="module")
def rows():
    return R.make_rows(M)


def test_rows_are_deterministic_sparse_and_fit_the_cells(rows):
    R._CACHE.clear()
    again = R.make_rows(M)
    assert len(rows) == len(again) == M
    for a, b in zip(rows, again):
        assert a.kind == b.kind and a.span == b.span and np.array_equal(a.bins, b.bins) and np.array_equal(a.counts, b.counts)
    for r in rows:
        assert r.counts.size == 0 or (1 <= int(r.counts.min()) and int(r.counts.max()) <= R.U32), r.kind
        assert np.all(np.diff(r.bins) > 0)
        if r.bins.size:                                    # the span that is marked is the tight one
            assert r.span == (int(r.bins[0]), int(r.bins[-1])), r.kind
    # the special rows lie where both extract kernels read them (extract(P, 1500, first=100))
    special = [m for m, r in enumerate(rows) if not r.kind.startswith("f_") and m]
    assert min(special) == R.FIRST_SPECIAL and max(special) < 1600


def test_each_route_at_each_alignment_and_each_last_group(rows):
    seen = {(R.route(r), r.span[0] % 4, R.last_group(r)) for r in rows if r.span is not None and r.bins.size}
    for rt in ("reg", "loop"):
        for align in range(4):
            for g in range(4):                             # g == 0: the last group starts AT hi; 1, 2: it straddles hi
                assert (rt, align, g) in seen, (rt, align, g)
    # the cell at hi is occupied in every one of them (tight spans): a reader that skips the last group loses samples
    assert all(int(r.bins[-1]) == r.span[1] for r in rows if r.bins.size)


def test_the_boundary_between_the_registers_and_the_loop(rows):
    by = {}
    for r in rows:
        by.setdefault(r.kind.split("/")[0], []).append(r)
    for c, rt in ((1, "reg"), (R.REG_CELL - 1, "reg"), (R.REG_CELL, "loop"), (1 << 31, "loop"), (R.U32, "loop")):
        got = by[f"one_cell_{c}"]
        assert len(got) == 4 and all(R.route(r) == rt and r.total() == c for r in got)
    assert all(R.route(r) == "reg" and r.total() == (1 << 32) - 1024 and r.span[1] - r.span[0] == 1023 for r in by["reg_max_total"])
    assert all(R.route(r) == "loop" and r.total() == (1 << 32) - 1023 for r in by["reg_max_total_one_cell_up"])
    # cells the registers must not take whose total would wrap a uint32 scan
    assert all(R.route(r) == "loop" and r.total() == 1 << 32 for r in by["span_1024_of_2^22"])
    assert all(R.route(r) == "loop" and r.total() > 1 << 32 and int(r.counts.max()) < 2 * R.REG_CELL for r in by["span_1024_below_2^23"])
    for w in range(1021, 1028):
        got = by[f"span_{w}"]
        assert sorted(r.span[0] % 4 for r in got) == [0, 1, 2, 3]
        assert all(r.span[1] - r.span[0] + 1 == w and R.route(r) == ("reg" if w <= 1024 else "loop") for r in got)
    # the largest total of any row on the register path fits the uint32 scan
    assert max(r.total() for r in rows if R.route(r) == "reg") == (1 << 32) - 1024


def test_the_ends_of_the_key_space(rows):
    tops = [r for r in rows if r.span is not None and r.span[1] == R.NKEYS - 1 and r.bins.size]
    for rt in ("reg", "loop"):
        assert {r.span[0] % 4 for r in tops if R.route(r) == rt} == {0, 1, 2, 3}, rt
    assert any(r.span == (R.NKEYS - 1, R.NKEYS - 1) for r in rows) and any(r.span == (0, 0) for r in rows)
    bottoms = [r for r in rows if r.span is not None and r.span[0] == 0 and r.bins.size > 1]
    assert {R.route(r) for r in bottoms} == {"reg", "loop"}
    full = [r for r in rows if r.bins.size == R.NKEYS]
    assert 1 <= len(full) <= 2


def test_totals_either_side_of_two_to_the_32(rows):
    totals = np.array([r.total() for r in rows], dtype=np.float64)
    assert np.any((totals > 0) & (totals < 2.0 ** 32)) and np.any(totals >= 2.0 ** 32)
    big = [r for r in rows if r.total() >= 1 << 32]
    assert any(r.span[1] - r.span[0] < R.EW_REG for r in big) and any(r.span[1] - r.span[0] >= R.EW_REG for r in big)
    assert any(r.kind.startswith("five_cells_of_2^32-1") and r.total() == 5 * R.U32 and r.span[1] - r.span[0] < 1024 for r in rows)
    assert any(r.kind == "3000_cells_of_2^21" and r.total() == 3000 << 21 and r.span[1] - r.span[0] >= 1024 for r in rows)


def test_empty_rows(rows):
    assert any(r.span is None and r.bins.size == 0 for r in rows)                       # never marked
    zero = [r for r in rows if r.span is not None and r.bins.size == 0]                 # marked, nothing but zeros
    assert {R.route(r) for r in zero} == {"reg", "loop"}
    for r in zero:
        ref = oracle.process_dense(r.dense(), [0.0, 0.5, 1.0])
        assert ref["count"] == 0 and ref["nbuckets"] == 0 and not ref["pvalid"].any() and ref["avg"] != ref["avg"]


def test_every_conversion_branch_by_the_oracles_sum(rows):
    seen = {}
    for r in rows:
        if r.bins.size > 4000:
            continue
        s = oracle.process_dense(r.dense(), [0.5])["sum"]
        br = R.conversion_branch(s)
        seen.setdefault(br, []).append(r.kind)
        assert R.f64_to_u64_model(s) == oracle.f64_to_u64_amd64(s), (r.kind, s)        # the restated branches are the oracle's
    for br in ("0_to_2_63", "2_63_to_2_64", "ge_2_64", "le_minus_2_63", "negative"):
        assert br in seen, br
        assert len(seen[br]) >= 2
    # the model at the edges of the branches
    for s, want in ((R.TWO63, 1 << 63), (float(np.nextafter(R.TWO63, 0)), (1 << 63) - 1024), (R.TWO64, 0),
                    (float(np.nextafter(R.TWO64, 0)), (1 << 64) - 2048), (-R.TWO63, 1 << 63),
                    (float(np.nextafter(-R.TWO63, 0)), (1 << 63) + 1024), (-1.5, (1 << 64) - 1), (-0.0, 0), (float("nan"), 1 << 63)):
        assert R.f64_to_u64_model(s) == want == oracle.f64_to_u64_amd64(s), s
