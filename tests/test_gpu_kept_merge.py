"""lh_kept_merge (Kept.merge): kept intervals rolled up into ONE kept handle -- exactly what lh_keep would return for a
snapshot whose cells are C[b] = the sum over the listed handles of c_i[b], in 64 bits.

The inputs are the crafted handles of tests/test_gpu_kept.py (70 rows, 6 handles, engines of 64- and of 32-bit cells: cells
either side of every tile edge in different handles, more than 64 entries of one handle in one tile, eight tiles, an empty
stretch between tiles, bins 0 and 65 535, rows no handle has, counts of 2^32 - 1 summed, a cell of 2^33, a total of 2^64 - 1,
a cell that wraps to 0 when its handle is listed twice, more rows than a workgroup has waves).  The model is Python integers
over the fixture's rows: per row the union of the bins, sums mod 2^64, zero sums dropped, ascending by bin, as the CSR arrays
lh_buckets_all would hand out.  Every check runs under both kernel shapes (lh_tool_kept_switch).
No test here can put handles on different devices with one GPU: that LH_EINVAL is not covered."""
import contextlib

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_across import P_MAIN
from tests.test_gpu_compare import rows_of
from tests.test_gpu_count_le import engine
from tests.test_gpu_kept import LISTS, arrays_of, call, crafted, same_listing, shape  # noqa: F401  (crafted: the fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
WRAP = 1 << 64
KINDS = ("wave", "block")
_MODEL = {}


def summed(c, lst, first=0, n=None):
    """Per row of [first, first + n): ({bin: C[b] mod 2^64, zeros dropped}, whether some cell passed 2^64)."""
    n = c.M - first if n is None else n
    key = (c.wide, tuple(lst))
    if key not in _MODEL:
        out = []
        for m in range(c.M):
            cells = {}
            for i in lst:
                for b, x in c.rows[i][m].items():
                    cells[b] = cells.get(b, 0) + x
            out.append(({b: x % WRAP for b, x in cells.items() if x % WRAP}, any(x >= WRAP for x in cells.values())))
        _MODEL[key] = out
    return _MODEL[key][first:first + n]


def listing(rows):
    """[{bin: count}] as lh_buckets_all's (offsets, keys, counts)."""
    off = np.zeros(len(rows) + 1, dtype=U64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=U64)
    bins = np.array([b for r in rows for b in sorted(r)], dtype=np.int64)
    counts = np.array([r[b] for r in rows for b in sorted(r)], dtype=U64)
    return [off, oracle.bin_to_key(bins).astype(np.int16) if bins.size else np.zeros(0, dtype=np.int16), counts]


def model(c, lst, first=0, n=None):
    return listing([r for r, _ in summed(c, lst, first, n)])


def merge(handles, **kw):
    return handles[-1].merge(handles[:-1], **kw)


def merged(stack, c, lst, **kw):
    return stack.enter_context(merge([c.kept[i] for i in lst], **kw))


def bytes_of(k):
    return [a.tobytes() for a in arrays_of(k)]


# ---- 1. the arrays -----------------------------------------------------------------------------------------------------------
def test_arrays_against_the_model_in_both_shapes(crafted):
    c = crafted
    got = {}
    with contextlib.ExitStack() as stack:
        for kind in KINDS:
            with shape(kind):
                for lst in LISTS:
                    k = merged(stack, c, lst)
                    same_listing(k, model(c, lst), (kind, lst[:8], len(lst)))
                    assert k.info["first"] == 0 and k.info["device"] == 0
                    got[kind, tuple(lst)] = bytes_of(k)
        for lst in LISTS:
            assert got["wave", tuple(lst)] == got["block", tuple(lst)], lst[:8]
        # what the crafted rows were made for
        m = c.at["half_of_2^64"]
        twice, once = summed(c, [3, 3])[m], summed(c, [3])[m]
        assert once[0] == {100: 1 << 63, 300: 7} and twice == ({300: 14}, True)          # the cell wrapped to 0: not listed
        assert summed(c, [0, 1])[c.at["two_cells_of_2^32-1"]][0] == {500: 0x1fffffffe}
        assert summed(c, [3])[c.at["total_2^64-1"]][0] == {100: (1 << 63) - 1, 200: 1 << 63}
        assert len(summed(c, list(range(6)))[c.at["dense300"]][0]) == 300 and not summed(c, list(range(6)))[c.at["never"]][0]


# ---- 2. reading the merged handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reading_the_merged_handle_equals_reading_the_list(crafted, kind):
    c = crafted
    with shape(kind), contextlib.ExitStack() as stack:
        for lst in LISTS:
            what = (kind, lst[:8], len(lst))
            one = merged(stack, c, lst).across((), P_MAIN)
            many = call(c, lst)
            for f in ("count", "nbuckets", "pkeys", "pvalid"):
                assert one[f].tobytes() == many[f].tobytes(), (what, f)
            # The float walk is fixed by the set of the row's non-zero bins: they decide where each tile starts, so which
            # lane weighs which bin and in what order the terms are added.  A cell whose sum passed 2^64 can leave that set on
            # one side only (wrapped to 0 it is still an entry of the listed handles, where the reader's tile may start, and
            # no entry of the merged one), so such rows are left out of this comparison -- and of no other.
            exact = np.array([not wrapped for _, wrapped in summed(c, lst)])
            assert exact.sum() >= c.M - 3
            assert one["sum"][exact].tobytes() == many["sum"][exact].tobytes(), what
            assert np.array_equal(one["present_bits"], (one["count"] > 0).astype(U64)), what


# ---- 3. blocks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_blocks(crafted, kind):
    import loghisto_amd
    c = crafted
    sub, sub_rec = c.extra["sub"]
    last, last_rec = c.extra["last"]
    with shape(kind), contextlib.ExitStack() as stack:
        k = merged(stack, c, [0], first=3, nmetrics=5)                            # nkept == 1 with a sub-block: a slice
        same_listing(k, sub_rec, "slice")
        assert bytes_of(k) == bytes_of(sub) and k.info == sub.info
        k = merged(stack, c, [0], first=c.M - 1)                                  # nmetrics=None: up to the end of the block
        same_listing(k, last_rec, "the last row")
        assert bytes_of(k) == bytes_of(last) and k.info == last.info
        k = merged(stack, c, [0])                                                 # ... with the full block: a copy
        assert bytes_of(k) == bytes_of(c.kept[0]) and k.info == c.kept[0].info
        k = stack.enter_context(sub.merge())                                      # first=None: the handle's own
        assert bytes_of(k) == bytes_of(sub) and k.info == sub.info
        k = merged(stack, c, list(range(6)), first=c.at["never"], nmetrics=2)     # rows without a cell in any handle
        assert k.info["cells"] == 0 and k.info["samples"] == 0 and k.info["bytes"] == 8 * 3 + 8 * 2
        assert k.info["first"] == c.at["never"] and k.info["nrows"] == 2
        assert [int(x) for x in arrays_of(k)[0]] == [0, 0, 0] and [int(x) for x in arrays_of(k)[3]] == [0, 0]
        both = [sub, c.kept[1]]                                                   # blocks [3, 8) and [0, M)
        k = stack.enter_context(merge(both, first=3, nmetrics=5))
        same_listing(k, model(c, [0, 1], 3, 5), "a sub-block handle in the list")
        assert k.info["first"] == 3
        for first, n in ((2, 5), (3, 6)):
            with pytest.raises(loghisto_amd.LhError) as ei:
                merge(both, first=first, nmetrics=n)
            assert ei.value.code == N.ERANGE, (first, n)


# ---- 4. hierarchy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_merge_of_merges_is_the_merge_of_all(crafted, kind):
    c = crafted
    with shape(kind), contextlib.ExitStack() as stack:
        ab, cd = merged(stack, c, [0, 1]), merged(stack, c, [2, 3])
        top = stack.enter_context(merge([ab, cd]))
        flat = merged(stack, c, [0, 1, 2, 3])
        assert bytes_of(top) == bytes_of(flat) and top.info == flat.info
        same_listing(top, model(c, [0, 1, 2, 3]), kind)


# ---- 5. independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_merged_handle_outlives_its_inputs(crafted, kind):
    c = crafted
    M, n = 9, 4000
    rng = np.random.default_rng(77)
    kept, rows = [], []
    with shape(kind):
        with engine(M, cell_bits=32) as e:
            for i in range(3):
                e.submit_pairs(rng.integers(0, M - 1, n).astype(np.uint32), rng.lognormal(3.0 + i, 1.0, n))   # the last name: none
                with e.flip() as s:
                    rows.append(rows_of(s, M))
                    kept.append(s.keep(M))
            before = [bytes_of(k) for k in kept]
            out = merge(kept)
            assert [bytes_of(k) for k in kept] == before                          # only read
        want = listing([{b: sum(r[m].get(b, 0) for r in rows) for b in set().union(*[r[m] for r in rows])} for m in range(M)])
        same_listing(out, want, "before the inputs are closed")
        assert out.info["samples"] == 3 * n
        held = bytes_of(out)
        for k in kept:
            k.close()                                                             # the engine is gone already
        with merge([c.kept[0], c.kept[1]]):                                       # other allocations come and go
            assert bytes_of(out) == held
        same_listing(out, want, "after the inputs were closed")
        out.close()
    for k, rec in zip(c.kept, c.recs):                                            # the fixture's handles, after all merges so far
        same_listing(k, rec, "an input of a merge")


# ---- 6. the arrays are a well-formed CSR for the importer ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_add_to_a_fresh_snapshot_gives_the_model(crafted, torch_cuda, kind):
    c, lst = crafted, [0, 1, 2]
    with shape(kind), contextlib.ExitStack() as stack:
        k = merged(stack, c, lst)
        with engine(c.M, cell_bits=64) as e, e.flip() as snap:
            k.add_to(snap)
            torch_cuda.cuda.ExternalStream(snap.stream()).synchronize()
            assert rows_of(snap, c.M) == [r for r, _ in summed(c, lst)]
