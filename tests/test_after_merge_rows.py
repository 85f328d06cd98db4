"""tests/_after_merge_driver.py's scenarios without a GPU: the intervals are what their descriptions claim, the reduce-scatter
of rs_wave gives both ranks a block the wave shape of k_unpack_rows takes, and tests/_span_contract's judge is clean on the
model's merged store and names an unpack-style stray (oracle cells, numpy and torch on the CPU only)."""
import numpy as np

from tests import _after_merge_driver as a
from tests import _span_contract as sc


def test_life_intervals_are_what_they_claim():
    """The single-holder row, the row rank 1 lacks, the rows nobody holds, the windows that end at bin 65 535 and start at bin 0,
    every lo % 4 at every class, another class in I2 than in I1 for every row below 40, the cell of 2^32 + 5, the empty intervals
    and five different plans in a row."""
    X = a.self_check_life()
    assert [k for k, iv in a.life_intervals().items() if iv.merged] == ["I1", "I2", "I3", "I4", "I5"]
    assert (X["I1"].info["cell_bytes"], X["I4"].info["cell_bytes"], X["I5"].info["cell_bytes"]) == (4, 8, 4)


def test_rs_wave_blocks_reach_the_wave_shape():
    import torch
    from loghisto_amd import merge
    X = a.self_check_wave()
    sc_ = a.wave_interval()
    bits = merge.row_bits(torch.from_numpy(X.rowmax), sc_.nranks, X.largest)
    assert np.array_equal(bits.numpy(), X.cls)
    W = merge.plan_windows(torch.from_numpy(X.merged_ranges.astype(np.int32)), sc_.nranks, "reduce_scatter", bits)
    brow = [int(b) for b in W["brow"]]
    assert brow == X.brow == [0, 2100, 4200], (brow, X.brow)
    assert min(b - f for f, b in zip(brow, brow[1:])) >= a.WAVE_MIN_BLOCK == 2048
    assert np.array_equal(W["words"].numpy(), X.words) and W["total"] == X.total


def test_the_judge_on_the_models_merged_store():
    """check_planted is clean on what the merge must leave (I1's 72 rows), and a cell one past a merged row's hi -- what an unpack
    that stores w + 1 cells, or starts at lo + 1, leaves -- is named as an S violation at that row and bin."""
    X = a.model(a.life_intervals()["I1"], "allreduce")
    store, ranges = a.merged_store(X, a.LIFE_M)
    rec = sc.check_planted(store, ranges)
    sc.assert_contract(rec)
    assert not rec.violations and int(rec.nnz.sum()) == X.merged.key.size
    assert np.array_equal(rec.total, store.sum(axis=1)) and np.array_equal(rec.ranges, X.merged_ranges)
    for row in (5, a.LACKS1, a.BOTTOM):
        hi = int(ranges[row, 1])
        planted = store.copy()
        planted[row, hi + 1] = 3
        rec = sc.check_planted(planted, ranges)
        assert rec.violations == [("S", row, hi + 1, 3)] and int(rec.nstray.sum()) == 1 and not rec.npad.any()
        try:
            sc.assert_contract(rec)
        except AssertionError as exc:
            assert f"row {row} bin {hi + 1} = 3" in str(exc)
        else:
            raise AssertionError("a stray cell passed the contract")
    planted = store.copy()                                     # the window that ends at bin 65 535: one past it is a padding cell
    planted[a.TOP, a.NKEYS] = 1
    rec = sc.check_planted(planted, ranges)
    assert rec.violations == [("P", a.TOP, a.NKEYS, 1)]
