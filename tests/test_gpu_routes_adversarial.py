"""Threshold-adjacent and special values (tests/_adversarial_values.py) through every ingest route, cell for cell against the
oracle.  Every sample of the threshold classes takes the kernels' exact decision (lh_codec.h: lh_bin_of's table compare,
lh_bin_fast plus fix-up), which is inlined into each kernel's own control flow:

  K1 (k_ingest_single)            the 64-sample survey, the unrolled full-wave body with its aggregated add, the guarded
                                  remainder pairs, the scalar head, the scalar tail
  SMALL (lh_kernels_small.hip)    the window add and the miss path
  DIRECT                          the cell table (k_scatter_clustered on its own, three configurations) and kp_add
                                  (k_ingest_pairs: calls below a tile, the rest behind the tiles, engines past 65 536 names)
  GEN1 (lh_kernels_part.hip)      one and two scatter levels

A wrong decision moves one count between two adjacent cells: every case compares the full dense row, or every occupied
(name, bin) cell of every row, and the counts; percentile keys and values are bit-identical.  Every case asserts the
`samples_*` counter of the route it means to take.  The second and third generation take the same classes through
tests/test_gpu_part2.py and tests/test_gpu_part3.py (the fixture tests there).
Reference semantics: Histogram(name, v) = histogramCache[name][compress(v)] += 1, metrics.go:273-295, 316-322."""
import functools

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests import _adversarial_values as av
from tests.test_gpu_key_edges import MBIG, _fresh, big_engine  # noqa: F401  (big_engine: the fixture, built once for this module)
from tests.test_gpu_parity import check_stats
from tests.test_gpu_part3 import PCTS, check

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    a = np.array(a)                                  # (a copy: the shared inputs are read-only, torch wants writable memory)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


@functools.lru_cache(maxsize=None)
def plain(order, odd):
    """The full set (weighted: 1 .. 3 copies of each threshold's neighbourhood, so that a shift across every threshold cannot
    cancel within the one row) in one of the two plain orders, with n odd or even; read-only."""
    v = av.sorted_by_key(av.weighted_set()) if order == "sorted_by_key" else av.shuffled(av.weighted_set())
    if (v.size & 1) != odd:
        v = av.drop_middle(v)
    assert (v.size & 1) == odd
    v.setflags(write=False)
    return v


def _moved(before, after):
    return {k: after[k] - before[k] for k in after if k.startswith("samples_") and isinstance(after[k], int) and after[k] != before[k]}


# ---- K1 ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def k1(native_lib, torch_cuda):
    import loghisto_amd
    with loghisto_amd.Engine(max_metrics=1, num_buffers=2, num_lanes=1, lane_samples=1 << 16) as e:
        yield e


def k1_check(e, launches, want_row, n):
    """launches: callables that submit; the interval must then hold exactly want_row."""
    before = e.counters()
    for go in launches:
        go()
    e.sync()
    assert _moved(before, e.counters()) == {"samples_single": n}
    with e.flip() as snap:
        row = snap.dense_row(0)
        got = snap.extract(PCTS, 1)
    if not np.array_equal(row, want_row):
        bad = np.nonzero(row != want_row)[0]
        raise AssertionError(f"{bad.size} cells differ, e.g. " + ", ".join(
            f"key {int(oracle.bin_to_key(b))}: {int(row[b])} != {int(want_row[b])}" for b in bad[:6]))
    assert int(got["count"][0]) == n
    check_stats(want_row, got, pcts=PCTS)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("order", ["sorted_by_key", "shuffled"])
def test_k1_plain_orders(k1, torch_cuda, order, odd, offset):
    """sorted: narrow tiles, two copies of a window that follows the stream.  shuffled: WIDE mode, both floating windows, the
    global row.  [1:] is 8-byte aligned only: the scalar head, and the other parity of what is left for the scalar tail.  Head
    and tail samples are exact thresholds (tests/test_adversarial_values.py)."""
    v = plain(order, odd)
    d = _dev(torch_cuda, v)
    assert d.data_ptr() % 16 == 0
    k1_check(k1, [lambda: k1.submit_device(0, d[offset:])], oracle.histogram_dense(v[offset:]), v.size - offset)


@pytest.mark.parametrize("seed", [None, 7], ids=["ascending", "runs_shuffled"])
@pytest.mark.parametrize("shape", sorted(av.WAVE_SHAPES))
def test_k1_aggregated_fullwave_add(k1, torch_cuda, shape, seed):
    """One k1_add_fullwave call per run of 128 samples: lane 0's bucket added as a count of 40 lanes, of exactly 24 (the
    minimum that aggregates), of 23 (not aggregated) or of all 64, while the other lanes' buckets differ from it only through the
    exact decision at V[j] against the double below it.  Ascending runs stay inside the window that follows the stream;
    shuffled runs send aggregated counts to the floating windows and the global row."""
    v, uniq, mult = av.wave_blocks(av.wave_subset(), shape, seed)
    d = _dev(torch_cuda, v)
    assert d.data_ptr() % 16 == 0 and v.size >= 8192 * 200                    # full tiles: the unrolled body
    k1_check(k1, [lambda: k1.submit_device(0, d)], av.row_of(uniq, mult), v.size)


@pytest.mark.parametrize("around", [4095, 0, 32767])
def test_k1_remainder_loop_alone(k1, torch_cuda, around):
    """Fewer than 8 192 samples: no full tile, the guarded remainder pairs (and head or tail) count everything.  Cut from the
    sorted set around keys 4095 | 4096, 0 and 32767."""
    s = plain("sorted_by_key", 0)
    keys = av.expected(s)
    mid = int(np.searchsorted(keys, around, side="right"))
    lo = max(0, min(mid - 4095, s.size - 8191))
    v = s[lo:lo + 8191]
    assert v.size == 8191 and (av.expected(v) == around).any() and av.is_exact_threshold(v).sum() > 500
    d = _dev(torch_cuda, s)
    k1_check(k1, [lambda: k1.submit_device(0, d[lo:lo + 8191])], oracle.histogram_dense(v), v.size)


def test_k1_two_launches_into_one_interval(k1, torch_cuda):
    v = plain("shuffled", 1)
    d = _dev(torch_cuda, v)
    k1_check(k1, [lambda: k1.submit_device(0, d)] * 2, 2 * oracle.histogram_dense(v), 2 * v.size)


def test_k1_through_host_staging(k1):
    """lh_submit: lanes of 65 536 samples, i.e. many launches of exactly eight tiles and one ragged one."""
    v = plain("shuffled", 1)
    k1_check(k1, [lambda: k1.submit(0, v)], oracle.histogram_dense(v), v.size)


# ---- mixed routes ------------------------------------------------------------------------------------------------------

def mixed_check(e, M, ids, v, submit, path):
    before = e.counters()
    submit()
    e.sync()
    moved = _moved(before, e.counters())
    assert moved == {path: v.size}, (path, moved)
    with e.flip() as snap:
        got = snap.extract(PCTS, M)
        assert int(got["count"].sum()) == v.size
        check(snap, ids, v, M, got)


def _engine(M, opts=None):
    import loghisto_amd
    e = loghisto_amd.Engine(max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
    for k, val in (opts or {}).items():
        e.set_option(k, val)
    return e


ROUTES = [
    # names, options, counter that must move by the call's size
    pytest.param(20, {}, "samples_small", id="small-20"),
    pytest.param(5, {}, "samples_small", id="small-5"),
    pytest.param(700, {}, "samples_direct", id="direct-cell-table"),
    pytest.param(1000, {N.OPT_PART_MIN_PAIRS: 1 << 17, N.OPT_PART_V2: 0}, "samples_partitioned", id="gen1-one-level"),
    pytest.param(30000, {N.OPT_PART_MIN_PAIRS: 1 << 17, N.OPT_PART_V3: 0}, "samples_partitioned", id="gen1-two-levels"),
]


@pytest.mark.parametrize("M,opts,path", ROUTES)
def test_mixed_route_device_resident(native_lib, torch_cuda, M, opts, path):
    v = av.full_set()
    ids = av.with_ids(v, M)
    d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
    with _engine(M, opts) as e:
        mixed_check(e, M, ids, v, lambda: e.submit_pairs_device(d_ids, d_v), path)


@pytest.fixture(scope="module")
def direct700(native_lib, torch_cuda):
    with _engine(700) as e:
        yield e


def test_cell_table_uint16_ids(direct700, torch_cuda):
    v = av.full_set()
    ids = av.with_ids(v, 700)
    d_ids, d_v = _dev(torch_cuda, ids.astype(np.uint16)), _dev(torch_cuda, v)
    mixed_check(direct700, 700, ids, v, lambda: direct700.submit_pairs_device(d_ids, d_v), "samples_direct")


def test_cell_table_odd_offset_slice(direct700, torch_cuda):
    """[1:] of both arrays: the first pair is peeled off into k_ingest_pairs (lh::peel_first), the rest is aligned again."""
    v = av.full_set()
    ids = av.with_ids(v, 700)
    d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
    assert d_ids.data_ptr() % 8 == 0 and d_v.data_ptr() % 16 == 0 and av.is_exact_threshold(v[1:2]).all()
    mixed_check(direct700, 700, ids[1:], v[1:], lambda: direct700.submit_pairs_device(d_ids[1:], d_v[1:]), "samples_direct")


def test_plain_atomics_below_a_table_tile(direct700, torch_cuda):
    """999 pairs: fewer than the cell table's smallest tile, k_ingest_pairs (kp_add) counts them all."""
    thr = av.values()["thresholds"]
    v = np.ascontiguousarray(thr[::425][:999])                                # 425 % 3 == 2: prev, V[j] and next all occur
    assert v.size == 999 and av.is_exact_threshold(v).sum() > 300 and (v < 0).sum() > 400
    ids = av.with_ids(v, 700)
    d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
    mixed_check(direct700, 700, ids, v, lambda: direct700.submit_pairs_device(d_ids, d_v), "samples_direct")


def test_plain_atomics_past_65536_names(big_engine, torch_cuda):
    """An engine of 66 048 names sends the whole call through k_ingest_pairs (launch_ingest_pairs_cells)."""
    v = np.ascontiguousarray(plain("shuffled", 0)[::10])
    v = v[:100_000]
    assert v.size == 100_000 and av.is_exact_threshold(v).sum() > 10_000
    ids = av.with_ids(v, MBIG)
    assert ids.max() == MBIG - 1
    d_ids, d_v = _dev(torch_cuda, ids), _dev(torch_cuda, v)
    _fresh(big_engine)
    mixed_check(big_engine, MBIG, ids, v, lambda: big_engine.submit_pairs_device(d_ids, d_v), "samples_direct")


@pytest.mark.parametrize("form", ["submit_pairs", "reserve_commit"])
def test_host_fed_pairs(direct700, form):
    """The copying form and reserve / commit in place: half-buffers of 65 536 pairs through the cell table's small
    configuration (1 024-pair tiles, 4 096 slots), the last one ragged."""
    v = av.full_set()
    ids = av.with_ids(v, 700)
    submit = direct700.submit_pairs if form == "submit_pairs" else direct700.submit_pairs_in_place
    mixed_check(direct700, 700, ids, v, lambda: submit(ids, v), "samples_direct")
