"""Keeps tests/_adversarial_values.py honest, without a GPU: the value set holds what it claims (every element of the
threshold classes inside lh_bin_fast's guard band, both signs of every key, the recorded Go keys), the stream orders have the
shape K1's code paths need, and the guard band takes the share of an ordinary stream the kernels' comments rely on."""
import math

import numpy as np

import oracle
from tests import _adversarial_values as av


def test_expected_equals_the_recorded_keys():
    x, keys, _ = av.fixture()
    assert x.size == 3 * oracle.KEXT_MAX == 212_934
    thr = av.values()["thresholds"]
    assert thr.size == 2 * x.size
    assert np.array_equal(av.expected(thr[:x.size]), keys)
    neg = (-keys.astype(np.int32)).astype(np.int16)                 # -1 * i in int16 arithmetic, metrics.go:319
    assert np.array_equal(av.expected(thr[x.size:]), neg)
    assert neg[keys == -32768].size and (neg[keys == -32768] == -32768).all()   # ... which wraps at the bottom key


def test_threshold_classes_lie_inside_the_guard_band():
    """The band is +-2 Q14 units ~ +-1.2e-4 bucket ~ 1.2e-6 relative in 1 + |v|; the classes are at most 3 ulp ~ 7e-16 away
    from a threshold."""
    vals = av.values()
    for k in ("thresholds", "near"):
        inside = av.in_guard_band(vals[k])
        assert inside.all(), (k, int((~inside).sum()), vals[k][~inside][:5])
    assert vals["near"].size == 8 * oracle.KEXT_MAX
    # the specials that are not finite are "uncertain" too; an ordinary value in the middle of a bucket is not
    assert av.in_guard_band(np.array([np.nan, np.inf, -np.inf])).all()
    assert not av.in_guard_band(oracle.decompress_table()[[40000, 33000, 20000]]).any()


def test_every_reachable_key_on_both_signs():
    _, keys, _ = av.fixture()
    reached = np.unique(keys)
    x = av.values()["thresholds"]
    half = x.size // 2
    pos, neg = np.unique(av.expected(x[:half])), np.unique(av.expected(x[half:]))
    assert np.array_equal(pos, reached)
    assert np.array_equal(neg, np.unique((-reached.astype(np.int32)).astype(np.int16)))
    both = np.union1d(pos, neg)
    assert both[0] == -32768 and both[-1] == 32767 and both.size == 65536     # every int16 key, thanks to the wrap region


def test_rounding_and_specials_hold_their_cases():
    r = av.values()["rounding"]
    k = av.expected(r)
    assert ((r != 0) & (k == 0)).any()                                        # 1 + v == 1, or below the first threshold
    assert 1.0 + 2.0 ** -53 == 1.0 and 2.0 ** -53 in r and 2.0 ** -1074 in r
    order = np.argsort(r)
    rs, ks = r[order], k[order]
    nb = np.nonzero((np.nextafter(rs[:-1], np.inf) == rs[1:]) & (ks[:-1] != ks[1:]))[0]
    assert nb.size, "no pair of neighbouring doubles with different keys"
    assert (1.0 + np.abs(rs[nb]) != 1.0 + np.abs(rs[nb + 1])).all()           # ... and it is the add's rounding that parts them
    s = av.values()["specials"]
    bits = s.view(np.uint64)
    nan = np.isnan(s)
    quiet = (bits & np.uint64(1 << 51)) != 0
    assert (nan & quiet).sum() == 6 and (nan & ~quiet).sum() == 6             # three payloads, two signs, each
    assert set((bits[nan] & np.uint64((1 << 51) - 1)).tolist()) == {1, 0x7ffffffffffff, 0x2aaaaaaaaaaaa}
    assert (av.expected(s[nan]) == 0).all() and (av.expected(s[np.isinf(s)]) == 0).all()
    assert np.signbit(s[s == 0]).tolist() == [False, True]
    ks = av.expected(s)
    fin = np.isfinite(s)
    for want in (32766, 32767, -32767, -32768):                               # the last in-domain keys and the first wrapped one
        assert (ks[fin] == want).any(), want
    wide = np.abs(s[fin]) >= 3e142
    assert wide.sum() >= 600 and np.unique(ks[fin][wide]).size > 100          # the wrap region lands all over the key space
    assert s[fin].max() == 1.7976931348623157e308 == -s[fin].min()


def test_full_set_fits_below_every_partitioned_threshold():
    n = av.full_set().size
    assert (1 << 19) < n < (1 << 20) - 2                                      # DIRECT by default, and a slice at [1:] too
    assert av.extra_classes().size + 2 * 212_934 == n


def test_a_shift_across_every_threshold_shows_in_one_row():
    """Two wrong decisions modelled on the host -- every +-V[j] one bucket towards zero (x > Tx[j] for x >= Tx[j]), every
    double below a threshold one bucket away from zero -- against the row of the weighted set: nearly every bucket changes.
    In the unweighted set the samples that leave a bucket are replaced by its neighbour's."""
    def rows(v):
        k = av.expected(v).astype(np.int64)
        exact = av.is_exact_threshold(v)
        below = av.is_exact_threshold((v.view(np.uint64) + np.uint64(1)).view(np.float64))
        sign = np.where(np.signbit(v), -1, 1)
        out = []
        for sel, step in ((exact, -1), (below, 1)):
            out.append(np.bincount(oracle.key_to_bin(np.where(sel, k + sign * step, k)), minlength=65536))
        return np.bincount(oracle.key_to_bin(k), minlength=65536), out
    good, wrong = rows(av.weighted_set())
    for w in wrong:
        assert np.count_nonzero(w != good) > 60000
    good, wrong = rows(av.full_set())
    assert max(np.count_nonzero(w != good) for w in wrong) < 1000
    assert np.array_equal(np.unique(av.weighted_set()[np.isfinite(av.weighted_set())]),
                          np.unique(av.full_set()[np.isfinite(av.full_set())]))       # the same values, other multiplicities


def test_plain_orders_end_on_exact_thresholds():
    v = av.weighted_set()
    row = oracle.histogram_dense(v)
    for order in (av.sorted_by_key(v), av.shuffled(v)):
        assert order.size == v.size and np.array_equal(oracle.histogram_dense(order), row)
        assert av.is_exact_threshold(order[[0, 1, -2, -1]]).all()
        fewer = av.drop_middle(order)
        assert fewer.size == v.size - 1 and av.is_exact_threshold(fewer[[0, 1, -2, -1]]).all()
    s = av.sorted_by_key(v)
    assert (np.diff(av.expected(s).astype(np.int32)) >= 0).all()
    # a tile of 8 192 sorted samples spans far fewer than the 7 168 bins up to which K1 keeps two copies of its window ...
    ks = av.expected(s).astype(np.int32)
    assert (ks[8191::8192] - ks[:ks.size - 8191:8192]).max() < 2048
    # ... and a shuffled one far more than the 16 384 of WIDE mode
    kh = av.expected(av.shuffled(v)[:8192]).astype(np.int32)
    assert kh.max() - kh.min() > 60000


def test_wave_blocks_shapes():
    j = av.wave_subset()
    assert j.size >= 10_000 and j[0] == 1 and (np.diff(j) > 0).all()
    key = av.expected(av.threshold_bits()[j - 1].astype(np.uint64).view(np.float64)).astype(np.int64)
    for c in (4095, 4096, -4095, -4096, 32767, -32767, 0):
        assert np.count_nonzero(np.abs(key - c) <= 8) >= 9, c
    for shape, (first, k) in av.WAVE_SHAPES.items():
        for seed in (None, 5):
            v, uniq, mult = av.wave_blocks(j, shape, seed)
            assert v.size == j.size * av.RUN and v.size // av.RUN >= 10_000
            assert int(mult.sum()) == v.size
            runs = v.view(np.uint64).reshape(-1, av.RUN)
            lane_x, lane_y = runs[:, 0::2], runs[:, 1::2]                    # what the 64 lanes hold in .x and in .y
            assert np.array_equal(lane_x, lane_y)
            led = (lane_x == lane_x[:, :1]).sum(axis=1)                       # lanes that share lane 0's value
            assert (led == (k + 1) // 2 if k < av.RUN else led == 64).all()
            kx = oracle.kext_many(1.0 + lane_x[::97].view(np.float64))       # extended keys: no int16 wrap in the difference
            assert ((kx.max(axis=1) - kx.min(axis=1)) == (1 if k < av.RUN else 0)).all()    # the two values: adjacent buckets
            assert np.array_equal(av.row_of(uniq, mult), oracle.histogram_dense(v))
    assert [(av.WAVE_SHAPES[s][1] + 1) // 2 for s in (1, 2, 3)] == [40, av.AGG_MIN, av.AGG_MIN - 1]


def test_with_ids_gives_every_name_the_whole_key_space():
    v = av.full_set()
    for M in (5, 20, 700, 30000):
        ids = av.with_ids(v, M)
        assert ids.dtype == np.uint32 and ids.max() == M - 1 and np.bincount(ids).min() >= v.size // M
    ids = av.with_ids(v, 700)
    k = av.expected(v[ids == 123]).astype(np.int32)
    assert k.min() < -32000 and k.max() > 32000


def test_guard_band_share_of_an_ordinary_stream():
    """The "1 sample in ~4 000" of lh_codec.h: 2 G / 2^14 = 1 / 4 096."""
    v = np.random.default_rng(4000).lognormal(math.log(1e5), 1.0, 1_000_000)
    share = av.in_guard_band(v).mean()
    assert 1 / 8000 < share < 1 / 2000, share
