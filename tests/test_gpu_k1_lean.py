"""K1 (k_ingest_single) tile by tile: the lean body (straight-line lh_bin_fast + LDS add, needs-care samples noted and
taken through lh_bin_of / k1_add by a cold loop after the tile's sixteen samples), the per-sample body, and the wave's
choice between them at the end of every tile.  Both bodies are exact, so every case is bit for bit against the oracle:
no tolerance.  Semantics: metrics.go:273-295 (one increment per sample), compress: metrics.go:316-322.

Geometry the cases are built on: a tile is 8 192 samples (512 threads x 8 register pairs x 2), the grid is at most 512
workgroups, tile t belongs to workgroup t % grid.  Inside a tile (16-byte-aligned start) sample i sits in
slot 2 * (i // 1024) + (i & 1) of thread (i // 2) % 512, i.e. lane (i // 2) % 64 of its wave.  A wave takes its first
tile on the per-sample body and may go lean from its second one."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 8192
GRID = 512
SIZES = [1, 2, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, GRID * TILE, GRID * TILE + TILE + 1, 1029 * TILE + 1]


@pytest.fixture(scope="module")
def la(native_lib, torch_cuda):
    import loghisto_amd
    return loghisto_amd


@pytest.fixture(scope="module")
def engine(la):
    e = la.Engine(max_metrics=1, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
    yield e
    e.close()


def lognormal(rng, n):
    return rng.lognormal(math.log(1e5), 1.0, n)


def on_thresholds(rng, n):
    """bench.make_samples' recipe: 100 * log(1 + v) = k - 0.5 to rounding, 500 boundaries around 1e5 -- every sample
    lies inside the guard band of a threshold"""
    return np.expm1((rng.integers(900, 1400, n).astype(np.float64) - 0.5) / 100.0)


def check(engine, torch, v, offsets=(0, 1)):
    """the oracle first, then the same samples from a 16-byte-aligned pointer and from one 8 bytes further"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    want = oracle.histogram_dense_mt(v) if len(v) > 1 << 22 else oracle.histogram_dense(v)
    assert int(want.sum()) == len(v)
    for off in offsets:
        buf = torch.from_numpy(np.concatenate([np.zeros(2 + off), v])).cuda()
        d = buf[2 + off:]
        assert d.data_ptr() % 16 == 8 * off
        engine.submit_device(0, d, len(v))
        with engine.flip() as snap:
            row = snap.dense_row(0)
        bad = np.flatnonzero(row != want)
        assert bad.size == 0, (off, bad[:8], row[bad[:8]], want[bad[:8]])


_LOGNORMAL = {}


def lognormal_of(n):
    """one lognormal stream per size, shared by the tests that need it and never written to"""
    if n not in _LOGNORMAL:
        v = lognormal(np.random.default_rng(n), n)
        v.setflags(write=False)
        _LOGNORMAL[n] = v
    return _LOGNORMAL[n]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_tile_and_the_grid(engine, torch_cuda, n, off):
    """head sample, odd tail, the remainder's owner, rotation with 1, 2 and 3 tiles per workgroup; the last three sizes
    are the many-bucket stream over several tiles per workgroup: the lean body"""
    check(engine, torch_cuda, lognormal_of(n), offsets=(off,))


def test_every_sample_in_the_guard_band(engine, torch_cuda):
    """every lane needs care in every slot of a lean tile: sixteen passes of the cold loop, then the wave backs off"""
    n = 6 * GRID * TILE + TILE + 1
    check(engine, torch_cuda, on_thresholds(np.random.default_rng(5), n))


SPECIALS = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -1e300, 1e300, 5e-324]


def test_planted_needs_care_samples(engine, torch_cuda):
    """a lognormal stream; one tile in four holds one guard-band value, and known (tile, slot, lane) positions of tiles
    the waves take lean (a workgroup's second tile onward) hold NaN, +-Inf, +-0.0, +-1e300 and the smallest subnormal: the
    cold loop runs from the lean body on exactly those samples, each counted once"""
    rng = np.random.default_rng(11)
    tiles = 6 * GRID
    n = tiles * TILE + 5
    v = lognormal(rng, n)
    thr = on_thresholds(rng, tiles)
    for t in range(1, tiles, 4):
        v[t * TILE + int(rng.integers(0, TILE))] = thr[t]
    k = 0
    for t in (GRID, GRID + 1, 2 * GRID + 7, 3 * GRID + 300, 4 * GRID + 511, 5 * GRID + 2, tiles - 1):
        for slot, thread in ((0, 0), (1, 0), (15, 511), (7, 63), (8, 64), (3, 257), (3, 258), (12, 130)):
            # two slots of one lane (thread 0), two lanes of one slot (257, 258), first / last thread and slot
            i = t * TILE + (slot // 2) * 1024 + 2 * thread + (slot & 1)
            v[i] = SPECIALS[k % len(SPECIALS)]
            k += 1
    check(engine, torch_cuda, v)


def few_valued(rng, n, kind):
    body = lognormal(rng, 3)
    if kind == "constant":
        return np.full(n, body[0])
    if kind == "two_values":
        return body[rng.integers(0, 2, n)]
    return body[rng.choice(3, n, p=[0.9, 0.09, 0.01])]  # 90 / 9 / 1


@pytest.mark.parametrize("rare_in_lane0", [False, True])
@pytest.mark.parametrize("kind", ["constant", "two_values", "skewed"])
def test_few_valued_streams_and_a_rare_lane0(engine, torch_cuda, kind, rare_in_lane0):
    """groups worth aggregating keep a wave on the per-sample body; with a rare value in every wave's lane 0 the group
    test sees a group of one in every sample and the wave goes lean on a stream of one or two hot words"""
    rng = np.random.default_rng(23)
    n = 4 * GRID * TILE + TILE + 1
    v = few_valued(rng, n, kind)
    if rare_in_lane0:
        i = np.arange(n)
        v[(i // 2) % 64 == 0] = 12345.678
    check(engine, torch_cuda, v)


@pytest.mark.parametrize("kind", ["thin_far_tail", "all_at_1e30", "signed_wide"])
def test_streams_that_leave_the_window(engine, torch_cuda, kind):
    rng = np.random.default_rng(31)
    n = 4 * GRID * TILE + 3
    if kind == "thin_far_tail":          # 0.1 % up to 1e60: about one miss per wave and tile, through the cold loop
        v = lognormal(rng, n)
        far = rng.random(n) < 1e-3
        v[far] = 10.0 ** rng.uniform(18, 60, int(far.sum()))
    elif kind == "all_at_1e30":          # the main window moves with the stream
        v = rng.lognormal(math.log(1e30), 1.0, n)
    else:                                # +-10^U(-3, 20): wide mode, one copy of 16 384 bins
        v = 10.0 ** rng.uniform(-3, 20, n) * rng.choice([-1.0, 1.0], n)
    check(engine, torch_cuda, v)


def test_stream_that_switches_character(engine, torch_cuda):
    """lognormal for the first third of the tiles, constant for the second, lognormal again: every wave goes lean, back to
    the per-sample body and lean again"""
    rng = np.random.default_rng(41)
    tiles = 9 * GRID
    n = tiles * TILE + 77
    v = lognormal(rng, n)
    v[3 * GRID * TILE:6 * GRID * TILE] = 98765.4321
    check(engine, torch_cuda, v)
