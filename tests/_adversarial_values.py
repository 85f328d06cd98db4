"""Threshold-adjacent and special doubles for every ingest route (tests/test_gpu_routes_adversarial.py feeds them to the
kernels; tests/test_adversarial_values.py checks, without a GPU, that the set is what it claims to be).

Every ingest kernel finds a bucket in two steps (loghisto_amd/csrc/lh_codec.h): a fast index from the hardware log2, and an
exact decision -- lh_bin_of's table compare, lh_bin_fast plus fix-up, v3_bin_exact -- for the samples inside the guard band of
a bucket threshold.  Random streams put about 1 sample in 4 000 there and none within a few ulp of a threshold, which is where
a wrong exact decision shows: it moves one count between two adjacent cells.  The values below are ALL inside the band, or are
the doubles where 1 + |v| itself rounds, or are not finite, or lie beyond the int16 key domain.

V[j], j = 1 .. 70 978, is the smallest non-negative double whose extended key reaches j (tests/golden/make_thresholds.py);
the fixture holds prev(V[j]), V[j], next(V[j]) with the keys real Go is checked against.
Reference semantics: compress, metrics.go:316-322."""
import functools
import os
import sys

import numpy as np

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_thresholds as mt  # noqa: E402

GUARD_Q14 = 2                                    # LH_GUARD_Q14, lh_codec.h
AGG_MIN = 24                                     # LH_K1_AGG_MIN, lh_kernels.hip
RUN = 128                                        # one k1_add_fullwave call's .x and .y over 64 lanes
MAX_BITS = int(np.float64(1.7976931348623157e308).view(np.uint64))
SIGN = np.uint64(1 << 63)


def _f(bits):
    return np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64)


def _b(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _both_signs(v):
    return np.concatenate([v, _f(_b(v) | SIGN)])   # the sign BIT: -0.0 and the NaNs keep their other bits


@functools.lru_cache(maxsize=None)
def fixture():
    """(values, keys, flags) of tests/golden/thresholds_x.bin, read-only."""
    x, keys, flags = mt.read()
    for a in (x, keys, flags):
        a.setflags(write=False)
    return x, keys, flags


@functools.lru_cache(maxsize=None)
def threshold_bits():
    """Bit patterns of V[1 .. 70 978] as int64 (index j - 1)."""
    x, _, _ = fixture()
    vb = _b(x[1::3]).astype(np.int64)
    vb.setflags(write=False)
    return vb


def is_exact_threshold(v):
    """+-V[j] for some j: the samples whose 1 + |v| EQUALS a table entry (the >= of lh_bin_of)."""
    return np.isin(_b(v) & ~SIGN, threshold_bits().astype(np.uint64))


@functools.lru_cache(maxsize=None)
def values():
    """{class: float64 array}, read-only.  Classes: thresholds, near, rounding, specials."""
    x, _, _ = fixture()
    vb = threshold_bits()
    out = {"thresholds": np.concatenate([x, -x])}
    # the fixture holds V[j] - 1, V[j], V[j] + 1 (in bits): two and three further out, clipped to [0, MaxFloat64]
    near = np.concatenate([np.clip(vb + d, 0, MAX_BITS) for d in (-3, -2, 2, 3)]).astype(np.uint64)
    out["near"] = _both_signs(_f(near))
    # 1 + |v| is inexact or absorbs v
    two53 = 2.0 ** 53
    r = [2.0 ** -53, np.nextafter(2.0 ** -53, 0.0), np.nextafter(2.0 ** -53, 1.0),     # tie to even: 1 + 2^-53 == 1
         2.0 ** -52, 2.0 ** -1074, 2.0 ** -1022,
         2.0 ** 52 - 0.5, 2.0 ** 52 + 0.5, two53, two53 + 2.0, np.nextafter(two53, np.inf), np.nextafter(two53, -np.inf),
         2.0 ** 54 + 2.0, 2.0 ** 54 + 4.0]
    # ... and the first thresholds, where ~2^7 neighbouring v share one x = 1 + v: between prev(V[j]) and V[j] it is the
    # ROUNDING of the add that moves x onto the table entry (neighbours with different keys)
    low = np.concatenate([vb[:8] - 1, vb[:8]]).astype(np.uint64)
    out["rounding"] = _both_signs(np.concatenate([np.array(r, dtype=np.float64), _f(low)]))
    # specials
    payloads = [1, 0x7ffffffffffff, 0x2aaaaaaaaaaaa]                                      # below the quiet bit (2^51)
    nans = [0x7ff8000000000000 | p for p in payloads] + [0x7ff0000000000000 | p for p in payloads]   # quiet, signalling
    edge = np.concatenate([vb[32766:32768] - 1, vb[32766:32768], vb[32766:32768] + 1]).astype(np.uint64)   # keys 32766 | 32767 | wrap
    wrap = np.geomspace(3e142, 1e308, 300)                                                # beyond int16: the amd64 wrap region
    out["specials"] = _both_signs(np.concatenate([np.array([0.0, np.inf, 1.7976931348623157e308]), _f(np.array(nans, dtype=np.uint64)),
                                                  _f(edge), wrap]))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def full_set():
    """All classes in one array (about one million values, below 2^20), read-only."""
    v = np.concatenate([values()[k] for k in ("thresholds", "near", "rounding", "specials")])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def weighted_set():
    """The full set plus j mod 3 further copies of the whole neighbourhood of threshold j (V[j] - 3 .. V[j] + 3 in bits, both
    signs), read-only: the stream for ONE row.  In the full set every bucket holds the same few neighbours of its two
    thresholds, so a decision that is wrong in the same way at every threshold takes one sample out of each bucket and puts
    its neighbour's in: the row hardly changes (x > Tx[j] for x >= Tx[j] moved 204 of 65 536 cells).  With 1, 2, 3, 1, ..
    copies from one threshold to the next whatever crosses a threshold changes both buckets."""
    vb = threshold_bits()
    reps = np.arange(1, vb.size + 1) % 3
    more = np.concatenate([np.repeat(np.clip(vb + d, 0, MAX_BITS), reps) for d in range(-3, 4)]).astype(np.uint64)
    v = np.concatenate([full_set(), _both_signs(_f(more))])
    v.setflags(write=False)
    return v


def extra_classes():
    """near + rounding + specials: what the fixture does not already hold."""
    return np.concatenate([values()[k] for k in ("near", "rounding", "specials")])


def expected(v):
    """int16 keys: the oracle's plain-C restatement of Go's arithmetic."""
    return oracle.compress_many(v)


def in_guard_band(v):
    """lh_bin_fast's `uncertain`, restated in float64 with an accurate log: u = (100 ln(1 + |v|) + 0.5) 2^14; inside the band
    when (floor(u) + G) mod 2^14 < 2 G, or when v is not finite."""
    v = np.asarray(v, dtype=np.float64)
    x = 1.0 + np.abs(v)
    fin = np.isfinite(x)
    u = np.floor((100.0 * np.log(np.where(fin, x, 1.0)) + 0.5) * 16384.0).astype(np.int64)
    return ~fin | (((u + GUARD_Q14) % 16384) < 2 * GUARD_Q14)


# ---- orders for a single-metric stream ---------------------------------------------------------------------------------
# Both plain orders begin and end with two exact thresholds (+-V[j]): K1's scalar head and tail, and the first sample of a
# slice taken at [1:], are then samples that the exact decision's >= decides.

def sorted_by_key(v):
    """Ascending key: every K1 workgroup's tile is narrow (two copies of an 8 192-bin window that follows the stream)."""
    v = np.asarray(v, dtype=np.float64)
    key = expected(v).astype(np.int64)
    exact = is_exact_threshold(v)
    second = np.where(key < 0, ~exact, exact)                # exact thresholds first in the lowest key, last in the highest
    return np.ascontiguousarray(v[np.lexsort((second, key))])


def shuffled(v, seed=20):
    """Seeded permutation: K1's survey sees the whole key space (WIDE mode, both floating windows, the global row)."""
    v = np.asarray(v, dtype=np.float64)
    out = v[np.random.default_rng(seed).permutation(v.size)]
    at = np.nonzero(is_exact_threshold(out))[0]
    at = at[(at > 1) & (at < out.size - 2)]                  # from the inside: the four swaps cannot undo one another
    for dst, src in zip((0, 1, out.size - 2, out.size - 1), (at[0], at[1], at[-2], at[-1])):
        out[[dst, src]] = out[[src, dst]]
    return np.ascontiguousarray(out)


def drop_middle(v):
    """The same order with one sample fewer (the other parity of n); the ends stay."""
    return np.ascontiguousarray(np.delete(v, v.size // 2))


@functools.lru_cache(maxsize=None)
def wave_subset():
    """j for wave_blocks: every 5th threshold plus every j whose key lies within 8 of +-4095, +-4096, +-32767 and 0 (where K1's
    default window, the int16 domain and the sign end).  int64, ascending."""
    vb = threshold_bits()
    key = expected(_f(vb.astype(np.uint64))).astype(np.int64)
    pick = np.zeros(vb.size, dtype=bool)
    pick[::5] = True
    for c in (4095, 4096, -4095, -4096, 32767, -32767, 0):
        pick |= np.abs(key - c) <= 8
    j = np.nonzero(pick)[0] + 1
    j.setflags(write=False)
    return j


WAVE_SHAPES = {
    # (first value, how many of it) of a 128-sample run; the rest is the other value.  at = V[j], prev = the double below it
    1: ("at", 80),       # lane 0 leads 40 lanes (aggregated), 24 lanes add 1 to the bucket below
    2: ("prev", 48),     # lane 0 leads exactly 24 lanes == LH_K1_AGG_MIN; 40 lanes add 1 to the bucket above
    3: ("prev", 46),     # lane 0's group has 23 lanes: nothing is aggregated
    4: ("at", 128),      # the whole wave is one bucket
}


def wave_blocks(j_subset, shape, seed=None):
    """(stream, unique values, their multiplicities).  For each j a run of 128 samples aligned to 128 from the array's start:
    one k1_add_fullwave call's .x and .y over 64 lanes (lane l holds samples 2 l and 2 l + 1 of the run).  seed: the runs in a
    seeded random order instead of ascending j (every tile then spans the key space)."""
    first, k = WAVE_SHAPES[shape]
    j = np.asarray(j_subset, dtype=np.int64)
    if seed is not None:
        j = j[np.random.default_rng(seed).permutation(j.size)]
    at = threshold_bits()[j - 1].astype(np.uint64)
    prev = at - np.uint64(1)
    a, b = (at, prev) if first == "at" else (prev, at)
    runs = np.empty((j.size, RUN), dtype=np.uint64)
    runs[:, :k] = a[:, None]
    runs[:, k:] = b[:, None]
    uniq = np.concatenate([a, b]) if k < RUN else a
    mult = np.concatenate([np.full(j.size, k), np.full(j.size, RUN - k)]) if k < RUN else np.full(j.size, RUN)
    return _f(runs.reshape(-1)), _f(uniq), mult.astype(np.uint64)


def row_of(uniq, mult):
    """The dense row of a stream given as unique values and multiplicities."""
    row = np.zeros(oracle.NKEYS, dtype=np.uint64)
    np.add.at(row, oracle.key_to_bin(expected(uniq)), np.asarray(mult, dtype=np.uint64))
    return row


# ---- mixed streams -----------------------------------------------------------------------------------------------------

def with_ids(v, M):
    """ids[i] = (i * 7919) mod M: every name sees the whole key space, so every per-name window misses."""
    return ((np.arange(len(v), dtype=np.uint64) * np.uint64(7919)) % np.uint64(M)).astype(np.uint32)
