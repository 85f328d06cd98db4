"""The percentile walk of lh_spread, lh_across, lh_kept_across and lh_top where it can go wrong, with K2 as the judge: what
lh_extract_rows (Snapshot.extract) returns for the same snapshot.  "The first bin whose inclusive prefix reaches
pct_threshold(p, total)" is lh_pct.h's for the first three and k_top_score's own text; K2 has its copy in another
translation unit, so it is independent of theirs.

One engine of 8 names per cell width.  Every row's span starts one, two or three bins above a multiple of 4 (BASE + 1 ..),
so the walk enters below the span, and the cells sit at offsets from that multiple of 4 either side of what the walk is cut
into: the lane's group of 4 bins (3 | 4), the step of 256 (255 | 256, and 259 in the second step's lane 0) and lh_kept's
tile of 1 024 (1 023 | 1 024).  Offset 0 itself lies below such a span; the first cell is the span's first bin, offset 1.
  ones        a cell of 1 at each of those offsets (total 8)
  hundreds    the same cells with prefixes 100 200 300 500 600 700 900 1000, so that 0.2 | 0.201, 0.5 | 0.501 and 0.9 | 0.901
              are the last sample of one cell and the first of the next across a lane, a step and a tile
  never       never marked;  zeros: marked over 1 030 bins, all zeros;  u32max: one cell of 0xffffffff
  at256, at1023, at1024   one cell, in a span marked from BASE + 2 or + 3 on
Asserted, under both launch shapes of each reader: count, pkeys and pvalid EQUAL to K2's, nbuckets equal to the number of
crafted cells, and lh_top by percentile in the order K2's keys give."""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_compare import _import, _write_narrow
from tests.test_gpu_count_le import engine

pytestmark = pytest.mark.gpu

M = 8
OFFS = [1, 3, 4, 255, 256, 259, 1023, 1024]
P = [0.0, 0.2, 0.201, 0.5, 0.501, 0.9, 0.901, 1.0, 1.5, float("nan")]
HUNDREDS = [100, 100, 100, 200, 100, 100, 200, 100]
SHAPES = {"wave": 1, "block": 1 << 30}


def base(m):
    return 1000 + 5000 * m  # a multiple of 4


def crafted_rows():
    """[(name, {bin: count}, span)]: span None = never marked, else (lo, hi) with lo no multiple of 4"""
    rows = [("ones", {base(0) + o: 1 for o in OFFS}, (base(0) + 1, base(0) + 1024)),
            ("hundreds", {base(1) + o: c for o, c in zip(OFFS, HUNDREDS)}, (base(1) + 1, base(1) + 1024)),
            ("never", {}, None),
            ("zeros", {}, (base(3) + 2, base(3) + 1031)),
            ("u32max", {base(4) + 3: 0xffffffff}, (base(4) + 3, base(4) + 3)),
            ("at256", {base(5) + 256: 7}, (base(5) + 2, base(5) + 256)),
            ("at1023", {base(6) + 1023: 7}, (base(6) + 3, base(6) + 1023)),
            ("at1024", {base(7) + 1024: 7}, (base(7) + 1, base(7) + 1030))]
    assert len(rows) == M and all(s is None or (s[0] % 4 and all(s[0] <= b <= s[1] for b in r)) for _, r, s in rows)
    return rows


@contextlib.contextmanager
def shape(switch, name):
    """Put every call of one reader through one kernel shape; the previous value comes back afterwards."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    fn = getattr(N.lib(), switch)
    assert fn(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert fn(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


@pytest.fixture(scope="module", params=["wide64", "narrow32"])
def crafted(request, native_lib, torch_cuda):
    wide = request.param == "wide64"
    rows = crafted_rows()
    cells, spans = [r for _, r, _ in rows], [s for _, _, s in rows]
    with engine(M, cell_bits=64 if wide else 32) as e:
        with e.flip() as s:
            if wide:
                _import(s, cells, spans)
            else:
                _write_narrow(torch_cuda, s, cells, spans)
            assert s.device_cells()[2] == (8 if wide else 4)
            ex = s.extract(P, M)  # K2: the reference, computed once
            yield types.SimpleNamespace(snap=s, ex=ex, rows=rows, cells=cells)


def same_as_k2(c, got, what):
    ex = c.ex
    assert np.array_equal(np.asarray(got["count"]).ravel(), ex["count"]), (what, got["count"], ex["count"])
    assert np.array_equal(np.asarray(got["pvalid"]).reshape(M, len(P)), ex["pvalid"]), (what, got["pvalid"], ex["pvalid"])
    assert np.array_equal(np.asarray(got["pkeys"]).reshape(M, len(P)), ex["pkeys"]), (what, got["pkeys"], ex["pkeys"])


def test_k2_selects_the_cells_either_side_of_each_boundary(crafted):
    """The judge itself, on the two rows whose thresholds were placed: the crafted percentiles do fall where the docstring
    says, and rows without a sample or percentiles beyond 1 have no key."""
    ex = crafted.ex
    want = {"ones": [1, 3, 3, 255, 256, 1024, 1024, 1024], "hundreds": [1, 3, 4, 255, 256, 1023, 1024, 1024]}
    for m, (name, cells, _) in enumerate(crafted.rows):
        assert int(ex["count"][m]) == sum(cells.values()) and int(ex["nbuckets"][m]) == len(cells), name
        assert list(ex["pvalid"][m]) == ([1] * 8 if cells else [0] * 8) + [0, 0], name
        if name in want:
            bins = [int(oracle.key_to_bin(int(k))) - base(m) for k in ex["pkeys"][m][:8]]
            assert bins == want[name], (name, bins)


@pytest.mark.parametrize("kind", ["wave", "block"])
def test_spread_equals_k2(crafted, kind):
    with shape("lh_tool_spread_switch", kind):
        same_as_k2(crafted, crafted.snap.spread(P, M), ("spread", kind))


@pytest.mark.parametrize("kind", ["wave", "block"])
def test_across_over_the_one_snapshot_equals_k2(crafted, kind):
    with shape("lh_tool_across_switch", kind):
        got = crafted.snap.across([], P, M)
    same_as_k2(crafted, got, ("across", kind))
    assert [int(x) for x in got["nbuckets"]] == [len(r) for r in crafted.cells], kind


@pytest.mark.parametrize("kind", ["wave", "block"])
def test_kept_across_over_the_kept_snapshot_equals_k2(crafted, kind):
    k = crafted.snap.keep(M)
    try:
        with shape("lh_tool_kept_switch", kind):
            got = k.across([], P, M)
    finally:
        k.close()
    same_as_k2(crafted, got, ("kept", kind))
    assert [int(x) for x in got["nbuckets"]] == [len(r) for r in crafted.cells], kind


def test_top_by_percentile_orders_the_rows_by_k2s_keys(crafted):
    ex = crafted.ex
    have = [m for m in range(M) if ex["count"][m]]
    for i, p in enumerate(P[:8]):
        got = crafted.snap.top(M, by="percentile", arg=p, nmetrics=M)
        order = sorted(have, key=lambda m: (-int(ex["pkeys"][m][i]), m))  # the bin grows with the int16 key
        assert [int(x) for x in got["id"]] == order, (p, got["id"], order)
        assert [int(x) for x in got["pkey"]] == [int(ex["pkeys"][m][i]) for m in order], p
        assert [int(x) for x in got["count"]] == [int(ex["count"][m]) for m in order], p
