"""lh_across_ids*, lh_count_le_ids*, lh_spread_ids*: the base forms' walks over rows ids[0 .. n) instead of
[first, first + nmetrics).  Entry m of every output is BIT-EQUAL to the base form's entry for row ids[m] in the same kernel
shape (same row, same span, same shape, same order: the float outputs too), whatever the order, the repeats and the length of
the list; a handful of entries are also held to Python integers and the oracle; an id beyond the rows is LH_ERANGE in a host
form and an all-zero entry in a device form; and nothing in any snapshot moves.
Two engines of 64 names, one of 64-bit cells (rows imported) and one of 32-bit cells (rows written into the narrow store; one
of its snapshots is then widened by the import of a cell of 2^33)."""
import contextlib
import ctypes as C
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle
from loghisto_amd import _native as N
from tests.test_gpu_across import FIELDS as AC_FIELDS, P_MAIN, check as across_check, model
from tests.test_gpu_compare import _import, _write_narrow, rows_of
from tests.test_gpu_count_le import engine, host_arrays, take_of

pytestmark = pytest.mark.gpu

U64 = np.uint64
NK = oracle.NKEYS
U32MAX = (1 << 32) - 1
INF = np.inf
M = 64                                                             # rows of both engines
SHAPES = {"wave": 1, "block": 1 << 30}
SWITCH = dict(across="lh_tool_across_switch", count_le="lh_tool_count_le_switch", spread="lh_tool_spread_switch")
AC_PER_P = ("pkeys", "pvalid")
SP_FIELDS = dict(count=U64, sum=np.float64, m2=np.float64, pkeys=np.int16, pvalid=np.uint8, count_le=U64, sum_le=np.float64)
SP_PER_P = ("pkeys", "pvalid", "count_le", "sum_le")
CL_FIELDS = dict(cum=U64, total=U64)
P_SPREAD = [0.5, 0.0, 1.0, 0.99, 1.5, 0.9]

# the crafted rows, by name; every other row of the 64 is never marked
PLAIN, NEVER, ZERO, BIN0, BIN_LAST, STEPS, FULL, ONES32, BIG, LOOSE, LAST = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, M - 1


@contextlib.contextmanager
def shape(unit, name):
    """Put every call of `unit` through one kernel shape, whatever the number of entries."""
    prev, now = C.c_uint32(0), C.c_uint32(0)
    fn = getattr(N.lib(), SWITCH[unit])
    assert fn(SHAPES[name], C.byref(prev)) == 0
    try:
        yield
    finally:
        assert fn(prev.value, C.byref(now)) == 0 and now.value == SHAPES[name]


def crafted_rows(i, wide):
    """Snapshot i's rows and spans ('tight', None: never marked, or (lo, hi) marked beside the cells)."""
    rows, spans = [{} for _ in range(M)], [None] * M

    def put(m, cells, span="tight"):
        rows[m], spans[m] = cells, span

    put(PLAIN, {100 + i: 3, 200: 5, 300 + 2 * i: 7})
    put(ZERO, {}, (700, 1200))                                     # marked, all zero
    put(BIN0, {0: 4 + i})
    put(BIN_LAST, {NK - 1: 2 + i})
    put(STEPS, {20002: 2, 20302: 1, 21027 + i: 3})                 # more than one 256-bin step, from a bin that is no multiple of 4
    put(FULL, {b: 1 + (b + i) % 3 for b in range(NK)})             # all 65 536 bins: the block shape's chunk scan
    put(ONES32, {500: U32MAX, 600 + i: U32MAX})                    # narrow cells of 0xffffffff
    put(BIG, {700: 1 << 33, 650: 5} if wide else {700: U32MAX, 650: 5})
    put(LOOSE, {40001: 2, 40100 + i: 1}, (39000, 42000))
    put(LAST, {123: 9 + i, 64000: 1})
    return rows, spans


def id_lists():
    rng = np.random.default_rng(11)
    mixed = np.concatenate([rng.integers(0, M, 30), [FULL, FULL, BIG, NEVER, LAST, 0, 0, ZERO, ONES32, BIN_LAST]])
    rng.shuffle(mixed)
    assert len(set(mixed.tolist())) < mixed.size                   # it repeats
    three = np.concatenate([rng.permutation(M) for _ in range(3)])
    lists = dict(identity=np.arange(M), reversed=np.arange(M)[::-1], repeats=mixed, last=[LAST], first=[0], one=[FULL],
                 three=[STEPS, NEVER, LAST], four=[LOOSE, FULL, ZERO, 0], five=[BIN_LAST, FULL, FULL, BIN0, BIG], thrice=three)
    return {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in lists.items()}


IDS = id_lists()


def bounds_rows():
    """A row of six bounds per name, every row different from every other."""
    at = [oracle.decompress(int(oracle.bin_to_key(np.array([b]))[0])) for b in (0, 100, 123, 200, 500, 600, 650, 700, 20002,
                                                                               20302, 40001, 40100, 64000, NK - 1)]
    pool = np.array([-INF, -1e25, -3.5, -0.0, 0.0, 1e-9, 0.25, 42.0, 1e25, INF] + at)
    B = np.sort(np.random.default_rng(5).choice(pool, (M, 6)), axis=1)
    assert len({r.tobytes() for r in B}) == M
    return B


def raw(d, fields):
    return {k: np.ascontiguousarray(d[k]).view(fields[k]) for k in fields}


def assert_gathered(got, base, ids, fields, what):
    """entry m of every output == the base form's entry at row ids[m], bit for bit"""
    idx = np.asarray(ids, dtype=np.int64)
    for k, t in fields.items():
        g, b = np.ascontiguousarray(got[k]).view(t), np.ascontiguousarray(base[k]).view(t)
        assert g.shape[0] == idx.size, (what, k, g.shape)
        assert g.tobytes() == np.ascontiguousarray(b[idx]).tobytes(), (what, k)


@pytest.fixture(scope="module")
def world(native_lib, torch_cuda):
    torch = torch_cuda
    with engine(M, cell_bits=64, num_buffers=4) as ew, engine(M, cell_bits=32, num_buffers=4) as en, \
            engine(48, cell_bits=64, num_buffers=2) as e48:
        with contextlib.ExitStack() as stack:
            W = [stack.enter_context(ew.flip()) for _ in range(3)]
            Nn = [stack.enter_context(en.flip()) for _ in range(3)]
            short = stack.enter_context(e48.flip())
            rows = {}
            for i, s in enumerate(W):
                r, sp = crafted_rows(i, True)
                _import(s, r, sp)
                rows[s] = r
            for i, s in enumerate(Nn):
                r, sp = crafted_rows(3 + i, False)
                _write_narrow(torch, s, r, sp)
                rows[s] = r
            # the import of one cell of 2^33 widens the second narrow snapshot
            Nn[1].add_buckets(np.array([BIG], dtype=np.uint32), oracle.bin_to_key(np.array([700])).astype(np.int16),
                              np.array([1 << 33], dtype=U64))
            rows[Nn[1]][BIG][700] += 1 << 33
            _import(short, [{77: 2}] + [{} for _ in range(47)], [None] * 48)
            rows[short] = [{77: 2}] + [{} for _ in range(47)]
            snaps = W + Nn
            widths = [s.device_cells()[2] for s in snaps]
            assert widths == [8, 8, 8, 4, 8, 4]
            assert all(s.device_cells()[1] == M for s in snaps) and short.device_cells()[1] == 48
            for s in snaps:
                assert rows_of(s, M) == [{b: c for b, c in r.items() if c} for r in rows[s]]
            lists = {"wide1": [W[0]], "wide3": [W[0], W[1], W[2]], "wide16": (W * 6)[:16],
                     "narrow1": [Nn[0]], "narrow3": [Nn[0], Nn[2], Nn[0]], "narrow16": [Nn[0], Nn[2]] * 8,
                     "mixed1": [Nn[1]], "mixed3": [Nn[0], W[1], Nn[1]], "mixed16": (snaps * 3)[:16]}
            state = [([x.copy() for x in s.buckets_all(M)], s.device_cells()) for s in snaps]
            yield types.SimpleNamespace(torch=torch, W=W, N=Nn, short=short, snaps=snaps, rows=rows, lists=lists, state=state,
                                        widths=widths, B=bounds_rows())
            assert [s.device_cells()[2] for s in snaps] == widths


def ids_on_device(torch, ids):
    t = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def wait(torch, snap):
    torch.cuda.ExternalStream(snap.stream()).synchronize()


# ---- the three units, each as (base form over all rows, host id form, device id form) ---------------------------------------
def across_base(w, lst):
    return raw(lst[-1].across(lst[:-1], P_MAIN, M), AC_FIELDS)


def across_host(w, lst, ids):
    return lst[-1].across_ids(ids, lst[:-1], P_MAIN)


def across_device(w, lst, ids, names=tuple(AC_FIELDS)):
    torch, n = w.torch, len(ids)
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int32, pkeys=torch.int16,
                 pvalid=torch.uint8)
    out = {k: torch.full((n, len(P_MAIN)) if k in AC_PER_P else (n,), 77, dtype=kinds[k], device="cuda") for k in names}
    back = lst[-1].across_ids(ids_on_device(torch, ids), lst[:-1], P_MAIN, out=out)
    wait(torch, lst[-1])
    assert all(back[k] is out[k] for k in names)
    return {k: v.cpu().numpy().view(AC_FIELDS[k]) for k, v in out.items()}


def spread_device(w, s, ids):
    torch, n = w.torch, len(ids)
    kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8,
                 count_le=torch.int64, sum_le=torch.float64)
    out = {k: torch.full((n, len(P_SPREAD)) if k in SP_PER_P else (n,), 77, dtype=kinds[k], device="cuda") for k in SP_FIELDS}
    s.spread_ids(ids_on_device(torch, ids), P_SPREAD, out=out)
    wait(torch, s)
    return {k: v.cpu().numpy().view(SP_FIELDS[k]) for k, v in out.items()}


def count_device(w, s, ids, b):
    torch, n = w.torch, len(ids)
    cum = torch.full((n, b.shape[-1]), 77, dtype=torch.int64, device="cuda")
    total = torch.full((n,), 77, dtype=torch.int64, device="cuda")
    s.count_le_ids(ids_on_device(torch, ids), b, out=(cum, total))
    wait(torch, s)
    return dict(cum=cum.cpu().numpy().view(U64), total=total.cpu().numpy().view(U64))


# ---- 1. gather equivalence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SHAPES))
def test_across_ids_gathers_the_base_form(world, kind):
    w = world
    with shape("across", kind):
        for tag, lst in w.lists.items():
            base = across_base(w, lst)
            for name, ids in IDS.items():
                assert_gathered(across_host(w, lst, ids), base, ids, AC_FIELDS, (kind, tag, name, "host"))
                assert_gathered(across_device(w, lst, ids), base, ids, AC_FIELDS, (kind, tag, name, "device"))


@pytest.mark.parametrize("kind", list(SHAPES))
def test_spread_ids_gathers_the_base_form(world, kind):
    w = world
    with shape("spread", kind):
        for s in (w.W[0], w.N[0], w.N[1]):                                       # wide, narrow, widened
            base = raw(s.spread(P_SPREAD, M), SP_FIELDS)
            for name, ids in IDS.items():
                assert_gathered(s.spread_ids(ids, P_SPREAD), base, ids, SP_FIELDS, (kind, name, "host"))
                assert_gathered(spread_device(w, s, ids), base, ids, SP_FIELDS, (kind, name, "device"))


@pytest.mark.parametrize("per_metric", [False, True])
@pytest.mark.parametrize("kind", list(SHAPES))
def test_count_le_ids_gathers_the_base_form(world, kind, per_metric):
    """Per-metric bounds: every row's bounds differ and travel with the id, so a mix-up of rows shows."""
    w = world
    B = w.B if per_metric else w.B[7]
    with shape("count_le", kind):
        for s in (w.W[0], w.N[0], w.N[1]):
            base = s.count_le(B, M)
            for name, ids in IDS.items():
                b = np.ascontiguousarray(B[ids.astype(np.int64)]) if per_metric else B
                assert_gathered(s.count_le_ids(ids, b), base, ids, CL_FIELDS, (kind, name, "host"))
                assert_gathered(count_device(w, s, ids, b), base, ids, CL_FIELDS, (kind, name, "device"))


# ---- 2. independent of the base forms: Python integers over buckets_all, the oracle's percentile walk, the _sum bound ---------
PICK = np.array([FULL, PLAIN, NEVER, BIG, LAST, ZERO, ONES32, PLAIN, BIN0, BIN_LAST, STEPS], dtype=np.uint32)


@pytest.mark.parametrize("kind", list(SHAPES))
def test_entries_against_the_oracle(world, kind):
    w = world
    listed = {s: rows_of(s, M) for s in w.snaps}
    with shape("across", kind):
        for tag in ("wide1", "narrow3", "mixed3", "mixed16"):
            lst = w.lists[tag]
            want = [model([listed[s][int(m)] for s in lst], P_MAIN) for m in PICK]
            across_check(across_host(w, lst, PICK), want, P_MAIN, (kind, tag))
    D = oracle.decompress_table()
    for s in (w.W[0], w.N[1]):
        E = take_of(w.B)
        with shape("count_le", kind):
            got = s.count_le_ids(PICK, np.ascontiguousarray(w.B[PICK.astype(np.int64)]))
        for m, r in enumerate(PICK):
            cells = listed[s][int(r)]
            assert int(got["total"][m]) == sum(cells.values()), (kind, m)
            for j in range(w.B.shape[1]):
                assert int(got["cum"][m, j]) == sum(c for b, c in cells.items() if b < int(E[int(r), j])), (kind, m, j)
        with shape("spread", kind):
            sp = s.spread_ids(PICK, P_SPREAD)
        for m, r in enumerate(PICK):
            cells = listed[s][int(r)]
            assert int(sp["count"][m]) == sum(cells.values()), (kind, m)
            dense = np.zeros(NK, dtype=U64)
            for b, c in cells.items():
                dense[b] = c
            ref = oracle.process_dense(dense, np.array(P_SPREAD))
            ok = ref["pvalid"] != 0
            assert np.array_equal(sp["pvalid"][m] != 0, ok) and np.array_equal(sp["pkeys"][m][ok], ref["pkeys"][ok]), (kind, m)
            exact = sum((Fraction(float(D[b])) * c for b, c in cells.items()), Fraction(0))
            mag = sum((abs(Fraction(float(D[b]))) * c for b, c in cells.items()), Fraction(0))
            err = abs(Fraction(float(sp["sum"][m])) - exact)
            print(f"{kind} spread_ids row {int(r)}: sum {sp['sum'][m]!r} error {float(err):.3e} bound {float(mag) * 1e-12:.3e}")
            assert err <= Fraction(1, 10 ** 12) * mag, (kind, m, float(err))


# ---- 3. ids beyond the rows --------------------------------------------------------------------------------------------------
def bad_lists():
    for bad in (M, 0xffffffff):
        for at in (0, 2, 4):                                                     # first, in the middle, last
            ids = np.array([PLAIN, FULL, LAST, BIG], dtype=np.uint32)
            yield np.insert(ids, min(at, ids.size), np.uint32(bad))


def test_host_forms_refuse_an_id_beyond_the_rows(world):
    import loghisto_amd
    w, torch = world, world.torch
    s, lst = w.N[1], w.lists["mixed3"]
    L = N.lib()
    for pinned in (True, False):
        for ids in bad_lists():
            n = ids.size
            out = {k: host_arrays(torch, pinned, (n, len(P_MAIN)) if k in AC_PER_P else (n,), t) for k, t in AC_FIELDS.items()}
            with pytest.raises(loghisto_amd.LhError) as ei:
                lst[-1].across_ids(ids, lst[:-1], P_MAIN, out=out)
            assert ei.value.code == N.ERANGE
            out2 = {k: host_arrays(torch, pinned, (n, len(P_SPREAD)) if k in SP_PER_P else (n,), t) for k, t in SP_FIELDS.items()}
            with pytest.raises(loghisto_amd.LhError) as ei:
                s.spread_ids(ids, P_SPREAD, out=out2)
            assert ei.value.code == N.ERANGE
            cum, total = host_arrays(torch, pinned, (n, 6), U64), host_arrays(torch, pinned, (n,), U64)
            for flags, b in ((0, w.B[3]), (N.LE_PER_METRIC, np.ascontiguousarray(w.B[:n]))):
                assert L.lh_count_le_ids(s._h, ids.ctypes.data, n, b.ctypes.data, 6, flags, cum.ctypes.data,
                                         total.ctypes.data) == N.ERANGE
            for a in list(out.values()) + list(out2.values()) + [cum, total]:
                assert np.all(a.view(np.uint8) == 0x77)                          # no output was written
    # an id that only one snapshot of the list has a row for
    for lst in ([w.short, w.W[0]], [w.W[0], w.short], [w.W[0], w.short, w.N[0]]):
        for ids in ([50], [0, 48, 1], [47, 63]):
            with pytest.raises(loghisto_amd.LhError) as ei:
                lst[-1].across_ids(ids, lst[:-1], P_MAIN)
            assert ei.value.code == N.ERANGE
        got = lst[-1].across_ids([47, 0, PLAIN], lst[:-1], P_MAIN)               # rows every snapshot has
        assert got["count"].shape == (3,) and int(got["count"][1]) == sum(sum(w.rows[x][0].values()) for x in lst)


@pytest.mark.parametrize("kind", list(SHAPES))
def test_device_forms_read_nothing_for_an_id_beyond_the_rows(world, kind):
    """(The guard is lh::row_of in lh_wave.h: an id at or beyond nrows opens an empty span, as a row never marked has.)"""
    w = world
    ids = np.array([FULL, M, PLAIN, 0xffffffff, LAST, 0xfffffffe, BIG], dtype=np.uint32)
    good = ids < M
    safe = np.where(good, ids, NEVER)                                            # a row never marked: all zero in the base form

    def zero_and_gathered(got, base, fields, what):
        assert_gathered(got, base, safe, fields, what)
        for k, t in fields.items():
            assert not np.ascontiguousarray(got[k]).view(t)[~good].view(np.uint8).any(), (what, k)

    s, lst = w.N[1], w.lists["mixed3"]
    with shape("across", kind):
        zero_and_gathered(across_device(w, lst, ids), across_base(w, lst), AC_FIELDS, (kind, "across"))
        # a list whose shortest snapshot has 48 rows: ids from 48 on are beyond it
        two = [w.W[0], w.short]
        got = across_device(w, two, np.array([47, 48, 0, 63], dtype=np.uint32))
        part = raw(w.short.across([w.W[0]], P_MAIN, 48), AC_FIELDS)
        assert_gathered({k: v[[0, 2]] for k, v in got.items()}, part, [47, 0], AC_FIELDS, (kind, "48 rows"))
        assert all(not v[[1, 3]].view(np.uint8).any() for v in got.values())
    with shape("spread", kind):
        zero_and_gathered(spread_device(w, s, ids), raw(s.spread(P_SPREAD, M), SP_FIELDS), SP_FIELDS, (kind, "spread"))
    with shape("count_le", kind):
        b = np.ascontiguousarray(w.B[safe.astype(np.int64)])
        zero_and_gathered(count_device(w, s, ids, b), s.count_le(w.B, M), CL_FIELDS, (kind, "count_le"))


# ---- 4. read-only, and the empty call ------------------------------------------------------------------------------------------
def test_nothing_moves_and_an_empty_list_writes_nothing(world):
    w = world
    L = N.lib()
    ids = IDS["repeats"]
    lst = w.lists["mixed16"]
    across_host(w, lst, ids)
    across_device(w, lst, ids)
    for s in (w.W[0], w.N[0], w.N[1]):
        s.spread_ids(ids, P_SPREAD)
        spread_device(w, s, ids)
        s.count_le_ids(ids, w.B[0])
        count_device(w, s, ids, np.ascontiguousarray(w.B[ids.astype(np.int64)]))
    # n == 0: LH_OK, nothing written, ids may be NULL
    guard = np.full(4, 7, dtype=U64)
    pp, bb = np.array(P_SPREAD), w.B[0]
    hs = (C.c_void_p * 2)(w.W[0]._h.value, w.N[0]._h.value)
    for fn_tail in ("", "_device"):
        assert getattr(L, "lh_across_ids" + fn_tail)(hs, 2, None, 0, pp.ctypes.data, pp.size, 0, guard.ctypes.data, 0, 0, 0, 0, 0) == 0
        assert getattr(L, "lh_spread_ids" + fn_tail)(w.N[0]._h, None, 0, pp.ctypes.data, pp.size, guard.ctypes.data, 0, 0, 0, 0, 0, 0) == 0
        assert getattr(L, "lh_count_le_ids" + fn_tail)(w.N[0]._h, None, 0, bb.ctypes.data, bb.size, 0, 0, guard.ctypes.data) == 0
    assert np.all(guard == 7)
    for s, (before, cells) in zip(w.snaps, w.state):
        after = s.buckets_all(M)
        assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
        assert s.device_cells() == cells                                          # the same cells, rows and cell_bytes
    assert [s.device_cells()[2] for s in w.snaps] == w.widths                    # a narrow snapshot stays narrow
