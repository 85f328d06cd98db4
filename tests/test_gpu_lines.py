"""lh_names_* / lh_lines* (Engine.device_names, Names.lines, Snapshot.spread_lines): wire lines for any per-name columns in
device memory, formatted on the device (graphite.go:37-48, opentsdb.go:45-58 over every key of a ProcessedMetricSet,
metrics.go:62-66).  The reference text is built here from the same inputs with oracle.format_f and
oracle.decompress_table(); every comparison is byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(__file__))
from test_gpu_serialize import GRAPHITE, TSDB, special_values  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [f"svc_{i}.rpc_latency" for i in range(37)] + ["x", "a_b_c_", "_lead", "empty_one"]
PLAIN = dict(prefix="", sep=" ", suffix="\n", underscore_to_dot=False)
_SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}
_FMT = {}


def dev(a):
    """A numpy array's bytes as a torch device tensor (unsigned types travel as the signed type of their width)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype))).cuda()


def fmt_f(v):
    key = np.float64(v).tobytes()
    if key not in _FMT:
        _FMT[key] = oracle.format_f(float(v))
    return _FMT[key]


def expect(names, ids, cols, wire, row_count=None, skip_nan=False):
    """The reference text: cols = [(label, float64 values per entry, valid per entry or None)], ids = the entries' names."""
    out = []
    for m, i in enumerate(ids):
        if i >= len(names) or (row_count is not None and row_count[m] == 0):
            continue
        for label, values, valid in cols:
            if (valid is not None and valid[m] == 0) or (skip_nan and np.isnan(values[m])):
                continue
            key = oracle.fmt_label(label, names[i])
            if wire["underscore_to_dot"]:
                key = key.replace("_", ".")
            out.append(f"{wire['prefix']}{key}{wire['sep']}{fmt_f(values[m])}{wire['suffix']}")
    return "".join(out).encode()


def same(got, want):
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [(k, a, b) for k, (a, b) in enumerate(zip(g, w)) if a != b][:3]
        raise AssertionError(f"{len(got)} bytes / {len(g)} lines against {len(want)} / {len(w)}; first differences {bad}")


def f64(a):
    return np.asarray(a).astype(np.float64)


@pytest.fixture(scope="module")
def world(native_lib, torch_cuda):
    import loghisto_amd
    with loghisto_amd.Engine(max_metrics=64, num_lanes=1, lane_samples=1 << 16) as eng:
        for nm in NAMES:
            eng.intern(nm)
        with eng.device_names() as names:
            assert names.count == len(NAMES)
            yield eng, names


def _integers(width):
    top = 2 ** width
    v = [int(x) for x in special_values() if np.isfinite(x) and 0 <= x < top]
    v += [0, 1, top - 1, top // 2, top // 2 + 1]
    if width == 64:   # float64(count) rounds half-even beyond 2^53
        v += [2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 64 - 1024, 2 ** 64 - 1025, 2 ** 64 - 1023, 2 ** 63 + 1024,
              2 ** 63 + 1025]
        v += [int(x) for x in np.random.default_rng(2).integers(0, 2 ** 64, 500, dtype=np.uint64)]
    return np.array(v, dtype=np.uint64 if width == 64 else np.uint32)


@pytest.mark.parametrize("wire", [GRAPHITE, TSDB], ids=["graphite", "opentsdb"])
@pytest.mark.parametrize("kind", ["f64", "u64", "u32"])
def test_values_print_as_go_prints_them(world, wire, kind):
    _, names = world
    v = special_values() if kind == "f64" else _integers(64 if kind == "u64" else 32)
    ids = (np.arange(v.size) * 7 % len(NAMES)).astype(np.uint32)
    got = names.lines([dict(label="%s_v", a=dev(v))], ids=dev(ids), **wire)
    same(got, expect(NAMES, ids, [("%s_v", f64(v), None)], wire))
    if kind == "f64":
        assert b" NaN" in got and b" +Inf" in got and b" -Inf" in got and b"18446744073709551616.000000" in got


def test_every_op_is_bit_exact_against_numpy(world):
    _, names = world
    rng = np.random.default_rng(4)
    n = 3000
    ids = rng.integers(0, len(NAMES), n).astype(np.uint32)
    ua = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    ub = rng.integers(0, 2 ** 40, n, dtype=np.uint64)
    wa = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    fa = rng.lognormal(3, 8, n) * np.where(rng.random(n) < 0.3, -1.0, 1.0)
    fb = rng.lognormal(0, 5, n)
    for arr in (ua, ub, wa, fa, fb):           # 0 / 0, x / 0, 0 / x, equal operands
        arr[:40] = 0
    ua[20:60] = rng.integers(1, 100, 40)
    fa[20:60] = rng.uniform(-5, 5, 40)
    ub[100:140] = ua[100:140]
    fa[200], fb[200], fa[201], fb[201], fa[202] = np.inf, np.inf, np.nan, 1.0, -0.0
    with np.errstate(all="ignore"):
        cols = [("%s_ratio_uu", dict(a=ua, b=ub, op="ratio"), f64(ua) / f64(ub)),
                ("%s_ratio_fu", dict(a=fa, b=ub, op="ratio"), fa / f64(ub)),
                ("%s_ratio_uf", dict(a=wa, b=fb, op="ratio"), f64(wa) / fb),
                ("%s_ratio_ff", dict(a=fa, b=fb, op="ratio"), fa / fb),
                ("%s_std_fu", dict(a=np.abs(fa), b=ub, op="sqrt_ratio"), np.sqrt(np.abs(fa) / f64(ub))),
                ("%s_std_uu", dict(a=ua, b=wa, op="sqrt_ratio"), np.sqrt(f64(ua) / f64(wa))),
                ("%s_std_neg", dict(a=fa, b=fb, op="sqrt_ratio"), np.sqrt(fa / fb)),
                ("%s_diff_uu", dict(a=ub, b=ua, op="diff"), f64(ub - ua)),              # wraps where a < b
                ("%s_diff_uw", dict(a=ua, b=wa, op="diff"), f64(ua - wa.astype(np.uint64))),
                ("%s_diff_wu", dict(a=wa, b=ub, op="diff"), f64(wa.astype(np.uint64) - ub)),
                ("%s_diff_ff", dict(a=fa, b=fb, op="diff"), fa - fb),
                ("%s_diff_uf", dict(a=ua, b=fb, op="diff"), f64(ua) - fb),              # one float: in float64
                ("%s_diff_fw", dict(a=fa, b=wa, op="diff"), fa - f64(wa)),
                ("100%%_%s", dict(a=wa), f64(wa))]
    assert (ub < ua).sum() > 1000 and np.isnan(cols[0][2]).sum() >= 20 and np.isinf(cols[0][2]).sum() >= 20
    spec = [dict(label=lab, op=c.get("op", "value"), a=dev(c["a"]), **({"b": dev(c["b"])} if "b" in c else {})) for lab, c, _ in cols]
    want = [(lab, v, None) for lab, _, v in cols]
    same(names.lines(spec, ids=dev(ids), **TSDB), expect(NAMES, ids, want, TSDB))
    same(names.lines(spec, ids=dev(ids), skip_nan=True, **GRAPHITE), expect(NAMES, ids, want, GRAPHITE, skip_nan=True))


def test_all_65536_keys_print_their_value(world):
    _, names = world
    keys = np.arange(-32768, 32768, dtype=np.int16)
    ids = (np.arange(keys.size) % len(NAMES)).astype(np.uint32)
    vals = oracle.decompress_table()[keys.view(np.uint16).astype(np.int64) ^ 0x8000]
    got = names.lines([dict(label="%s_upper", a=dev(keys), key=True)], ids=dev(ids), **PLAIN)
    same(got, expect(NAMES, ids, [("%s_upper", vals, None)], PLAIN))


def test_gates(world):
    import torch
    _, names = world
    rng = np.random.default_rng(6)
    n, np_ = len(NAMES), 5
    a = rng.normal(0, 100, (n, np_))
    a[rng.random((n, np_)) < 0.2] = np.nan
    valid = (rng.random((n, np_)) < 0.6).astype(np.uint8)
    count = rng.integers(0, 3, n).astype(np.uint64)
    count[-1] = 0                                                       # "empty_one"
    d_a, d_valid, d_count = dev(a), dev(valid), dev(count)
    spec = [dict(label=f"%s_p{i}", a=d_a[:, i], valid=d_valid[:, i]) for i in range(np_)]        # byte strides 40 and 5
    cols = [(f"%s_p{i}", a[:, i], valid[:, i]) for i in range(np_)]
    ids = np.arange(n)
    for skip in (False, True):
        same(names.lines(spec, row_count=d_count, skip_nan=skip, **GRAPHITE),
             expect(NAMES, ids, cols, GRAPHITE, row_count=count, skip_nan=skip))
        same(names.lines(spec, skip_nan=skip, **TSDB), expect(NAMES, ids, cols, TSDB, skip_nan=skip))
    got = names.lines(spec, row_count=d_count, **GRAPHITE)
    assert b"empty" not in got and b"NaN" in got
    # a call in which nothing emits
    assert names.lines(spec, row_count=torch.zeros_like(d_count), **TSDB) == b""
    assert names.lines([dict(label="%s_x", a=d_a[:, 0], valid=torch.zeros_like(d_valid)[:, 0])], **TSDB) == b""
    assert names.lines([dict(label="%s_x", a=torch.full_like(d_a, float("nan"))[:, 0])], skip_nan=True, **TSDB) == b""
    assert names.lines(spec, n=0, **TSDB) == b""


def test_rows_first_and_id_lists(world):
    _, names = world
    rng = np.random.default_rng(8)
    n = len(NAMES)
    v = rng.exponential(1e4, 200)
    spec = lambda t: [dict(label="%s_a", a=t), dict(label="pre_%s", a=t, b=t, op="diff")]     # noqa: E731
    cols = lambda x: [("%s_a", x, None), ("pre_%s", x - x, None)]                                # noqa: E731
    for first, cnt in ((0, n), (13, 21), (40, 1), (n, 0), (n - 1, 1)):
        same(names.lines(spec(dev(v[:cnt])), n=cnt, first=first, **TSDB), expect(NAMES, range(first, first + cnt), cols(v[:cnt]), TSDB))
    # duplicates, any order, ids at and beyond the names held: no line, no fault
    ids = np.array([5, 5, 40, 0, 41, 0xffffffff, 3, 64, 39, 2 ** 31, 5, 1000, 0], dtype=np.uint32)
    same(names.lines(spec(dev(v[:ids.size])), ids=dev(ids), **GRAPHITE), expect(NAMES, ids, cols(v[:ids.size]), GRAPHITE))
    wide = rng.integers(0, 80, 200).astype(np.uint32)
    assert (wide >= n).sum() > 50
    same(names.lines(spec(dev(v)), ids=dev(wide), **TSDB), expect(NAMES, wide, cols(v), TSDB))
    # a strided id list: every third element of an array
    same(names.lines(spec(dev(v[:67])), ids=dev(wide)[::3], **TSDB), expect(NAMES, wide[::3], cols(v[:67]), TSDB))


def test_a_block_beyond_the_names_held_is_a_range_error(world):
    from loghisto_amd import _native as N
    _, names = world
    t = dev(np.zeros(64))
    for first, n in ((0, 42), (41, 1), (42, 1), (1, 41), (0xffffffff, 2)):
        with pytest.raises(N.LhError) as e:
            names.lines([dict(label="%s_a", a=t)], n=n, first=first)
        assert e.value.code == N.ERANGE


def test_the_records_of_top_device_name_the_lines(world):
    import torch
    eng, names = world
    rng = np.random.default_rng(12)
    ids = rng.integers(0, 30, 50_000).astype(np.uint32)
    v = rng.lognormal(5, 2, ids.size) * (1 + ids)
    eng.submit_pairs(ids, v)
    with eng.flip() as snap:
        before = [x.copy() for x in snap.buckets_all(len(NAMES))]
        want = snap.top(12, "sum")
        for k in (12, 40):                               # 40: more wanted than there are -- the rest keeps its 0xff fill
            ent = torch.full((k * 32,), 0xff, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            snap.top(k, "sum", out=(ent, cnt))
            got = names.lines([dict(label="%s_count", a=ent.view(torch.int64).view(-1, 4)[:, 1]),
                               dict(label="%s_sum", a=ent.view(torch.float64).view(-1, 4)[:, 2])],
                              ids=ent.view(torch.int32).view(-1, 8)[:, 0], stream=snap.stream(), **GRAPHITE)   # stride 32
            full = snap.top(k, "sum")
            assert int(cnt.item()) == full.size == min(k, 30)
            same(got, expect(NAMES, full["id"], [("%s_count", f64(full["count"]), None), ("%s_sum", full["sum"], None)], GRAPHITE))
        assert np.array_equal(want["id"], full["id"][:12])
        after = snap.buckets_all(len(NAMES))
        assert all(np.array_equal(a, b) for a, b in zip(before, after))        # read-only


# ---- layout -------------------------------------------------------------------------------------------------------------
def test_every_16_byte_phase_of_the_output(world):
    _, names = world
    rng = np.random.default_rng(14)
    v = rng.lognormal(8, 4, 600)
    ids = rng.integers(0, len(NAMES), 600).astype(np.uint32)
    d_v, d_ids = dev(v), dev(ids)
    for plen in range(18):
        wire = dict(prefix="p" * plen, sep=" ", suffix="\n", underscore_to_dot=bool(plen & 1))
        same(names.lines([dict(label="%s_v", a=d_v)], ids=d_ids, **wire), expect(NAMES, ids, [("%s_v", v, None)], wire))


@pytest.mark.parametrize("n, ncols", [(1, 1), (255, 1), (256, 1), (257, 1), (85, 3), (64, 4), (2, 128), (3, 128), (41, 128)])
def test_workgroup_seams_and_many_columns(world, n, ncols):
    _, names = world
    rng = np.random.default_rng(n * 131 + ncols)
    a = rng.lognormal(2, 6, (n, ncols))
    ids = rng.integers(0, len(NAMES), n).astype(np.uint32)
    d_a = dev(a)
    spec = [dict(label=f"%s_c{j}", a=d_a[:, j]) for j in range(ncols)]
    same(names.lines(spec, ids=dev(ids), **GRAPHITE), expect(NAMES, ids, [(f"%s_c{j}", a[:, j], None) for j in range(ncols)], GRAPHITE))


def test_long_names_take_the_unstaged_path(native_lib, torch_cuda):
    """300 names of 200 bytes x 3 columns: a workgroup's 256 lines exceed its staging area in LDS and go straight to HBM;
    one name of 3 000 bytes among short ones."""
    import loghisto_amd
    long_names = [("n%03d_" % i) + "y_" * 97 + "z" for i in range(300)]
    assert all(len(s) == 200 for s in long_names)
    mixed = ["short", "q" * 3000, "a_b"]
    rng = np.random.default_rng(16)
    for names_list in (long_names, mixed):
        n = len(names_list)
        a = rng.lognormal(4, 3, (n, 3))
        with loghisto_amd.Engine(max_metrics=n) as eng:
            for s in names_list:
                eng.intern(s)
            with eng.device_names() as names:
                d_a = dev(a)
                spec = [dict(label=f"%s_c{j}", a=d_a[:, j]) for j in range(3)]
                cols = [(f"%s_c{j}", a[:, j], None) for j in range(3)]
                for wire in (GRAPHITE, TSDB):
                    same(names.lines(spec, **wire), expect(names_list, range(n), cols, wire))


# ---- sizing ---------------------------------------------------------------------------------------------------------------
def test_size_then_call(world):
    import torch
    from loghisto_amd import _native as N
    _, names = world
    L = N.lib()
    v = np.random.default_rng(18).lognormal(3, 3, len(NAMES))
    d_v = dev(v)
    want = expect(NAMES, range(len(NAMES)), [("%s_v", v, None)], TSDB)
    col = (N.LhColumn * 1)(N.LhColumn(b"%s_v", d_v.data_ptr(), 0, 0, 8, 0, 0, N.COL_F64, 0, N.OP_VALUE, 0, 0))
    fmt = N.LhLineFormat(TSDB["prefix"].encode(), TSDB["sep"].encode(), TSDB["suffix"].encode(), 0, 0)
    lead = (names._h, 0, len(NAMES), None, 0, col, 1, C.byref(fmt), 0, None)
    need = C.c_size_t(0)
    assert L.lh_lines(*lead, None, 0, C.byref(need)) == 0 and need.value == len(want)          # out NULL: the size
    buf = C.create_string_buffer(b"\xaa" * (len(want) + 8), len(want) + 8)
    need = C.c_size_t(0)
    assert L.lh_lines(*lead, buf, len(want) - 1, C.byref(need)) == 0                             # one byte short
    assert need.value == len(want) and buf.raw == b"\xaa" * (len(want) + 8)
    assert L.lh_lines(*lead, buf, len(want), C.byref(need)) == 0                                 # the exact fit
    assert need.value == len(want) and buf.raw == want + b"\xaa" * 8                             # no trailing NUL
    # the device form: d_len always, d_out only when the total fits; d_out at every alignment
    for cap, off in ((len(want) - 1, 0), (len(want), 0), (len(want), 1), (len(want) + 5, 7), (len(want), 13), (0, 0)):
        text = torch.full((len(want) + 64,), 0xaa, dtype=torch.uint8, device="cuda")
        d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert names.lines([dict(label="%s_v", a=d_v)], out=(text[off:off + cap], d_len), **TSDB)[1] is d_len
        torch.cuda.synchronize()
        got = bytes(text.cpu().numpy())
        assert int(d_len.item()) == len(want)
        if cap >= len(want):
            assert got == b"\xaa" * off + want + b"\xaa" * (64 - off)
        else:
            assert got == b"\xaa" * (len(want) + 64)
    # the device form's empty call stores the total too
    d_len = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    names.lines([dict(label="%s_v", a=d_v)], n=0, out=(torch.zeros(8, dtype=torch.uint8, device="cuda"), d_len), **TSDB)
    torch.cuda.synchronize()
    assert int(d_len.item()) == 0


# ---- the handle -------------------------------------------------------------------------------------------------------------
def test_names_interned_later_arrive_with_refresh(native_lib, torch_cuda):
    import loghisto_amd
    first, later = [f"early_{i}" for i in range(7)], [f"late_{i}" for i in range(10)]
    v = np.arange(17, dtype=np.float64) + 0.25
    ids = np.arange(17, dtype=np.uint32)[::-1].copy()
    with loghisto_amd.Engine(max_metrics=32) as eng:
        for s in first:
            eng.intern(s)
        with eng.device_names() as names, eng.device_names() as other:
            for s in later:
                eng.intern(s)
            spec = [dict(label="%s_v", a=dev(v))]
            same(names.lines(spec, ids=dev(ids), **TSDB), expect(first, ids, [("%s_v", v, None)], TSDB))     # ids beyond: nothing
            assert names.count == 7 and names.refresh() == 17 and other.count == 7
            same(names.lines(spec, ids=dev(ids), **TSDB), expect(first + later, ids, [("%s_v", v, None)], TSDB))
            same(other.lines(spec, ids=dev(ids), **TSDB), expect(first, ids, [("%s_v", v, None)], TSDB))
            assert other.refresh() == 17 and names.refresh() == 17
            assert other.lines(spec, **GRAPHITE) == names.lines(spec, **GRAPHITE) == expect(first + later, range(17), [("%s_v", v, None)],
                                                                                            GRAPHITE)
    with loghisto_amd.Engine(max_metrics=4) as eng:            # an engine without names yet
        with eng.device_names() as names:
            assert names.count == 0 and names.lines([dict(label="%s_v", a=dev(v))], ids=dev(ids)) == b""
            eng.intern("only")
            assert names.refresh() == 1 and names.lines([dict(label="%s_v", a=dev(v))], **PLAIN) == b"only_v 0.250000\n"


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interval(native_lib, torch_cuda):
    """1 000 names (the last 50 without samples), lognormal pairs, flipped once."""
    import loghisto_amd
    M = 1000
    rng = np.random.default_rng(20)
    n = 400_000
    ids = rng.integers(0, M - 50, n).astype(np.uint32)
    v = rng.lognormal(9.0, 1.5, n) * (1.0 + 0.01 * ids)
    names_list = [f"api_{i:04d}.latency_us" for i in range(M)]
    with loghisto_amd.Engine(max_metrics=M, num_lanes=1, lane_samples=1 << 19) as eng:
        for s in names_list:
            eng.intern(s)
        eng.submit_pairs(ids, v)
        with eng.device_names() as names, eng.flip() as snap:
            yield eng, names, snap, names_list


def test_spread_lines_equal_the_text_built_from_spread(interval):
    _, names, snap, names_list = interval
    M = len(names_list)
    before = [x.copy() for x in snap.buckets_all(M)]
    ps = list(oracle.DEFAULT_PERCENTILES.values()) + [1.5]             # (1.5: no bucket, its keys are omitted)
    tags = ["0", "50", "75", "90", "95", "99", "99.9", "99.99", "100", "150"]
    host = snap.spread(ps)
    assert (host["count"] == 0).sum() == 50
    cols = [("%s_std", host["std"], None)]
    for i, tag in enumerate(tags):
        ok = host["pvalid"][:, i]
        cols += [(f"%s_mean_{tag}", host["mean_le"][:, i], ok), (f"%s_upper_{tag}", host["upper"][:, i], ok),
                 (f"%s_count_{tag}", f64(host["count_le"][:, i]), ok), (f"%s_sum_{tag}", host["sum_le"][:, i], ok)]
    for wire in (GRAPHITE, TSDB):
        got = snap.spread_lines(names, ps, **wire)
        same(got, expect(names_list, range(M), cols, wire, row_count=host["count"]))
    assert got.count(b"\n") == 950 * (1 + 4 * 9) and b"_150 " not in got
    part = snap.spread_lines(names, {"median": 0.5}, first=100, nmetrics=30, **TSDB)
    same(part, expect(names_list, range(100, 130), [(lab.replace("_50", "_median"), x[100:130], None if ok is None else ok[100:130])
                                                    for lab, x, ok in cols[:1] + cols[5:9]], TSDB, row_count=host["count"][100:130]))
    after = snap.buckets_all(M)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))            # read-only


def test_count_le_buckets_as_lines(interval):
    import torch
    _, names, snap, names_list = interval
    M = len(names_list)
    bounds = [1e3, 1e4, 1e5, 1e6]
    host = snap.count_le(bounds)
    cum = torch.empty((M, len(bounds)), dtype=torch.int64, device="cuda")
    total = torch.empty((M,), dtype=torch.int64, device="cuda")
    snap.count_le(bounds, out=(cum, total))
    spec, cols = [], []
    for j, b in enumerate(bounds):
        spec += [dict(label="%s_le_" + "%g" % b, a=cum[:, j]), dict(label="%s_above_" + "%g" % b, a=total, b=cum[:, j], op="diff")]
        cols += [("%s_le_" + "%g" % b, f64(host["cum"][:, j]), None), ("%s_above_" + "%g" % b, f64(host["total"] - host["cum"][:, j]), None)]
    spec.append(dict(label="%s_le_+Inf", a=total))
    cols.append(("%s_le_+Inf", f64(host["total"]), None))
    got = names.lines(spec, row_count=total, stream=snap.stream(), **TSDB)
    same(got, expect(names_list, range(M), cols, TSDB, row_count=host["total"]))
    assert got.count(b"\n") == 950 * 9


def test_across_ids_columns_equal_the_lines_of_serialize(interval):
    import torch
    _, names, snap, names_list = interval
    pct = dict(oracle.DEFAULT_PERCENTILES)
    pct["p%s_bad"] = 1.5
    labels = list(pct)
    ids = np.array([17, 3, 960, 500, 17, 949, 0, 999], dtype=np.uint32)       # 960 and 999 have no samples
    d_ids = dev(ids)
    n, np_ = ids.size, len(labels)
    out = dict(count=torch.empty(n, dtype=torch.int64, device="cuda"), sum=torch.empty(n, dtype=torch.float64, device="cuda"),
               pkeys=torch.empty((n, np_), dtype=torch.int16, device="cuda"), pvalid=torch.empty((n, np_), dtype=torch.uint8, device="cuda"))
    snap.across_ids(d_ids, (), [pct[k] for k in labels], out=out)
    spec = [dict(label="%s_count", a=out["count"]), dict(label="%s_sum", a=out["sum"])]
    spec += [dict(label=lab, a=out["pkeys"][:, i], key=True, valid=out["pvalid"][:, i]) for i, lab in enumerate(labels)]
    for wire in (GRAPHITE, TSDB):
        got = names.lines(spec, ids=d_ids, row_count=out["count"], stream=snap.stream(), **wire)
        sums = out["sum"].cpu().numpy()
        want = []
        for m, i in enumerate(ids):
            key = names_list[i].replace("_", ".") if wire["underscore_to_dot"] else names_list[i]
            for ln in snap.serialize(pct, first=int(i), nmetrics=1, **wire).split(b"\n")[:-1]:
                kind = ln[len(wire["prefix"]) + len(key):].split(b" ")[0]
                if kind in (b"_avg", b".avg"):
                    continue
                if kind in (b"_sum", b".sum"):     # lh_across' own sum, which may differ from lh_stats.sum in the last bits
                    sk = "_sum".replace("_", ".") if wire["underscore_to_dot"] else "_sum"
                    ln = f"{wire['prefix']}{key}{sk}{wire['sep']}{fmt_f(sums[m])}{wire['suffix']}".encode()[:-1]
                want.append(ln + b"\n")
        same(got, b"".join(want))
        assert got.count(b"\n") == 6 * (2 + 9)
