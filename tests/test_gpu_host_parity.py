"""The C++ MetricSystem (include/loghisto.hpp, loghisto_amd/csrc/host/metric_system.cc) held to the oracle cell by cell and key
by key.  Python writes a scenario (seeded numpy), tests/cpp/host_parity.cc replays it through a MetricSystem in ONE child
process per case and dumps every interval; the checks are all here.

Stepped scenarios: producers replay step j and meet at a barrier, the main thread collects -- what interval j must hold is
fully determined.  Per interval and per name: raw cells == oracle.histogram_pairs of exactly that interval's events; names
without an event are absent from Histograms() and own no key; _count == the cell sum; every percentile key bit-identical to
oracle.process_dense; |_sum - exact| <= 1e-12 x sum |D[b] C[b]| with exact a fractions.Fraction (the project's _sum rule,
tests/test_gpu_across.py); _avg == reported sum / float64(count) bit for bit; _agg_count the running count, _agg_sum the sum of
oracle.f64_to_u64_amd64(reported _sum) mod 2^64 (test_serialize_aggregates_and_lifetime's rule), _agg_avg their integer
quotient; counters' rates and lifetime totals; the wire text, sorted by line, == oracle.wire_lines + the host's lines.
Concurrent scenarios: the cells conserved per (name, key) over all intervals, every interval consistent with its own cells.

A child that dies by a signal, with 134 or 139, or at its timeout ends the module: every later case skips, nothing more is
started on the GPU from this file.  The one test without the gpu mark replays counters only and pins both file formats."""
import os
import socket
import struct
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYER = os.path.join(ROOT, "loghisto_amd", "build", "host_parity")
NK = oracle.NKEYS
U64 = np.uint64
HIST, COUNTER = 0, 1
NO_COLLECT, COLLECT, KEEP = 0, 1, 2
LH_ENODEVICE, LH_EBUSY = 4, 5
MIN_LANE_SAMPLES = 2                                  # lh_create: cfg->lane_samples < 2 is LH_EINVAL (lh_engine.cc)
CUSTOM_PCT = {"%s_p50": 0.5, "q99.9_%s": 0.999, "%s_bad": 1.5, "%s_lo": 0.0, "100%%_%s": 1.0, "%s_p25": 0.25}

_TROUBLE = []                                         # module state: why nothing more may be started from this file


# ---- scenario and dump files (layouts: tests/cpp/host_parity.cc) -----------------------------------------------------------
def scenario(names, steps, flags, T, *, max_metrics=1024, num_buffers=3, num_lanes=2, stage_samples=64,
             lane_samples=MIN_LANE_SAMPLES, device_counters=False, max_counters=64, concurrent=False, wire=0,
             keys_in_map=True, pct=None):
    """steps[j][t] = (kind uint8[], name index uint32[], payload uint64[])."""
    assert len(steps) == len(flags) and all(len(s) == T for s in steps)
    return types.SimpleNamespace(**locals())


def _s(text):
    b = text.encode()
    return struct.pack("<I", len(b)) + b


def write_scenario(path, sc):
    out = [b"LHSCN001", struct.pack("<IIIIQIIIII", sc.max_metrics, sc.num_buffers, sc.num_lanes, sc.stage_samples,
                                    sc.lane_samples, int(sc.device_counters), sc.max_counters, int(sc.concurrent), sc.wire,
                                    int(sc.keys_in_map))]
    if sc.pct is None:
        out.append(struct.pack("<i", -1))
    else:
        out.append(struct.pack("<i", len(sc.pct)))
        out += [_s(k) + struct.pack("<d", p) for k, p in sc.pct.items()]
    out.append(struct.pack("<I", len(sc.names)))
    out += [_s(n) for n in sc.names]
    out.append(struct.pack("<II", sc.T, len(sc.steps)))
    out.append(np.asarray(sc.flags, dtype="<u4").tobytes())
    for step in sc.steps:
        for kind, name, payload in step:
            assert len(kind) == len(name) == len(payload)
            out += [struct.pack("<I", len(kind)), np.asarray(kind, dtype="u1").tobytes(),
                    np.asarray(name, dtype="<u4").tobytes(), np.asarray(payload, dtype="<u8").tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(out))


class _Cursor:
    def __init__(self, data):
        self.b, self.at = data, 0

    def get(self, fmt):
        v = struct.unpack_from("<" + fmt, self.b, self.at)
        self.at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def str(self):
        n = self.get("I")
        self.at += n
        return self.b[self.at - n:self.at]

    def array(self, dtype, n):
        a = np.frombuffer(self.b, dtype=dtype, count=n, offset=self.at)
        self.at += a.nbytes
        return a

    def pairs(self, fmt):
        return {self.str().decode(): self.get(fmt) for _ in range(self.get("I"))}


def parse_dump(path):
    with open(path, "rb") as f:
        c = _Cursor(f.read())
    assert c.b[:8] == b"LHDMP001"
    c.at = 8
    intervals, end = [], None
    while c.at < len(c.b):
        tag = c.get("I")
        if tag == 2:
            status, dropped, ready = c.get("iQI")
            end = types.SimpleNamespace(status=status, dropped=dropped, engine_ready=bool(ready))
            break
        assert tag == 1, tag
        iv = types.SimpleNamespace()
        iv.step, iv.status, iv.dropped, iv.time_ns, iv.has_snapshot = c.get("IiQqI")
        iv.hist = {}
        for _ in range(c.get("I")):
            name, n = c.str().decode(), c.get("I")
            iv.hist[name] = (c.array("<i2", n), c.array("<u8", n))
        iv.rates, iv.counters, iv.gauges, iv.metrics = c.pairs("Q"), c.pairs("Q"), c.pairs("Q"), c.pairs("Q")   # floats: bits
        iv.wire_format = c.get("I")
        iv.wire = c.str()
        intervals.append(iv)
    assert end is not None and c.at == len(c.b), "the dump has no end record: the replayer did not finish"
    return types.SimpleNamespace(intervals=intervals, end=end)


def replay(sc, tmp_path, timeout):
    """One child process; trouble (signal, abort, segmentation fault, timeout) ends the module."""
    if _TROUBLE:
        pytest.skip("nothing more is started from this file: " + _TROUBLE[0])
    spath, dpath = str(tmp_path / "scenario.bin"), str(tmp_path / "dump.bin")
    write_scenario(spath, sc)
    try:
        r = subprocess.run([REPLAYER, spath, dpath], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired:
        _TROUBLE.append(f"host_parity did not finish within {timeout} s")
        pytest.fail(_TROUBLE[0])
    tail = r.stdout.decode(errors="replace")[-2000:]
    if r.returncode < 0 or r.returncode in (134, 139):
        _TROUBLE.append(f"host_parity ended with status {r.returncode}")
        pytest.fail(_TROUBLE[0] + "\n" + tail)
    assert r.returncode == 0, tail
    return parse_dump(dpath)


# ---- values ----------------------------------------------------------------------------------------------------------------
def _pool_bits():
    from tests import _adversarial_values as AV
    special = np.array([0.0, np.inf, 5e-324, 1.7976931348623157e308], dtype=np.float64).view(U64)
    nans = np.array([0x7ff8000000000001, 0x7ff800000badcafe, 0x7ff0000000000001, 0x7ff4aaaaaaaaaaaa], dtype=U64)
    special = np.concatenate([special, nans])
    special = np.concatenate([special, special | U64(1 << 63)])        # -0.0, -Inf, -5e-324, -MaxFloat64, NaNs with the sign
    adv = AV.full_set()                                                  # threshold-adjacent doubles, both signs
    adv = adv[np.random.default_rng(1234).integers(0, adv.size, 4096)].view(U64)
    return np.concatenate([np.tile(special, 32), adv])


_POOL = []


def draw_bits(rng, name_idx):
    """float64 bit patterns for events of the given names: lognormal around a per-name centre, 15 % negative, 20 % from the
    pool of specials and threshold-adjacent doubles."""
    n = len(name_idx)
    if n == 0:
        return np.zeros(0, dtype=U64)
    if not _POOL:
        _POOL.append(_pool_bits())
    v = rng.lognormal(3.0 + (np.asarray(name_idx) % 9), 2.0, n)
    v[rng.random(n) < 0.15] *= -1.0
    bits = v.view(U64).copy()
    sel = rng.random(n) < 0.2
    bits[sel] = _POOL[0][rng.integers(0, _POOL[0].size, int(sel.sum()))]
    return bits


def hist_names(n):
    return [f"svc_{i % 7}.lat_{i:04d}" for i in range(n)]


CTR_NAMES = ["req_total", "bytes.in", "bytes_out", "errs", "big"]


def thread_events(rng, n_hist, hist_pool, n_names, n_ctr):
    """One thread's list for one step: n_hist Histogram events over the names in hist_pool, n_ctr Counter events (counter k
    is name n_names + k), shuffled together."""
    hn = hist_pool[rng.integers(0, len(hist_pool), n_hist)].astype(np.uint32) if n_hist else np.zeros(0, np.uint32)
    hb = draw_bits(rng, hn)
    cn = rng.integers(0, len(CTR_NAMES), n_ctr).astype(np.uint32)
    amt = rng.integers(0, 1000, n_ctr).astype(U64)
    amt[cn == 1] += U64(1 << 31)                        # two such events pass 2^32
    amt[cn == 4] = U64((1 << 62) + 12345)               # the lifetime total wraps 2^64 after four
    kind = np.concatenate([np.full(n_hist, HIST, np.uint8), np.full(n_ctr, COUNTER, np.uint8)])
    name = np.concatenate([hn, cn + np.uint32(n_names)])
    payload = np.concatenate([hb, amt])
    order = rng.permutation(kind.size)
    return kind[order], name[order], payload[order]


def stepped_scenario(seed, n_names, *, stage_samples, T=4, extra_steps=(), flags=None, **opts):
    """Thread step lengths rotate through 0, 1, S - 1, S, S + 1 (S = stage_samples); one step in which nobody submits anything;
    one step of several x num_lanes x lane_samples events per thread, longer than a stage, so that the producers ship
    concurrently, lanes are reused and wait for their previous launch inside one interval.  The names of a step come from a
    random half of a prefix of the name list that grows from a third to all of it: names appear for the first time in later
    steps, and names interned earlier go without events."""
    rng = np.random.default_rng(seed)
    S = stage_samples
    lens = [0, 1, S - 1, S, S + 1]
    big = 3 * S + 5 * opts.get("num_lanes", 2) * opts.get("lane_samples", MIN_LANE_SAMPLES) + 1
    plan = [[lens[(j + t) % 5] for t in range(T)] for j in range(5)]
    plan.insert(2, [0] * T)                                                  # nobody submits anything
    plan.insert(4, [big + t for t in range(T)])
    plan += list(extra_steps)
    steps = []
    for j, row in enumerate(plan):
        avail = max(1, n_names * (j + 2) // (len(plan) + 1)) if j < len(plan) - 1 else n_names
        pool = rng.choice(avail, size=max(1, avail // 2), replace=False)
        quiet = not any(row)
        steps.append([thread_events(rng, n, pool, n_names, 0 if quiet else int(rng.integers(0, 5))) for n in row])
    flags = [COLLECT] * len(plan) if flags is None else flags
    return scenario(hist_names(n_names) + CTR_NAMES, steps, flags, T, stage_samples=S, **opts)


# ---- the model -------------------------------------------------------------------------------------------------------------
def model_rows(ids, bits):
    """{name index: (bins ascending, counts)} of oracle.histogram_pairs over the events, dense 128 names at a time."""
    out = {}
    if not len(ids):
        return out
    present, compact = np.unique(ids, return_inverse=True)
    vals = np.ascontiguousarray(bits, dtype=U64).view(np.float64)
    for lo in range(0, present.size, 128):
        sel = (compact >= lo) & (compact < lo + 128)
        rows = oracle.histogram_pairs((compact[sel] - lo).astype(np.uint32), vals[sel], min(128, present.size - lo))
        r, b = np.nonzero(rows)
        cut = np.searchsorted(r, np.arange(rows.shape[0] + 1))
        for i in range(rows.shape[0]):
            bb = b[cut[i]:cut[i + 1]]
            out[int(present[lo + i])] = (bb.astype(np.int64), rows[i, bb].copy())
    return out


def cells_of(keys, counts):
    bins = oracle.key_to_bin(keys)
    assert np.all(np.diff(bins) > 0), "Histograms() keys are not ascending"
    return bins, np.asarray(counts, dtype=U64)


class Exact:
    """Sums of D[b] C[b] as Python integers scaled by 2^-EMIN: the fractions.Fraction sum without one Fraction per cell."""

    def __init__(self):
        self.D = oracle.decompress_table()
        mant, ex = np.frexp(self.D)
        self.mant = (mant * 2.0 ** 53).astype(np.int64)
        self.ex = ex.astype(np.int64) - 53
        self.emin = int(self.ex.min())
        self.unit = Fraction(2) ** self.emin
        self.cache = {}
        self.row = np.zeros(NK, dtype=U64)

    def term(self, b):
        t = self.cache.get(b)
        if t is None:
            t = self.cache[b] = int(self.mant[b]) << int(self.ex[b] - self.emin)
            assert Fraction(t) * self.unit == Fraction(float(self.D[b]))
        return t

    def sums(self, bins, counts):
        terms = [self.term(int(b)) * int(c) for b, c in zip(bins, counts)]
        return sum(terms) * self.unit, sum(abs(t) for t in terms) * self.unit


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def bits_of(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def check_name(ex, metrics, name, bins, counts, labels, ps, at):
    """_count, every percentile key, _sum and _avg of one name against its cells; returns (count, reported _sum, keys)."""
    ex.row[bins] = counts
    ref = oracle.process_dense(ex.row, ps)
    ex.row[bins] = 0
    count = int(sum(int(c) for c in counts))
    assert ref["count"] == count
    keys = {f"{name}_count", f"{name}_sum", f"{name}_avg"}
    assert metrics.get(f"{name}_count") == bits_of(float(count)), (at, name, "_count")
    for i, lab in enumerate(labels):
        key = oracle.fmt_label(lab, name)
        if ref["pvalid"][i]:
            keys.add(key)
            assert metrics.get(key) == bits_of(float(ref["pvals"][i])), (at, key, metrics.get(key), float(ref["pvals"][i]))
        else:
            assert key not in metrics, (at, key, "an invalid percentile has a key")
    got = f64(metrics[f"{name}_sum"])
    exact, mag = ex.sums(bins, counts)
    assert np.isfinite(got), (at, name, got)
    err = abs(Fraction(got) - exact)
    assert err <= Fraction(1, 10 ** 12) * mag, (at, name, "_sum", got, float(exact), float(err), float(mag))
    assert metrics.get(f"{name}_avg") == bits_of(got / float(count)), (at, name, "_avg")
    return count, got, keys


def wire_shape(wire, t, host):
    if wire == 1:
        return dict(prefix=f"cockroach.{host}.", sep=" ", suffix=f" {t}\n", underscore_to_dot=True)
    return dict(prefix="put ", sep=f" {t} ", suffix=f" host={host}\n", underscore_to_dot=False)


def host_lines(iv, shape):
    vals = {k: float(v) for k, v in iv.counters.items()}
    vals.update({k + "_rate": float(v) for k, v in iv.rates.items()})
    vals.update({k: f64(v) for k, v in iv.gauges.items()})
    out = []
    for k, v in vals.items():
        k = k.replace("_", ".") if shape["underscore_to_dot"] else k
        out.append(f"{shape['prefix']}{k}{shape['sep']}{oracle.format_f(v)}{shape['suffix']}")
    return out


def step_events(step, n_names):
    kind = np.concatenate([e[0] for e in step])
    name = np.concatenate([e[1] for e in step])
    payload = np.concatenate([e[2] for e in step])
    h = kind == HIST
    assert np.all(name[h] < n_names) and np.all(name[~h] >= n_names)
    return name[h], payload[h], name[~h], payload[~h]


def check_stepped(sc, dump):
    ex = Exact()
    n_names = len(sc.names) - len(CTR_NAMES)
    pct = oracle.DEFAULT_PERCENTILES if sc.pct is None else sc.pct
    labels = sorted(pct)                                                       # std::map order
    ps = [pct[k] for k in labels]
    host = socket.gethostname()
    life_c, life_s, totals = {}, {}, {}
    pend_ids, pend_bits, pend_ctr = [], [], {}
    engine = seen_busy = False
    kept_live = 0
    intervals = iter(dump.intervals)
    sums_by_step = {}
    for j, flag in enumerate(sc.flags):
        hid, hbits, cid, camt = step_events(sc.steps[j], n_names)
        pend_ids.append(hid)
        pend_bits.append(hbits)
        for c, a in zip(cid.tolist(), camt.tolist()):
            pend_ctr[sc.names[c]] = (pend_ctr.get(sc.names[c], 0) + a) % (1 << 64)
        engine = engine or hid.size > 0 or (sc.device_counters and cid.size > 0)
        if flag == NO_COLLECT:
            continue
        iv = next(intervals)
        at = f"step {j}"
        busy = engine and kept_live >= sc.num_buffers - 1
        flipped = engine and not busy
        seen_busy = seen_busy or busy
        assert iv.step == j and iv.dropped == 0
        assert bool(iv.has_snapshot) == flipped, (at, iv.has_snapshot, flipped)
        assert iv.status == (LH_EBUSY if seen_busy else 0), (at, iv.status)       # last_status() keeps the last non-zero code
        # counters: host maps are stolen at every collect, device counters come back with the snapshot
        if flipped or not sc.device_counters:
            rates, pend_ctr = pend_ctr, {}
        else:
            rates = {}
        for k, a in rates.items():
            totals[k] = (totals.get(k, 0) + a) % (1 << 64)
        assert iv.rates == rates, (at, iv.rates, rates)
        assert iv.counters == totals, (at, iv.counters, totals)
        assert iv.gauges == {}
        want_keys = set(totals) | {k + "_rate" for k in rates}
        for k, a in totals.items():
            assert iv.metrics.get(k) == bits_of(float(a)), (at, k)
        for k, a in rates.items():
            assert iv.metrics.get(k + "_rate") == bits_of(float(a)), (at, k)
        if not flipped:                                                         # LH_EBUSY (or no engine yet): no histogram key
            assert iv.hist == {} and set(iv.metrics) == want_keys, (at, sorted(set(iv.metrics) ^ want_keys)[:8])
            assert iv.wire_format == 0 and iv.wire == b""
            kept_live = 0 if flag == COLLECT else kept_live      # (a raw set without a snapshot holds no buffer)
            continue
        rows = model_rows(np.concatenate(pend_ids), np.concatenate(pend_bits))
        pend_ids, pend_bits = [], []
        # raw cells, and only the names with an event in this interval
        assert set(iv.hist) == {sc.names[i] for i in rows}, (at, sorted(set(iv.hist) ^ {sc.names[i] for i in rows})[:8])
        for i, (bins, counts) in rows.items():
            gb, gc = cells_of(*iv.hist[sc.names[i]])
            assert np.array_equal(gb, bins) and np.array_equal(gc, counts), (at, sc.names[i])
        sums = {}
        if sc.keys_in_map:
            for i, (bins, counts) in rows.items():
                name = sc.names[i]
                count, got, keys = check_name(ex, iv.metrics, name, bins, counts, labels, ps, at)
                sums[i] = got
                life_c[i] = life_c.get(i, 0) + count
                life_s[i] = (life_s.get(i, 0) + oracle.f64_to_u64_amd64(got)) % (1 << 64)
                assert iv.metrics.get(f"{name}_agg_count") == bits_of(float(life_c[i])), (at, name, "_agg_count")
                assert iv.metrics.get(f"{name}_agg_sum") == bits_of(float(life_s[i])), (at, name, "_agg_sum")
                assert iv.metrics.get(f"{name}_agg_avg") == bits_of(float(life_s[i] // life_c[i])), (at, name, "_agg_avg")
                want_keys |= keys | {f"{name}_agg_count", f"{name}_agg_sum", f"{name}_agg_avg"}
        # nothing else: no key of an absent name, no invalid percentile, no _agg_* of a name without events
        assert set(iv.metrics) == want_keys, (at, sorted(set(iv.metrics) ^ want_keys)[:8])
        sums_by_step[j] = sums
        if sc.wire and sc.keys_in_map:
            assert iv.wire_format == sc.wire
            shape = wire_shape(sc.wire, iv.time_ns // 10 ** 9, host)
            order = sorted(rows)
            dense = np.zeros((len(order), NK), dtype=U64)
            for r, i in enumerate(order):
                dense[r, rows[i][0]] = rows[i][1]
            want = oracle.wire_lines([sc.names[i] for i in order], dense, {k: pct[k] for k in labels},
                                     life=([life_c[i] for i in order], [life_s[i] for i in order]),
                                     sums=[sums[i] for i in order], **shape) + host_lines(iv, shape)
            got = iv.wire.decode().split("\n")
            assert got[-1] == "" and sorted(got[:-1]) == sorted(w.rstrip("\n") for w in want), at
        elif not sc.wire:
            assert iv.wire_format == 0 and iv.wire == b""
        if flag == KEEP:
            kept_live += 1
        else:
            kept_live = 0
    assert next(intervals, None) is None
    assert dump.end.dropped == 0 and dump.end.engine_ready == engine
    return sums_by_step


# ---- stepped cases ---------------------------------------------------------------------------------------------------------
STEPPED = {
    # name count -> max_metrics just above it; the host lanes' launches take the few-name kernel at 3 names and the direct
    # kernel above (lh_dispatch.cc: a lane's half-buffer goes to PATH_SMALL or PATH_DIRECT unless lane blocks are switched on)
    "3-names-graphite": dict(seed=1, n_names=3, max_metrics=4, stage_samples=64, wire=1),
    "40-names-device-counters-opentsdb": dict(seed=2, n_names=40, max_metrics=64, stage_samples=64, wire=2,
                                              device_counters=True, pct=CUSTOM_PCT),
    "300-names-stage-4096": dict(seed=3, n_names=300, max_metrics=1024, stage_samples=4096, pct=CUSTOM_PCT),
    "2000-names-device-counters": dict(seed=4, n_names=2000, max_metrics=2048, stage_samples=64, device_counters=True,
                                       num_lanes=3, extra_steps=([5000, 4000, 3000, 2001],)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(STEPPED))
def test_stepped_intervals_match_the_oracle(native_lib, torch_cuda, tmp_path, case):
    sc = stepped_scenario(**STEPPED[case])
    check_stepped(sc, replay(sc, tmp_path, timeout=40))


@pytest.mark.gpu
def test_stepped_uint32_reservations_past_65536_names(native_lib, torch_cuda, tmp_path):
    """max_metrics = 65 537 (two 16.1 GiB epoch buffers of 32-bit cells): the stages ship uint32 ids through lh_reserve_pairs.
    300 names are in use; the name count of the engine is what selects the path.
    Measured on an MI355X: the whole replay -- process start, lh_create, seven intervals, dump -- takes 0.28 - 0.35 s of wall
    clock here against 0.41 - 0.43 s for the same scenario at max_metrics = 1024, the engine size of metrics_test's creates
    (default Options): the create costs nothing that shows, so the engine keeps its 65 537 names."""
    sc = stepped_scenario(seed=5, n_names=300, max_metrics=65537, num_buffers=2, stage_samples=64, pct=CUSTOM_PCT)
    check_stepped(sc, replay(sc, tmp_path, timeout=60))


def busy_scenario():
    """num_buffers = 2: one kept raw set makes the next lh_flip LH_EBUSY.  Steps: 0 collect; 1 collect and keep; 2 collect ->
    busy, no histogram key, this step's host counters, then everything is released; 3 collect -> the union of steps 2 and 3;
    4 no collect; 5 collect -> the union of 4 and 5."""
    rng = np.random.default_rng(6)
    n_names, T = 40, 3
    pools = [np.arange(0, 20), np.arange(10, 30), np.arange(5, 25), np.arange(15, 40), np.arange(0, 8), np.arange(4, 12)]
    steps = [[thread_events(rng, 70 + 13 * t + j, pool, n_names, 3) for t in range(T)] for j, pool in enumerate(pools)]
    flags = [COLLECT, KEEP, COLLECT, COLLECT, NO_COLLECT, COLLECT]
    return scenario(hist_names(n_names) + CTR_NAMES, steps, flags, T, max_metrics=64, num_buffers=2, stage_samples=64, wire=1)


@pytest.mark.gpu
def test_busy_flip_keeps_the_epoch_for_the_next_interval(native_lib, torch_cuda, tmp_path):
    sc = busy_scenario()
    dump = replay(sc, tmp_path, timeout=40)
    check_stepped(sc, dump)
    assert [iv.status for iv in dump.intervals] == [0, 0, LH_EBUSY, LH_EBUSY, LH_EBUSY]
    assert [iv.has_snapshot for iv in dump.intervals] == [1, 1, 0, 1, 1] and dump.intervals[2].rates


def _lines_without_time(iv):
    t = str(iv.time_ns // 10 ** 9).encode()
    return sorted(line.replace(b" " + t, b" T") for line in iv.wire.split(b"\n"))


@pytest.mark.gpu
def test_histogram_keys_out_of_the_map_leave_the_text_unchanged(native_lib, torch_cuda, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    opts = dict(seed=7, n_names=40, max_metrics=64, stage_samples=64, wire=1, pct=CUSTOM_PCT)
    with_map = stepped_scenario(**opts)
    a = replay(with_map, tmp_path / "a", timeout=40)
    check_stepped(with_map, a)
    without = stepped_scenario(keys_in_map=False, **opts)
    b = replay(without, tmp_path / "b", timeout=40)
    check_stepped(without, b)                            # raw cells, counters, and no histogram key in the map
    assert len(a.intervals) == len(b.intervals)
    for x, y in zip(a.intervals, b.intervals):
        assert y.wire_format == x.wire_format and _lines_without_time(x) == _lines_without_time(y), f"step {x.step}"
        assert not any("lat_" in k for k in y.metrics)


# ---- concurrent ------------------------------------------------------------------------------------------------------------
def concurrent_scenario(max_metrics):
    rng = np.random.default_rng(8)
    n_names, T, n = 300, 8, 100_000
    pool = np.arange(n_names)
    return scenario(hist_names(n_names) + CTR_NAMES, [[thread_events(rng, n, pool, n_names, n // 50) for _ in range(T)]],
                    [COLLECT], T, max_metrics=max_metrics, num_buffers=2 if max_metrics > 65536 else 3, num_lanes=4,
                    stage_samples=64, lane_samples=512, concurrent=True, pct=CUSTOM_PCT)


@pytest.mark.gpu
@pytest.mark.parametrize("max_metrics", [1024, 65537], ids=["uint16-ids", "uint32-ids"])
def test_concurrent_collects_conserve_every_cell(native_lib, torch_cuda, tmp_path, max_metrics):
    sc = concurrent_scenario(max_metrics)
    dump = replay(sc, tmp_path, timeout=60)
    ex = Exact()
    n_names = len(sc.names) - len(CTR_NAMES)
    labels = sorted(sc.pct)
    ps = [sc.pct[k] for k in labels]
    hid, hbits, cid, camt = step_events(sc.steps[0], n_names)
    index = {n: i for i, n in enumerate(sc.names)}
    total = np.zeros(n_names * NK, dtype=U64)
    agg, rate_sum = {}, {}
    print(len(dump.intervals), "intervals")
    assert len(dump.intervals) >= 2
    for iv in dump.intervals:
        at = f"interval {iv.step}"
        assert iv.dropped == 0 and iv.status in (0, LH_EBUSY), (at, iv.status)
        for name, (keys, counts) in iv.hist.items():
            bins, counts = cells_of(keys, counts)
            assert np.all(counts > 0)
            total[index[name] * NK + bins] += counts
            count, _, _ = check_name(ex, iv.metrics, name, bins, counts, labels, ps, at)
            got = f64(iv.metrics[f"{name}_agg_count"])
            assert got == agg.get(name, 0) + count, (at, name, "_agg_count")   # the running count: never decreases
            agg[name] = got
        assert {k[:-6] for k in iv.metrics if k.endswith("_count") and not k.endswith("_agg_count")} == set(iv.hist), at
        for k, a in iv.rates.items():
            rate_sum[k] = (rate_sum.get(k, 0) + a) % (1 << 64)
    # conservation per (name, key), against the oracle's histogram of the whole script
    want = model_rows(hid, hbits)
    want_flat = np.zeros(n_names * NK, dtype=U64)
    for i, (bins, counts) in want.items():
        want_flat[i * NK + bins] = counts
    bad = np.nonzero(total != want_flat)[0]
    assert bad.size == 0, [(sc.names[b // NK], int(b % NK), int(total[b]), int(want_flat[b])) for b in bad[:8]]
    assert agg == {sc.names[i]: float(int(c.sum())) for i, (_, c) in want.items()}
    totals = {}
    for c, a in zip(cid.tolist(), camt.tolist()):
        totals[sc.names[c]] = totals.get(sc.names[c], 0) + a
    totals = {k: v % (1 << 64) for k, v in totals.items()}
    assert totals == dump.intervals[-1].counters and rate_sum == totals
    assert dump.end.dropped == 0 and dump.end.status in (0, LH_EBUSY) and dump.end.engine_ready


# ---- no device: counters only; pins the scenario and dump formats --------------------------------------------------------
def test_counters_only_scenario_replays_without_a_device(native_lib, tmp_path):
    rng = np.random.default_rng(9)
    n_names, T = 5, 3
    steps = [[thread_events(rng, 0, np.arange(n_names), n_names, int(rng.integers(0, 9))) for _ in range(T)] for _ in range(6)]
    steps[2] = [thread_events(rng, 0, np.arange(n_names), n_names, 0) for _ in range(T)]
    flags = [COLLECT, COLLECT, COLLECT, NO_COLLECT, COLLECT, KEEP]
    sc = scenario(hist_names(n_names) + CTR_NAMES, steps, flags, T, max_metrics=8, device_counters=False, pct=CUSTOM_PCT)
    dump = replay(sc, tmp_path, timeout=60)
    assert [iv.step for iv in dump.intervals] == [0, 1, 2, 4, 5]
    assert not dump.end.engine_ready and dump.end.status == 0   # no Histogram call: the engine was never asked for
    check_stepped(sc, dump)                                      # rates and lifetime totals exact, no histogram key
    assert dump.intervals[-1].counters["big"] >= 0 and any(iv.rates for iv in dump.intervals)
    assert not any("lat_" in k for iv in dump.intervals for k in iv.metrics)
