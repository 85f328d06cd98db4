"""What std and percentile-trimmed sums per name cost on the device (lh_spread*) against one read of the same windows and
against the route a user had before, same box, same run, same snapshot.

S = the snapshot of BASELINE config 4's one-rank slice (65 536 Zipf names, 1.25e8 lognormal pairs: bench.py's stream).
Reported: the device form (HIP events on the snapshot's stream around the call) at np = 0, 1 and 9 in BOTH kernel shapes
(a wave per row / a workgroup per row: lh_tool_spread_switch); lh_count_le_device at nb = np on the same snapshot -- one
read of the same windows: the floor; extract_compact with the nine default percentiles (wall); the host form at np = 9
(wall); the host route this replaces, buckets_all + the weighted walk in numpy (wall); both shapes over the first
256 .. 16 384 names of S, which is where the default switch comes from; and one name whose row is filled over the full key
range, in both shapes.  Medians of --reps calls after --warmup, with the spread (min .. max).  No number is fixed in advance.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/spread_bench.py [--names 65536] [--pairs 1.25e8] [--reps 25] [--warmup 5] [--out profiles/spread.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchkit as kit  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

PCTS = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]       # metrics.go:145-155
PSETS = {0: [], 1: [0.9], 9: PCTS}
TOOL = "spread_bench"


def numpy_route(snap, M, D, P):
    """What the device call replaces: every occupied cell to the host, then the walks in numpy (count, sum, m2 and, per
    percentile, the prefix count and sum at the first cell whose share of the total reaches p)."""
    off, keys, counts = snap.buckets_all(M)
    off = off.astype(np.int64)
    d = D[(keys.astype(np.int64) & 0xffff) ^ 0x8000]
    c = counts.astype(np.float64)
    seg = np.repeat(np.arange(M), np.diff(off))
    has = np.diff(off) > 0
    count = np.bincount(seg, weights=c, minlength=M)
    s = np.bincount(seg, weights=d * c, minlength=M)
    run = np.cumsum(counts)
    run = run - np.concatenate([[0], run]).astype(np.uint64)[off[:-1]][seg]
    runs = np.cumsum(d * c)
    runs = runs - np.concatenate([[0.0], runs])[off[:-1]][seg]
    total = np.zeros(M, dtype=np.uint64)
    total[has] = run[off[1:][has] - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s / count
        m2 = np.bincount(seg, weights=c * (d - mean[seg]) ** 2, minlength=M)
        frac = run.astype(np.float64) / count[seg]
    cle = np.zeros((M, len(P)), dtype=np.uint64)
    sle = np.zeros((M, len(P)))
    for i, p in enumerate(P):
        below = np.bincount(seg, weights=frac < p, minlength=M).astype(np.int64)   # cells that do not reach p yet
        at = np.minimum(off[:-1] + below, np.maximum(off[1:] - 1, 0))
        cle[has, i] = run[at[has]]
        sle[has, i] = runs[at[has]]
    return dict(count=total.astype(np.uint64), sum=s, m2=m2, count_le=cle, sum_le=sle)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=1.25e8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread.txt"))
    a = ap.parse_args()
    M, n = a.names, int(a.pairs)
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=62)
    row = rep.row
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# S = snapshot of config 4's one-rank slice (Zipf(1.0) names, lognormal values: bench.py's stream); us are medians "
                  "(min .. max) of the timed calls;", "# device forms: HIP events on the snapshot's stream around the call; "
                  "host form, extract_compact and the numpy route: wall time"]

    def quantiles(data):
        return torch.quantile(data[:1_000_000], torch.linspace(0.02, 0.999, 64, dtype=torch.float64, device=data.device)).cpu().numpy()

    eng, snap, q = kit.c4_slice(M, n, TOOL, look=quantiles)
    bounds = {1: q[31:32].copy(), 9: q[3::7][:9].copy()}
    xs = torch.cuda.ExternalStream(snap.stream())
    cells = snap.device_cells()
    D = eng.codec_tables()[1]
    rep.note(f"# S: {M} names, {n:g} samples, cells of {cells[2]} bytes")
    kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8,
                 count_le=torch.int64, sum_le=torch.float64)

    def events(what, call):
        return kit.timed_events(xs, call, a.reps, a.warmup, what, 120, TOOL)

    def spread_device(what, P, nmetrics):
        out = {k: torch.zeros((nmetrics,) if k in ("count", "sum", "m2") else (nmetrics, len(P)), dtype=t, device="cuda")
               for k, t in kinds.items() if P or k in ("count", "sum", "m2")}
        ts = events(what, lambda: snap.spread(P, nmetrics, out=out))
        return ts, {k: v.cpu().numpy() for k, v in out.items()}

    def count_le_device(what, b, nmetrics):
        cum = torch.zeros((nmetrics, b.size), dtype=torch.int64, device="cuda")
        total = torch.zeros((nmetrics,), dtype=torch.int64, device="cuda")
        return events(what, lambda: snap.count_le(b, nmetrics, out=(cum, total))), total.cpu().numpy().view(np.uint64)

    def wall(what, call, reps, warmup=2):
        return kit.timed_wall(call, reps, warmup, what, 300, TOOL)

    def same_integers(x, y, what):
        for k in ("count", "pkeys", "pvalid", "count_le"):
            if k in x and k in y:
                assert np.array_equal(x[k].view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)), (what, k)

    # ---- the whole snapshot, both shapes
    t, res = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_spread_switch):
        for k, P in PSETS.items():
            ts, res[shape, k] = spread_device(f"{shape} np={k}", P, M)
            t[shape, k] = row(f"spread device form, {M} names, np = {k}, a {shape} per row", ts)
    for k in PSETS:
        same_integers(res["wave", k], res["workgroup", k], f"shapes np={k}")
        for f in ("sum", "m2", "sum_le"):                      # the shapes associate the sums differently
            if f in res["wave", k]:
                assert np.allclose(res["wave", k][f], res["workgroup", k][f], rtol=1e-9, atol=0), (k, f)
    assert int(res["wave", 9]["count"].view(np.uint64).sum()) == n
    for nb in (1, 9):
        ts, total = count_le_device(f"count_le nb={nb}", bounds[nb], M)
        row(f"count_le device form, {M} names, nb = {nb} (one read: the floor)", ts)
        assert np.array_equal(total, res["wave", 9]["count"].view(np.uint64))
    ts, ex = wall("extract_compact", lambda: snap.extract_compact(PCTS, M), a.reps)
    row(f"extract_compact (wall), {M} names, 9 percentiles", ts)
    assert np.array_equal(ex["count"], res["wave", 9]["count"].view(np.uint64))
    assert np.array_equal(ex["pkeys"], res["wave", 9]["pkeys"])
    ts, host = wall("host np=9", lambda: snap.spread(PCTS, M), a.reps)
    row(f"spread host form (wall, with the derived arrays), {M} names, np = 9", ts)
    pinned = {k: torch.zeros((M,) if k in ("count", "sum", "m2") else (M, 9), dtype=t, pin_memory=True).numpy()
              for k, t in kinds.items()}
    pp = np.array(PCTS)
    args = [pinned[k].ctypes.data for k in ("count", "sum", "m2", "pkeys", "pvalid", "count_le", "sum_le")]
    ts, rc = wall("host C call", lambda: L.lh_spread(snap._h, 0, M, pp.ctypes.data, 9, *args), a.reps)
    assert rc == 0
    row(f"lh_spread into the caller's pinned arrays (wall), {M} names, np = 9", ts)
    same_integers(pinned, host, "C call")
    prev = C.c_uint32(0)
    assert L.lh_tool_spread_switch(0, C.byref(prev)) == 0      # prev: the default (the shapes' loop has put it back)
    default = "wave" if M >= prev.value else "workgroup"
    same_integers(res[default, 9], host, "host form")
    ts, ref = wall("numpy route", lambda: numpy_route(snap, M, D, PCTS), a.host_reps, 1)
    row(f"buckets_all + numpy (wall): the route this replaces, {M} names, np = 9", ts)
    assert np.array_equal(ref["count"], host["count"]) and np.array_equal(ref["count_le"], host["count_le"])
    assert np.allclose(ref["sum"], host["sum"], rtol=1e-9, atol=1e-9 * float(np.abs(host["sum"]).sum())) and np.allclose(ref["m2"], host["m2"], rtol=1e-6)
    # (the numpy route takes its per-name prefixes as differences of one running sum over all cells: absolute error)
    assert np.allclose(ref["sum_le"], host["sum_le"], rtol=1e-9, atol=1e-9 * float(np.abs(host["sum"]).sum()))

    # ---- where a row gets a wave and where a workgroup: the first names of S (Zipf: the widest windows) in both shapes
    rep.note("# both kernel shapes, device form, np = 9, over the first names of S:")
    for k in (256, 1024, 2048, 4096, 16384):
        if k > M:
            continue
        for shape, _ in kit.shapes(L.lh_tool_spread_switch):
            ts, got = spread_device(f"{shape} {k}", PCTS, k)
            same_integers(got, {f: v[:k] for f, v in res["wave", 9].items()}, f"{shape} {k}")
            row(f"  {k:>6} names, a {shape} per row", ts)
    snap.release()
    eng.close()

    # ---- one name, its row filled over the full key range (64-bit cells; 512 KiB)
    one, snap = kit.full_row_snapshot(TOOL)
    xs = torch.cuda.ExternalStream(snap.stream())
    rep.note("# one name, all 65 536 cells occupied, device form:")
    for k, P in PSETS.items():
        for shape, _ in kit.shapes(L.lh_tool_spread_switch):
            ts, got = spread_device(f"one row {shape}", P, 1)
            assert int(got["count"][0]) == 3 * 65536 and (k != 9 or int(got["count_le"][0, -1]) == 3 * 65536)
            row(f"  1 name, full span, np = {k}, a {shape} per row", ts)
        ts, _ = count_le_device("one row count_le", np.array([0.0] * max(k, 1)), 1)
        row(f"  1 name, full span, count_le nb = {max(k, 1)} (default shape)", ts)
    snap.release()
    one.close()

    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
