"""What counting an interval's samples at or below given values costs on the device (lh_count_le*) against the code paths a
user had before, same box, same run, same snapshot.

S = the snapshot of BASELINE config 4's one-rank slice (65 536 Zipf names, 1.25e8 lognormal pairs: bench.py's stream).
Reported: the device form (HIP events on the snapshot's stream around the call) at nb = 1, 9, 64 shared bounds and nb = 2
per-metric bounds; the host form (wall) at nb = 9; beside them, unchanged code paths on S: extract_compact with the nine
default percentiles (wall) and buckets_all (wall); the device form over the first 256 .. 16 384 names of S in BOTH kernel
shapes (a wave per row / a workgroup per row: lh_tool_count_le_switch), which is where the default switch comes from; and
one name whose row is filled over the full key range, in both shapes.  Medians of --reps calls after --warmup, with the
spread (min .. max).  TWO conditions, both relative and taken in this run:
  host form at nb = 9   <= 2 x extract_compact's wall median
  device form at nb = 9 <=     extract_compact's wall median

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is
started on the GPU after a step that hung).
usage: python tools/count_le_bench.py [--names 65536] [--pairs 1.25e8] [--reps 25] [--warmup 5] [--out profiles/count_le.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchkit as kit  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

TOOL = "count_le_bench"

PCTS = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]       # metrics.go:145-155


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=1.25e8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_le.txt"))
    a = ap.parse_args()
    M, n = a.names, int(a.pairs)
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=58)
    row = rep.row
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# S = snapshot of config 4's one-rank slice (Zipf(1.0) names, lognormal values: bench.py's stream); us are medians "
                  "(min .. max) of the timed calls;", "# device form: HIP events on the snapshot's stream around the call; "
                  "host form, extract_compact and buckets_all: wall time"]

    def quantiles(data):
        return torch.quantile(data[:1_000_000], torch.linspace(0.02, 0.999, 64, dtype=torch.float64, device=data.device)).cpu().numpy()

    eng, snap, q = kit.c4_slice(M, n, TOOL, look=quantiles)
    bounds = {1: q[31:32].copy(), 9: q[3::7][:9].copy(), 64: q.copy()}        # thresholds inside the stream's own range
    xs = torch.cuda.ExternalStream(snap.stream())
    cells = snap.device_cells()
    rep.note(f"# S: {M} names, {n:g} samples, cells of {cells[2]} bytes")

    call_ms = []          # wall time of the last count_le_device's calls themselves (the device form returns after enqueueing)

    def count_le_device(what, b, nmetrics):
        cum = torch.zeros((nmetrics, b.shape[-1]), dtype=torch.int64, device="cuda")
        total = torch.zeros((nmetrics,), dtype=torch.int64, device="cuda")
        ts, call_ms[:] = kit.timed_events(xs, lambda: snap.count_le(b, nmetrics, out=(cum, total)), a.reps, a.warmup, what, 120, TOOL,
                                          wall=True)
        return ts, cum, total

    def wall(what, call, reps, warmup=2):
        return kit.timed_wall(call, reps, warmup, what, 240, TOOL)

    # ---- the whole snapshot
    dev = {}
    for nb in (1, 9, 64):
        ts, cum, total = count_le_device(f"device nb={nb}", bounds[nb], M)
        dev[nb] = row(f"count_le device form, {M} names, nb = {nb} shared", ts,
                      f"  calling thread inside the call {statistics.median(call_ms) * 1e3:.1f} us")
        if nb == 9:
            d_cum9, d_total9 = cum.cpu().numpy().view(np.uint64), total.cpu().numpy().view(np.uint64)
    per = np.sort(np.stack([bounds[9][2] * (1.0 + 1e-5 * np.arange(M)), bounds[9][6] * (1.0 + 1e-5 * np.arange(M))], axis=1), axis=1)
    row(f"count_le device form, {M} names, nb = 2 per metric", count_le_device("device per-metric", per, M)[0],
        f"  of which the calling thread is inside the call (copies {per.nbytes:,d} B of bounds) {statistics.median(call_ms) * 1e3:.1f} us")
    ts, host9 = wall("host nb=9", lambda: snap.count_le(bounds[9], M), a.reps)
    host_ms = row(f"count_le host form (wall), {M} names, nb = 9 shared", ts)
    assert np.array_equal(host9["cum"], d_cum9) and np.array_equal(host9["total"], d_total9)
    assert int(host9["total"].sum()) == n and np.all(host9["cum"][:, -1] <= host9["total"])
    ts, ex = wall("extract_compact", lambda: snap.extract_compact(PCTS, M), a.reps)
    ex_ms = row(f"extract_compact (wall), {M} names, 9 percentiles", ts)
    assert np.array_equal(ex["count"], host9["total"])
    ts, S = wall("buckets_all", lambda: snap.buckets_all(M), a.host_reps, 1)
    row(f"buckets_all (wall), {M} names, {S[1].size:,d} occupied cells", ts)

    # ---- where a row gets a wave and where a workgroup: the first names of S (Zipf: the widest windows) in both shapes
    rep.note("# both kernel shapes, device form, nb = 9 shared, over the first names of S:")
    for k in (256, 1024, 2048, 4096, 16384):
        if k > M:
            continue
        t = {}
        for shape, _ in kit.shapes(L.lh_tool_count_le_switch):
            ts, cum, _ = count_le_device(f"{shape} {k}", bounds[9], k)
            assert np.array_equal(cum.cpu().numpy().view(np.uint64), d_cum9[:k])
            t[shape] = row(f"  {k:>6} names, a {shape} per row", ts)
    snap.release()
    eng.close()

    # ---- one name, its row filled over the full key range (64-bit cells; 512 KiB)
    one, snap = kit.full_row_snapshot(TOOL)
    xs = torch.cuda.ExternalStream(snap.stream())
    rep.note("# one name, all 65 536 cells occupied, device form, nb = 9:")
    b1 = np.array([-1e100, -1e3, -1.0, 0.0, 1.0, 1e3, 1e9, 1e100, np.inf])
    for shape, _ in kit.shapes(L.lh_tool_count_le_switch, (("workgroup (default)", 0), ("wave", 1))):
        ts, cum, total = count_le_device(f"one row {shape}", b1, 1)
        assert int(total[0]) == 3 * 65536 and int(cum[0, -1]) == 3 * 65536 and int(cum[0, 3]) == 3 * 32769
        row(f"  1 name, full span, a {shape} per row", ts)
    snap.release()
    one.close()

    c1, c2 = host_ms <= 2 * ex_ms, dev[9] <= ex_ms
    rep.note(f"# condition 1: host form nb = 9 ({host_ms * 1e3:.1f} us) <= 2 x extract_compact wall ({ex_ms * 1e3:.1f} us): "
             f"{'MET' if c1 else 'NOT MET'}; ratio {host_ms / ex_ms:.2f}")
    rep.note(f"# condition 2: device form nb = 9 ({dev[9] * 1e3:.1f} us) <= extract_compact wall ({ex_ms * 1e3:.1f} us): "
             f"{'MET' if c2 else 'NOT MET'}; ratio {dev[9] / ex_ms:.2f}")
    print("\n".join(rep.lines[-2:]), flush=True)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
