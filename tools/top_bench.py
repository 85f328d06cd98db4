"""What the k leading names cost on the device (lh_top*) against the route a caller has without it, same box, same run, same
snapshot.

S = the snapshot of BASELINE config 4's one-rank slice (65 536 Zipf names, 1.25e8 lognormal pairs: bench.py's stream).
Reported for k = 100 and each `by`, over all names of S and over its first 1 024: the device time of the score pass and of
the select pass (HIP events on the snapshot's stream around each: lh_tool_top_passes_ms); the host form's round trip (wall,
lh_top into a caller's array); and today's route on the same snapshot (wall): lh_extract_rows_compact with the nine default
percentiles over the same names plus numpy.argpartition -- for "count above", lh_count_le plus numpy.argpartition.  Then one
name whose row is filled over the full key range: what the single wave shape costs there.  Every result is compared with
today's route before its time is reported.  Medians of --reps calls after --warmup, with the spread (min .. max).  No number
is fixed in advance.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/top_bench.py [--names 65536] [--pairs 1.25e8] [--k 100] [--reps 25] [--warmup 5] [--out profiles/top.txt]"""
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
BYS = (("count", N.TOP_BY_COUNT, 0.0), ("sum", N.TOP_BY_SUM, 0.0), ("percentile 0.99", N.TOP_BY_PERCENTILE, 0.99),
       ("count above 250", N.TOP_BY_COUNT_ABOVE, 250.0))
TOOL = "top_bench"


def leaders(score, count, k):
    """numpy.argpartition, then the order lh_top defines: descending score, lowest id first among equals, names with
    samples only."""
    cand = np.nonzero(count)[0]
    s = score[cand]
    k = min(k, cand.size)
    if k == 0:
        return cand[:0]
    part = np.argpartition(s, cand.size - k)[cand.size - k:]
    kth = s[part].min()
    ahead = cand[s > kth]
    equal = cand[s == kth][:k - ahead.size]
    pick = np.concatenate([ahead, equal])
    return pick[np.lexsort((pick, -score[pick].astype(np.float64) if score.dtype.kind == "f" else ~score[pick]))]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=1.25e8)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top.txt"))
    a = ap.parse_args()
    M, n, K = a.names, int(a.pairs), a.k
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=72)
    row = rep.row
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --k {K} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# S = snapshot of config 4's one-rank slice (Zipf(1.0) names, lognormal values: bench.py's stream); us are medians "
                  "(min .. max) of the timed calls;", "# score / select pass: HIP events on the snapshot's stream around each kernel; "
                  "host form and today's route: wall time"]
    eng, snap, _ = kit.c4_slice(M, n, TOOL)
    rep.note(f"# S: {M} names, {n:g} samples, cells of {snap.device_cells()[2]} bytes; k = {K}")

    def passes(s, what, by, arg, nmetrics, k=K):
        sc, se = C.c_float(0), C.c_float(0)
        score, select = [], []
        with kit.limit(120, what, TOOL):
            for r in range(a.warmup + a.reps):
                rc = L.lh_tool_top_passes_ms(s._h, 0, nmetrics, by, arg, k, 0, C.byref(sc), C.byref(se))
                assert rc == 0, rc
                if r >= a.warmup:
                    score.append(sc.value)
                    select.append(se.value)
        return score, select

    def wall(what, call, reps, warmup=2):
        return kit.timed_wall(call, reps, warmup, what, 300, TOOL)

    out = np.zeros(K, dtype=N.TOP_ENTRY)
    n_out = C.c_size_t(0)

    def host_form(by, arg, nmetrics):
        assert L.lh_top(snap._h, 0, nmetrics, by, arg, K, 0, out.ctypes.data, C.addressof(n_out)) == 0
        return out[:n_out.value].copy()

    def today(by, arg, nmetrics):
        if by == N.TOP_BY_COUNT_ABOVE:
            le = snap.count_le(np.array([arg]), nmetrics)
            return leaders(le["total"] - le["cum"][:, 0], le["total"], K)
        ex = snap.extract_compact(PCTS, nmetrics)
        if by == N.TOP_BY_COUNT:
            return leaders(ex["count"], ex["count"], K)
        if by == N.TOP_BY_SUM:
            return leaders(ex["sum"], ex["count"], K)
        return leaders((ex["pkeys"][:, PCTS.index(arg)].astype(np.int64) & 0xffff ^ 0x8000).astype(np.uint64), ex["count"], K)

    share = {}
    for nmetrics in sorted({M, min(M, 1024)}, reverse=True):
        rep.note(f"# the first {nmetrics} names of S:")
        for name, by, arg in BYS:
            sc, se = passes(snap, f"passes {name} {nmetrics}", by, arg, nmetrics)
            a_sc = row(f"  {nmetrics:>6} names, by {name}: score pass", sc)
            a_se = row(f"  {nmetrics:>6} names, by {name}: select pass", se)
            share[nmetrics, name] = (a_sc, a_se)
            ts, got = wall(f"host {name}", lambda: host_form(by, arg, nmetrics), a.reps)
            row(f"  {nmetrics:>6} names, by {name}: lh_top host form, round trip (wall)", ts)
            ts, want = wall(f"today {name}", lambda: today(by, arg, nmetrics), a.reps)
            what = "lh_count_le" if by == N.TOP_BY_COUNT_ABOVE else "extract_compact (9 percentiles)"
            row(f"  {nmetrics:>6} names, by {name}: today, {what} + argpartition (wall)", ts)
            if by != N.TOP_BY_SUM:       # (lh_stats.sum and this unit's sum associate differently: equal to rounding only)
                assert got["id"].tolist() == want.tolist(), (name, nmetrics)
            else:
                assert sorted(got["id"].tolist()) == sorted(want.tolist()), (name, nmetrics)
    snap.release()
    eng.close()

    # ---- one name, its row filled over the full key range (64-bit cells; 512 KiB): the single wave shape's worst case
    one, snap1 = kit.full_row_snapshot(TOOL)
    rep.note("# one name, all 65 536 cells occupied (a wave walks 256 steps per walk):")
    for name, by, arg in BYS:
        sc, se = passes(snap1, f"one row {name}", by, arg, 1, 1)
        row(f"  1 name, full span, by {name}: score pass", sc)
        row(f"  1 name, full span, by {name}: select pass", se)
    got = snap1.top(1, "percentile", 0.99, nmetrics=1)               # (no name was interned: the engine counts none)
    assert got["id"].tolist() == [0] and int(got["count"][0]) == 3 * 65536
    snap1.release()
    one.close()
    big = [f"{name}: score {s * 1e3:.1f} us, select {e * 1e3:.1f} us" for (nm, name), (s, e) in share.items() if nm == M]
    rep.note(f"# at {M} names the larger share of the device time -- " + "; ".join(big))

    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
