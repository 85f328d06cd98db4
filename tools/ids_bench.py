"""What stats of a CHOSEN set of names cost through the id-list forms (lh_across_ids*, lh_count_le_ids*, lh_spread_ids*)
against the two routes there were before, same box, same process, same snapshots.

Two intervals of one engine of 32-bit cells (Zipf names, lognormal values: bench.py's stream) stay alive as two snapshots;
lh_across* runs over both, lh_count_le* (three shared bounds) and lh_spread* (the nine default percentiles) over the later one.
For 20 and 1 024 ids drawn at random from all names, per unit:
  the id-list device form (HIP events on the snapshot's stream around 8 calls, per call) and host form (wall);
  route 1 (wall): n one-row calls of the base form's host form;
  route 2 (wall): one call of the base form's host form over the whole range of names;
  the results of all of them compared (integers equal; float sums equal where the kernel shape is the same, to 1e-9 otherwise).
Asserted at 20 ids, after every figure is on file: the id-list host form's slowest call is faster than the fastest call of
either route (a miss is written out as a "# MISSED" line and ends the run with an error).  Nothing else is fixed in advance.  At 1 024: the id-list device form per id beside the base device form per row over 1 024 contiguous rows,
in the same kernel shape -- over the drawn ids, and over those same contiguous rows handed in as a shuffled id list (the same
cells: what is left is the indirection).
--base-only [--lib PATH]: only the base forms' device times (whole range, 1 024 rows, 20 rows), for a library that may be an
earlier build: that this change did not slow the shared kernels.  Its rows are APPENDED to the file.
Medians of --reps calls after --warmup, with the spread (min .. max).

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/ids_bench.py [--names 8192] [--pairs 1e7] [--reps 25] [--warmup 5] [--out profiles/ids.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

PCTS = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]       # metrics.go:145-155
BOUNDS = [10.0, 100.0, 1000.0]
CALLS = 8                                                   # device-form calls between two events: the time is per call
TOOL = "ids_bench"
MARK = "# ==== measured: tools/ids_bench.py"
BASE_MARK = "# ==== base forms only: tools/ids_bench.py --base-only"
INT_OUT = dict(across=("count", "nbuckets", "present_bits", "pkeys", "pvalid"), count_le=("cum", "total"),
               spread=("count", "pkeys", "pvalid", "count_le"))
FLOAT_OUT = dict(across=("sum",), count_le=(), spread=("sum", "m2", "sum_le"))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=8192)
    ap.add_argument("--pairs", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=9)
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of the library (with --base-only: it may lack the id-list forms)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ids.txt"))
    a = ap.parse_args()
    if a.lib:
        assert a.base_only, "--lib goes with --base-only"
        N.LIB_PATH, N.ALLOW_OLDER_ABI = os.path.abspath(a.lib), True
    M, n = a.names, int(a.pairs)
    assert M >= 2048
    torch.cuda.set_device(0)
    mark = BASE_MARK if a.base_only else MARK
    rep = kit.Report(width=92)
    row = rep.row
    rep.lines += [mark + (f" --lib {a.lib}" if a.lib else ""),
                  *kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup} --host-reps {a.host_reps}", torch),
                  "# two intervals of one engine of 32-bit cells (Zipf(1.0) names, lognormal values); us are medians (min .. max) of the "
                  "timed calls;", f"# device forms: HIP events on the snapshot's stream around {CALLS} calls, per call; host forms and routes: wall time"]

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=4, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    snaps = []
    with kit.limit(300, "ingest", TOOL):
        for i in range(2):
            ids = bench.zipf_ids(n, M, 4000 + i)
            data = bench.make_samples(n, "lognormal", seed=40 + i)
            eng.submit_pairs_device(ids, data, n)
            snaps.append(eng.flip())
            torch.cuda.synchronize()
            del ids, data
        torch.cuda.empty_cache()
    first, last = snaps
    xs = torch.cuda.ExternalStream(last.stream())
    rep.note(f"# {M} names, 2 snapshots of {n:g} samples each, cells of {[s.device_cells()[2] for s in snaps]} bytes; across: both "
             f"snapshots, np = 9; count_le: the later one, {len(BOUNDS)} shared bounds; spread: the later one, np = 9")
    B = np.array(BOUNDS)
    np_ = len(PCTS)

    def events(what, call):
        return kit.timed_events(xs, call, a.reps, a.warmup, what, 120, TOOL, calls=CALLS)

    def wall(what, call, reps, warmup=2):
        return kit.timed_wall(call, reps, warmup, what, 300, TOOL)

    def device_out(unit, k):
        """the device form's output tensors for k entries"""
        if unit == "across":
            kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int32, pkeys=torch.int16,
                         pvalid=torch.uint8)
            return {f: torch.zeros((k, np_) if f in ("pkeys", "pvalid") else (k,), dtype=d, device="cuda") for f, d in kinds.items()}
        if unit == "spread":
            kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8,
                         count_le=torch.int64, sum_le=torch.float64)
            return {f: torch.zeros((k,) if f in ("count", "sum", "m2") else (k, np_), dtype=d, device="cuda") for f, d in kinds.items()}
        return (torch.zeros((k, len(BOUNDS)), dtype=torch.int64, device="cuda"), torch.zeros((k,), dtype=torch.int64, device="cuda"))

    # base(unit, nmetrics, first, out) / by_id(unit, ids, out): one call; out=None is the host form
    def base(unit, k, f=0, out=None):
        if unit == "across":
            return last.across([first], PCTS, k, f, out=out)
        if unit == "spread":
            return last.spread(PCTS, k, f, out=out)
        return last.count_le(B, k, f, out=out)

    def by_id(unit, ids, out=None):
        if unit == "across":
            return last.across_ids(ids, [first], PCTS, out=out)
        if unit == "spread":
            return last.spread_ids(ids, PCTS, out=out)
        return last.count_le_ids(ids, B, out=out)

    def same(unit, got, want, idx, exact, what):
        for f in INT_OUT[unit]:
            assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])[idx]), (what, f)
        for f in FLOAT_OUT[unit]:
            g, w = np.asarray(got[f]), np.asarray(want[f])[idx]
            ok = (g.tobytes() == np.ascontiguousarray(w).tobytes()) if exact else np.allclose(g, w, rtol=1e-9, atol=0, equal_nan=True)
            assert ok, (what, f)

    units = ("across", "count_le", "spread")
    missed = []
    if a.base_only:
        for unit in units:
            for k in (M, 1024, 20):
                out = device_out(unit, k)
                ts = events(f"{unit} base {k}", lambda: base(unit, k, 0, out))
                row(f"{unit} base device form, rows [0, {k})", ts, f"   {kit.med(ts)[0] * 1e3 / k:8.4f} us per row")
    else:
        rng = np.random.default_rng(2024)
        for k in (20, 1024):
            ids = np.sort(rng.choice(M, k, replace=False)).astype(np.uint32)
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            idx = ids.astype(np.int64)
            for unit in units:
                out = device_out(unit, k)
                ts = events(f"{unit}_ids device {k}", lambda: by_id(unit, d_ids, out))
                t_dev = row(f"{unit}_ids device form, {k} ids of {M} names", ts, f"   {kit.med(ts)[0] * 1e3 / k:8.4f} us per id")
                ids_ts, got = wall(f"{unit}_ids host {k}", lambda: by_id(unit, ids), a.host_reps)
                row(f"{unit}_ids host form (wall), {k} ids of {M} names", ids_ts)
                dev = ({f: v.cpu().numpy() for f, v in out.items()} if isinstance(out, dict)
                       else dict(cum=out[0].cpu().numpy(), total=out[1].cpu().numpy()))
                for f in INT_OUT[unit] + FLOAT_OUT[unit]:
                    assert np.asarray(got[f]).tobytes() == dev[f].tobytes(), (unit, k, f, "host form against device form")

                def one_by_one():
                    return [base(unit, 1, int(r)) for r in ids]

                r1_ts, rows1 = wall(f"{unit} one-row calls {k}", one_by_one, a.host_reps if k <= 64 else 3, 1)
                row(f"route 1 (wall): {k} one-row calls of {unit}'s host form", r1_ts)
                r2_ts, whole = wall(f"{unit} whole range", lambda: base(unit, M), a.host_reps)
                row(f"route 2 (wall): one call of {unit}'s host form over all {M} names", r2_ts)
                same(unit, got, whole, idx, False, (unit, k, "whole range"))
                for m, one in enumerate(rows1):                      # a one-row call takes the workgroup form, as k < 1 024 entries do
                    same(unit, {f: np.asarray(got[f])[m:m + 1] for f in INT_OUT[unit] + FLOAT_OUT[unit]}, one, slice(None), k < 1024,
                         (unit, k, "one-row call", m))
                if k == 20:
                    best = min(("route 1", r1_ts), ("route 2", r2_ts), key=lambda x: statistics.median(x[1]))
                    if not (max(ids_ts) < min(r1_ts) and max(ids_ts) < min(r2_ts)):   # asserted once everything is on file
                        missed.append(f"{unit}, 20 ids: the id-list host form's slowest call ({max(ids_ts) * 1e3:.1f} us) is not below "
                                      f"the fastest call of route 1 ({min(r1_ts) * 1e3:.1f} us) and of route 2 ({min(r2_ts) * 1e3:.1f} us)")
                    rep.note(f"#   {unit}, 20 ids: the faster of today's routes is {best[0]} at {statistics.median(best[1]) * 1e3:.1f} us; "
                             f"the id-list host form takes {statistics.median(ids_ts) * 1e3:.1f} us "
                             f"({statistics.median(best[1]) / statistics.median(ids_ts):.1f} x), slowest call {max(ids_ts) * 1e3:.1f} "
                             f"against the routes' fastest {min(min(r1_ts), min(r2_ts)) * 1e3:.1f}")
                    print(rep.lines[-1], flush=True)
                else:
                    # the indirection alone: rows [0, 1 024) by the base form, and the same rows as a shuffled id list
                    bout = device_out(unit, k)
                    ts = events(f"{unit} base contiguous {k}", lambda: base(unit, k, 0, bout))
                    t_base = row(f"{unit} base device form, rows [0, {k}) (same kernel shape)", ts,
                                 f"   {kit.med(ts)[0] * 1e3 / k:8.4f} us per row")
                    perm = rng.permutation(k).astype(np.uint32)
                    d_perm = torch.from_numpy(perm.view(np.int32)).cuda()
                    pout = device_out(unit, k)
                    ts = events(f"{unit}_ids shuffled contiguous {k}", lambda: by_id(unit, d_perm, pout))
                    t_perm = row(f"{unit}_ids device form, rows [0, {k}) as a shuffled id list", ts,
                                 f"   {kit.med(ts)[0] * 1e3 / k:8.4f} us per id")
                    b0, p0 = (bout, pout) if isinstance(bout, dict) else (dict(cum=bout[0], total=bout[1]), dict(cum=pout[0], total=pout[1]))
                    for f in INT_OUT[unit] + FLOAT_OUT[unit]:
                        assert p0[f].cpu().numpy().tobytes() == np.ascontiguousarray(b0[f].cpu().numpy()[perm.astype(np.int64)]).tobytes(), (unit, f)
                    rep.note(f"#   {unit}, {k} rows: id list / contiguous = {t_perm / t_base:.3f} on the same rows; the drawn ids "
                             f"(lighter rows: Zipf names beyond the first {k}) take {t_dev / t_base:.3f} of it")
                    print(rep.lines[-1], flush=True)
    for s in snaps:
        s.release()
    eng.close()

    # the compile-time resource table at the top of the file stays; the measured part is replaced, base-only runs are appended
    if a.base_only and os.path.exists(a.out):               # (appended: everything the file holds stays, MARK's part too)
        with open(a.out) as f:
            rep.lines[:0] = f.read().splitlines()
    rep.lines += ["# MISSED: " + m for m in missed]
    rep.write(a.out, mark=None if a.base_only else MARK)
    assert not missed, missed
    return 0


if __name__ == "__main__":
    sys.exit(main())
