"""What spread and compare per window of kept intervals cost on the device (lh_kept_spread_series*_device, lh_kept_drift*_device)
against the route there was before them: one lh_kept_spread*_device call per window over the slice, one
lh_kept_compare*_device call per pair of slices, on the same handles -- same box, same process, same stream.

K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the scale moving 0.5 %
per interval) are each flipped, kept and released.  Reported, in BOTH kernel shapes (lh_tool_kept_switch, which for the new
readers takes the ENTRIES of a call, windows x rows), with the nine default percentiles:
  lh_kept_spread_series_ids_device   20 ids x K one-handle windows                    against  K calls of lh_kept_spread_ids_device
  lh_kept_drift_ids_device           20 ids x K - 1 consecutive pairs                 against  K - 1 calls of lh_kept_compare_ids_device
  lh_kept_drift_device               all names x 6 windows of K / 6 handles against   against  6 calls of lh_kept_compare_device
                                     a baseline of the first K / 6
Every call goes straight to the C ABI with arguments made beforehand (the Python wrappers' own time would count K times against
the route).  us are HIP events on the caller's stream around the one call, or around all calls of the route; "host" is the time
the calling thread spent inside them.  Medians with the spread (min .. max).  Before anything is written every window's block is
compared byte for byte with the route's output for its slices, and the two shapes with each other.

THE GATE, with K >= 60: the one-call form's median for the 20 ids lies below the MINIMUM of the route in the same run, in both
shapes and both families; the tool writes its file and then ends with status 1 if it does not.  (With fewer intervals the verdict
is a note.)  For all names x 6 windows no number is fixed: the work is the same as 6 calls, and the tool says beside the number
whether the one call's median lies inside the route's min .. max.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_drift_bench.py [--names 65536] [--pairs 2e7] [--k 60] [--reps 15] [--warmup 3]
                                        [--out profiles/kept_drift.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

PCTS = np.array([0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0])       # metrics.go:145-155
TOOL = "kept_drift_bench"
NIDS = 20
SP_KINDS = ("count", "sum", "m2", "pkeys", "pvalid", "count_le", "sum_le")
CMP_KINDS = ("count_a", "count_b", "ks", "key", "below_a", "below_b", "w1", "shift")


def run(torch, a, M, n, rep):
    L = N.lib()
    K = a.k
    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    kept = []
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        for i in range(K):
            data.mul_(1.005)
            eng.submit_pairs_device(ids, data, n)
            with eng.flip() as s:
                kept.append(s.keep(M))
        del ids, data
        torch.cuda.empty_cache()
    st = torch.cuda.Stream()
    sth = int(st.cuda_stream)
    npct = len(PCTS)
    handles, _ = loghisto_amd.Kept._handles(kept)
    list_at = C.addressof(handles)
    kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8, count_le=torch.int64,
                 sum_le=torch.float64, count_a=torch.int64, count_b=torch.int64, ks=torch.float64, key=torch.int16,
                 below_a=torch.int64, below_b=torch.int64, w1=torch.float64, shift=torch.float64)
    per = dict(pkeys=npct, pvalid=npct, count_le=npct, sum_le=npct)

    def outs(names, entries):
        return {k: torch.zeros((entries * per.get(k, 1),), dtype=kinds[k], device="cuda") for k in names}

    def ptrs(o):
        return [int(t.data_ptr()) for t in o.values()]

    def sliced(o, w, rows):
        """window w's block of window-major outputs, as pointers"""
        return [int(t.data_ptr()) + w * rows * per.get(k, 1) * t.element_size() for k, t in o.items()]

    def host(o):
        return {k: v.cpu().numpy() for k, v in o.items()}

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}")

    rng = np.random.default_rng(20)
    ids20 = np.sort(rng.choice(min(M, 2000), NIDS, replace=False)).astype(np.uint32)   # busy names: the head of the Zipf order
    d_ids20 = torch.from_numpy(ids20.astype(np.int32)).cuda()
    ids_at = int(d_ids20.data_ptr())
    part = max(K // 6, 1)
    ones = [(i, i + 1) for i in range(K)]
    pairs = [(i, i + 1, i + 1, i + 2) for i in range(K - 1)]
    fixed = [(0, part, lo, lo + part) for lo in range(0, 6 * part, part) if lo + part <= K]
    p_at = PCTS.ctypes.data

    def win(windows):
        return np.array([v for w in windows for v in w], dtype=np.uint32)

    def at(i):
        return list_at + 8 * i

    # (key, rows' text, windows' text, windows, rows, outputs, the route's, the windows' array, the one call, the route's call for
    #  window w, the two names, what else the row says)
    def cases():
        w1, w2, w3 = win(ones), win(pairs), win(fixed)
        o1, r1 = outs(SP_KINDS, len(ones) * NIDS), outs(SP_KINDS, len(ones) * NIDS)
        yield ("spread_series_ids", f"{NIDS} ids", f"{len(ones)} windows of 1", ones, NIDS, o1, r1, w1,
               lambda: L.lh_kept_spread_series_ids_device(list_at, K, w1.ctypes.data, len(ones), ids_at, NIDS, p_at, npct, 0, sth, *ptrs(o1)),
               lambda w, q: L.lh_kept_spread_ids_device(at(q[0]), q[1] - q[0], ids_at, NIDS, p_at, npct, 0, sth, *sliced(r1, w, NIDS)),
               "lh_kept_spread_series_ids_device", "lh_kept_spread_ids_device", f"np = {npct}")
        o2, r2 = outs(CMP_KINDS, len(pairs) * NIDS), outs(CMP_KINDS, len(pairs) * NIDS)
        yield ("drift_ids", f"{NIDS} ids", f"{len(pairs)} windows of 1 against 1", pairs, NIDS, o2, r2, w2,
               lambda: L.lh_kept_drift_ids_device(list_at, K, w2.ctypes.data, len(pairs), ids_at, NIDS, 0, sth, *ptrs(o2)),
               lambda w, q: L.lh_kept_compare_ids_device(at(q[0]), q[1] - q[0], at(q[2]), q[3] - q[2], ids_at, NIDS, 0, sth,
                                                         *sliced(r2, w, NIDS)),
               "lh_kept_drift_ids_device", "lh_kept_compare_ids_device", "consecutive pairs")
        o3, r3 = outs(CMP_KINDS, len(fixed) * M), outs(CMP_KINDS, len(fixed) * M)
        yield ("drift", f"{M} names", f"{len(fixed)} windows of {part} against {part}", fixed, M, o3, r3, w3,
               lambda: L.lh_kept_drift_device(list_at, K, w3.ctypes.data, len(fixed), 0, M, 0, sth, *ptrs(o3)),
               lambda w, q: L.lh_kept_compare_device(at(q[0]), q[1] - q[0], at(q[2]), q[3] - q[2], 0, M, 0, sth, *sliced(r3, w, M)),
               "lh_kept_drift_device", "lh_kept_compare_device", "a fixed baseline")

    res, verdicts = {}, []
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        for key, rows_text, win_text, windows, rows, o, r, _keep, one, route_call, name, route_name, extra in cases():
            nw = len(windows)

            def one_call():
                check(one(), name)

            def route():
                for w, q in enumerate(windows):
                    check(route_call(w, q), route_name)

            ts, inside = kit.timed_events(st, one_call, a.reps, a.warmup, f"{name} {shape}", 180, TOOL, wall=True)
            t_one = rep.row(f"{name}, {rows_text} x {win_text}, {extra}, a {shape} per entry", ts,
                            f"  host {kit.med(inside)[0] * 1e3:.1f}")
            rs, inside = kit.timed_events(st, route, a.reps, a.warmup, f"{route_name} x {nw} {shape}", 180, TOOL, wall=True)
            rep.row(f"  the route: {nw} x {route_name} over the slices, a {shape} per row", rs, f"  host {kit.med(inside)[0] * 1e3:.1f}")
            got, want = host(o), host(r)                             # every window's block is the route's, byte for byte
            for f in got:
                assert got[f].tobytes() == want[f].tobytes(), (key, shape, f)
            res[key, shape] = got
            lo_r, hi_r = min(rs), max(rs)
            if key == "drift":
                where = "inside" if lo_r <= t_one <= hi_r else "BELOW" if t_one < lo_r else "ABOVE"
                rep.note(f"#   {name} ({shape}): the one call's median lies {where} the route's min .. max "
                         f"({lo_r * 1e3:.1f} .. {hi_r * 1e3:.1f} us); route median / one call: {kit.med(rs)[0] / t_one:.2f} x", echo=True)
            else:
                met = t_one < lo_r
                verdicts.append(met)
                rep.note(f"#   gate, {name} ({shape}): median {t_one * 1e3:.1f} us {'<' if met else '>='} the route's minimum "
                         f"{lo_r * 1e3:.1f} us: {'met' if met else 'MISSED'};  route median / one call: {kit.med(rs)[0] / t_one:.1f} x", echo=True)
    for key in ("spread_series_ids", "drift_ids", "drift"):          # the two shapes: the same bytes, floats included
        for f, v in res[key, "wave"].items():
            assert v.tobytes() == res[key, "workgroup"][f].tobytes(), (key, f)
    counts = res["drift", "wave"]["count_b"].view(np.uint64).reshape(len(fixed), M)
    assert all(int(counts[w].sum()) == part * n for w in range(len(fixed)))
    for k in kept:
        k.close()
    eng.close()
    torch.cuda.empty_cache()
    return all(verdicts)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="65536")
    ap.add_argument("--pairs", default="2e7")
    ap.add_argument("--k", type=int, default=60)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_drift.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=124, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed runs:",
                  "# HIP events on the stream around the one call, or around ALL calls of the route; host: the calling thread's",
                  "# median time inside them, us; every call straight to the C ABI",
                  "# ONE run, nothing tuned: the four kernels and the switch are as first written"]
    met = True
    for M, n in zip(names, pairs):
        met = run(torch, a, M, n, rep) and met
    rep.write(a.out)
    if not met and a.k >= 60:
        sys.stderr.write(f"{TOOL}: the gate of the {NIDS} ids x {a.k} windows was missed\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
