"""What top and movers per window of kept intervals cost on the device (lh_kept_top_series_device, lh_kept_movers_series_device)
against the route there was before them: one lh_kept_top_device call per window over the slice, one lh_kept_movers_device call per
pair of slices, on the same handles -- same box, same process, same stream.

K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the scale moving 0.5 %
per interval) are each flipped, kept and released.  Reported, in BOTH kernel shapes of the score pass (lh_tool_kept_switch, which
for the new readers takes the ENTRIES of a call, windows x rows), at k = 20:
  lh_kept_top_series_device      the first 1 024 names x K one-handle windows, by percentile 0.99   against  K calls of lh_kept_top_device
  lh_kept_movers_series_device   the first 1 024 names x K - 1 consecutive pairs, by ks             against  K - 1 calls of lh_kept_movers_device
  lh_kept_top_series_device      all names x 6 windows of K / 6 handles, by sum                     against  6 calls of lh_kept_top_device
and the device time of each one's score and select passes (lh_tool_kept_top_series_passes_ms / _movers_series_passes_ms, summed
over the chunks of a call).  Every call goes straight to the C ABI with arguments made beforehand (the Python wrappers' own time
would count K times against the route).  us are HIP events on the caller's stream around the one call, or around all calls of the
route; "host" is the time the calling thread spent inside them.  Medians with the spread (min .. max).  Before anything is written
every window's entries and count are compared byte for byte with the route's output for its slices, and the two shapes with each
other.

THE GATE, with K >= 60: at the two 1 024-name rows the one call's median lies below the MINIMUM of the route in the same run, in
the shape the switch selects by itself (a wave per entry: 1 024 x 60 entries, and 1 024 rows a call of the route); the tool writes
its file and then ends with status 1 if it does not.  The route is existing code measured beside it and no ratio is fixed in
advance: the margin is "below the minimum" because the route pays K times two launches, the mutex and a hold where the one call
pays them once.  The other shape's verdict is a note, as every verdict is with fewer intervals.  For all names x 6 windows no
number is fixed: the work is the same as 6 calls, and the tool says beside the number whether the one call's median lies inside
the route's min .. max.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_top_series_bench.py [--names 65536] [--pairs 2e7] [--k 60] [--reps 15] [--warmup 3]
                                             [--out profiles/kept_top_series.txt]"""
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

TOOL = "kept_top_series_bench"
TOP_K = 20
HEAD = 1024                                                              # the names of the two gated rows: the head of the Zipf order
SELECTED = "wave"                                                        # the shape the switch selects at HEAD names x 60 windows


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
    handles, _ = loghisto_amd.Kept._handles(kept)
    list_at = C.addressof(handles)
    head = min(HEAD, M)

    def outs(nwin):
        return (torch.zeros((nwin * TOP_K * 32,), dtype=torch.uint8, device="cuda"), torch.zeros((nwin,), dtype=torch.int32, device="cuda"))

    def host(o):
        return o[0].cpu().numpy().tobytes(), o[1].cpu().numpy().tobytes()

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}")

    def win(windows):
        return np.array([v for w in windows for v in w], dtype=np.uint32)

    def at(i):
        return list_at + 8 * i

    def block(o, w):
        return int(o[0].data_ptr()) + w * TOP_K * 32, int(o[1].data_ptr()) + 4 * w

    part = max(K // 6, 1)
    ones = [(i, i + 1) for i in range(K)]
    pairs = [(i, i + 1, i + 1, i + 2) for i in range(K - 1)]
    sixths = [(lo, lo + part) for lo in range(0, 6 * part, part) if lo + part <= K]
    PCT, KS, SUM = N.TOP_BY_PERCENTILE, N.MOVERS_BY_KS, N.TOP_BY_SUM

    # (key, rows' text, windows' text, windows, the outputs, the route's, the windows' array, the one call, the route's call for
    #  window w, the passes tool, the two names, what else the row says, gated?)
    def cases():
        w1, w2, w3 = win(ones), win(pairs), win(sixths)
        o1, r1 = outs(len(ones)), outs(len(ones))
        yield ("top_head", f"{head} names", f"{len(ones)} windows of 1", ones, o1, r1, w1,
               lambda: L.lh_kept_top_series_device(list_at, K, w1.ctypes.data, len(ones), 0, head, PCT, 0.99, TOP_K, 0, sth,
                                                   int(o1[0].data_ptr()), int(o1[1].data_ptr())),
               lambda w, q: L.lh_kept_top_device(at(q[0]), q[1] - q[0], 0, head, PCT, 0.99, TOP_K, 0, sth, *block(r1, w)),
               lambda sc, se: L.lh_tool_kept_top_series_passes_ms(list_at, K, w1.ctypes.data, len(ones), 0, head, PCT, 0.99, TOP_K, 0, sth,
                                                                  sc, se),
               "lh_kept_top_series_device", "lh_kept_top_device", "by percentile 0.99", True)
        o2, r2 = outs(len(pairs)), outs(len(pairs))
        yield ("movers_head", f"{head} names", f"{len(pairs)} windows of 1 against 1", pairs, o2, r2, w2,
               lambda: L.lh_kept_movers_series_device(list_at, K, w2.ctypes.data, len(pairs), 0, head, KS, 0.0, TOP_K, 0, sth,
                                                      int(o2[0].data_ptr()), int(o2[1].data_ptr())),
               lambda w, q: L.lh_kept_movers_device(at(q[0]), q[1] - q[0], at(q[2]), q[3] - q[2], 0, head, KS, 0.0, TOP_K, 0, sth,
                                                    *block(r2, w)),
               lambda sc, se: L.lh_tool_kept_movers_series_passes_ms(list_at, K, w2.ctypes.data, len(pairs), 0, head, KS, 0.0, TOP_K, 0,
                                                                     sth, sc, se),
               "lh_kept_movers_series_device", "lh_kept_movers_device", "consecutive pairs, by ks", True)
        o3, r3 = outs(len(sixths)), outs(len(sixths))
        yield ("top_all", f"{M} names", f"{len(sixths)} windows of {part}", sixths, o3, r3, w3,
               lambda: L.lh_kept_top_series_device(list_at, K, w3.ctypes.data, len(sixths), 0, M, SUM, 0.0, TOP_K, 0, sth,
                                                   int(o3[0].data_ptr()), int(o3[1].data_ptr())),
               lambda w, q: L.lh_kept_top_device(at(q[0]), q[1] - q[0], 0, M, SUM, 0.0, TOP_K, 0, sth, *block(r3, w)),
               lambda sc, se: L.lh_tool_kept_top_series_passes_ms(list_at, K, w3.ctypes.data, len(sixths), 0, M, SUM, 0.0, TOP_K, 0, sth,
                                                                  sc, se),
               "lh_kept_top_series_device", "lh_kept_top_device", "by sum", False)

    res, verdicts = {}, []
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        for key, rows_text, win_text, windows, o, r, _keep, one, route_call, passes, name, route_name, extra, gated in cases():
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
            got, want = host(o), host(r)                             # every window's entries and count are the route's, byte for byte
            assert got == want and any(got[1]), (key, shape)
            res[key, shape] = got
            score, select = [], []
            with kit.limit(180, f"{name} passes {shape}", TOOL):
                for i in range(a.warmup + a.reps):
                    sc, se = C.c_float(-1.0), C.c_float(-1.0)
                    check(passes(C.byref(sc), C.byref(se)), "the passes tool")
                    if i >= a.warmup:
                        score.append(sc.value)
                        select.append(se.value)
            rep.row(f"  its score pass ({name}, {rows_text} x {nw} windows, {shape})", score)
            rep.row(f"  its select pass ({name}, {rows_text} x {nw} windows, {shape})", select)
            lo_r, hi_r = min(rs), max(rs)
            if not gated:
                where = "inside" if lo_r <= t_one <= hi_r else "BELOW" if t_one < lo_r else "ABOVE"
                rep.note(f"#   {name}, {rows_text} ({shape}): the one call's median lies {where} the route's min .. max "
                         f"({lo_r * 1e3:.1f} .. {hi_r * 1e3:.1f} us); route median / one call: {kit.med(rs)[0] / t_one:.2f} x", echo=True)
            else:
                met = t_one < lo_r
                counts = shape == SELECTED
                if counts:
                    verdicts.append(met)
                rep.note(f"#   gate, {name} ({shape}{'' if counts else ', not the shape the switch selects: a note'}): median "
                         f"{t_one * 1e3:.1f} us {'<' if met else '>='} the route's minimum {lo_r * 1e3:.1f} us: "
                         f"{'met' if met else 'MISSED'};  route median / one call: {kit.med(rs)[0] / t_one:.1f} x", echo=True)
    for key in ("top_head", "movers_head", "top_all"):               # the two shapes: the same bytes, sum and score included
        assert res[key, "wave"] == res[key, "workgroup"], key
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_top_series.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=124, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed runs:",
                  "# HIP events on the stream around the one call, or around ALL calls of the route; host: the calling thread's",
                  f"# median time inside them, us; every call straight to the C ABI; k = {TOP_K}",
                  "# the passes: device time of the score and the select kernels of the one call, summed over its chunks",
                  "# ONE run, nothing tuned: the kernels, the switch and the records' 64 MiB are as first written"]
    met = True
    for M, n in zip(names, pairs):
        met = run(torch, a, M, n, rep) and met
    rep.write(a.out)
    if not met and a.k >= 60:
        sys.stderr.write(f"{TOOL}: the gate of the {HEAD} names x {a.k} windows was missed\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
