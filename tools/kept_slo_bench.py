"""What per-name bounds over kept intervals cost on the device (lh_kept_slo*_device, lh_kept_burn*_device) against the routes there
were before them, on the same handles -- same box, same process, same stream.

K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the scale moving 0.5 %
per interval) are each flipped, kept and released.  Every name has its own row of eight bounds (the shared row of
tools/kept_series_bench.py scaled by a factor per name) and its own budget.  Reported, in BOTH kernel shapes (lh_tool_kept_switch):
  lh_kept_slo_ids_device    20 ids x K one-handle windows x 8 bounds   against  20 calls of lh_kept_heat_ids_device, one per name
                                                                                with its row: the route to per-name bounds so far
  lh_kept_burn_ids_device   the same ids and windows, one bound a name, K rates: reported beside it
  lh_kept_slo_device        all names x K / 10 windows of 10 x 8       against  lh_kept_heat_device on the same list and windows with
                                                                                ONE shared row: the same walk plus a load a wave
  lh_kept_burn_device       all names x 2 windows (the last interval, all K)   against  lh_kept_heat_device on those windows with one
                                                                                shared bound, its cum / total copied to the host, and
                                                                                the NumPy rule (burn_fires) there: wall time of both
Every call goes straight to the C ABI with arguments made beforehand.  us are HIP events on the caller's stream around the one call,
or around all calls of the route; "host" is the time the calling thread spent inside them; the last pair is wall time, the burn call's
with its count read back.  Medians with the spread (min .. max).  Before anything is written the one call's bytes are compared with
the route's (slo), the records with burn_fires on the call's own cum / total (burn), and the two shapes with each other.

THE GATE, with K >= 60 windows: the median of lh_kept_slo_ids_device lies below the MINIMUM of the 20-call route in the same run, in
both shapes; the tool writes its file and then ends with status 1 if it does not.  (With fewer windows the verdict is a note.)  For
all names no number is fixed: the ratio to the shared-row call is reported.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started on the
GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_slo_bench.py [--names 65536] [--pairs 2e7] [--k 60] [--reps 15] [--warmup 3] [--out profiles/kept_slo.txt]"""
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

BOUNDS = np.array([1.0, 5.0, 10.0, 25.0, 50.0, 100.0, 250.0, 1000.0])  # cumulative `le` buckets across the lognormal body
TOOL = "kept_slo_bench"
NIDS = 20


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
    nb = len(BOUNDS)
    handles, _ = loghisto_amd.Kept._handles(kept)
    list_at = C.addressof(handles)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} returned {rc}")

    def win(pairs):
        return np.array([v for p in pairs for v in p], dtype=np.uint32)

    def u64(entries):
        return torch.zeros((max(entries, 1),), dtype=torch.int64, device="cuda")

    def at(t):
        return int(t.data_ptr())

    def host(t, count=None):
        return t.cpu().numpy().view(np.uint64)[:count]

    rng = np.random.default_rng(20)
    ids20 = np.sort(rng.choice(min(M, 2000), NIDS, replace=False)).astype(np.uint32)   # busy names: the head of the Zipf order
    d_ids20 = torch.from_numpy(ids20.astype(np.int32)).cuda()
    rows = BOUNDS[None, :] * (1.0 + 0.01 * (np.arange(M) % 97))[:, None]              # a row per name, neighbours differ
    budget = 0.001 * (1 + np.arange(M) % 50)
    rows20, budget20 = np.ascontiguousarray(rows[ids20]), np.ascontiguousarray(budget[ids20])
    d_rows, d_rows20 = torch.from_numpy(rows).cuda(), torch.from_numpy(rows20).cuda()
    d_first, d_first20 = torch.from_numpy(np.ascontiguousarray(rows[:, nb - 1])).cuda(), torch.from_numpy(np.ascontiguousarray(rows20[:, nb - 1])).cuda()
    d_budget, d_budget20 = torch.from_numpy(budget).cuda(), torch.from_numpy(budget20).cuda()
    ones, tens, two = [(i, i + 1) for i in range(K)], [(i, min(i + 10, K)) for i in range(0, K, 10)], [(K - 1, K), (0, K)]
    w1, w10, w2 = win(ones), win(tens), win(two)
    rates1, rates2 = np.full(K, 14.4), np.array([14.4, 6.0])
    torch.cuda.synchronize()

    res, verdicts = {}, []
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        # ---- 20 ids x K one-handle windows x 8 bounds: one call against a call per name
        cum, tot, rcum, rtot = u64(K * NIDS * nb), u64(K * NIDS), u64(NIDS * K * nb), u64(NIDS * K)

        def slo_ids():
            check(L.lh_kept_slo_ids_device(list_at, K, w1.ctypes.data, K, at(d_ids20), NIDS, at(d_rows20), nb, 0, sth, at(cum), at(tot)),
                  "lh_kept_slo_ids_device")

        def per_name():                                              # name j: K windows of its one id with its own HOST row
            for j in range(NIDS):
                check(L.lh_kept_heat_ids_device(list_at, K, w1.ctypes.data, K, at(d_ids20) + 4 * j, 1, rows20.ctypes.data + 8 * nb * j, nb,
                                                0, sth, at(rcum) + 8 * j * K * nb, at(rtot) + 8 * j * K), "lh_kept_heat_ids_device")

        ts, inside = kit.timed_events(st, slo_ids, a.reps, a.warmup, f"slo_ids {shape}", 180, TOOL, wall=True)
        t_one = rep.row(f"lh_kept_slo_ids_device, {NIDS} ids x {K} windows of 1, nb = {nb}, a {shape} per entry", ts,
                        f"  host {kit.med(inside)[0] * 1e3:.1f}")
        rs, inside = kit.timed_events(st, per_name, a.reps, a.warmup, f"heat_ids x {NIDS} {shape}", 180, TOOL, wall=True)
        rep.row(f"  the route: {NIDS} x lh_kept_heat_ids_device, one name and its row a call, a {shape} per entry", rs,
                f"  host {kit.med(inside)[0] * 1e3:.1f}")
        got = host(cum, K * NIDS * nb).reshape(K, NIDS, nb)
        want = host(rcum, NIDS * K * nb).reshape(NIDS, K, nb).transpose(1, 0, 2)           # the route is name-major
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), ("slo_ids", shape)
        assert host(tot, K * NIDS).reshape(K, NIDS).tobytes() == np.ascontiguousarray(host(rtot, NIDS * K).reshape(NIDS, K).T).tobytes()
        res["slo_ids", shape] = got.copy()
        met = t_one < min(rs)
        verdicts.append(met)
        rep.note(f"#   gate, lh_kept_slo_ids_device ({shape}): median {t_one * 1e3:.1f} us {'<' if met else '>='} the route's minimum "
                 f"{min(rs) * 1e3:.1f} us: {'met' if met else 'MISSED'};  route median / one call: {kit.med(rs)[0] / t_one:.1f} x", echo=True)
        # ---- the alert on the same shape: one bound a name, K rates; k = NIDS records
        hits, n_out, bcum, btot = torch.zeros((2 * NIDS,), dtype=torch.int32, device="cuda"), u64(1), u64(K * NIDS), u64(K * NIDS)

        def burn_ids():
            check(L.lh_kept_burn_ids_device(list_at, K, w1.ctypes.data, K, at(d_ids20), NIDS, rates1.ctypes.data, at(d_first20),
                                            at(d_budget20), NIDS, 0, sth, at(hits), at(n_out), at(bcum), at(btot)), "lh_kept_burn_ids_device")

        ts, inside = kit.timed_events(st, burn_ids, a.reps, a.warmup, f"burn_ids {shape}", 180, TOOL, wall=True)
        rep.row(f"lh_kept_burn_ids_device, {NIDS} ids x {K} windows of 1, cum and total too, a {shape} per entry", ts,
                f"  host {kit.med(inside)[0] * 1e3:.1f}")
        fires = loghisto_amd.burn_fires(host(bcum, K * NIDS).reshape(K, NIDS), host(btot, K * NIDS).reshape(K, NIDS), budget20, rates1)
        want = np.flatnonzero(fires.all(axis=0))
        count = int(host(n_out, 1)[0])
        assert count == want.size and hits.cpu().numpy().view(np.uint32).reshape(-1, 2)[:count, 0].tolist() == want.tolist(), ("burn_ids", shape)
        res["burn_ids", shape] = (count, hits.cpu().numpy().copy())
        # ---- all names x K / 10 windows of 10 x 8 bounds: a row per name against ONE shared row
        nw = len(tens)
        cum, tot, rcum, rtot = u64(nw * M * nb), u64(nw * M), u64(nw * M * nb), u64(nw * M)

        def slo_all():
            check(L.lh_kept_slo_device(list_at, K, w10.ctypes.data, nw, 0, M, at(d_rows), nb, 0, sth, at(cum), at(tot)), "lh_kept_slo_device")

        def heat_all():
            check(L.lh_kept_heat_device(list_at, K, w10.ctypes.data, nw, 0, M, BOUNDS.ctypes.data, nb, 0, sth, at(rcum), at(rtot)),
                  "lh_kept_heat_device")

        ts = kit.timed_events(st, slo_all, a.reps, a.warmup, f"slo {shape}", 180, TOOL)
        t_slo = rep.row(f"lh_kept_slo_device, {M} names x {nw} windows of {tens[0][1]}, nb = {nb}, a {shape} per entry", ts)
        rs = kit.timed_events(st, heat_all, a.reps, a.warmup, f"heat {shape}", 180, TOOL)
        t_heat = rep.row(f"  beside it: lh_kept_heat_device, the same list and windows, ONE shared row, a {shape} per entry", rs)
        rep.note(f"#   lh_kept_slo_device / lh_kept_heat_device ({shape}): {t_slo / t_heat:.3f} x (not gated: the same walk plus a load a wave)",
                 echo=True)
        assert host(tot, nw * M).tobytes() == host(rtot, nw * M).tobytes(), ("totals", shape)   # the bounds play no part in total
        same = np.flatnonzero(np.arange(M) % 97 == 0)                                            # names whose factor is 1: the shared row
        assert host(cum, nw * M * nb).reshape(nw, M, nb)[:, same].tobytes() == host(rcum, nw * M * nb).reshape(nw, M, nb)[:, same].tobytes()
        res["slo", shape] = host(cum, nw * M * nb).copy()
        # ---- all names x 2 windows: the alert in one call against heat + a copy + the rule on the host (wall time)
        hits, n_out, hcum, htot = torch.zeros((2 * M,), dtype=torch.int32, device="cuda"), u64(1), u64(2 * M), u64(2 * M)
        shared = np.array([float(BOUNDS[nb - 1])])

        def burn_all():
            check(L.lh_kept_burn_device(list_at, K, w2.ctypes.data, 2, 0, M, rates2.ctypes.data, at(d_first), at(d_budget), M, 0, sth,
                                        at(hits), at(n_out), None, None), "lh_kept_burn_device")
            st.synchronize()
            return int(host(n_out, 1)[0])

        def heat_and_rule():
            check(L.lh_kept_heat_device(list_at, K, w2.ctypes.data, 2, 0, M, shared.ctypes.data, 1, 0, sth, at(hcum), at(htot)),
                  "lh_kept_heat_device")
            st.synchronize()
            f = loghisto_amd.burn_fires(host(hcum, 2 * M).reshape(2, M), host(htot, 2 * M).reshape(2, M), budget, rates2)
            return int(f.all(axis=0).sum())

        ts, count = kit.timed_wall(burn_all, a.reps, a.warmup, f"burn {shape}", 180, TOOL, sync=torch.cuda.synchronize)
        t_burn = rep.row(f"lh_kept_burn_device, {M} names x 2 windows (1 and {K} handles), k = {M}, count read back: WALL", ts)
        rs, _ = kit.timed_wall(heat_and_rule, a.reps, a.warmup, f"heat and rule {shape}", 180, TOOL, sync=torch.cuda.synchronize)
        t_rule = rep.row("  the route: lh_kept_heat_device (one shared bound), cum / total to the host, burn_fires there: WALL", rs)
        rep.note(f"#   the route / lh_kept_burn_device ({shape}): {t_rule / t_burn:.2f} x (not gated; {count} of {M} names reported)", echo=True)
        bc, bt = u64(2 * M), u64(2 * M)                                # once more with cum / total: the records are the rule's
        check(L.lh_kept_burn_device(list_at, K, w2.ctypes.data, 2, 0, M, rates2.ctypes.data, at(d_first), at(d_budget), M, 0, sth,
                                    at(hits), at(n_out), at(bc), at(bt)), "lh_kept_burn_device")
        st.synchronize()
        want = np.flatnonzero(loghisto_amd.burn_fires(host(bc, 2 * M).reshape(2, M), host(bt, 2 * M).reshape(2, M), budget, rates2).all(axis=0))
        assert int(host(n_out, 1)[0]) == want.size == count, ("burn", shape)
        assert hits.cpu().numpy().view(np.uint32).reshape(-1, 2)[:count, 0].tolist() == want.tolist(), ("burn", shape)
        res["burn", shape] = hits.cpu().numpy()[:2 * count].copy()
    for key in ("slo_ids", "slo", "burn"):                             # the two shapes: the same bytes
        assert res[key, "wave"].tobytes() == res[key, "workgroup"].tobytes(), key
    assert res["burn_ids", "wave"][0] == res["burn_ids", "workgroup"][0]
    assert res["burn_ids", "wave"][1].tobytes() == res["burn_ids", "workgroup"][1].tobytes()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_slo.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT and min(names) >= NIDS
    torch.cuda.set_device(0)
    rep = kit.Report(width=118, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed runs:",
                  "# HIP events on the stream around the one call, or around ALL calls of the route; host: the calling thread's",
                  "# median time inside them, us; WALL rows: the calling thread's time up to the answer on the host; every call",
                  "# straight to the C ABI.  ONE run, nothing tuned: the kernels and the switch are as first written"]
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
