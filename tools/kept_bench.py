"""What a minute of history costs with intervals kept in compact form on the device (lh_keep, lh_kept_across*) against the
routes there were before, same box, same process, same intervals.

Per name count: K intervals of one engine of 32-bit cells (Zipf names, lognormal values: bench.py's stream, the scale moving
0.5 % per interval) are each flipped, kept and released.  Reported, with the nine default percentiles:
  lh_keep per interval (wall, the call returns when the copy is complete), bytes per kept interval against the dense buffer;
  lh_kept_across over the K handles for all names -- device form (HIP events on the caller's stream) in BOTH kernel shapes
  (lh_tool_kept_switch), host form (wall) -- and lh_kept_across_ids for 20 ids;
  the route available before (wall): K x lh_snapshot_add_buckets_csr_device into a spare empty snapshot, then
  lh_extract_rows_compact there (for the 20 ids: lh_across_ids on the spare).  The CSR arrays it imports are the handles' own,
  already on the device: a caller without lh_keep would first have pulled them out with lh_buckets_all and pushed them back,
  which is NOT timed -- the comparison flatters the old route.  Taking and releasing the spare snapshot is not timed either;
  lh_across over the last 14 live snapshots -- what ONE engine of 16 buffers can keep alive beside a spare snapshot and the
  buffer it ingests into (only where 16 dense buffers fit: up to 8 192 names) -- a quarter of the window, for scale.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance; the integer results of the new and
the old route are compared before anything is written.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_bench.py [--names 1024,65536] [--k 60] [--pairs 2e6,2e7] [--reps 15] [--out profiles/kept.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

PCTS = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]       # metrics.go:145-155
TOOL = "kept_bench"
NIDS = 20


def run(torch, a, M, n, rep):
    L = N.lib()
    K = a.k
    dense_too = M <= 8192                                    # 16 dense buffers fit
    live = min(K, 14)                                        # an engine has at most 16 buffers: 14 live snapshots, the spare, ingest

    row = rep.row

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=16 if dense_too else 3, num_lanes=1,
                              lane_samples=1 << 16, cell_bits=32)
    kept, snaps, keep_ms = [], [], []
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        for i in range(K):
            data.mul_(1.005)
            eng.submit_pairs_device(ids, data, n)
            s = eng.flip()
            torch.cuda.synchronize()
            width = s.device_cells()[2]
            t0 = time.perf_counter()
            kept.append(s.keep(M))
            keep_ms.append((time.perf_counter() - t0) * 1e3)
            if dense_too and i >= K - live:
                snaps.append(s)
            else:
                s.release()
        del ids, data
        torch.cuda.empty_cache()
    info = [k.info for k in kept]
    dense = M * loghisto_amd.Snapshot.row_stride() * width
    rep.note(f"# {M} names, {K} intervals of {n:g} samples each, cells of {width} bytes: a dense buffer is {dense / 2**20:.0f} MiB; a kept "
             f"interval holds {statistics.median(i['cells'] for i in info):.0f} cells in {statistics.median(i['bytes'] for i in info) / 2**20:.2f} MiB "
             f"(median; {sum(i['bytes'] for i in info) / 2**20:.1f} MiB for all {K}), 1 / {dense / statistics.median(i['bytes'] for i in info):.0f} of it")
    print(rep.lines[-1], flush=True)
    row(f"lh_keep (wall), {M} names, one interval (the first call allocates the unit's blocks: left out)", keep_ms[1:])
    assert all(i["samples"] == n for i in info)

    st = torch.cuda.Stream()
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int64, pkeys=torch.int16,
                 pvalid=torch.uint8)

    def outs(rows):
        return {k: torch.zeros((rows, len(PCTS)) if k in ("pkeys", "pvalid") else (rows,), dtype=d, device="cuda") for k, d in kinds.items()}

    def events(what, call, stream):
        return kit.timed_events(stream, call, a.reps, a.warmup, what, 180, TOOL)

    def wall(what, call, reps, warmup, before=None, after=None):
        return kit.timed_wall(call, reps, warmup, what, 420, TOOL, before, after, sync=torch.cuda.synchronize)

    def release(spare, out):
        spare.release()
        return out

    rng = np.random.default_rng(20)
    ids20 = np.sort(rng.choice(min(M, 2000), NIDS, replace=False)).astype(np.uint32)   # busy names: the head of the Zipf order
    d_ids20 = torch.from_numpy(ids20.astype(np.int32)).cuda()
    prev = C.c_uint32(0)
    res, t = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        out = outs(M)
        ts = events(f"kept across {shape}", lambda: kept[-1].across(kept[:-1], PCTS, M, out=out, stream=st), st)
        res[shape] = {k: v.cpu().numpy() for k, v in out.items()}
        t[shape] = row(f"lh_kept_across_device, {M} names x {K} handles, np = 9, a {shape} per row", ts)
        out20 = outs(NIDS)
        ts = events(f"kept across ids {shape}", lambda: kept[-1].across(kept[:-1], PCTS, ids=d_ids20, out=out20, stream=st), st)
        res[shape + "20"] = {k: v.cpu().numpy() for k, v in out20.items()}
        t[shape + "20"] = row(f"lh_kept_across_ids_device, {NIDS} ids x {K} handles, np = 9, a {shape} per row", ts)
    assert L.lh_tool_kept_switch(0, C.byref(prev)) == 0         # prev: the default (the shapes' loop has put it back)
    for k in kinds:
        assert res["wave"][k].tobytes() == res["workgroup"][k].tobytes(), k
        assert res["wave20"][k].tobytes() == res["workgroup20"][k].tobytes() == res["wave"][k][ids20].tobytes(), k
    assert int(res["wave"]["count"].view(np.uint64).sum()) == K * n
    ts, host = wall("kept across host form", lambda: kept[-1].across(kept[:-1], PCTS, M), a.reps, 2)
    t["host"] = row(f"lh_kept_across host form (wall, with the derived arrays), {M} names x {K} handles, np = 9", ts)
    ts, host20 = wall("kept across ids host form", lambda: kept[-1].across(kept[:-1], PCTS, ids=ids20), a.reps, 2)
    t["host20"] = row(f"lh_kept_across_ids host form (wall), {NIDS} ids x {K} handles, np = 9", ts)
    assert host["count"].tobytes() == res["wave"]["count"].tobytes() and host["pkeys"].tobytes() == res["wave"]["pkeys"].tobytes()

    # ---- the route there was: K imports into a spare empty snapshot, then the compact extract there
    def old_route(spare):
        for k in kept:
            k.add_to(spare)
        ex = spare.extract_compact(PCTS, M)
        return {k: ex[k].copy() for k in ("count", "sum", "nbuckets", "pkeys")}

    def old_route20(spare):
        for k in kept:
            k.add_to(spare)
        return spare.across_ids(ids20, [], PCTS)

    ts, old = wall("old route", old_route, a.host_reps, 1, before=eng.flip, after=release)
    t["old"] = row(f"old route (wall): {K} x add_buckets_csr_device into a spare snapshot + extract_rows_compact, {M} names", ts)
    ts, old20 = wall("old route, 20 ids", old_route20, a.host_reps, 1, before=eng.flip, after=release)
    t["old20"] = row(f"old route (wall): {K} x add_buckets_csr_device into a spare snapshot + lh_across_ids there, {NIDS} ids", ts)
    assert np.array_equal(old["count"], host["count"]) and np.array_equal(old["nbuckets"], host["nbuckets"])
    assert np.array_equal(old["pkeys"], host["pkeys"]) and np.allclose(old["sum"], host["sum"], rtol=1e-9, atol=0)
    assert np.array_equal(old20["count"], host20["count"]) and np.array_equal(old20["pkeys"], host20["pkeys"])

    if dense_too:
        last = snaps[-1]
        xs = torch.cuda.ExternalStream(last.stream())
        ak = dict(kinds, present_bits=torch.int32)
        aout = {k: torch.zeros((M, len(PCTS)) if k in ("pkeys", "pvalid") else (M,), dtype=d, device="cuda") for k, d in ak.items()}
        ts = events("across", lambda: last.across(snaps[:-1], PCTS, M, out=aout), xs)
        t["across"] = row(f"lh_across_device over the last {live} LIVE snapshots (of 16 dense buffers), {M} names, np = 9", ts)
        kout = outs(M)
        ts = events("kept across 16", lambda: kept[-1].across(kept[-live:-1], PCTS, M, out=kout, stream=st), st)
        t["kept16"] = row(f"lh_kept_across_device over the same {live} intervals' handles, {M} names, np = 9", ts)
        for k in ("count", "nbuckets", "pkeys", "pvalid"):
            assert aout[k].cpu().numpy().tobytes() == kout[k].cpu().numpy().tobytes(), k
    else:
        rep.note(f"# lh_across over 14 live snapshots is not measured at {M} names: 16 dense buffers of {dense / 2**30:.0f} GiB do not fit")
    default = "wave" if M >= prev.value else "workgroup"
    rep.note(f"# {M} names: old route / lh_kept_across host form: {t['old'] / t['host']:.2f} x;  {NIDS} ids: {t['old20'] / t['host20']:.2f} x"
             f"   (device form, default shape '{default}': {t[default] * 1e3:.0f} us for all names)")
    print(rep.lines[-1], flush=True)
    for s in snaps:
        s.release()
    for k in kept:
        k.close()
    eng.close()
    torch.cuda.empty_cache()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="1024,65536")
    ap.add_argument("--pairs", default="2e6,2e7")
    ap.add_argument("--k", type=int, default=60)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=96, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --k {a.k} --pairs {a.pairs} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed calls;",
                  "# device forms: HIP events on the caller's stream around the call; host forms, lh_keep and the old route: wall time"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
