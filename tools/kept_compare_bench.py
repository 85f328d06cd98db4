"""What the distribution shift between two lists of kept intervals costs on the device (lh_kept_compare_device), against the
route there was before it and against lh_compare_device on live snapshots -- same box, same process, same intervals.

Per name count: 2 K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the
scale moving 0.5 % per interval; the second K another 10 % higher) are each flipped, kept and released: K handles of a
baseline, K of the current window.  Reported for every K of --k:
  lh_kept_compare_device, K + K handles, all names, in BOTH kernel shapes (lh_tool_kept_switch): HIP events on the caller's
  stream, and wall time of the call plus the wait for the stream;
  the route available before (wall, the wait included): two snapshots are flipped (not timed), every handle of each side is
  poured into its snapshot with lh_snapshot_add_buckets_csr_device, then lh_compare_device.  It needs two dense buffers to be
  alive; releasing them afterwards, which has the engine clear what the imports wrote, is timed apart;
  the floor: lh_compare_device alone on those two live snapshots (HIP events).
The width of the compare's two tiles is a constant of the library (lh_tool_kept_compare_tile): a run with --lib PATH measures
a build at another width (tools/build_tuning.py -DLH_KEPT_COMPARE_TILE=1024 --name tile1024), and --other LABEL=FILE copies the
lh_kept_compare_device rows of such a run of the same session into this one's file.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance.  Before anything is written the
integer results and ks of the two shapes and of the old route are compared with each other.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_compare_bench.py [--names 1024,65536] [--pairs 2e6,2e7] [--k 1,30] [--reps 15] [--warmup 3]
                                          [--host-reps 3] [--lib PATH] [--other LABEL=FILE ...] [--out profiles/kept_compare.txt]"""
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

TOOL = "kept_compare_bench"
EXACT = ("count_a", "count_b", "ks", "key", "below_a", "below_b")


def run(torch, a, M, n, ks, rep, T):
    L = N.lib()
    row = rep.row
    K = max(ks)
    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    sides = ([], [])
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        for side in sides:
            for i in range(K):
                data.mul_(1.005)
                eng.submit_pairs_device(ids, data, n)
                with eng.flip() as s:
                    side.append(s.keep(M))
            data.mul_(1.1)
        del ids, data
        torch.cuda.empty_cache()
    st = torch.cuda.Stream()
    kinds = dict(count_a=torch.int64, count_b=torch.int64, ks=torch.float64, key=torch.int16, below_a=torch.int64,
                 below_b=torch.int64, w1=torch.float64, shift=torch.float64)

    def outputs():
        return {k: torch.zeros((M,), dtype=t, device="cuda") for k, t in kinds.items()}

    def host(out):
        return {k: v.cpu().numpy() for k, v in out.items()}

    for k in ks:
        base, cur = sides[0][:k], sides[1][:k]
        res, t = {}, {}
        for shape, _ in kit.shapes(L.lh_tool_kept_switch):
            out = outputs()
            what = f"lh_kept_compare_device, {M} names x {k} + {k} handles, tiles of {T} bins, a {shape} per row"
            ts = kit.timed_events(st, lambda: cur[-1].compare(base, M, earlier=cur[:-1], out=out, stream=st), a.reps, a.warmup,
                                  f"kept compare {shape} {k}", 180, TOOL)
            t[shape] = row(what, ts)
            res[shape] = host(out)

            def call_and_wait():
                cur[-1].compare(base, M, earlier=cur[:-1], out=out, stream=st)
                st.synchronize()
            ts, _ = kit.timed_wall(call_and_wait, a.reps, a.warmup, f"kept compare wall {shape} {k}", 180, TOOL, sync=torch.cuda.synchronize)
            row("  " + what + " (wall, with the wait)", ts)
        for f in kinds:                                        # the two shapes walk alike: the same bits, sums included
            assert res["wave"][f].tobytes() == res["workgroup"][f].tobytes(), f

        # ---- the route there was: pour each side back into a live snapshot, then lh_compare_device
        out = outputs()
        state = {}

        def flip_two():
            for s in state.pop("snaps", ()):
                s.release()
            return eng.flip(), eng.flip()

        def old_route(snaps):
            for side, snap in zip((base, cur), snaps):
                for h in side:
                    h.add_to(snap)
            snaps[1].compare(snaps[0], M, out=out)
            torch.cuda.synchronize()

        def keep_snaps(snaps, _):
            state["snaps"] = snaps
            return snaps

        ts, snaps = kit.timed_wall(old_route, a.host_reps, 1, f"old route {k}", 420, TOOL, before=flip_two, after=keep_snaps,
                                   sync=torch.cuda.synchronize)
        t["old"] = row(f"old route (wall, with the wait): {k} + {k} x add_buckets_csr_device into two live snapshots + "
                       f"lh_compare_device, {M} names", ts)
        old = host(out)
        for f in EXACT:
            assert old[f].tobytes() == res["wave"][f].tobytes(), f
        for f in ("w1", "shift"):                               # another walk, another order of the adds
            assert np.allclose(old[f], res["wave"][f], rtol=1e-9, atol=1e-9, equal_nan=True), f
        # ---- the floor: lh_compare_device alone on the two live snapshots the route has just filled
        xs = torch.cuda.ExternalStream(snaps[1].stream())
        ts = kit.timed_events(xs, lambda: snaps[1].compare(snaps[0], M, out=out), a.reps, a.warmup, f"compare live {k}", 120, TOOL)
        t["live"] = row(f"lh_compare_device on the two live snapshots ({k} intervals a side), {M} names", ts)

        def release_two():
            for s in state.pop("snaps"):
                s.release()
            torch.cuda.synchronize()
        ts, _ = kit.timed_wall(release_two, 1, 0, f"release {k}", 120, TOOL, sync=torch.cuda.synchronize)
        row(f"  releasing the two snapshots (wall: the engine clears what the imports wrote), {M} names", ts)
        default = "wave" if M >= 1024 else "workgroup"
        ok = ~np.isnan(res["wave"]["shift"])
        rep.note(f"# {M} names x {k} + {k}: old route / lh_kept_compare_device (default shape '{default}'): "
                 f"{t['old'] / t[default]:.1f} x;  lh_kept_compare_device / lh_compare_device on live snapshots: "
                 f"{t[default] / t['live']:.1f} x;  wave / workgroup: {t['wave'] / t['workgroup']:.2f};  "
                 f"{int(ok.sum())} names with samples on both sides, median shift {np.median(res['wave']['shift'][ok]):.2f} buckets",
                 echo=True)
    rep.note(f"# {M} names: a kept interval holds {sides[0][0].info['bytes'] / 2**20:.2f} MiB; a dense buffer of 32-bit cells "
             f"{M * 65540 * 4 / 2**20:.0f} MiB", echo=True)
    for side in sides:
        for h in side:
            h.close()
    eng.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="1024,65536")
    ap.add_argument("--pairs", default="2e6,2e7")
    ap.add_argument("--k", default="1,30", help="handles a side")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of the library (another tile width)")
    ap.add_argument("--other", action="append", default=[], metavar="LABEL=FILE",
                    help="an output of this tool of the same session: its lh_kept_compare_device rows are copied in under LABEL")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_compare.txt"))
    a = ap.parse_args()
    if a.lib:
        N.LIB_PATH = os.path.abspath(a.lib)
    import torch
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    ks = [int(x) for x in a.k.split(",")]
    assert len(names) == len(pairs) and all(1 <= k and 2 * k <= N.MAX_KEPT for k in ks)
    torch.cuda.set_device(0)
    tile = C.c_uint32(0)
    assert N.lib().lh_tool_kept_compare_tile(C.byref(tile)) == 0
    rep = kit.Report(width=118, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --reps {a.reps} --warmup {a.warmup}"
                                + (f" --lib {a.lib}" if a.lib else ""), torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher, the current window another 10 %; us are medians "
                  "(min .. max) of the timed calls;",
                  "# device forms: HIP events on the stream around the call; wall: the call and the wait for what it enqueued;",
                  f"# this library's compare tiles are {tile.value} bins wide, two a row"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, ks, rep, tile.value)
    for spec in a.other:
        label, path = spec.rsplit("=", 1)
        rep.note(f"# --other: lh_kept_compare_device as this tool measured it in the same session with {label}")
        rep.lines += [f"# [{label}] {x.rstrip()}" for x in open(path) if x.lstrip().startswith("lh_kept_compare_device,")]
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
