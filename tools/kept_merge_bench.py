"""What rolling K kept intervals up into ONE kept handle costs (lh_kept_merge), against the route there was before, and what
a read of the window gains from it -- same box, same process, same intervals.

Per name count: K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the
scale moving 0.5 % per interval) are each flipped, kept and released.  Reported:
  lh_kept_merge of the K handles, all names (wall: the call returns when the new handle is complete), in BOTH kernel shapes
  (lh_tool_kept_switch);
  the route available before (wall): K x Kept.add_to (lh_snapshot_add_buckets_csr_device) into a live empty snapshot, then
  lh_keep there.  It needs a dense buffer to be alive; taking and releasing that snapshot is not timed;
  lh_kept_across_device with the nine default percentiles over the ONE merged handle against the K, in both shapes (HIP
  events on the caller's stream);
  bytes of the merged handle against the sum of the K.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance.  Before anything is written the
merged handle's arrays are compared byte for byte between the two shapes and with the old route's handle, and the integer
results of the two reads with each other.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_merge_bench.py [--names 1024,65536] [--k 60] [--pairs 2e6,2e7] [--reps 15] [--out profiles/kept_merge.txt]
                                        [--across LABEL=FILE ...]   (tools/kept_bench.py outputs of the same session, e.g. of the
                                        parent commit and of this tree: their lh_kept_across_device lines are copied in)"""
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

PCTS = [0.0, .5, .75, .9, .95, .99, .999, .9999, 1.0]       # metrics.go:145-155
TOOL = "kept_merge_bench"


def listing(k):
    return [t.cpu().numpy().tobytes() for t in k.arrays()]


def run(torch, a, M, n, rep):
    L = N.lib()
    K = a.k

    row = rep.row

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
    assert all(k.info["samples"] == n for k in kept)

    def wall(what, call, reps, warmup, before=None):
        """Every call makes a kept handle: the one of the call before is closed (untimed) once the next is made; the last is returned."""
        held = []

        def after(spare, new):
            if spare:
                spare.release()
            if held:
                held.pop().close()
            held.append(new)
            return new
        return kit.timed_wall(call, reps, warmup, what, 420, TOOL, before, after, sync=torch.cuda.synchronize)

    def events(what, call, stream):
        return kit.timed_events(stream, call, a.reps, a.warmup, what, 180, TOOL)

    # ---- the merge, in both shapes
    prev = C.c_uint32(0)
    t, one = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        ts, one[shape] = wall(f"merge {shape}", lambda: kept[-1].merge(kept[:-1]), a.reps, a.warmup)
        t["merge " + shape] = row(f"lh_kept_merge (wall), {M} names x {K} handles, a {shape} per row", ts)
    assert L.lh_tool_kept_switch(0, C.byref(prev)) == 0         # prev: the default (the shapes' loop has put it back)
    default = "wave" if M >= prev.value else "workgroup"
    merged = one["wave"]
    assert listing(merged) == listing(one["workgroup"]) and merged.info == one["workgroup"].info
    one["workgroup"].close()
    assert merged.info["samples"] == K * n and merged.info["nrows"] == M

    # ---- the route there was: K imports into a live snapshot, then lh_keep there
    def old_route(spare):
        for k in kept:
            k.add_to(spare)
        return spare.keep(M)

    ts, old = wall("old route", old_route, a.host_reps, 1, before=eng.flip)
    t["old"] = row(f"old route (wall): {K} x add_buckets_csr_device into a live snapshot + lh_keep there, {M} names", ts)
    assert listing(old) == listing(merged) and old.info == merged.info
    old.close()

    # ---- reading the window: the one merged handle against the K
    st = torch.cuda.Stream()
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int64, pkeys=torch.int16,
                 pvalid=torch.uint8)
    res = {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        for what, last, earlier in (("the ONE merged handle", merged, []), (f"the {K} handles", kept[-1], kept[:-1])):
            out = {k: torch.zeros((M, len(PCTS)) if k in ("pkeys", "pvalid") else (M,), dtype=d, device="cuda") for k, d in kinds.items()}
            ts = events(f"across {what} {shape}", lambda: last.across(earlier, PCTS, M, out=out, stream=st), st)
            res[shape, what] = {k: v.cpu().numpy() for k, v in out.items()}
            t[shape, what] = row(f"lh_kept_across_device over {what}, {M} names, np = 9, a {shape} per row", ts)
    first = res["wave", "the ONE merged handle"]
    for key, r in res.items():
        for k in ("count", "nbuckets", "pkeys", "pvalid"):
            assert r[k].tobytes() == first[k].tobytes(), (key, k)
    assert int(first["count"].view(np.uint64).sum()) == K * n

    total = sum(k.info["bytes"] for k in kept)
    rep.note(f"# {M} names: the merged handle holds {merged.info['cells']} cells in {merged.info['bytes'] / 2**20:.2f} MiB; the {K} "
             f"handles hold {sum(k.info['cells'] for k in kept)} in {total / 2**20:.1f} MiB ({total / merged.info['bytes']:.1f} x)")
    rep.note(f"# {M} names: old route / lh_kept_merge (default shape '{default}'): {t['old'] / t['merge ' + default]:.1f} x;  "
             f"lh_kept_across_device over the {K} / over the merged one (default shape): "
             f"{t[default, f'the {K} handles'] / t[default, 'the ONE merged handle']:.1f} x;  merge, wave / workgroup: "
             f"{t['merge wave'] / t['merge workgroup']:.2f}")
    print("\n".join(rep.lines[-2:]), flush=True)
    merged.close()
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
    ap.add_argument("--across", action="append", default=[], metavar="LABEL=FILE",
                    help="a tools/kept_bench.py output of the same session: its lh_kept_across_device lines are copied in under LABEL")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_merge.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=100, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --k {a.k} --pairs {a.pairs} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed calls;",
                  "# lh_kept_merge and the old route: wall time; lh_kept_across_device: HIP events on the caller's stream around the call"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    if a.across:                                             # the reader before and after a change to it, same session
        rep.note("# --across: lh_kept_across_device as tools/kept_bench.py measured it in the same session, by library")
    for spec in a.across:
        label, path = spec.split("=", 1)
        rep.lines += [f"# [{label}] {x.rstrip()}" for x in open(path) if x.startswith("lh_kept_across_device,")]
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
