"""What bringing kept intervals of OTHER name orders into one name space costs in ONE call (lh_kept_gather_device), against the route
there was before -- same box, same process, same intervals.

Kept intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the scale moving 0.5 %
per interval) stand in for the handles of a fleet: each gets a random permutation of its rows as its map.  Measured, each in BOTH
kernel shapes (lh_tool_kept_switch), wall time (the call returns when the new handle is complete; the handle it makes is closed
untimed):
  1 handle x --names rows under a random permutation: by the direct route (the default for one handle), by the tile route, and by
  the tile route over a map first transposed on the device (lh_tool_kept_gather_route);
  --k handles x --names rows with a permutation per handle: the tile route as it is, and over the transposed map;
  --fleet-names names x --fleet-handles handles: the same two.
Beside each, the route there was, per handle: lh_kept_save, the permutation of the CSR arrays on the host in whole-array NumPy
(loghisto_amd.keptfile.gather of one blob, unchecked), lh_kept_load; then lh_kept_merge of the loaded handles when there are several.
Medians of the timed calls with the spread (min .. max).  No ratio is fixed in advance: the "gate" lines say whether the one call's
median lies below the old route's minimum, and one line says whether transposing the map pays.  Before anything is written every
route's handle is compared byte for byte with the old route's.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_gather_bench.py [--names 65536] [--pairs 2e7] [--k 8] [--fleet-names 1024] [--fleet-handles 60]
                                         [--fleet-pairs 2e6] [--reps 15] [--host-reps 3] [--out profiles/kept_gather.txt]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402
from loghisto_amd import keptfile  # noqa: E402

TOOL = "kept_gather_bench"
ROUTES = {"the direct route": N.GATHER_DIRECT, "the tile route": N.GATHER_TILE, "the tile route, map transposed": N.GATHER_TRANSPOSED}


def intervals(torch, M, n, K):
    """K kept intervals of one engine of M names, n pairs each"""
    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    kept = []
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        for _ in range(K):
            data.mul_(1.005)
            eng.submit_pairs_device(ids, data, n)
            with eng.flip() as s:
                kept.append(s.keep(M))
        del ids, data
        torch.cuda.empty_cache()
    assert all(k.info["samples"] == n for k in kept)
    eng.close()
    return kept


def measure(torch, a, rep, kept, routes, seed):
    """One measured thing: len(kept) handles x M rows, a random permutation per handle"""
    L = N.lib()
    K, M = len(kept), kept[0].info["nrows"]
    src = np.stack([np.random.default_rng(seed + i).permutation(M).astype(np.uint32) for i in range(K)])
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    what = f"{K} handle{'s' if K > 1 else ''} x {M} rows"

    def wall(label, call, reps, warmup):
        held = []

        def after(_, new):
            if held:
                held.pop().close()
            held.append(new)
            return new
        return kit.timed_wall(call, reps, warmup, label, 420, TOOL, None, after, sync=torch.cuda.synchronize)

    def old_route():
        loaded = [loghisto_amd.Kept.from_bytes(keptfile.gather([k.to_bytes()], line, checked=False)) for k, line in zip(kept, src)]
        if K == 1:
            return loaded[0]
        out = loaded[-1].merge(loaded[:-1])
        for k in loaded:
            k.close()
        return out

    t, blobs = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        for name in routes:
            with route(ROUTES[name]):
                ts, made = wall(f"{what} {name} {shape}", lambda: kept[-1].gather(d_src, kept[:-1]), a.reps, a.warmup)
            t[name, shape] = rep.row(f"lh_kept_gather_device (wall), {what}, {name}, a {shape} per row", ts)
            blobs[name, shape] = made.to_bytes()
            made.close()
        ts, old = wall(f"{what} old route {shape}", old_route, a.host_reps, 1)
        t["old", shape] = rep.row(f"  the route there was (wall), {what}: per handle save + host permutation + load"
                                  f"{', then lh_kept_merge' if K > 1 else ''}, a {shape} per row", ts)
        t["old min", shape] = min(ts)
        blobs["old", shape] = old.to_bytes()
        old.close()
    assert len(set(blobs.values())) == 1, [key for key, b in blobs.items() if b != blobs["old", "wave"]]
    for shape, _ in kit.SHAPES:
        for name in routes:
            met = t[name, shape] < t["old min", shape]
            rep.note(f"#   gate, lh_kept_gather_device, {what}, {name}, a {shape} per row: median {t[name, shape] * 1e3:.1f} us "
                     f"{'below' if met else 'NOT below'} the old route's minimum {t['old min', shape] * 1e3:.1f} us "
                     f"({t['old', shape] / t[name, shape]:.1f} x its median)", echo=True)
    plain, turned = t["the tile route", "wave"], t["the tile route, map transposed", "wave"]
    rep.note(f"#   transposing the staged map on the device, {what}, a wave per row: {turned * 1e3:.1f} us against {plain * 1e3:.1f} us: "
             f"{'pays' if turned < plain else 'does not pay'} ({plain / turned:.2f} x)", echo=True)
    if "the direct route" in routes:
        d, tl = t["the direct route", "wave"], t["the tile route", "wave"]
        rep.note(f"#   one handle, a wave per row: the direct route {d * 1e3:.1f} us, the tile route {tl * 1e3:.1f} us ({tl / d:.2f} x)", echo=True)
    del d_src


class route:
    """lh_tool_kept_gather_route set for a block; the value in force before comes back"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        import ctypes as C
        self.prev = C.c_uint32(0)
        assert N.lib().lh_tool_kept_gather_route(self.value, C.byref(self.prev)) == 0

    def __exit__(self, *exc):
        assert N.lib().lh_tool_kept_gather_route(self.prev.value, None) == 0


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=2e7)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--fleet-names", type=int, default=1024)
    ap.add_argument("--fleet-handles", type=int, default=60)
    ap.add_argument("--fleet-pairs", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_gather.txt"))
    a = ap.parse_args()
    assert 2 <= a.k <= N.MAX_KEPT and 2 <= a.fleet_handles <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=128, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs:g} --k {a.k} --fleet-names {a.fleet_names} --fleet-handles "
                                      f"{a.fleet_handles} --fleet-pairs {a.fleet_pairs:g} --reps {a.reps} --warmup {a.warmup} "
                                      f"--host-reps {a.host_reps}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher, a random permutation of the rows per handle;",
                  "# us are medians (min .. max) of the timed calls, wall time: every call returns when its new handle is complete"]
    kept = intervals(torch, a.names, int(a.pairs), a.k)
    measure(torch, a, rep, kept[-1:], list(ROUTES), 100)
    measure(torch, a, rep, kept, list(ROUTES)[1:], 200)
    for k in kept:
        k.close()
    torch.cuda.empty_cache()
    kept = intervals(torch, a.fleet_names, int(a.fleet_pairs), a.fleet_handles)
    measure(torch, a, rep, kept, list(ROUTES)[1:], 300)
    for k in kept:
        k.close()
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
