"""What rolling kept rows up ACROSS names costs in ONE call (lh_kept_group_device), against the route there was before -- same box,
same process, same intervals.

Kept intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the scale moving 0.5 %
per interval).  The groups are a random partition of the names (a random permutation cut into groups).  Measured, each in BOTH
kernel shapes (lh_tool_kept_switch), wall time (the call returns when the new handle is complete; the handle it makes is closed
untimed):
  --names names in groups of each of --sizes x 1 handle                                   (gated)
  --fleet-names names in groups of --fleet-size x --fleet-handles handles                 (gated)
  --names names in ONE group x 1 handle -- one workgroup (or one wave) does it all        (reported)
  --names names in --zipf-groups groups whose sizes fall off as 1 / rank x 1 handle       (reported)
Beside each, the route there was: lh_kept_gather_device with the handles listed repeatedly -- a round takes at most 64 sources of
every group, floor(64 / handles) members of each, LH_KEPT_NO_ROW where a group is shorter, its map built on the device beforehand
and not timed -- and, where there is more than one round, lh_kept_merge of the rounds' handles, 64 at a time, until one is left.
Medians of the timed calls with the spread (min .. max).  No ratio is fixed in advance: a "gate" line says whether the one call's
median lies below the old route's minimum (met / NOT met); a "reported" line gives the same two numbers without a verdict.  Before
anything is written the one call's handle is compared byte for byte with the old route's, in both shapes.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_group_bench.py [--names 65536] [--pairs 2e7] [--sizes 64,256] [--zipf-groups 256] [--fleet-names 1024]
                                        [--fleet-handles 60] [--fleet-size 64] [--fleet-pairs 2e6] [--reps 15] [--host-reps 3]
                                        [--out profiles/kept_group.txt]"""
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

TOOL = "kept_group_bench"
NO = N.KEPT_NO_ROW


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


def cut(M, sizes, seed):
    """a random permutation of the M names cut into groups of `sizes` (which add up to M at most)"""
    perm = np.random.default_rng(seed).permutation(M).astype(np.uint32)
    goff = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint64)
    assert int(goff[-1]) <= M
    return goff, perm[:int(goff[-1])]


def old_maps(torch, goff, members, K):
    """the maps of the old route's rounds, on the device: per round [K * c, ngroups], c = floor(64 / K) copies of every handle"""
    ngroups, c = goff.size - 1, N.MAX_KEPT // K
    sizes = np.diff(goff).astype(np.int64)
    rounds = max(1, -(-int(sizes.max()) // c))
    padded = np.full((ngroups, rounds * c), NO, dtype=np.uint32)              # member j of group g at [g, j]
    col = np.arange(members.size, dtype=np.int64) - np.repeat(goff[:-1].astype(np.int64), sizes)
    padded[np.repeat(np.arange(ngroups), sizes), col] = members
    maps = []
    for r in range(rounds):
        one = np.ascontiguousarray(padded[:, r * c:(r + 1) * c].T)            # [c, ngroups]: copy k takes member r * c + k
        maps.append(torch.from_numpy(np.tile(one, (K, 1)).view(np.int32)).cuda())   # handle-major, c consecutive entries a handle
    return maps, c


def measure(torch, a, rep, kept, goff, members, what, gated):
    """One measured thing: the groups (goff, members) over the handles `kept`"""
    L = N.lib()
    K = len(kept)
    d_goff, d_members = torch.from_numpy(goff.view(np.int64)).cuda(), torch.from_numpy(members.view(np.int32)).cuda()
    maps, c = old_maps(torch, goff, members, K)
    listed = [k for k in kept for _ in range(c)]

    def wall(label, call, reps, warmup):
        held = []

        def after(_, new):
            if held:
                held.pop().close()
            held.append(new)
            return new
        return kit.timed_wall(call, reps, warmup, label, 420, TOOL, None, after, sync=torch.cuda.synchronize)

    def old_route():
        parts = [listed[-1].gather(m, listed[:-1]) for m in maps]
        while len(parts) > 1:
            merged = []
            for at in range(0, len(parts), N.MAX_KEPT):
                some = parts[at:at + N.MAX_KEPT]
                merged.append(some[-1].merge(some[:-1]) if len(some) > 1 else some[0])
                for k in some:
                    if k is not merged[-1]:
                        k.close()
            parts = merged
        return parts[0]

    rounds = len(maps)
    route = f"{rounds} round{'s' if rounds > 1 else ''} of lh_kept_gather_device{', then lh_kept_merge' if rounds > 1 else ''}"
    t, blobs = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        ts, made = wall(f"{what} {shape}", lambda: kept[-1].group((d_goff, d_members), kept[:-1]), a.reps, a.warmup)
        t["new", shape] = rep.row(f"lh_kept_group_device (wall), {what}, a {shape} per row", ts)
        blobs["new", shape] = made.to_bytes()
        made.close()
        ts, old = wall(f"{what} old route {shape}", old_route, a.host_reps, 1)
        t["old", shape] = rep.row(f"  the route there was (wall), {what}: {route}, a {shape} per row", ts)
        t["old min", shape] = min(ts)
        blobs["old", shape] = old.to_bytes()
        old.close()
    assert len(set(blobs.values())) == 1, [key for key, b in blobs.items() if b != blobs["old", "wave"]]
    for shape, _ in kit.SHAPES:
        new, low, old = t["new", shape], t["old min", shape], t["old", shape]
        numbers = (f"median {new * 1e3:.1f} us {'below' if new < low else 'NOT below'} the old route's minimum {low * 1e3:.1f} us "
                   f"({old / new:.1f} x its median)")
        if gated:
            rep.note(f"#   gate, lh_kept_group_device, {what}, a {shape} per row: {'met' if new < low else 'NOT met'}: {numbers}", echo=True)
        else:
            rep.note(f"#   reported, lh_kept_group_device, {what}, a {shape} per row: {numbers}", echo=True)
    del d_goff, d_members, maps


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=2e7)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--zipf-groups", type=int, default=256)
    ap.add_argument("--fleet-names", type=int, default=1024)
    ap.add_argument("--fleet-handles", type=int, default=60)
    ap.add_argument("--fleet-size", type=int, default=64)
    ap.add_argument("--fleet-pairs", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_group.txt"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    assert all(1 <= g <= a.names for g in sizes) and 1 <= a.fleet_handles <= N.MAX_KEPT and 1 <= a.fleet_size <= a.fleet_names
    assert 1 <= a.zipf_groups <= a.names
    torch.cuda.set_device(0)
    rep = kit.Report(width=136, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs:g} --sizes {a.sizes} --zipf-groups {a.zipf_groups} --fleet-names "
                                      f"{a.fleet_names} --fleet-handles {a.fleet_handles} --fleet-size {a.fleet_size} --fleet-pairs "
                                      f"{a.fleet_pairs:g} --reps {a.reps} --warmup {a.warmup} --host-reps {a.host_reps}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; the groups are a random permutation of the names, cut;",
                  "# us are medians (min .. max) of the timed calls, wall time: every call returns when its new handle is complete"]
    plural = lambda n, word: f"{n} {word}{'s' if n != 1 else ''}"             # noqa: E731
    M = a.names
    kept = intervals(torch, M, int(a.pairs), 1)
    for G in sizes:
        goff, members = cut(M, [G] * (M // G), 100 + G)
        measure(torch, a, rep, kept, goff, members, f"{M} names -> {plural(M // G, 'group')} of {G} x 1 handle", True)
    goff, members = cut(M, [M], 200)
    measure(torch, a, rep, kept, goff, members, f"{M} names -> ONE group x 1 handle", False)
    weights = 1.0 / np.arange(1, a.zipf_groups + 1)
    zipf = np.maximum(1, np.floor(weights / weights.sum() * (M - a.zipf_groups)).astype(np.int64))
    goff, members = cut(M, zipf, 300)
    measure(torch, a, rep, kept, goff, members,
            f"{M} names -> {plural(a.zipf_groups, 'group')} of Zipf sizes {int(zipf[0])} .. {int(zipf[-1])} x 1 handle", False)
    for k in kept:
        k.close()
    torch.cuda.empty_cache()
    M, G = a.fleet_names, a.fleet_size
    kept = intervals(torch, M, int(a.fleet_pairs), a.fleet_handles)
    goff, members = cut(M, [G] * (M // G), 400)
    measure(torch, a, rep, kept, goff, members, f"{M} names -> {plural(M // G, 'group')} of {G} x {plural(a.fleet_handles, 'handle')}", True)
    for k in kept:
        k.close()
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
