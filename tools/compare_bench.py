"""What the per-name distribution shift between two snapshots costs on the device (lh_compare*) beside two moment-only
lh_spread_device calls, one per snapshot -- those read the same cells the same number of times (two walks of each row) --
same box, same process, same snapshots.

Two intervals of one engine (num_buffers = 3): --names names, lognormal values whose scale drifts with the name, the second
interval 10 % higher.  Reported, for --names and for the first 1 024 names: the device form (HIP events on cur's stream around
the call) in BOTH kernel shapes (a wave per row / a workgroup per row: lh_tool_compare_switch), each beside the two spread
reads in the shape the same switch value gives lh_spread, with the ratio; the host form (wall); both shapes over the first
256 .. 16 384 names, which is where a switch default would come from; and one name whose rows are filled over the full key
range.  Medians of --reps calls after --warmup, with the spread (min .. max).  No number is fixed in advance.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started on
the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/compare_bench.py [--names 65536] [--pairs 6e7] [--reps 25] [--warmup 5] [--out profiles/compare.txt]"""
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

TOOL = "compare_bench"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=6e7, help="per interval")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare.txt"))
    a = ap.parse_args()
    M, n = a.names, int(a.pairs)
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=66)
    row = rep.row
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# two intervals of one engine (Zipf(1.0) names, lognormal values, the second interval 10 % higher); us are medians "
                  "(min .. max) of the timed calls;", "# device forms: HIP events on cur's stream around the call(s); host form: wall time"]

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16)
    snaps = []
    for k, scale in enumerate((1.0, 1.1)):
        with kit.limit(300, f"interval {k}", TOOL):
            ids = bench.zipf_ids(n, M, 4000 + k)
            data = bench.make_samples(n, "lognormal", seed=40 + k)
            data.mul_(scale * torch.exp(3e-5 * ids.to(torch.float64)))
            bi, bd = bench.OwnBuffer(ids), bench.OwnBuffer(data)
            torch.cuda.synchronize()
            eng.submit_pairs_device(bi.tensor, bd.tensor, n)
            snaps.append(eng.flip())
            torch.cuda.synchronize()
            bi.free()
            bd.free()
            del ids, data
            torch.cuda.empty_cache()
    base, cur = snaps
    xs = torch.cuda.ExternalStream(cur.stream())
    rep.note(f"# {M} names, {n:g} samples per interval, cells of {base.device_cells()[2]} and {cur.device_cells()[2]} bytes")
    kinds = dict(count_a=torch.int64, count_b=torch.int64, ks=torch.float64, key=torch.int16, below_a=torch.int64,
                 below_b=torch.int64, w1=torch.float64, shift=torch.float64)

    def events(what, call):
        return kit.timed_events(xs, call, a.reps, a.warmup, what, 120, TOOL)

    def compare_device(what, c, b, nmetrics):
        out = {k: torch.zeros((nmetrics,), dtype=t, device="cuda") for k, t in kinds.items()}
        ts = events(what, lambda: c.compare(b, nmetrics, out=out))
        return ts, {k: v.cpu().numpy() for k, v in out.items()}

    def spread_reads(what, c, b, nmetrics):
        """two moment-only lh_spread_device calls, one per snapshot (both are snapshots of one engine: one stream)"""
        outs = [{k: torch.zeros((nmetrics,), dtype=t, device="cuda") for k, t in
                 (("count", torch.int64), ("sum", torch.float64), ("m2", torch.float64))} for _ in range(2)]

        def call():
            b.spread([], nmetrics, out=outs[0])
            c.spread([], nmetrics, out=outs[1])
        assert b.stream() == c.stream()
        ts = events(what, call)
        return ts, [o["count"].cpu().numpy().view(np.uint64) for o in outs]

    def both(c, b, nmetrics, indent=""):
        """lh_compare_device and the two spread reads in each shape, alternating; the integer outputs of the shapes agree"""
        res = {}
        for shape, _ in kit.shapes(lambda w, prev: L.lh_tool_compare_switch(w, prev) or L.lh_tool_spread_switch(w, prev)):
            tc, res[shape] = compare_device(f"compare {shape} {nmetrics}", c, b, nmetrics)
            tr, counts = spread_reads(f"spread {shape} {nmetrics}", c, b, nmetrics)
            assert np.array_equal(counts[0], res[shape]["count_a"].view(np.uint64))
            assert np.array_equal(counts[1], res[shape]["count_b"].view(np.uint64))
            mc = row(f"{indent}compare device form, {nmetrics} names, a {shape} per row", tc)
            mr = row(f"{indent}  two moment-only spread reads, {nmetrics} names, a {shape} per row", tr)
            rep.note(f"{indent}  ratio compare / two spread reads: {mc / mr:.2f}")
            print(rep.lines[-1], flush=True)
        for k in ("count_a", "count_b", "ks", "key", "below_a", "below_b"):
            assert res["wave"][k].tobytes() == res["workgroup"][k].tobytes(), k
        for k in ("w1", "shift"):                               # the shapes associate the sums differently
            assert np.allclose(res["wave"][k], res["workgroup"][k], rtol=1e-9, atol=1e-9, equal_nan=True), k
        return res["wave"]

    full = both(cur, base, M)
    assert int(full["count_a"].view(np.uint64).sum()) == n and int(full["count_b"].view(np.uint64).sum()) == n
    ok = ~np.isnan(full["shift"])
    rep.note(f"# names with samples in both intervals: {int(ok.sum())}; median shift {np.median(full['shift'][ok]):.2f} buckets "
             f"(a scale of 1.1 is 100 ln 1.1 = 9.53 buckets where 1 + v ~ v), median ks {np.median(full['ks'][ok]):.4f}")
    ts, host = kit.timed_wall(lambda: cur.compare(base, M), a.reps, 2, "host form", 300, TOOL)
    row(f"compare host form (wall, pinned results), {M} names", ts)
    for k in ("count_a", "count_b", "ks", "key", "below_a", "below_b"):
        assert host[k].tobytes() == full[k].tobytes(), k
    rep.note("# both kernel shapes over the first names (Zipf: the widest windows):")
    for k in (256, 1024, 2048, 4096, 16384):
        if k < M:
            part = both(cur, base, k, indent="  ")
            assert part["key"].tobytes() == full["key"][:k].tobytes()
    for s in snaps:
        s.release()
    eng.close()

    # ---- one name, both rows filled over the full key range (64-bit cells; 512 KiB each)
    with kit.limit(120, "one full row", TOOL):     # (two snapshots of one engine: not benchkit.full_row_snapshot)
        one = loghisto_amd.Engine(device=0, max_metrics=1, num_buffers=3, num_lanes=1, lane_samples=1 << 16)
        base, cur = one.flip(), one.flip()
        keys = np.arange(-32768, 32768, dtype=np.int16)
        base.add_buckets(np.zeros(keys.size, dtype=np.uint32), keys, np.full(keys.size, 3, dtype=np.uint64))
        cur.add_buckets(np.zeros(keys.size, dtype=np.uint32), keys, (1 + np.arange(keys.size) % 5).astype(np.uint64))
        xs = torch.cuda.ExternalStream(cur.stream())
    rep.note("# one name, all 65 536 cells occupied on both sides, device form:")
    got = both(cur, base, 1, indent="  ")
    assert int(got["count_a"][0]) == 3 * 65536 and int(got["count_b"][0]) == int((1 + np.arange(65536) % 5).sum())
    base.release()
    cur.release()
    one.close()

    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
