"""What stats and percentiles of a name over K snapshots cost on the device (lh_across*) against the only exact route there was
before, same box, same process, same snapshots.

K intervals of one engine of 32-bit cells (Zipf names, lognormal values: bench.py's stream, each interval its own seed and a
slowly moving scale) stay alive as K snapshots.  Reported, with the nine default percentiles:
  the device form (HIP events on the last snapshot's stream around the call) in BOTH kernel shapes (lh_tool_across_switch);
  the host form (wall);
  the old route (wall): K x buckets_all, a merge of the K listings on the host (sort by (name, bin), sum runs), add_buckets_csr
  into a spare empty snapshot, extract_compact there -- every occupied cell crosses PCIe twice, and the spare snapshot then
  no longer holds one interval.  Taking and releasing the spare snapshot is NOT timed;
  for scale: K x one lh_spread_device call with np = 9, one per snapshot -- roughly the cost of reading the same cells.
Medians of --reps calls after --warmup, with the spread (min .. max).  One thing is asserted: the old route's fastest run
is slower than the host form's slowest.  No other number is fixed in advance; the two ratios are recorded.  The results of the old route and of both shapes are compared before anything is written.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/across_bench.py [--names 8192] [--k 8] [--pairs 2e7] [--reps 25] [--warmup 5] [--out profiles/across.txt]"""
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
TOOL = "across_bench"
MARK = "# ==== measured: tools/across_bench.py"


def merge_listings(listings, M):
    """K x (offsets, keys, counts) of buckets_all -> one: runs of equal (name, bin) summed in uint64."""
    gid, cnt = [], []
    for off, keys, counts in listings:
        name = np.repeat(np.arange(M, dtype=np.int64), np.diff(off.astype(np.int64)))
        gid.append(name << 16 | ((keys.astype(np.int64) & 0xffff) ^ 0x8000))
        cnt.append(counts)
    gid, cnt = np.concatenate(gid), np.concatenate(cnt)
    order = np.argsort(gid, kind="stable")
    gid, cnt = gid[order], cnt[order]
    starts = np.flatnonzero(np.concatenate([[True], gid[1:] != gid[:-1]])) if gid.size else np.zeros(0, dtype=np.int64)
    sums = np.add.reduceat(cnt, starts) if gid.size else cnt
    g = gid[starts]
    offsets = np.searchsorted(g >> 16, np.arange(M + 1)).astype(np.uint64)
    keys = ((g & 0xffff) ^ 0x8000).astype(np.uint16).view(np.int16)
    return offsets, keys, sums.astype(np.uint64)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=8192)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--pairs", type=float, default=2e7)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "across.txt"))
    a = ap.parse_args()
    M, K, n = a.names, a.k, int(a.pairs)
    assert 1 <= K <= N.MAX_ACROSS
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=78)
    row = rep.row
    rep.lines += [MARK, *kit.header(TOOL, f"--names {M} --k {K} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  f"# {K} intervals of one engine of 32-bit cells (Zipf(1.0) names, lognormal values, each interval 2 % higher); us are "
                  "medians (min .. max) of the timed calls;", "# device forms: HIP events on the last snapshot's stream around the call(s); "
                  "host form and the old route: wall time"]

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=K + 2, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    snaps = []
    with kit.limit(420, "ingest", TOOL):
        for i in range(K):
            ids = bench.zipf_ids(n, M, 4000 + i)
            data = bench.make_samples(n, "lognormal", seed=40 + i)
            data.mul_(1.02 ** i)
            eng.submit_pairs_device(ids, data, n)
            snaps.append(eng.flip())
            torch.cuda.synchronize()
            del ids, data
        torch.cuda.empty_cache()
    last = snaps[-1]
    xs = torch.cuda.ExternalStream(last.stream())
    widths = [s.device_cells()[2] for s in snaps]
    rep.note(f"# {M} names, {K} snapshots of {n:g} samples each, cells of {widths} bytes")
    kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int32, pkeys=torch.int16,
                 pvalid=torch.uint8)

    def events(what, call):
        return kit.timed_events(xs, call, a.reps, a.warmup, what, 120, TOOL)

    def wall(what, call, reps, warmup=2, before=None, after=None):
        return kit.timed_wall(call, reps, warmup, what, 420, TOOL, before, after)

    # ---- lh_across: the device form in both shapes, the host form
    prev = C.c_uint32(0)
    t, res = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_across_switch):
        out = {k: torch.zeros((M, len(PCTS)) if k in ("pkeys", "pvalid") else (M,), dtype=d, device="cuda") for k, d in kinds.items()}
        ts = events(f"across {shape}", lambda: last.across(snaps[:-1], PCTS, M, out=out))
        res[shape] = {k: v.cpu().numpy() for k, v in out.items()}
        t[shape] = row(f"across device form, {M} names x {K} snapshots, np = 9, a {shape} per row", ts)
    assert L.lh_tool_across_switch(0, C.byref(prev)) == 0      # prev: the default (the shapes' loop has put it back)
    for k in ("count", "nbuckets", "present_bits", "pkeys", "pvalid"):
        assert np.array_equal(res["wave"][k], res["workgroup"][k]), k
    assert np.allclose(res["wave"]["sum"], res["workgroup"]["sum"], rtol=1e-9, atol=0)
    assert int(res["wave"]["count"].view(np.uint64).sum()) == K * n
    default = "wave" if M >= prev.value else "workgroup"
    ts, host = wall("across host form", lambda: last.across(snaps[:-1], PCTS, M), a.reps)
    t["host"] = row(f"across host form (wall, with the derived arrays), {M} names x {K} snapshots, np = 9", ts)
    host_ts = ts
    assert np.array_equal(host["count"], res[default]["count"].view(np.uint64)) and np.array_equal(host["pkeys"], res[default]["pkeys"])

    # ---- the old route: K x buckets_all, a host merge, add_buckets_csr into a spare snapshot, extract_compact there
    def old_route(spare):
        merged = merge_listings([s.buckets_all(M) for s in snaps], M)
        spare.add_buckets_csr(*merged)
        ex = spare.extract_compact(PCTS, M)
        return {k: ex[k].copy() for k in ("count", "sum", "nbuckets", "pkeys")}, int(merged[2].size)

    def release(spare, out):
        spare.release()
        return out

    ts, (old, ncells) = wall("old route", old_route, a.host_reps, 1, before=eng.flip, after=release)
    old_ts = ts
    t["old"] = row(f"old route (wall): {K} x buckets_all + host merge + add_buckets_csr + extract_compact", ts)
    rep.note(f"#   the old route moves {ncells} merged cells back to the device after pulling every snapshot's occupied cells out")
    assert np.array_equal(old["count"], host["count"]) and np.array_equal(old["nbuckets"], host["nbuckets"])
    assert np.array_equal(old["pkeys"], host["pkeys"])
    assert np.allclose(old["sum"], host["sum"], rtol=1e-9, atol=0)

    # ---- for scale: K x lh_spread_device with np = 9, one call per snapshot (all on one engine: one stream)
    sk = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8, count_le=torch.int64,
              sum_le=torch.float64)
    sout = {k: torch.zeros((M,) if k in ("count", "sum", "m2") else (M, len(PCTS)), dtype=d, device="cuda") for k, d in sk.items()}

    def k_spreads():
        for s in snaps:
            s.spread(PCTS, M, out=sout)

    assert all(s.stream() == last.stream() for s in snaps)
    t["spread"] = row(f"{K} x spread device form, one snapshot each, {M} names, np = 9 (for scale)", events("K x spread", k_spreads))

    # the acceptance: lh_across beats the old route by more than the run-to-run spread of either
    assert min(old_ts) > max(host_ts), (min(old_ts), max(host_ts))
    rep.note(f"# old route / across host form: {t['old'] / t['host']:.1f} x      across device form ({default}) / {K} x spread: "
             f"{t[default] / t['spread']:.2f}")
    print(rep.lines[-1], flush=True)
    for s in snaps:
        s.release()
    eng.close()

    # the compile-time resource table at the top of the file stays; the measured part is replaced
    rep.write(a.out, mark=MARK)
    return 0


if __name__ == "__main__":
    sys.exit(main())
