"""What lh_count_le's and lh_spread's outputs over a window of kept intervals cost on the device (lh_kept_count_le_device,
lh_kept_spread_device), against the route there was before them and against lh_kept_across_device over the same list -- same
box, same process, same intervals.

Per name count: K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the
scale moving 0.5 % per interval) are each flipped, kept and released.  Reported, with eight bounds and the nine default
percentiles:
  lh_kept_count_le_device and lh_kept_spread_device over the K handles for all names, in BOTH kernel shapes
  (lh_tool_kept_switch), and their *_ids_device forms for 20 ids: HIP events on the caller's stream;
  (b) lh_kept_across_device over the same list, in the same shapes: the reader whose row walk the two share;
  (a) the import route (wall, the wait included): K x lh_snapshot_add_buckets_csr_device into a spare empty snapshot, then
  lh_count_le_device / lh_spread_device there.  It needs a dense buffer to be alive; taking and releasing the spare is not timed;
  the snapshot readers alone on that filled snapshot (HIP events), for scale.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance: the tool records.  Before anything is
written the two shapes are compared bit for bit, the ids forms with the rows they name, and the integer outputs with the
import route's.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_readers_bench.py [--names 1024,65536] [--pairs 2e6,2e7] [--k 60] [--reps 15] [--warmup 3]
                                          [--host-reps 3] [--out profiles/kept_readers.txt]"""
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
BOUNDS = [1.0, 5.0, 10.0, 25.0, 50.0, 100.0, 250.0, 1000.0]  # cumulative `le` buckets across the lognormal body
TOOL = "kept_readers_bench"
NIDS = 20
SP_PER_P = ("pkeys", "pvalid", "count_le", "sum_le")
SP_EXACT = ("count", "pkeys", "pvalid", "count_le")


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
    st = torch.cuda.Stream()
    nb, npct = len(BOUNDS), len(PCTS)
    sp_kinds = dict(count=torch.int64, sum=torch.float64, m2=torch.float64, pkeys=torch.int16, pvalid=torch.uint8,
                    count_le=torch.int64, sum_le=torch.float64)
    ac_kinds = dict(count=torch.int64, sum=torch.float64, nbuckets=torch.int32, present_bits=torch.int64, pkeys=torch.int16,
                    pvalid=torch.uint8)

    def le_out(rows):
        return dict(cum=torch.zeros((rows * nb,), dtype=torch.int64, device="cuda"), total=torch.zeros((rows,), dtype=torch.int64, device="cuda"))

    def sp_out(rows):
        return {k: torch.zeros((rows * (npct if k in SP_PER_P else 1),), dtype=d, device="cuda") for k, d in sp_kinds.items()}

    def ac_out(rows):
        return {k: torch.zeros((rows * (npct if k in ("pkeys", "pvalid") else 1),), dtype=d, device="cuda") for k, d in ac_kinds.items()}

    def host(out):
        return {k: v.cpu().numpy() for k, v in out.items()}

    def events(what, call, stream=st):
        return kit.timed_events(stream, call, a.reps, a.warmup, what, 180, TOOL)

    rng = np.random.default_rng(20)
    ids20 = np.sort(rng.choice(min(M, 2000), NIDS, replace=False)).astype(np.uint32)   # busy names: the head of the Zipf order
    d_ids20 = torch.from_numpy(ids20.astype(np.int32)).cuda()
    last, earlier = kept[-1], kept[:-1]
    res, t = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        o = le_out(M)
        t["le", shape] = row(f"lh_kept_count_le_device, {M} names x {K} handles, nb = {nb}, a {shape} per row",
                             events(f"kept count_le {shape}", lambda: last.count_le(BOUNDS, earlier, M, out=o, stream=st)))
        res["le", shape] = host(o)
        o = sp_out(M)
        t["sp", shape] = row(f"lh_kept_spread_device, {M} names x {K} handles, np = {npct}, a {shape} per row",
                             events(f"kept spread {shape}", lambda: last.spread(PCTS, earlier, M, out=o, stream=st)))
        res["sp", shape] = host(o)
        o = ac_out(M)
        t["ac", shape] = row(f"(b) lh_kept_across_device, {M} names x {K} handles, np = {npct}, a {shape} per row",
                             events(f"kept across {shape}", lambda: last.across(earlier, PCTS, M, out=o, stream=st)))
        res["ac", shape] = host(o)
        o = le_out(NIDS)
        t["le20", shape] = row(f"lh_kept_count_le_ids_device, {NIDS} ids x {K} handles, nb = {nb}, a {shape} per row",
                               events(f"kept count_le ids {shape}", lambda: last.count_le(BOUNDS, earlier, ids=d_ids20, out=o, stream=st)))
        res["le20", shape] = host(o)
        o = sp_out(NIDS)
        t["sp20", shape] = row(f"lh_kept_spread_ids_device, {NIDS} ids x {K} handles, np = {npct}, a {shape} per row",
                               events(f"kept spread ids {shape}", lambda: last.spread(PCTS, earlier, ids=d_ids20, out=o, stream=st)))
        res["sp20", shape] = host(o)
        o = ac_out(NIDS)
        t["ac20", shape] = row(f"(b) lh_kept_across_ids_device, {NIDS} ids x {K} handles, np = {npct}, a {shape} per row",
                               events(f"kept across ids {shape}", lambda: last.across(earlier, PCTS, ids=d_ids20, out=o, stream=st)))
    # the two shapes walk alike: the same bits, floating-point sums included; the ids forms give the rows they name
    for what in ("le", "sp", "le20", "sp20"):
        for f, v in res[what, "wave"].items():
            assert v.tobytes() == res[what, "workgroup"][f].tobytes(), (what, f)
    for what in ("le", "sp"):
        for f, v in res[what, "wave"].items():
            assert res[what + "20", "wave"][f].tobytes() == v.reshape(M, -1)[ids20].tobytes(), (what, f)
    assert int(res["le", "wave"]["total"].view(np.uint64).sum()) == K * n
    assert res["sp", "wave"]["count"].tobytes() == res["ac", "wave"]["count"].tobytes() == res["le", "wave"]["total"].tobytes()
    assert res["sp", "wave"]["pkeys"].tobytes() == res["ac", "wave"]["pkeys"].tobytes()

    # ---- (a) the import route: K imports into a spare empty snapshot, then the snapshot reader there
    lo, so = le_out(M), sp_out(M)
    state = {}

    def fresh():
        if "spare" in state:
            state.pop("spare").release()
        return eng.flip()

    def keep_spare(spare, _):
        state["spare"] = spare
        return spare

    def route(reader):
        def go(spare):
            for k in kept:
                k.add_to(spare)
            if reader == "le":
                spare.count_le(BOUNDS, M, out=(lo["cum"], lo["total"]))
            else:
                spare.spread(PCTS, M, out=so)
            torch.cuda.synchronize()
        return go

    for reader, name in (("le", "lh_count_le_device"), ("sp", "lh_spread_device")):
        ts, spare = kit.timed_wall(route(reader), a.host_reps, 1, f"import route {reader}", 420, TOOL, before=fresh, after=keep_spare,
                                   sync=torch.cuda.synchronize)
        t[reader, "old"] = row(f"(a) import route (wall, with the wait): {K} x add_buckets_csr_device into a spare snapshot + {name}, {M} names", ts)
    old_le, old_sp = host(lo), host(so)
    for f in ("cum", "total"):
        assert old_le[f].tobytes() == res["le", "wave"][f].tobytes(), f
    for f in SP_EXACT:
        assert old_sp[f].tobytes() == res["sp", "wave"][f].tobytes(), f
    for f in ("sum", "m2", "sum_le"):                           # another walk, another order of the adds
        assert np.allclose(old_sp[f], res["sp", "wave"][f], rtol=1e-9, atol=0), f
    # ---- the snapshot readers alone on the snapshot the route has just filled
    xs = torch.cuda.ExternalStream(spare.stream())
    t["le", "live"] = row(f"lh_count_le_device on the filled snapshot, {M} names, nb = {nb}",
                          events("count_le live", lambda: spare.count_le(BOUNDS, M, out=(lo["cum"], lo["total"])), xs))
    t["sp", "live"] = row(f"lh_spread_device on the filled snapshot, {M} names, np = {npct}",
                          events("spread live", lambda: spare.spread(PCTS, M, out=so), xs))
    state.pop("spare").release()
    prev = C.c_uint32(0)
    assert L.lh_tool_kept_switch(0, C.byref(prev)) == 0        # prev: the default (the shapes' loop has put it back)
    default = "wave" if M >= prev.value else "workgroup"
    for reader, name in (("le", "lh_kept_count_le_device"), ("sp", "lh_kept_spread_device")):
        rep.note(f"# {M} names x {K}: {name} (default shape '{default}') / lh_kept_across_device: "
                 f"{t[reader, default] / t['ac', default]:.2f} x;  import route / {name}: {t[reader, 'old'] / t[reader, default]:.1f} x;  "
                 f"wave / workgroup: {t[reader, 'wave'] / t[reader, 'workgroup']:.2f};  {NIDS} ids / lh_kept_across_ids_device: "
                 f"{t[reader + '20', 'workgroup'] / t['ac20', 'workgroup']:.2f} x", echo=True)
    rep.note(f"# {M} names: a kept interval holds {kept[0].info['bytes'] / 2**20:.2f} MiB; a dense buffer of 32-bit cells "
             f"{M * loghisto_amd.Snapshot.row_stride() * 4 / 2**20:.0f} MiB", echo=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_readers.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=100, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed calls;",
                  "# device forms: HIP events on the stream around the call; the import route: wall time, the wait included;",
                  "# measured once, nothing tuned: the two kernels are as first written"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
