"""What "the k names whose distribution moved most" costs on the device (lh_movers*) beside what a caller does without it:
lh_compare in the host form for ks only, its copy back, and numpy.argpartition plus a sort of k = 20 -- same box, same
process, same snapshots as tools/compare_bench.py.

Two intervals of one engine (num_buffers = 3): --names names, lognormal values whose scale drifts with the name, the second
interval 10 % higher.  Reported, for --names and for the first 1 024 names: lh_movers_device per `by` (HIP events on cur's
stream around the call), its two passes through lh_tool_movers_passes_ms, the host form (wall), and the baseline (wall).
Medians of --reps calls after --warmup, with the spread (min .. max).  No number is fixed in advance.  The ids of the device
form, the host form and the baseline must agree.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started on
the GPU after a step that hung), and the first failed check ends the run.  The file's lines before MARK (the compile-time resource table)
are kept.
usage: python tools/movers_bench.py [--names 65536] [--pairs 6e7] [--reps 25] [--warmup 5] [--k 20] [--out profiles/movers.txt]"""
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

MARK = "# ==== measured: tools/movers_bench.py"
TOOL = "movers_bench"
BYS = (("ks", None), ("w1", None), ("shift", None), ("percentile", 0.99))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=6e7, help="per interval")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "movers.txt"))
    a = ap.parse_args()
    M, n, K = a.names, int(a.pairs), a.k
    torch.cuda.set_device(0)
    L = N.lib()
    rep = kit.Report(width=72)
    row = rep.row
    rep.lines += [MARK, *kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup} --k {K}", torch),
                  "# two intervals of one engine (Zipf(1.0) names, lognormal values, the second interval 10 % higher); us are medians "
                  "(min .. max) of the timed calls;", "# device forms and passes: HIP events on cur's stream; host form and baseline: wall time"]

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

    def events(what, call):
        return kit.timed_events(xs, call, a.reps, a.warmup, what, 120, TOOL)

    def wall(what, call):
        return kit.timed_wall(call, a.reps, 2, what, 300, TOOL)

    select_over_score = {}

    def one_size(nmetrics, indent=""):
        ent = torch.zeros((K * 32,), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        for by, arg in BYS:
            name = by if arg is None else f"{by} p={arg}"
            ts = events(f"movers {name} {nmetrics}", lambda: cur.movers(base, K, by, arg, False, nmetrics, out=(ent, cnt)))
            row(f"{indent}movers device form by {name}, k = {K}, {nmetrics} names", ts)
            dev = ent.cpu().numpy().view(N.MOVER_ENTRY)[:int(cnt.cpu()[0])].copy()
            sc, se = [], []
            s_ms, e_ms = C.c_float(0), C.c_float(0)
            with kit.limit(120, f"passes {name} {nmetrics}", TOOL):
                for r in range(a.warmup + a.reps):
                    rc = L.lh_tool_movers_passes_ms(base._h, cur._h, 0, nmetrics, N.MOVERS_BY_KS + [b for b, _ in BYS].index(by), arg or 0.0,
                                                    K, 0, C.byref(s_ms), C.byref(e_ms))
                    assert rc == 0, rc
                    if r >= a.warmup:
                        sc.append(s_ms.value)
                        se.append(e_ms.value)
            ms = row(f"{indent}  score pass", sc)
            me = row(f"{indent}  select pass (one workgroup)", se)
            select_over_score[(nmetrics, name)] = me / ms
            ts, host = wall(f"movers host {name} {nmetrics}", lambda: cur.movers(base, K, by, arg, False, nmetrics))
            row(f"{indent}  movers host form (wall)", ts)
            assert host.tobytes() == dev.tobytes(), (by, nmetrics)
            if by == "ks":
                def today():
                    res = cur.compare(base, nmetrics, out=today.out)
                    ks = res["ks"]
                    ok = np.nonzero(~np.isnan(ks))[0]
                    kk = min(K, ok.size)
                    if not kk:
                        return ok
                    # (argpartition leaves ties at the cut to chance: everything at or above the k-th value is sorted)
                    kth = ks[ok[np.argpartition(-ks[ok], kk - 1)[kk - 1]]]
                    part = ok[ks[ok] >= kth]
                    return part[np.lexsort((part, -ks[part]))][:kk]
                today.out = {"ks": torch.zeros((nmetrics,), dtype=torch.float64).pin_memory().numpy()}
                ts, ids = wall(f"baseline {nmetrics}", today)
                row(f"{indent}  baseline: compare host form for ks (pinned), argpartition + sort (wall)", ts)
                rep.note(f"{indent}  the baseline copies {nmetrics * 8} bytes back, lh_movers {K * 32 + 8}")
                print(rep.lines[-1], flush=True)
                assert ids.tolist() == host["id"].tolist(), (ids[:5], host["id"][:5])

    one_size(M)
    if M > 1024:
        rep.note("# the first 1 024 names (Zipf: the widest windows):")
        one_size(1024, indent="  ")
    worst = max((v, k) for k, v in select_over_score.items() if k[0] == M)
    rep.note(f"# select pass / score pass at {M} names: at most {worst[0]:.2f} (by {worst[1][1]})" +
             (": the one-workgroup select costs more than the score pass -- a histogram pass over several workgroups is the "
                  "next lever (not built here)" if worst[0] > 1 else ""))
    print(rep.lines[-1], flush=True)
    for s in snaps:
        s.release()
    eng.close()

    rep.write(a.out, mark=MARK)
    return 0


if __name__ == "__main__":
    sys.exit(main())
