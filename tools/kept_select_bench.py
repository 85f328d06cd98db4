"""What lh_top's and lh_movers' selections over a window of kept intervals cost on the device (lh_kept_top*, lh_kept_movers*),
against the two routes there were before them -- same box, same process, same intervals.

Per name count: K intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the
scale moving 0.5 % per interval) are each flipped, kept and released; lh_kept_top ranks all K, lh_kept_movers the first K / 2
against the second K / 2.  Reported for each `by`, at k = 20:
  the score pass and the select pass (lh_tool_kept_top_passes_ms / lh_tool_kept_movers_passes_ms: HIP events on the stream around
  each), at 1 024 names in BOTH kernel shapes of the score pass (lh_tool_kept_switch), otherwise in the default shape;
  (b) the per-name route (wall, the wait included): lh_kept_across_device / lh_kept_compare_device over all names, the D2H copy of
  the arrays, a host argsort; and the per-name reader alone (HIP events), which is the walk the score pass takes;
  (a) the import route (wall, the wait included): K x lh_snapshot_add_buckets_csr_device into spare empty snapshots (one for top,
  two for movers), then lh_top_device / lh_movers_device there.  Taking and releasing the spares is not timed.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance: the tool records.  Before anything is
written the selections of the three routes are compared: ids for the integer scores, ids as sets otherwise.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_select_bench.py [--names 1024,65536] [--pairs 2e6,2e7] [--k 60] [--top 20] [--reps 15] [--warmup 3]
                                         [--host-reps 3] [--out profiles/kept_select.txt]"""
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

TOOL = "kept_select_bench"
TOP_BYS = (("count", None), ("sum", None), ("percentile", 0.99), ("count_above", 250.0))
MOVER_BYS = (("ks", None), ("w1", None), ("shift", None), ("percentile", 0.99))


def run(torch, a, M, n, rep):
    L = N.lib()
    K, k = a.k, a.top
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
    base, cur = kept[:K // 2], kept[K // 2:]
    h_all = (C.c_void_p * K)(*[h._h.value for h in kept])
    h_base = (C.c_void_p * len(base))(*[h._h.value for h in base])
    h_cur = (C.c_void_p * len(cur))(*[h._h.value for h in cur])
    prev = C.c_uint32(0)
    assert L.lh_tool_kept_switch(0, C.byref(prev)) == 0        # prev: the default
    default = "wave" if M >= prev.value else "workgroup"
    both = M <= 1024
    t = {}

    def passes(what, call):
        sc, se = [], []
        with kit.limit(240, what, TOOL):
            for r in range(a.warmup + a.reps):
                x, y = C.c_float(0), C.c_float(0)
                assert call(C.byref(x), C.byref(y)) == 0
                if r >= a.warmup:
                    sc.append(x.value)
                    se.append(y.value)
        return sc, se

    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        if not both and shape != default:
            continue
        for j, (by, arg) in enumerate(TOP_BYS):
            sc, se = passes(f"top passes {by} {shape}", lambda x, y: L.lh_tool_kept_top_passes_ms(
                C.addressof(h_all), K, 0, M, j, arg or 0.0, k, 0, st.cuda_stream, x, y))
            t["top", by, shape] = row(f"lh_kept_top by {by}: score pass, {M} names x {K} handles, a {shape} per row", sc)
            t["top_sel", by, shape] = row(f"lh_kept_top by {by}: select pass, {M} records, k = {k}", se)
        for j, (by, arg) in enumerate(MOVER_BYS):
            sc, se = passes(f"movers passes {by} {shape}", lambda x, y: L.lh_tool_kept_movers_passes_ms(
                C.addressof(h_base), len(base), C.addressof(h_cur), len(cur), 0, M, j, arg or 0.0, k, 0, st.cuda_stream, x, y))
            t["mov", by, shape] = row(f"lh_kept_movers by {by}: score pass, {M} names x {len(base)} + {len(cur)} handles, a {shape} per row", sc)
            t["mov_sel", by, shape] = row(f"lh_kept_movers by {by}: select pass, {M} records, k = {k}", se)
    new_top = {by: kept[-1].top(k, by, arg, False, kept[:-1], M, 0).copy() for by, arg in TOP_BYS}
    new_mov = {by: cur[-1].movers(base, k, by, arg, False, cur[:-1], M, 0).copy() for by, arg in MOVER_BYS}

    # ---- (b) the per-name route: the per-name reader over all names, the arrays to the host, an argsort there
    ac = dict(count=torch.zeros(M, dtype=torch.int64, device="cuda"), sum=torch.zeros(M, dtype=torch.float64, device="cuda"),
              nbuckets=torch.zeros(M, dtype=torch.int32, device="cuda"), present_bits=torch.zeros(M, dtype=torch.int64, device="cuda"),
              pkeys=torch.zeros(M, dtype=torch.int16, device="cuda"), pvalid=torch.zeros(M, dtype=torch.uint8, device="cuda"))
    cm = {f: torch.zeros(M, dtype=(torch.int16 if f == "key" else torch.float64 if f in ("ks", "w1", "shift") else torch.int64), device="cuda")
          for f in ("count_a", "count_b", "ks", "key", "below_a", "below_b", "w1", "shift")}
    t["ac"] = row(f"(b) lh_kept_across_device alone, {M} names x {K} handles, np = 1, default shape",
                  kit.timed_events(st, lambda: kept[-1].across(kept[:-1], [0.99], M, out=ac, stream=st), a.reps, a.warmup, "across", 180, TOOL))
    t["cm"] = row(f"(b) lh_kept_compare_device alone, {M} names x {len(base)} + {len(cur)} handles, default shape",
                  kit.timed_events(st, lambda: cur[-1].compare(base, M, 0, earlier=cur[:-1], out=cm, stream=st), a.reps, a.warmup, "compare",
                                   180, TOOL))
    state = {}

    def per_name_top():
        kept[-1].across(kept[:-1], [0.99], M, out=ac, stream=st)
        st.synchronize()
        h = {f: v.cpu().numpy() for f, v in ac.items()}
        order = np.argsort(-h["sum"], kind="stable")
        order = order[h["count"][order] != 0]
        state["top"] = [int(m) for m in order[:k] if len(order) <= k or h["sum"][m] > h["sum"][order[k]]]   # (clear of a tie at the cut)

    def per_name_movers():
        cur[-1].compare(base, M, 0, earlier=cur[:-1], out=cm, stream=st)
        st.synchronize()
        h = {f: v.cpu().numpy() for f, v in cm.items()}
        order = np.argsort(-np.nan_to_num(h["ks"], nan=-1.0), kind="stable")
        order = order[(h["count_a"][order] != 0) & (h["count_b"][order] != 0)]
        state["mov"] = [int(m) for m in order[:k] if len(order) <= k or h["ks"][m] > h["ks"][order[k]]]

    ts, _ = kit.timed_wall(per_name_top, a.host_reps, 1, "per-name route top", 240, TOOL, sync=torch.cuda.synchronize)
    t["top", "per_name"] = row(f"(b) per-name route (wall): lh_kept_across_device + 6 arrays D2H + argsort by sum, {M} names", ts)
    ts, _ = kit.timed_wall(per_name_movers, a.host_reps, 1, "per-name route movers", 240, TOOL, sync=torch.cuda.synchronize)
    t["mov", "per_name"] = row(f"(b) per-name route (wall): lh_kept_compare_device + 8 arrays D2H + argsort by ks, {M} names", ts)
    assert set(state["top"]) <= set(int(x) for x in new_top["sum"]["id"]) and len(state["top"]) >= min(k, 1)
    assert set(state["mov"]) <= set(int(x) for x in new_mov["ks"]["id"])

    # ---- (a) the import route: the handles into spare empty snapshots, then the snapshot's selecting reader there
    ent = torch.zeros((k * 32,), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    spares = []

    def fresh(nspare):
        def go():
            while spares:
                spares.pop().release()
            spares.extend(eng.flip() for _ in range(nspare))
            return list(spares)
        return go

    def import_top(sp):
        for h in kept:
            h.add_to(sp[0])
        sp[0].top(k, "sum", None, False, M, 0, out=(ent, cnt))
        torch.cuda.synchronize()

    def import_movers(sp):
        for h in base:
            h.add_to(sp[0])
        for h in cur:
            h.add_to(sp[1])
        sp[1].movers(sp[0], k, "ks", None, False, M, 0, out=(ent, cnt))
        torch.cuda.synchronize()

    ts, _ = kit.timed_wall(import_top, a.host_reps, 1, "import route top", 420, TOOL, before=fresh(1), sync=torch.cuda.synchronize)
    t["top", "import"] = row(f"(a) import route (wall): {K} x add_buckets_csr_device into a spare snapshot + lh_top_device by sum, {M} names", ts)
    got = ent.cpu().numpy().view(N.TOP_ENTRY)[:int(cnt.cpu()[0])]
    assert sorted(got["id"]) == sorted(new_top["sum"]["id"]) and list(got["count"][np.argsort(got["id"])]) == \
        list(new_top["sum"]["count"][np.argsort(new_top["sum"]["id"])])
    ts, _ = kit.timed_wall(import_movers, a.host_reps, 1, "import route movers", 420, TOOL, before=fresh(2), sync=torch.cuda.synchronize)
    t["mov", "import"] = row(f"(a) import route (wall): {K} x add_buckets_csr_device into two spare snapshots + lh_movers_device by ks, {M} names",
                             ts)
    got = ent.cpu().numpy().view(N.MOVER_ENTRY)[:int(cnt.cpu()[0])]
    assert got.tobytes() == new_mov["ks"].tobytes()             # ks: a fixed function of exact integers
    while spares:
        spares.pop().release()

    top_ms = t["top", "sum", default] + t["top_sel", "sum", default]
    mov_ms = t["mov", "ks", default] + t["mov_sel", "ks", default]
    rep.note(f"# {M} names x {K}: lh_kept_top by sum (default shape '{default}'), score + select {top_ms * 1e3:.0f} us | per-name route "
             f"{t['top', 'per_name'] * 1e3:.0f} us | import route {t['top', 'import'] * 1e3:.0f} us;  score pass / lh_kept_across_device: "
             f"{t['top', 'sum', default] / t['ac']:.2f} x", echo=True)
    rep.note(f"# {M} names x {len(base)} + {len(cur)}: lh_kept_movers by ks (default shape '{default}'), score + select {mov_ms * 1e3:.0f} us | "
             f"per-name route {t['mov', 'per_name'] * 1e3:.0f} us | import route {t['mov', 'import'] * 1e3:.0f} us;  score pass / "
             f"lh_kept_compare_device: {t['mov', 'ks', default] / t['cm']:.2f} x", echo=True)
    for h in kept:
        h.close()
    eng.close()
    torch.cuda.empty_cache()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="1024,65536")
    ap.add_argument("--pairs", default="2e6,2e7")
    ap.add_argument("--k", type=int, default=60)
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_select.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT and a.k % 2 == 0 and 1 <= a.top <= N.MAX_TOP
    torch.cuda.set_device(0)
    rep = kit.Report(width=112, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --k {a.k} --top {a.top} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed calls;",
                  "# passes: HIP events on the stream around each; the routes (a) and (b): wall time, the wait included;",
                  "# measured once, nothing tuned: the two score kernels and the shape switch are as first written"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
