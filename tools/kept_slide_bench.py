"""What advancing a rolling window of K kept intervals by one costs with lh_kept_slide -- new window = old window + newest
interval - oldest interval -- against the route it replaces, lh_kept_merge of the new window's K handles: same box, same
process, same intervals.

Per name count: K + 1 intervals of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values, the
scale moving 0.5 % per interval) are each flipped, kept and released; the first K are merged once into the window so far
(untimed).  Reported:
  lh_kept_slide(add = [window, newest], sub = [oldest]), all names (wall: the call returns when the new handle is complete), in
  BOTH kernel shapes (lh_tool_kept_switch);
  lh_kept_merge of the new window's K handles (wall), in both shapes;
  the slide's two passes alone, k_slide_count and k_slide_fill (HIP events around each, lh_tool_kept_slide_passes_ms), in both
  shapes;
  the bytes each route reads, and the ratio of the two calls.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance.  Before anything is written the slid
handle's arrays are compared byte for byte with the merged one's, and between the two shapes.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_slide_bench.py [--names 1024,65536] [--k 60] [--pairs 2e6,2e7] [--reps 15] [--out profiles/kept_slide.txt]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from loghisto_amd import _native as N  # noqa: E402

TOOL = "kept_slide_bench"


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
        for i in range(K + 1):
            data.mul_(1.005)
            eng.submit_pairs_device(ids, data, n)
            with eng.flip() as s:
                kept.append(s.keep(M))
        del ids, data
        torch.cuda.empty_cache()
    assert all(k.info["samples"] == n for k in kept)
    oldest, newest, window = kept[0], kept[K], kept[1:]
    with kit.limit(120, "the window so far", TOOL):
        so_far = kept[K - 1].merge(kept[:K - 1])
    assert so_far.info["samples"] == K * n

    def wall(what, call):
        """Every call makes a kept handle: the one of the call before is closed (untimed) once the next is made; the last is returned."""
        held = []

        def after(_, new):
            if held:
                held.pop().close()
            held.append(new)
            return new
        return kit.timed_wall(call, a.reps, a.warmup, what, 420, TOOL, None, after, sync=torch.cuda.synchronize)

    t, one = {}, {}
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        ts, one["slide", shape] = wall(f"slide {shape}", lambda: so_far.slide(add=[newest], sub=[oldest]))
        t["slide", shape] = row(f"lh_kept_slide (wall), add = [window, newest], sub = [oldest], {M} names, a {shape} per row", ts)
        ts, one["merge", shape] = wall(f"merge {shape}", lambda: window[-1].merge(window[:-1]))
        t["merge", shape] = row(f"lh_kept_merge (wall) of the window's {K} handles, {M} names, a {shape} per row", ts)
    prev = C.c_uint32(0)
    assert L.lh_tool_kept_switch(0, C.byref(prev)) == 0         # prev: the default (the shapes' loop has put it back)
    default = "wave" if M >= prev.value else "workgroup"
    want = listing(one["merge", "wave"])
    for key, k in one.items():
        assert listing(k) == want and k.info == one["merge", "wave"].info, key
    slid = one["slide", "wave"]
    assert slid.info["samples"] == K * n and slid.info["nrows"] == M

    # ---- the two passes alone
    VP = C.c_void_p
    add, sub = (VP * 2)(so_far._h.value, newest._h.value), (VP * 1)(oldest._h.value)
    for shape, _ in kit.shapes(L.lh_tool_kept_switch):
        with kit.limit(180, f"passes {shape}", TOOL):
            tc, tf = [], []
            for r in range(a.warmup + a.reps):
                m0, m1 = C.c_float(0), C.c_float(0)
                N.check(L.lh_tool_kept_slide_passes_ms(add, 2, sub, 1, 0, M, None, C.byref(m0), C.byref(m1)), "lh_tool_kept_slide_passes_ms")
                if r >= a.warmup:
                    tc.append(m0.value)
                    tf.append(m1.value)
        t["count", shape] = row(f"k_slide_count alone (events), {M} names, a {shape} per row", tc)
        t["fill", shape] = row(f"k_slide_fill alone (events), {M} names, a {shape} per row", tf)

    read_slide = so_far.info["bytes"] + newest.info["bytes"] + oldest.info["bytes"]
    read_merge = sum(k.info["bytes"] for k in window)
    rep.note(f"# {M} names: each pass of lh_kept_slide reads {read_slide / 2**20:.1f} MiB (the window {so_far.info['bytes'] / 2**20:.1f}, "
             f"the newest {newest.info['bytes'] / 2**20:.1f}, the oldest {oldest.info['bytes'] / 2**20:.1f}), each pass of lh_kept_merge "
             f"{read_merge / 2**20:.1f} MiB ({read_merge / read_slide:.1f} x); the new handle holds {slid.info['cells']} cells in "
             f"{slid.info['bytes'] / 2**20:.2f} MiB")
    rep.note(f"# {M} names: lh_kept_merge of the {K} / lh_kept_slide (default shape '{default}'): "
             f"{t['merge', default] / t['slide', default]:.1f} x;  slide, wave / workgroup: {t['slide', 'wave'] / t['slide', 'workgroup']:.2f};  "
             f"count + fill: {(t['count', default] + t['fill', default]) * 1e3:.1f} us of the {t['slide', default] * 1e3:.1f} us of the call")
    print("\n".join(rep.lines[-2:]), flush=True)
    for k in list(one.values()) + [so_far] + kept:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_slide.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs) and 2 <= a.k <= N.MAX_KEPT
    torch.cuda.set_device(0)
    rep = kit.Report(width=100, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --k {a.k} --pairs {a.pairs} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, each interval 0.5 % higher; us are medians (min .. max) of the timed calls;",
                  "# lh_kept_slide and lh_kept_merge: wall time (complete on return); the passes alone: HIP events around each kernel;",
                  "# ONE run, nothing tuned"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
