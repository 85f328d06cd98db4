"""What saving a kept interval and loading it back costs (lh_kept_save*, lh_kept_load*), against the routes there were before,
and what the load's check costs on its own -- same box, same process, same interval.

Per name count: one interval of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values) is
flipped and kept.  Reported:
  lh_kept_save into pageable and into pinned host memory and lh_kept_save_device (wall: a save is complete on return), against
  the route there was (wall): lh_kept_arrays and four copies to the host;
  lh_kept_load from pageable and from pinned host memory and lh_kept_load_device (wall: a load is complete on return; the
  handle it makes is closed untimed), against the route there was (wall): lh_snapshot_add_buckets_csr of the host arrays into a
  live empty snapshot, then lh_keep there.  That route needs an engine and a dense buffer; taking and releasing the snapshot is
  not timed;
  the check alone (HIP events around each kernel, lh_tool_kept_check_ms): k_kept_check and k_kept_check_samples over the
  handle's own block, and beside them the yardstick: k_keep_count over the same interval while its snapshot is alive
  (lh_tool_keep_count_ms).  The check reads 10 B a cell and 16 B a row, once: its rate over those bytes is noted.
Medians of the timed calls with the spread (min .. max).  No number is fixed in advance.  Before anything is written the blob is
compared byte for byte between the three saves and with loghisto_amd.keptfile.pack of the arrays, and the arrays of every
loaded handle and of the old route's handle with the original's.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_store_bench.py [--names 1024,65536] [--pairs 2e6,2e7] [--reps 15] [--out profiles/kept_store.txt]"""
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
from loghisto_amd import keptfile  # noqa: E402

TOOL = "kept_store_bench"


def listing(k):
    return [t.cpu().numpy().tobytes() for t in k.arrays()]


def run(torch, a, M, n, rep):
    L = N.lib()
    row = rep.row
    fp = C.POINTER(C.c_float)

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        eng.submit_pairs_device(ids, data, n)
        snap = eng.flip()
        k = snap.keep(M)
        del ids, data
        torch.cuda.empty_cache()
    assert k.info["samples"] == n and k.info["nrows"] == M
    cells, size = k.info["cells"], 64 + k.info["bytes"]
    want = listing(k)

    # ---- the yardstick while the snapshot is alive: lh_keep's first pass alone
    with kit.limit(180, "k_keep_count", TOOL):
        ts = []
        for r in range(a.warmup + a.reps):
            ms = C.c_float(0)
            N.check(L.lh_tool_keep_count_ms(snap._h, 0, M, C.byref(ms)), "lh_tool_keep_count_ms")
            if r >= a.warmup:
                ts.append(ms.value)
    t_count = row(f"k_keep_count alone (events), {M} names", ts)
    snap.release()

    # ---- the check alone
    with kit.limit(180, "k_kept_check", TOOL):
        tc, tsamp = [], []
        for r in range(a.warmup + a.reps):
            m0, m1 = C.c_float(0), C.c_float(0)
            N.check(L.lh_tool_kept_check_ms(k._h, None, C.byref(m0), C.byref(m1)), "lh_tool_kept_check_ms")
            if r >= a.warmup:
                tc.append(m0.value)
                tsamp.append(m1.value)
    t_check = row(f"k_kept_check alone (events), {M} names, {cells} cells", tc)
    t_samples = row(f"k_kept_check_samples alone (events), {M} names", tsamp)

    def wall(what, call, reps, before=None, after=None):
        return kit.timed_wall(call, reps, a.warmup if reps > 1 else 1, what, 420, TOOL, before, after, sync=torch.cuda.synchronize)

    # ---- save
    pageable = np.zeros(size, dtype=np.uint8)
    pinned = torch.zeros(size, dtype=torch.uint8, pin_memory=True).numpy()
    dev = torch.zeros(size, dtype=torch.uint8, device="cuda")
    t = {}
    for what, fn, buf in (("lh_kept_save, pageable host memory", L.lh_kept_save, pageable.ctypes.data),
                          ("lh_kept_save, pinned host memory", L.lh_kept_save, pinned.ctypes.data),
                          ("lh_kept_save_device", L.lh_kept_save_device, int(dev.data_ptr()))):
        ts, _ = wall(what, lambda fn=fn, buf=buf: N.check(fn(k._h, buf, size, None, None), what), a.reps)
        t[what] = row(f"{what} (wall), {M} names, {size / 2**20:.2f} MiB", ts)
    blob = pageable.tobytes()
    assert pinned.tobytes() == blob and dev.cpu().numpy().tobytes() == blob
    off, keys, counts, _ = [x.cpu().numpy() for x in k.arrays()]
    assert keptfile.pack(off.view(np.uint64), keys, counts.view(np.uint64), first=0) == blob and keptfile.check(blob) is None
    ts, host_arrays = wall("four copies", lambda: [x.cpu() for x in k.arrays()], a.reps)
    t["old save"] = row(f"old route (wall): lh_kept_arrays + four copies to the host, {M} names", ts)

    # ---- load
    def closing(_, new):
        assert new.info == k.info
        got = listing(new)
        new.close()
        return got

    def loader(fn, addr):
        def call():
            h = C.c_void_p(0)
            N.check(fn(0, addr, size, 0, None, None, C.byref(h)), "load")
            return loghisto_amd.Kept(h, None)
        return call

    for what, fn, buf in (("lh_kept_load, pageable host memory", L.lh_kept_load, pageable.ctypes.data),
                          ("lh_kept_load, pinned host memory", L.lh_kept_load, pinned.ctypes.data),
                          ("lh_kept_load_device", L.lh_kept_load_device, int(dev.data_ptr()))):
        ts, got = wall(what, loader(fn, buf), a.reps, after=closing)
        assert got == want, what
        t[what] = row(f"{what} (wall), {M} names, {size / 2**20:.2f} MiB", ts)

    h_off, h_keys, h_counts = off.view(np.uint64), keys, counts.view(np.uint64)

    def old_load(spare):
        spare.add_buckets_csr(h_off, h_keys, h_counts)
        return spare.keep(M)

    def release(spare, new):
        got = closing(None, new)
        spare.release()
        return got

    ts, got = wall("old load", old_load, a.host_reps, before=eng.flip, after=release)
    assert got == want
    t["old load"] = row(f"old route (wall): add_buckets_csr into a live snapshot + lh_keep there, {M} names", ts)

    read = 10 * cells + 16 * M
    rep.note(f"# {M} names: k_kept_check reads {read / 2**20:.2f} MiB once: {read / (t_check * 1e-3) / 1e9:.1f} GB/s;  k_kept_check / "
             f"k_keep_count: {t_check / t_count:.2f};  check + samples: {(t_check + t_samples) * 1e3:.1f} us of the "
             f"{t['lh_kept_load_device'] * 1e3:.1f} us of lh_kept_load_device")
    rep.note(f"# {M} names: old save / lh_kept_save (pinned): {t['old save'] / t['lh_kept_save, pinned host memory']:.2f} x;  "
             f"old load / lh_kept_load (pinned): {t['old load'] / t['lh_kept_load, pinned host memory']:.2f} x")
    print("\n".join(rep.lines[-2:]), flush=True)
    k.close()
    eng.close()
    del dev
    torch.cuda.empty_cache()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="1024,65536")
    ap.add_argument("--pairs", default="2e6,2e7")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_store.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs)
    torch.cuda.set_device(0)
    rep = kit.Report(width=100, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, one interval; us are medians (min .. max) of the timed calls;",
                  "# saves and loads: wall time (complete on return); the kernels alone: HIP events around each"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
