"""What adding an interval as CELLS costs (lh_snapshot_add_buckets*) against re-ingesting its SAMPLES, same box, same run.

S = the cells of BASELINE config 4's one-rank slice (65 536 Zipf names, 1.25e8 lognormal pairs: bench.py's stream), taken
with buckets_all.  Reported: cells in S, bytes in, HIP-event time on the snapshot's stream and cells/s for the CSR device
form and the COO device form (K = 1, and S eight times over: the duplicate-heavy fleet case), wall time of the two host
forms; beside them (a) submit_pairs_device of the pairs that produced S and (b) buckets_all of S, both unchanged code paths.
Medians of --reps calls after --warmup, with the spread (min .. max).  THE timing condition: CSR device, K = 1, takes less
device time than (a).

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is
started on the GPU after a step that hung).
usage: python tools/import_bench.py [--names 65536] [--pairs 1.25e8] [--reps 25] [--warmup 5] [--out profiles/import_cells.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
from benchkit import limit, med  # noqa: E402

TOOL = "import_bench"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=1.25e8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "import_cells.txt"))
    a = ap.parse_args()
    M, n = a.names, int(a.pairs)
    torch.cuda.set_device(0)
    rep = kit.Report(width=34)
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# S = cells of config 4's one-rank slice (Zipf(1.0) names, lognormal values: bench.py's stream); ms are medians "
                  "(min .. max) of the timed calls;", "# device forms: HIP events on the snapshot's stream around the call "
                  "(validation pre-pass, its read-back and the add); host forms and buckets_all: wall time"]

    def row(name, cells, nbytes, ts, extra=""):           # (its own columns: cells, bytes in, ms and cells/s)
        m, lo, hi = med(ts)
        rep.note(f"{name:<34} cells {cells:>11,d}  bytes in {nbytes:>13,d}  ms {m:8.3f} ({lo:.3f} .. {hi:.3f})  "
                 f"{cells / (m * 1e-3):.3e} cells/s{extra}", echo=True)

    bi, bd, _ = kit.c4_inputs(M, n, TOOL)
    ids, data = bi.tensor, bd.tensor
    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
    stream = torch.cuda.Stream()

    # (a) the parent's path: the samples through submit_pairs_device; the last interval becomes S
    with limit(240, "submit_pairs_device", TOOL):
        ts = []
        S = None
        for r in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.submit_pairs_device(ids, data, n, stream=stream)
            e1.record(stream)
            snap = eng.flip()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ts.append(e0.elapsed_time(e1))
            if r == a.warmup + a.reps - 1:
                tb = []
                for _ in range(max(3, a.host_reps)):                         # (b) buckets_all of S
                    t0 = time.perf_counter()
                    S = snap.buckets_all(M)
                    tb.append((time.perf_counter() - t0) * 1e3)
            snap.release()
        ingest_ms = med(ts)
    offsets, keys, counts = S
    cells = int(keys.size)
    assert int(counts.sum()) == n and int(offsets[-1]) == cells
    row("(a) submit_pairs_device, samples", n, n * 12, ts, "  [pairs, not cells]")
    row("(b) buckets_all of S (host arrays)", cells, 0, tb)
    bi.free()
    bd.free()
    del ids, data
    torch.cuda.empty_cache()

    def dev(x):
        x = np.ascontiguousarray(x)
        x = x.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(x.dtype, x.dtype))
        return torch.from_numpy(x).cuda()

    coo_ids = np.repeat(np.arange(M, dtype=np.uint32), np.diff(offsets.astype(np.int64)))
    d_off, d_keys, d_counts, d_ids = dev(offsets), dev(keys), dev(counts), dev(coo_ids)
    K = 8
    d_ids8, d_keys8, d_counts8 = d_ids.repeat(K), d_keys.repeat(K), d_counts.repeat(K)    # S eight times over, source-major
    torch.cuda.synchronize()

    def timed_adds(what, call, reps, warmup, times_s):
        """Every call adds into ONE empty snapshot: the first (untimed) call moves it to its wide store.  (Not
        benchkit.timed_events: the step takes and checks the snapshot too, and the first call's own time is reported.)"""
        with limit(240, what, TOOL):
            snap = eng.flip()
            xs = torch.cuda.ExternalStream(snap.stream())
            ts, first = [], None
            for r in range(warmup + reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(xs)
                call(snap)
                e1.record(xs)
                xs.synchronize()
                if r == 0:
                    first = e0.elapsed_time(e1)
                if r >= warmup:
                    ts.append(e0.elapsed_time(e1))
            got = snap.extract([0.5], M)["count"]
            assert int(got.sum()) == n * times_s * (warmup + reps), what     # every call went in, whole
            snap.release()
            torch.cuda.synchronize()
        return ts, first

    ts_csr, first_csr = timed_adds("csr device", lambda s: s.add_buckets_csr(d_off, d_keys, d_counts), a.reps, a.warmup, 1)
    row("CSR device, K = 1", cells, cells * 10 + (M + 1) * 8, ts_csr, f"  first call on the narrow snapshot {first_csr:.3f} ms")
    ts_coo, _ = timed_adds("coo device", lambda s: s.add_buckets(d_ids, d_keys, d_counts), a.reps, a.warmup, 1)
    row("COO device, K = 1", cells, cells * 14, ts_coo)
    ts_coo8, _ = timed_adds("coo device x8", lambda s: s.add_buckets(d_ids8, d_keys8, d_counts8), a.reps, a.warmup, K)
    row("COO device, K = 8 (S eight times)", cells * K, cells * K * 14, ts_coo8)

    def timed_host(what, call):                             # (not benchkit.timed_wall: the step takes and checks the snapshot too)
        with limit(240, what, TOOL):
            snap = eng.flip()
            ts = []
            for r in range(1 + a.host_reps):
                t0 = time.perf_counter()
                call(snap)
                if r:
                    ts.append((time.perf_counter() - t0) * 1e3)
            assert int(snap.extract([0.5], M)["count"].sum()) == n * (1 + a.host_reps), what
            snap.release()
        return ts

    row("CSR host arrays (wall)", cells, cells * 10 + (M + 1) * 8, timed_host("csr host", lambda s: s.add_buckets_csr(offsets, keys, counts)))
    row("COO host arrays (wall)", cells, cells * 14, timed_host("coo host", lambda s: s.add_buckets(coo_ids, keys, counts)))
    eng.close()

    c, lo, hi = med(ts_csr)
    k1, k8 = med(ts_coo)[0], med(ts_coo8)[0]
    ok = hi < ingest_ms[1]                      # beyond the run-to-run spread: the slowest import against the fastest ingest
    rep.note(f"# condition: CSR device K = 1 ({c:.3f} ms, max {hi:.3f}) < submit_pairs_device of the same interval "
             f"({ingest_ms[0]:.3f} ms, min {ingest_ms[1]:.3f}): {'MET' if c < ingest_ms[0] else 'NOT MET'}"
             f"{' (also max < min)' if ok else ''}; ratio {ingest_ms[0] / c:.2f} x")
    rep.note(f"# CSR device / buckets_all wall: {c / med(tb)[0]:.3f};  COO K = 8 / K = 1: {k8 / k1:.2f} x "
             f"({'more' if k8 > 8 * k1 else 'not more'} than 8 x)")
    print("\n".join(rep.lines[-2:]), flush=True)
    rep.write(a.out)
    return 0 if c < ingest_ms[0] else 1


if __name__ == "__main__":
    sys.exit(main())
