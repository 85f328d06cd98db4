"""What the reader bench tools (tools/*_bench.py) share: the per-step alarm, the "median (min .. max)" row, the two timing
loops, config 4's one-rank slice, the one-name full-span snapshot, the loop over a unit's two kernel shapes and the writer.
Plain functions and one small class; a tool stays a script that reads top to bottom and keeps its own comparisons,
assertions and output lines.  A new reader's tool starts here.  tests/test_benchkit.py holds the CPU part to its text."""
import contextlib
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("wave", 1), ("workgroup", 1 << 30))              # a unit's switch value that gives every row a wave / a workgroup


@contextlib.contextmanager
def limit(seconds, what, tool):
    """One step under an alarm of its own that ENDS the process (status 124): nothing is started on the GPU after a step
    that hung."""
    def expired(*_):
        sys.stderr.write(f"{tool}: step '{what}' passed its limit of {seconds} s; ending\n")
        sys.stderr.flush()
        os._exit(124)
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def med(ts):
    return statistics.median(ts), min(ts), max(ts)


class Report:
    """The lines of a tool's output file.  width and digits are the tool's own label width and median field."""

    def __init__(self, width, digits=10):
        self.lines, self.width, self.digits = [], width, digits

    def note(self, text, echo=False):
        self.lines.append(text)
        if echo:
            print(text, flush=True)

    def row(self, name, ts, extra="", width=None, digits=None):
        """ts in ms -> 'name  us median (min .. max)extra', on file and on the screen; returns the median (ms)"""
        m, lo, hi = med(ts)
        width, digits = self.width if width is None else width, self.digits if digits is None else digits
        self.note(f"{name:<{width}} us {m * 1e3:{digits}.1f} ({lo * 1e3:.1f} .. {hi * 1e3:.1f}){extra}", echo=True)
        return m

    def write(self, out, mark=None):
        """With mark, what the file holds above its first line starting with mark stays (a compile-time resource table)."""
        head = []
        if mark is not None and os.path.exists(out):
            with open(out) as f:
                for ln in f.read().splitlines():
                    if ln.startswith(mark):
                        break
                    head.append(ln)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(head + self.lines) + "\n")


def header(tool, argv_text, torch):
    """-> the stamp line, the command and device line"""
    import bench
    return f"# tree_stamp: {bench.tree_stamp()}", f"# tools/{tool}.py {argv_text}: {torch.cuda.get_device_name(0)}"


def timed_events(stream, call, reps, warmup, what, seconds, tool, calls=1, wall=False):
    """ms between two HIP events on `stream` around `calls` calls, per call, for each of reps runs after warmup.
    wall=True: -> (ts, ms the calling thread spent inside each timed call)."""
    import torch
    with limit(seconds, what, tool):
        torch.cuda.synchronize()
        ts, inside = [], []
        for r in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter() if wall else 0.0
            for _ in range(calls):
                call()
            t1 = time.perf_counter() if wall else 0.0
            e1.record(stream)
            stream.synchronize()
            if r >= warmup:
                ts.append(e0.elapsed_time(e1) / calls)
                inside.append((t1 - t0) * 1e3)
    return (ts, inside) if wall else ts


def timed_wall(call, reps, warmup, what, seconds, tool, before=None, after=None, sync=None):
    """Wall ms of each of reps calls after warmup -> (ts, the last call's result).  before() runs untimed and its result
    is handed to call; sync() runs just before the clock starts; after(ctx, result) runs untimed and returns the result."""
    with limit(seconds, what, tool):
        ts, out = [], None
        for r in range(warmup + reps):
            ctx = before() if before else None
            if sync:
                sync()
            t0 = time.perf_counter()
            out = call(ctx) if before else call()
            dt = (time.perf_counter() - t0) * 1e3
            if after:
                out = after(ctx, out)
            if r >= warmup:
                ts.append(dt)
    return ts, out


def c4_inputs(M, n, tool, look=None):
    """BASELINE config 4's one-rank stream (bench.py's) in hipMalloc'ed memory -> (ids, values, look(values)): look sees
    torch's own tensor of values before it is dropped."""
    import bench
    import torch
    with limit(240, "inputs", tool):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        data.mul_(torch.exp(3e-5 * ids.to(torch.float64)))
        seen = look(data) if look else None
        bi, bd = bench.OwnBuffer(ids), bench.OwnBuffer(data)
        del ids, data
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
    return bi, bd, seen


def c4_slice(M, n, tool, look=None):
    """-> (engine, the snapshot of config 4's one-rank slice, look(values)); the inputs are freed.  The caller releases
    the snapshot and closes the engine."""
    import loghisto_amd
    import torch
    bi, bd, seen = c4_inputs(M, n, tool, look)
    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
    with limit(240, "ingest", tool):
        eng.submit_pairs_device(bi.tensor, bd.tensor, n)
        snap = eng.flip()
        torch.cuda.synchronize()
    bi.free()
    bd.free()
    torch.cuda.empty_cache()
    return eng, snap, seen


def full_row_snapshot(tool):
    """-> (engine of one name, its snapshot with all 65 536 cells occupied, 3 each: 64-bit cells, 512 KiB)"""
    import loghisto_amd
    import numpy as np
    with limit(120, "one full row", tool):
        one = loghisto_amd.Engine(device=0, max_metrics=1, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
        snap = one.flip()
        keys = np.arange(-32768, 32768, dtype=np.int16)
        snap.add_buckets(np.zeros(keys.size, dtype=np.uint32), keys, np.full(keys.size, 3, dtype=np.uint64))
    return one, snap


def shapes(switch, pairs=SHAPES):
    """Yields each (shape, wave_from) with the unit's switch (lh_tool_*_switch) set to it; the default is back afterwards."""
    import ctypes as C
    prev = C.c_uint32(0)
    for shape, wave_from in pairs:
        assert switch(wave_from, C.byref(prev)) == 0
        yield shape, wave_from
    assert switch(0, C.byref(prev)) == 0
