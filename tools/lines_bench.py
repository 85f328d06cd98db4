"""What lh_lines* costs against lh_serialize (K6), same process, same engine, same snapshot, same box -- and what
Snapshot.spread_lines costs against the same text built on the host from Snapshot.spread.

S = a snapshot of --names interned names with lognormal pairs, accumulated once (so that lh_serialize emits its 15 keys per
name: _count, _sum, _avg, the nine default percentiles, _agg_avg, _agg_count, _agg_sum).  lh_lines is handed the same 15
values per name as device columns (count as uint64, sum, avg, the nine percentile values as strided
float64 columns, the lifetime stores as uint64) and its text is compared with lh_serialize's BYTE FOR BYTE before any time is
reported: the same lines, the same bytes.  Each is timed two ways:
  device   HIP events on the snapshot's stream around the call.  For lh_lines_device that is the descriptor copy and the three
           kernels.  lh_serialize has no device form: the span holds everything it enqueues (its extract, K6's three kernels
           and the copy of the text to the host); the extract alone (lh_extract_rows_view over the same names and percentiles)
           is reported beside it so that it can be told apart.
  wall     the host form, the copy of the text included.
Medians of --reps calls after --warmup, with the spread (min .. max).  No number is fixed in advance.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started on
the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/lines_bench.py [--names 65536] [--pairs 2e7] [--reps 25] [--warmup 5] [--out profiles/lines.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchkit as kit  # noqa: E402
import loghisto_amd  # noqa: E402
import oracle  # noqa: E402

PCT = dict(oracle.DEFAULT_PERCENTILES)                       # metrics.go:145-155
TOOL = "lines_bench"
WIRE = dict(prefix="cockroach.box-1_a.", sep=" ", suffix=" 1411104988\n", underscore_to_dot=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", type=int, default=65536)
    ap.add_argument("--pairs", type=float, default=2e7)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lines.txt"))
    a = ap.parse_args()
    M, n = a.names, int(a.pairs)
    torch.cuda.set_device(0)
    rep = kit.Report(width=84)
    rep.lines += [*kit.header(TOOL, f"--names {M} --pairs {n:g} --reps {a.reps} --warmup {a.warmup}", torch),
                  "# us are medians (min .. max) of the timed calls; device: HIP events on the snapshot's stream around the call; wall: "
                  "the host form, text copied to the host"]

    def row(name, ts, nlines=0, nbytes=0):               # (its own columns: ts in us, lines/us and GB/s)
        m, lo, hi = kit.med(ts)
        rate = f"   {nlines / m:8.1f} lines/us {nbytes / m / 1e3:7.2f} GB/s" if nlines else ""
        rep.note(f"{name:<84} us {m:10.1f} ({lo:.1f} .. {hi:.1f}){rate}", echo=True)
        return m

    with kit.limit(240, "ingest", TOOL):
        rng = np.random.default_rng(30)
        ids = torch.from_numpy(rng.integers(0, M, n).astype(np.int32)).cuda()
        vals = torch.from_numpy(rng.lognormal(11.5, 1.0, n)).cuda()
        eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=2, num_lanes=1, lane_samples=1 << 16)
        for i in range(M):
            eng.intern(f"svc_{i:05d}.rpc_latency")
        names = eng.device_names()
        eng.submit_pairs_device(ids, vals, n)
        snap = eng.flip()
        snap.accumulate()
        torch.cuda.synchronize()
    xs = torch.cuda.ExternalStream(snap.stream())

    def device_span(what, call):                          # (not benchkit.timed_events: us, and it waits for the closing event alone)
        ts = []
        with kit.limit(300, what, TOOL):
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(xs)
                call()
                e1.record(xs)
                e1.synchronize()
                if r >= a.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e3)
        return ts

    def wall(what, call, reps=a.reps, warmup=a.warmup):   # (not benchkit.timed_wall: us, as this tool's rows take them)
        ts, out = [], None
        with kit.limit(600, what, TOOL):
            for r in range(warmup + reps):
                t0 = time.perf_counter()
                out = call()
                if r >= warmup:
                    ts.append((time.perf_counter() - t0) * 1e6)
        return ts, out

    # ---- the yardstick: lh_serialize, 15 keys a name
    ps = [PCT[k] for k in PCT]
    serialize = lambda: snap.serialize(PCT, aggregates=True, **WIRE)       # noqa: E731
    text = serialize()
    nl, nb = text.count(b"\n"), len(text)
    rep.note(f"# S: {M} names, {n:g} samples; {nl} lines, {nb} bytes ({nb / nl:.1f} a line), the same for both")
    t_ser_dev = row("lh_serialize, 15 keys: device span (extract + K6 + text copy)", device_span("serialize span", serialize), nl, nb)
    t_ext_dev = row("  of which lh_extract_rows_view alone (same names, same percentiles)",
                    device_span("extract span", lambda: snap.extract_view(ps, M)))
    t_ser_wall = row("lh_serialize, 15 keys: host form, wall", wall("serialize wall", serialize)[0], nl, nb)

    # ---- lh_lines over the same 15 values a name, as device columns
    with kit.limit(120, "columns", TOOL):
        st = snap.extract(ps, M)
        lc, ls = eng.lifetime(M)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        count, total, pvals = up(st["count"].view(np.int64)), up(st["sum"]), up(st["pvals"])
        pvalid = up(st["pvalid"])
        d_lc, d_ls = up(lc.view(np.int64)), up(ls.view(np.int64))
        d_avg = up((ls // np.maximum(lc, 1)).view(np.int64))              # _agg_avg is an INTEGER division (metrics.go:603)
        cols = [dict(label="%s_count", a=count), dict(label="%s_sum", a=total), dict(label="%s_avg", a=up(st["avg"]))]
        cols += [dict(label=k, a=pvals[:, i], valid=pvalid[:, i]) for i, k in enumerate(PCT)]
        cols += [dict(label="%s_agg_avg", a=d_avg), dict(label="%s_agg_count", a=d_lc), dict(label="%s_agg_sum", a=d_ls)]
        d_text = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
    host_form = lambda: names.lines(cols, row_count=count, stream=snap.stream(), **WIRE)                          # noqa: E731
    device_form = lambda: names.lines(cols, row_count=count, stream=snap.stream(), out=(d_text, d_len), **WIRE)   # noqa: E731
    got = host_form()
    assert got == text, "lh_lines and lh_serialize differ"
    device_form()
    torch.cuda.synchronize()
    assert int(d_len.item()) == nb and bytes(d_text[:nb].cpu().numpy()) == text
    t_lin_dev = row("lh_lines_device, 15 columns: device span (descriptor copy + 3 kernels)", device_span("lines span", device_form),
                    nl, nb)
    t_lin_wall = row("lh_lines, 15 columns: host form, wall", wall("lines wall", host_form)[0], nl, nb)
    rep.note(f"# per output byte, lh_lines / lh_serialize: device span {t_lin_dev / t_ser_dev:.4f} x "
             f"({t_lin_dev / max(t_ser_dev - t_ext_dev, 1e-9):.4f} x with the extract's own span taken off lh_serialize's), "
             f"wall {t_lin_wall / t_ser_wall:.2f} x  (equal bytes: the ratio of the times)")

    # ---- the case the feature exists for: statsd's keys for every name
    tags = ["%.10g" % (100.0 * p) for p in ps]

    def on_the_host():
        h = snap.spread(ps)
        out = []
        for m in np.nonzero(h["count"])[0]:
            key = f"svc.{m:05d}.rpc.latency"
            out.append(f"{WIRE['prefix']}{key}.std{WIRE['sep']}{h['std'][m]:f}{WIRE['suffix']}")
            for i, tag in enumerate(tags):
                if h["pvalid"][m, i]:
                    tg = tag.replace("_", ".")
                    for what, v in (("mean", h["mean_le"][m, i]), ("upper", h["upper"][m, i]), ("count", float(h["count_le"][m, i])),
                                    ("sum", h["sum_le"][m, i])):
                        out.append(f"{WIRE['prefix']}{key}.{what}.{tg}{WIRE['sep']}{v:f}{WIRE['suffix']}")
        return "".join(out).encode()

    on_device = lambda: snap.spread_lines(names, ps, **WIRE)       # noqa: E731
    stext = on_device()
    sl, sb = stext.count(b"\n"), len(stext)
    rep.note(f"# spread_lines: {M} names x (std + 4 keys x {len(ps)} percentiles): {sl} lines, {sb} bytes")
    ts, htext = wall("spread on the host", on_the_host, reps=3, warmup=1)
    same = htext == stext      # (Python's %f rounds the exact value half-even as Go's does; reported, not assumed)
    t_host = row("Snapshot.spread + one Python format per key, wall (3 calls)", ts, sl, sb)
    t_dev = row("Snapshot.spread_lines (lh_spread_device + lh_lines), wall", wall("spread_lines", on_device)[0], sl, sb)
    rep.note(f"# spread_lines: host route / device route = {t_host / t_dev:.0f} x; the two texts are "
             f"{'equal byte for byte' if same else 'NOT equal'}")
    assert same, "spread_lines and the host's text differ"

    snap.release()
    names.close()
    eng.close()
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
