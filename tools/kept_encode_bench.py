"""What the compact blob of a kept interval saves and costs (lh_kept_encode*, lh_kept_decode*), against the verbatim route
(lh_kept_save*, lh_kept_load*) measured in the same run -- same box, same process, same interval.

Per name count: one interval of one engine of 32-bit cells (tools/kept_bench.py's stream: Zipf names, lognormal values) is
flipped and kept.  Reported:
  the sizes: encoded bytes against verbatim bytes and bytes per cell, and how the rows split over count widths and key modes;
  lh_kept_encode_device against lh_kept_save_device, lh_kept_encode against lh_kept_save into pinned host memory (wall: each
  is complete on return);
  lh_kept_decode_device against lh_kept_load_device, lh_kept_decode against lh_kept_load from pinned host memory (wall; the
  handle each makes is closed untimed);
  each kernel alone (HIP events, lh_tool_kept_encode_ms / lh_tool_kept_decode_ms): k_enc_size, the scan, k_enc_fill; k_dec_dir,
  the two scans, k_dec_fill, k_kept_check_samples.
Medians of the timed calls with the spread (min .. max).  Nothing is tuned and no number is fixed in advance.  Before anything is
written the encoded blob is compared byte for byte between the forms and with loghisto_amd.keptfile.encode of the verbatim
blob, and every decoded handle's verbatim blob with the original's.

One process; every step runs under a limit of its own (tools/benchkit.py's alarm, which ends the process: nothing is started
on the GPU after a step that hung), and the first failed check ends the run.
usage: python tools/kept_encode_bench.py [--names 1024,65536] [--pairs 2e6,2e7] [--reps 15] [--out profiles/kept_encode.txt]"""
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

TOOL = "kept_encode_bench"


def run(torch, a, M, n, rep):
    L = N.lib()
    row = rep.row

    eng = loghisto_amd.Engine(device=0, max_metrics=M, num_buffers=3, num_lanes=1, lane_samples=1 << 16, cell_bits=32)
    with kit.limit(600, "ingest and keep", TOOL):
        ids = bench.zipf_ids(n, M, 4000)
        data = bench.make_samples(n, "lognormal", seed=40)
        eng.submit_pairs_device(ids, data, n)
        snap = eng.flip()
        k = snap.keep(M)
        snap.release()
        del ids, data
        torch.cuda.empty_cache()
    assert k.info["samples"] == n and k.info["nrows"] == M
    cells, size = k.info["cells"], 64 + k.info["bytes"]
    blob = k.to_bytes()
    with kit.limit(600, "the reference encoding", TOOL):
        want = keptfile.encode(blob)
    esize = k.encoded_size()
    assert esize == len(want) <= keptfile.encoded_bound(M, cells) <= size
    desc = np.frombuffer(want, dtype="<u4", count=M, offset=64)
    filled = (desc & 0x1ffff) > 0
    widths = [int((((desc >> 20 & 3) == w) & filled).sum()) for w in range(4)]
    rep.note(f"# {M} names, {cells} cells ({cells / M:.1f} a name), {n} samples: verbatim {size} B ({size / 2**20:.2f} MiB), encoded "
             f"{esize} B ({esize / 2**20:.2f} MiB): {size / esize:.2f} x smaller;  {size / max(cells, 1):.2f} -> "
             f"{esize / max(cells, 1):.2f} B a cell", echo=True)
    rep.note(f"# {M} names: rows with 1- / 2- / 4- / 8-byte counts: {widths[0]} / {widths[1]} / {widths[2]} / {widths[3]};  rows in raw "
             f"key mode: {int((desc >> 24 & 1).sum())};  rows without a cell: {int(((desc & 0x1ffff) == 0).sum())}", echo=True)

    # ---- each kernel alone
    fp = C.c_float
    with kit.limit(180, "the encoder's kernels", TOOL):
        ts = [[], [], []]
        for r in range(a.warmup + a.reps):
            ms = [fp(0), fp(0), fp(0)]
            N.check(L.lh_tool_kept_encode_ms(k._h, None, *[C.byref(x) for x in ms]), "lh_tool_kept_encode_ms")
            if r >= a.warmup:
                for t, x in zip(ts, ms):
                    t.append(x.value)
    t_size = row(f"k_enc_size alone (events), {M} names, {cells} cells", ts[0])
    row(f"k_keep_scan of S alone (events), {M} names", ts[1])
    t_fill = row(f"k_enc_fill alone (events), {M} names", ts[2])
    dev_enc = k.encode_device()
    assert dev_enc.cpu().numpy().tobytes() == want
    with kit.limit(180, "the decoder's kernels", TOOL):
        ts = [[], [], [], []]
        for r in range(a.warmup + a.reps):
            ms = [fp(0), fp(0), fp(0), fp(0)]
            N.check(L.lh_tool_kept_decode_ms(0, int(dev_enc.data_ptr()), esize, None, *[C.byref(x) for x in ms]), "lh_tool_kept_decode_ms")
            if r >= a.warmup:
                for t, x in zip(ts, ms):
                    t.append(x.value)
    row(f"k_dec_dir alone (events), {M} names", ts[0])
    row(f"k_keep_scan twice (events), {M} names", ts[1])
    t_dfill = row(f"k_dec_fill alone (events), {M} names, {cells} cells", ts[2])
    row(f"k_kept_check_samples behind it (events), {M} names", ts[3])

    def wall(what, call, after=None):
        return kit.timed_wall(call, a.reps, a.warmup, what, 420, TOOL, None, after, sync=torch.cuda.synchronize)

    # ---- encode against save
    pinned_v = torch.zeros(size, dtype=torch.uint8, pin_memory=True).numpy()
    pinned_e = torch.full((esize,), 0xff, dtype=torch.uint8, pin_memory=True).numpy()
    dev_v = torch.zeros(size, dtype=torch.uint8, device="cuda")
    dev_e = torch.full((esize,), 0xff, dtype=torch.uint8, device="cuda")
    t = {}
    for what, fn, buf, cap in (("lh_kept_save_device", L.lh_kept_save_device, int(dev_v.data_ptr()), size),
                               ("lh_kept_encode_device", L.lh_kept_encode_device, int(dev_e.data_ptr()), esize),
                               ("lh_kept_save, pinned host memory", L.lh_kept_save, pinned_v.ctypes.data, size),
                               ("lh_kept_encode, pinned host memory", L.lh_kept_encode, pinned_e.ctypes.data, esize)):
        ts, _ = wall(what, lambda fn=fn, buf=buf, cap=cap: N.check(fn(k._h, buf, cap, None, None), what))
        t[what] = row(f"{what} (wall), {M} names, {cap / 2**20:.2f} MiB", ts)
    assert pinned_v.tobytes() == blob and dev_v.cpu().numpy().tobytes() == blob
    assert pinned_e.tobytes() == want and dev_e.cpu().numpy().tobytes() == want

    # ---- decode against load
    def closing(_, new):
        assert new.info == k.info
        got = new.to_bytes()
        new.close()
        return got

    def loader(fn, addr, length):
        def call():
            h = C.c_void_p(0)
            N.check(fn(0, addr, length, 0, None, None, C.byref(h)), "load")
            return loghisto_amd.Kept(h, None)
        return call

    for what, fn, buf, length in (("lh_kept_load_device", L.lh_kept_load_device, int(dev_v.data_ptr()), size),
                                  ("lh_kept_decode_device", L.lh_kept_decode_device, int(dev_e.data_ptr()), esize),
                                  ("lh_kept_load, pinned host memory", L.lh_kept_load, pinned_v.ctypes.data, size),
                                  ("lh_kept_decode, pinned host memory", L.lh_kept_decode, pinned_e.ctypes.data, esize)):
        ts, got = wall(what, loader(fn, buf, length), after=closing)
        assert got == blob, what
        t[what] = row(f"{what} (wall), {M} names, {length / 2**20:.2f} MiB", ts)

    def against(new, old):
        r = t[old] / t[new]
        return f"{t[new] * 1e3:.1f} us against {t[old] * 1e3:.1f} us: {r:.2f} x faster" if r >= 1 else \
            f"{t[new] * 1e3:.1f} us against {t[old] * 1e3:.1f} us: {1 / r:.2f} x SLOWER"

    rep.note(f"# {M} names: pinned encode against pinned save: {against('lh_kept_encode, pinned host memory', 'lh_kept_save, pinned host memory')};  "
             f"device encode against device save: {against('lh_kept_encode_device', 'lh_kept_save_device')}", echo=True)
    rep.note(f"# {M} names: pinned decode against pinned load: {against('lh_kept_decode, pinned host memory', 'lh_kept_load, pinned host memory')};  "
             f"device decode against device load: {against('lh_kept_decode_device', 'lh_kept_load_device')}", echo=True)
    moved = 10 * cells + 16 * M + esize
    rep.note(f"# {M} names: k_enc_size reads {(10 * cells + 16 * M) / 2**20:.2f} MiB: {(10 * cells + 16 * M) / (t_size * 1e-3) / 1e9:.1f} GB/s;  "
             f"k_enc_fill moves {moved / 2**20:.2f} MiB: {moved / (t_fill * 1e-3) / 1e9:.1f} GB/s;  k_dec_fill moves {moved / 2**20:.2f} MiB: "
             f"{moved / (t_dfill * 1e-3) / 1e9:.1f} GB/s", echo=True)
    k.close()
    eng.close()
    del dev_v, dev_e, dev_enc
    torch.cuda.empty_cache()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--names", default="1024,65536")
    ap.add_argument("--pairs", default="2e6,2e7")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kept_encode.txt"))
    a = ap.parse_args()
    names, pairs = [int(x) for x in a.names.split(",")], [int(float(x)) for x in a.pairs.split(",")]
    assert len(names) == len(pairs)
    torch.cuda.set_device(0)
    rep = kit.Report(width=100, digits=11)
    stamp, command = kit.header(TOOL, f"--names {a.names} --pairs {a.pairs} --reps {a.reps} --warmup {a.warmup}", torch)
    rep.lines += [command, stamp,
                  "# Zipf(1.0) names, lognormal values, one interval; us are medians (min .. max) of the timed calls;",
                  "# encodes, saves, decodes and loads: wall time (complete on return); the kernels alone: HIP events around each"]
    for M, n in zip(names, pairs):
        run(torch, a, M, n, rep)
    rep.write(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
