"""lh_kept_save* / lh_kept_load* / lh_kept_values (Kept.to_bytes, save, to_device_blob, from_bytes, load, from_device_blob):
kept intervals saved and loaded, the block checked on the device before a handle exists.

The rows are crafted through add_buckets on a 12-name engine: an empty row, a one-cell row, rows of 63, 64, 65 and 129 cells
(the check's wave-step edges), cells at bin 0 and bin 65 535, a row whose first key lies below the previous row's last, two
cells whose counts sum past 2^64, a block with no cell at all and a handle with first > 0.  What a load refuses is held to
loghisto_amd.keptfile.check, the NumPy restatement of the rules, never to constants copied from the kernel."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from loghisto_amd import _native as N
from loghisto_amd import keptfile as KF
from tests.test_gpu_count_le import engine
from tests.test_kept_store_abi import mutate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NK = 65536
P = [0.0, 0.5, 0.99, 1.0]
BOUNDS = [-1.0, 0.0, 3.5, 1e3, 1e9, float("inf")]


def crafted_rows():
    def run(n, start, step=3):
        return {start + step * i: 1 + (i % 5) for i in range(n)}

    rng = np.random.default_rng(7)
    bins = np.unique(rng.normal(33000, 80, 300).astype(np.int64))
    return [
        {},                                                # 0  empty (never marked)
        {500: 7},                                          # 1  one cell
        run(63, 1000),                                     # 2
        run(64, 2000),                                     # 3
        run(65, 3000),                                     # 4
        run(129, 40000, 5),                                # 5
        {0: 5, NK - 1: 6},                                 # 6  bin 0 and bin 65 535
        {10: 1, 20: 2},                                    # 7  its first key lies below row 6's last
        {100: 1 << 63, 200: (1 << 63) + 5},                # 8  row_count wraps to 5
        {int(b): int(c) for b, c in zip(bins, rng.integers(1, 1000, bins.size))},   # 9
        {},                                                # 10
        {NK - 1: 1},                                       # 11
    ]


def host(t):
    a = t.cpu().numpy()
    return a.view(U64) if a.dtype == np.int64 else a


def arrays_of(k):
    return [host(t) for t in k.arrays()]


def same_handle(a, b, what=""):
    """info equal, the four arrays bit-equal"""
    assert a.info == b.info, (what, a.info, b.info)
    for x, y in zip(arrays_of(a), arrays_of(b)):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


def packed(k):
    off, keys, counts, _ = arrays_of(k)
    return KF.pack(off, keys, counts, first=k.info["first"])


@pytest.fixture(scope="module")
def store(native_lib, torch_cuda):
    import loghisto_amd
    rows = crafted_rows()
    M = len(rows)
    ids = np.concatenate([np.full(len(r), m, dtype=np.uint32) for m, r in enumerate(rows)])
    bins = np.concatenate([np.array(sorted(r), dtype=np.int64) for r in rows])
    counts = np.concatenate([np.array([r[b] for b in sorted(r)], dtype=U64) for r in rows])
    keys = (bins.astype(np.uint16) ^ np.uint16(0x8000)).view(np.int16)
    with engine(M, cell_bits=64) as e:
        _, D = e.codec_tables()
        with e.flip() as s:
            s.add_buckets(ids, keys, counts)
            kept = dict(all=s.keep(M), part=s.keep(6, 3), empty=s.keep(1, 0), tail=s.keep(2, 10))
    # the engine is gone from here on: every load below happens without one
    blobs = {name: k.to_bytes() for name, k in kept.items()}
    yield types.SimpleNamespace(rows=rows, M=M, kept=kept, blobs=blobs, D=D, torch=torch_cuda, Kept=loghisto_amd.Kept)
    for k in kept.values():
        k.close()


def test_the_fixture_holds_the_rows_it_was_made_for(store):
    off, keys, counts, row_count = arrays_of(store.kept["all"])
    assert np.diff(off.astype(np.int64)).tolist() == [len(r) for r in store.rows]
    assert [len(r) for r in store.rows][:6] == [0, 1, 63, 64, 65, 129]
    b = (keys.view(np.uint16) ^ np.uint16(0x8000)).astype(np.int64)
    assert b[int(off[6])] == 0 and b[int(off[7]) - 1] == NK - 1 and b[int(off[7])] < b[int(off[7]) - 1]
    assert int(row_count[8]) == 5 and int(counts[int(off[8])]) + int(counts[int(off[8]) + 1]) == (1 << 64) + 5
    assert store.kept["empty"].info["cells"] == 0 and store.kept["part"].info["first"] == 3
    assert store.kept["empty"].info["bytes"] == 24 and len(store.blobs["empty"]) == KF.BLOB_MIN


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all", "part", "empty", "tail"])
def test_round_trip_host_and_device_forms(store, name):
    k, blob = store.kept[name], store.blobs[name]
    assert len(blob) == 64 + k.info["bytes"] and KF.check(blob) is None
    assert blob == packed(k)                                                      # the bytes are keptfile's
    u = KF.unpack(blob)
    assert {x: u[x] for x in ("first", "nrows", "cells", "samples", "bytes")} == {x: k.info[x] for x in
                                                                                   ("first", "nrows", "cells", "samples", "bytes")}
    with store.Kept.from_bytes(blob) as back:
        same_handle(k, back, name)
        assert back.to_bytes() == blob                                            # a second save: byte for byte
        assert bytes(back.to_device_blob().cpu().numpy()) == blob
    t = k.to_device_blob()
    assert t.dtype == store.torch.uint8 and t.is_cuda and bytes(t.cpu().numpy()) == blob
    with store.Kept.from_device_blob(t) as back:
        same_handle(k, back, name + " (device)")
        assert back.to_bytes() == blob
    # an unaligned device blob (what a collective's receive buffer may be), on a stream of the caller's
    st = store.torch.cuda.Stream()
    pad = store.torch.zeros(len(blob) + 3, dtype=store.torch.uint8, device="cuda")
    pad[3:] = t
    store.torch.cuda.synchronize()
    with store.Kept.from_device_blob(pad[3:], stream=st) as back:
        same_handle(k, back, name + " (device, odd address)")
        assert back.to_bytes(stream=st) == blob


def test_save_refuses_a_buffer_that_is_too_small(store):
    k, blob = store.kept["all"], store.blobs["all"]
    L = N.lib()
    n = C.c_size_t(0)
    assert L.lh_kept_save_size(k._h, C.byref(n)) == 0 and n.value == len(blob)
    buf = np.full(len(blob) + 8, 7, dtype=np.uint8)
    written = C.c_size_t(0x77)
    for cap in (KF.BLOB_MIN, len(blob) - 1):
        assert L.lh_kept_save(k._h, buf.ctypes.data, cap, None, C.byref(written)) == N.ERANGE
    d = store.torch.full((len(blob),), 7, dtype=store.torch.uint8, device="cuda")
    assert L.lh_kept_save_device(k._h, d.data_ptr(), len(blob) - 1, None, C.byref(written)) == N.ERANGE
    assert written.value == 0x77 and np.all(buf == 7) and bool((d == 7).all())     # nothing written
    assert L.lh_kept_save(k._h, buf.ctypes.data, len(blob) + 8, None, C.byref(written)) == 0
    assert written.value == len(blob) and bytes(buf[:len(blob)]) == blob and np.all(buf[len(blob):] == 7)
    assert L.lh_kept_save(k._h, buf.ctypes.data, len(blob), None, None) == 0      # written may be NULL


def test_save_and_load_through_a_file(store, tmp_path):
    k = store.kept["part"]
    path = tmp_path / "part.lhkept"
    k.save(path)
    assert path.read_bytes() == store.blobs["part"]
    with store.Kept.load(path) as back:
        same_handle(k, back)


# ---- 2. the readers take a loaded handle ---------------------------------------------------------------------------------------
def same_dict(a, b, what):
    assert set(a) == set(b), what
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (what, key)


def test_readers_on_a_loaded_handle_equal_the_original(store):
    k = store.kept["all"]
    with store.Kept.from_bytes(store.blobs["all"]) as back, store.Kept.from_device_blob(k.to_device_blob()) as dback:
        for b in (back, dback):
            same_dict(b.across([], P), k.across([], P), "across")
            same_dict(b.count_le(BOUNDS), k.count_le(BOUNDS), "count_le")
            same_dict(b.spread(P), k.spread(P), "spread")
            same_dict(b.across([], P, ids=[9, 1, 5]), k.across([], P, ids=[9, 1, 5]), "across_ids")
            c = b.compare(k)                                                      # lh_kept_compare(original, loaded)
            empty = np.array([not r for r in store.rows])
            assert np.array_equal(c["count_a"], c["count_b"]) and np.array_equal(c["count_a"] == 0, empty)
            for key in ("ks", "w1", "shift"):
                assert np.all(np.isnan(c[key][empty])) and np.all(c[key][~empty] == 0.0), key
            with b.merge() as m:                                                  # lh_kept_merge([loaded])
                same_handle(k, m, "merge of a loaded handle")
        # a list that mixes originals and loaded handles
        same_dict(k.across([back, dback], P), k.across([k, k], P), "mixed list")
        same_dict(back.spread(P, earlier=[k]), k.spread(P, earlier=[k]), "mixed list, spread")
        with k.merge([back]) as m, k.merge([k]) as want:
            same_handle(want, m, "mixed merge")
    # a loaded handle of a sub-block beside the whole
    with store.Kept.from_bytes(store.blobs["part"]) as part:
        same_dict(part.across([k], P, 6, 3), store.kept["part"].across([k], P, 6, 3), "sub-block")


def test_values_equal_the_engines_table(store):
    D = store.Kept.values(0)
    assert D.dtype == np.float64 and D.shape == (NK,) and D.tobytes() == store.D.tobytes()


# ---- 3. lifetime ---------------------------------------------------------------------------------------------------------------
def test_load_after_the_engine_is_closed_and_release_under_a_reader(native_lib, torch_cuda):
    import loghisto_amd
    rows = crafted_rows()
    M = len(rows)
    ids = np.concatenate([np.full(len(r), m, dtype=np.uint32) for m, r in enumerate(rows)])
    bins = np.concatenate([np.array(sorted(r), dtype=np.int64) for r in rows])
    counts = np.concatenate([np.array([r[b] for b in sorted(r)], dtype=U64) for r in rows])
    with engine(M, cell_bits=64) as e:
        with e.flip() as s:
            s.add_buckets(ids, (bins.astype(np.uint16) ^ np.uint16(0x8000)).view(np.int16), counts)
            with s.keep(M) as k:
                blob = k.to_bytes()
                want = k.across([], P)
    back = loghisto_amd.Kept.from_bytes(blob)                                     # engine, snapshot and original are gone
    same_dict(back.across([], P), want, "after the engine")
    # a device-form reader is enqueued, then the handle is released: the release waits for it
    t = torch_cuda
    out = dict(count=t.zeros(M, dtype=t.int64, device="cuda"), sum=t.zeros(M, dtype=t.float64, device="cuda"),
               pkeys=t.zeros((M, len(P)), dtype=t.int16, device="cuda"), pvalid=t.zeros((M, len(P)), dtype=t.uint8, device="cuda"))
    st = t.cuda.Stream()
    back.across([], P, out=out, stream=st)
    back.close()
    st.synchronize()
    assert np.array_equal(out["count"].cpu().numpy().view(U64), want["count"])
    assert out["sum"].cpu().numpy().tobytes() == want["sum"].tobytes()
    assert np.array_equal(out["pkeys"].cpu().numpy(), want["pkeys"]) and np.array_equal(out["pvalid"].cpu().numpy(), want["pvalid"])


def test_a_fresh_process_without_an_engine_reads_a_saved_interval(store, tmp_path):
    k = store.kept["all"]
    path = tmp_path / "all.lhkept"
    k.save(path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_kept_store_child.py"), str(path)] + [repr(p) for p in P],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert child["info"] == k.info
    want = k.across([], P)
    assert child["count"] == [int(x) for x in want["count"]]
    assert child["pkeys"] == want["pkeys"].tolist() and child["pvalid"] == want["pvalid"].tolist()
    D = store.Kept.values(0)                                                      # the parent's own way from pkeys to values
    mine = np.where(want["pvalid"] != 0, D[want["pkeys"].astype(np.int64) & 0xffff ^ 0x8000], np.nan)
    theirs = np.array([[float(v) for v in row] for row in child["pvals"]])
    assert theirs.tobytes() == mine.tobytes()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def load_raw(store, blob, form):
    """lh_kept_load / lh_kept_load_device on `blob` -> (status, (cause, row, index), *out)"""
    L = N.lib()
    why = N.LhKeptCheck(struct_size=16, cause=0x77, row=0x77, index=0x77)
    out = C.c_void_p(0x77)
    a = np.frombuffer(blob, dtype=np.uint8)
    if form == "host":
        rc = L.lh_kept_load(0, a.ctypes.data, a.size, 0, None, C.byref(why), C.byref(out))
    else:
        t = store.torch.from_numpy(a.copy()).cuda()
        rc = L.lh_kept_load_device(0, t.data_ptr(), a.size, 0, None, C.byref(why), C.byref(out))
    return rc, (why.cause, why.row, why.index), out


def held_to_the_reference(store, blob, what, forms=("host", "device")):
    """the load's answer for `blob` is keptfile.check's; a blob it takes round-trips; a valid load right afterwards succeeds"""
    want = KF.check(blob)
    for form in forms:
        rc, why, out = load_raw(store, blob, form)
        if want is None:
            assert rc == 0 and out.value not in (None, 0x77), (what, form, why)
            with store.Kept(out, store.D) as k:
                assert k.to_bytes() == blob, (what, form)
        else:
            assert rc == N.EINVAL, (what, form, rc)
            assert why == want, (what, form, [KF.CAUSES.get(why[0]), *why[1:]], [KF.CAUSES[want[0]], *want[1:]])
            assert out.value == 0x77, (what, form)                                # *out untouched
        with store.Kept.from_bytes(store.blobs["all"]) as ok:                     # nothing is left behind by a refusal
            assert ok.info == store.kept["all"].info
    return want


def listed_mutations(store):
    blob = store.blobs["all"]
    u = KF.unpack(blob)
    o = [int(x) for x in u["offsets"]]
    key = lambda i: int(u["keys"][i])                                             # noqa: E731
    nrows, cells = u["nrows"], u["cells"]
    return [
        # (row 0 is empty and off[1] = 0: with off[1] above off[2] row 0 spans cells that are not its own, and it is the lowest row)
        ("off[1] > off[2]", mutate(blob, "offsets", 1, o[2] + 1), KF.BAD_ROW_COUNT),
        ("off[2] > off[3]", mutate(blob, "offsets", 3, 0), KF.BAD_OFFSET_ORDER),
        ("off[nrows] != cells", mutate(blob, "offsets", nrows, cells - 1), KF.BAD_OFFSET_LAST),
        ("off[0] != 0", mutate(blob, "offsets", 0, 1), KF.BAD_OFFSET_FIRST),
        ("an offset beyond cells", mutate(blob, "offsets", 5, cells + 1), KF.BAD_OFFSET_ORDER),
        ("off[nrows] beyond cells", mutate(blob, "offsets", nrows, cells + 1), KF.BAD_OFFSET_ORDER),
        ("an offset of 2^64 - 1", mutate(blob, "offsets", 3, 2**64 - 1), KF.BAD_OFFSET_ORDER),
        ("two equal keys in a row", mutate(blob, "keys", o[5] + 10, key(o[5] + 9)), KF.BAD_KEY_ORDER),
        ("a descending pair inside a step", mutate(blob, "keys", o[5] + 70, key(o[5] + 60)), KF.BAD_KEY_ORDER),
        ("a descending pair across the step boundary", mutate(blob, "keys", o[5] + 64, key(o[5] + 63) - 1), KF.BAD_KEY_ORDER),
        ("... across the second boundary", mutate(blob, "keys", o[5] + 128, key(o[5] + 127)), KF.BAD_KEY_ORDER),
        ("... at the boundary of a 65-cell row", mutate(blob, "keys", o[4] + 64, key(o[4] + 63)), KF.BAD_KEY_ORDER),
        ("a zero count", mutate(blob, "counts", o[3] + 63, 0), KF.BAD_ZERO_COUNT),
        ("a zero count in the one-cell row", mutate(blob, "counts", o[1], 0), KF.BAD_ZERO_COUNT),
        ("a row_count off by one", mutate(blob, "row_count", 4, int(u["row_count"][4]) + 1), KF.BAD_ROW_COUNT),
        ("the wrapped row_count off by one", mutate(blob, "row_count", 8, 4), KF.BAD_ROW_COUNT),
        ("an empty row's row_count", mutate(blob, "row_count", 0, 1), KF.BAD_ROW_COUNT),
        ("the header's samples off by one", mutate(blob, "samples", 0, (u["samples"] + 1) % 2**64), KF.BAD_SAMPLES),
    ]


def test_each_listed_mutation_is_refused_with_the_references_verdict(store):
    for what, bad, cause in listed_mutations(store):
        want = held_to_the_reference(store, bad, what)
        assert want is not None and want[0] == cause, (what, want)                # the mutation is the one its name says


def test_two_violations_report_the_lowest_row_then_index_then_cause(store):
    blob = store.blobs["all"]
    u = KF.unpack(blob)
    o = [int(x) for x in u["offsets"]]
    k5 = lambda i: int(u["keys"][o[5] + i])                                       # noqa: E731
    cases = [
        mutate(mutate(blob, "counts", o[9] + 3, 0), "counts", o[3] + 40, 0),      # two rows, far apart in the grid
        mutate(mutate(blob, "counts", o[5] + 9, 0), "keys", o[5] + 9, k5(8)),     # one cell, two causes
        mutate(mutate(blob, "counts", o[5] + 100, 0), "keys", o[5] + 8, k5(7)),   # two steps of one row
        mutate(mutate(blob, "counts", o[5] + 9, 0), "row_count", 5, 1),           # a cell and the row's sum
        mutate(mutate(blob, "samples", 0, 0), "row_count", 11, 5),                # a row and the block's sum
        mutate(mutate(blob, "offsets", 0, 1), "offsets", 1, 0),                   # row 0: two offset causes
        mutate(mutate(blob, "offsets", 12, 0), "counts", o[11], 0),               # the last row: its offsets win over its cell
    ]
    for i, bad in enumerate(cases):
        assert held_to_the_reference(store, bad, i) is not None


def test_seeded_random_single_field_mutations_agree_with_the_reference(store):
    rng = np.random.default_rng(20240611)
    refused = taken = 0
    for name in ("all", "part", "tail"):
        blob = store.blobs[name]
        u = KF.unpack(blob)
        sizes = dict(offsets=u["nrows"] + 1, row_count=u["nrows"], counts=u["cells"], keys=u["cells"])
        for trial in range(16):
            what = ("offsets", "keys", "counts", "row_count")[trial % 4]
            at = int(rng.integers(0, sizes[what]))
            old = int(u[what][at])
            if what == "keys":
                value = int(np.clip(old + int(rng.integers(-40, 41)), -32768, 32767)) if trial % 8 < 4 else int(rng.integers(-32768, 32768))
            else:
                value = (old + int(rng.integers(-3, 4))) % 2**64 if trial % 8 < 4 else int(rng.integers(0, 2**64, dtype=U64))
            bad = mutate(blob, what, at, value)
            want = held_to_the_reference(store, bad, (name, what, at, old, value), forms=("host",) if trial % 2 else ("device",))
            refused += want is not None
            taken += want is None
    assert refused >= 24 and taken >= 1, (refused, taken)                         # both kinds occurred (seeded)


def test_header_causes_reach_the_device_form_too(store):
    """lh_kept_load_device decides the header once its 64 bytes have come over: the same causes, *out untouched"""
    blob = np.frombuffer(store.blobs["all"], dtype=np.uint8).copy()
    for at, cause in ((0, KF.BAD_MAGIC), (8, KF.BAD_VERSION), (12, KF.BAD_HEADER_SIZE), (16, KF.BAD_NKEYS), (28, KF.BAD_RESERVED),
                      (60, KF.BAD_RESERVED)):
        bad = blob.copy()
        bad[at] ^= 0x40
        rc, why, out = load_raw(store, bad.tobytes(), "device")
        assert rc == N.EINVAL and why == (cause, 0, 0) == KF.check(bad.tobytes()) and out.value == 0x77, KF.CAUSES[cause]
    rc, why, out = load_raw(store, blob[:-2].tobytes(), "device")
    assert rc == N.EINVAL and why == (KF.BAD_LENGTH, 0, 0) and out.value == 0x77
    with pytest.raises(ValueError, match="BAD_MAGIC"):
        store.Kept.from_bytes(b"x" * 100)
