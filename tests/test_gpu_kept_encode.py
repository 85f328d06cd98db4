"""lh_kept_encode* / lh_kept_decode* (Kept.encode, encode_device, encoded_size, decode, decode_device, save / load encoded=True)
on the device, held to loghisto_amd.keptfile byte for byte.

The handles are crafted with keptfile.pack + Kept.from_bytes, no engine and no ingest, from tests/test_keptfile_encode.py's rows:
0, 1, 2, 63, 64, 65, 128 and 129 cells and a row of all 65 536 bins; gaps of exactly 256 and 257 in the first and in the last
step of a row; bin 0 and bin 65 535; 255 / 256, 65 535 / 65 536, 2^32 - 1 / 2^32 and 2^64 - 1 as the single largest count of an
otherwise small row; 1, 2, 3, 9 and 26 rows; first > 0; no cell at all.  What a decode refuses is held to
keptfile.check_encoded on mutated well-formed blobs: ordinary input validation."""
import ctypes as C
import types

import numpy as np
import pytest

from loghisto_amd import _native as N
from loghisto_amd import keptfile as KF
from tests.test_keptfile_encode import crafted_blobs, single_mutations, two_violations

pytestmark = pytest.mark.gpu

NAMES = ["all", "one", "two", "three", "nine", "every_bin", "empty", "empty3"]
P = [0.0, 0.5, 0.99, 1.0]


@pytest.fixture(scope="module")
def codec(native_lib, torch_cuda):
    import loghisto_amd
    blobs = crafted_blobs()
    kept = {name: loghisto_amd.Kept.from_bytes(b) for name, b in blobs.items()}
    enc = {name: KF.encode(b) for name, b in blobs.items()}                        # the reference, once
    yield types.SimpleNamespace(blobs=blobs, kept=kept, enc=enc, torch=torch_cuda, Kept=loghisto_amd.Kept)
    for k in kept.values():
        k.close()


def on_device(codec, data, lead=0):
    """`data` in device memory, `lead` bytes behind an aligned address"""
    t = codec.torch.full((len(data) + lead,), 0xff, dtype=codec.torch.uint8, device="cuda")
    t[lead:] = codec.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    codec.torch.cuda.synchronize()
    return t[lead:]


@pytest.mark.parametrize("name", NAMES)
def test_encode_is_the_references_byte_for_byte(codec, name):
    k, want = codec.kept[name], codec.enc[name]
    t, L = codec.torch, N.lib()
    assert k.encoded_size() == len(want)
    got = k.encode()
    assert got.dtype == np.uint8 and got.tobytes() == want
    d = k.encode_device()
    assert d.dtype == t.uint8 and d.is_cuda and bytes(d.cpu().numpy()) == want
    # into memory that held 0xff, with room to spare, at an aligned address and one byte behind it; on a stream of the caller's
    st = t.cuda.Stream()
    for lead in (0, 1):
        room = t.full((len(want) + lead + 16,), 0xff, dtype=t.uint8, device="cuda")
        t.cuda.synchronize()
        written = C.c_size_t(0)
        rc = L.lh_kept_encode_device(k._h, room.data_ptr() + lead, room.numel() - lead, C.c_void_p(st.cuda_stream), C.byref(written))
        assert rc == 0 and written.value == len(want)
        back = room.cpu().numpy()
        assert back[lead:lead + len(want)].tobytes() == want, lead
        assert np.all(back[:lead] == 0xff) and np.all(back[lead + len(want):] == 0xff), lead
    buf = np.full(len(want) + 16, 0xff, dtype=np.uint8)
    assert L.lh_kept_encode(k._h, buf.ctypes.data, buf.size, None, None) == 0     # written may be NULL
    assert buf[:len(want)].tobytes() == want and np.all(buf[len(want):] == 0xff)


@pytest.mark.parametrize("name", NAMES)
def test_decode_gives_the_handle_back_byte_for_byte(codec, name):
    k, blob, enc = codec.kept[name], codec.blobs[name], codec.enc[name]
    with codec.Kept.decode(enc) as back:
        assert back.info == k.info and back.to_bytes() == blob
        assert back.encode().tobytes() == enc                                     # and once more round
    with codec.Kept.decode(np.frombuffer(enc, dtype=np.uint8)) as back:
        assert back.to_bytes() == blob
    st = codec.torch.cuda.Stream()
    for lead in (0, 1):
        with codec.Kept.decode_device(on_device(codec, enc, lead), stream=st) as back:
            assert back.info == k.info and back.to_bytes(stream=st) == blob, lead
    with codec.Kept.decode_device(k.encode_device()) as back:
        assert back.to_bytes() == blob


def test_a_capacity_one_below_the_size_is_refused_and_nothing_written(codec):
    L, t = N.lib(), codec.torch
    for name in ("nine", "empty"):
        k, want = codec.kept[name], codec.enc[name]
        written = C.c_size_t(0x77)
        buf = np.full(len(want) + 8, 7, dtype=np.uint8)
        d = t.full((len(want) + 8,), 7, dtype=t.uint8, device="cuda")
        for cap in {KF.ENC_MIN, len(want) - 1} - {len(want)}:
            assert L.lh_kept_encode(k._h, buf.ctypes.data, cap, None, C.byref(written)) == N.ERANGE, (name, cap)
            assert L.lh_kept_encode_device(k._h, d.data_ptr(), cap, None, C.byref(written)) == N.ERANGE, (name, cap)
            assert L.lh_kept_encode_device(k._h, d.data_ptr() + 1, cap, None, C.byref(written)) == N.ERANGE, (name, cap)
        assert L.lh_kept_encode(k._h, buf.ctypes.data, 71, None, C.byref(written)) == N.ERANGE
        assert written.value == 0x77 and np.all(buf == 7) and bool((d == 7).all())
        assert L.lh_kept_encode(k._h, buf.ctypes.data, len(want), None, C.byref(written)) == 0 and written.value == len(want)
        assert buf[:len(want)].tobytes() == want and np.all(buf[len(want):] == 7)


def test_save_and_load_encoded_through_a_file(codec, tmp_path):
    k = codec.kept["nine"]
    path = tmp_path / "nine.lhkenc"
    k.save(path, encoded=True)
    assert path.read_bytes() == codec.enc["nine"]
    with codec.Kept.load(path, encoded=True) as back:
        assert back.to_bytes() == codec.blobs["nine"]
    with pytest.raises(ValueError, match="BAD_MAGIC"):
        codec.Kept.load(path)                                                     # the verbatim loader does not read it
    with pytest.raises(ValueError, match="BAD_MAGIC"):
        codec.Kept.decode(codec.blobs["nine"])


def test_across_reads_a_decoded_handle_like_the_original(codec):
    k = codec.kept["all"]
    want = k.across([], P)
    with codec.Kept.decode(codec.enc["all"]) as back, codec.Kept.decode_device(k.encode_device()) as dback:
        for b in (back, dback, ):
            got = b.across([], P)
            assert set(got) == set(want)
            for key in want:
                assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
        mixed, twice = k.across([back, dback], P), k.across([k, k], P)
        for key in twice:
            assert mixed[key].tobytes() == twice[key].tobytes(), key


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def decode_raw(codec, enc, form):
    """lh_kept_decode / lh_kept_decode_device on `enc` -> (status, (cause, row, index), *out)"""
    L = N.lib()
    why = N.LhKeptCheck(struct_size=16, cause=0x77, row=0x77, index=0x77)
    out = C.c_void_p(0x77)
    a = np.frombuffer(enc, dtype=np.uint8)
    if form == "host":
        rc = L.lh_kept_decode(0, a.ctypes.data, a.size, 0, None, C.byref(why), C.byref(out))
    else:
        lead = 1 if form == "device, odd address" else 0
        t = on_device(codec, enc, lead)
        rc = L.lh_kept_decode_device(0, t.data_ptr(), a.size, 0, None, C.byref(why), C.byref(out))
    return rc, (why.cause, why.row, why.index), out


def held_to_the_reference(codec, cases, forms=("host", "device", "device, odd address")):
    good = codec.enc["nine"]
    for what, bad, want in cases:
        assert KF.check_encoded(bad) == want, what
        for form in forms:
            rc, why, out = decode_raw(codec, bad, form)
            assert rc == N.EINVAL, (what, form, rc)
            assert why == want, (what, form, [KF.ENC_CAUSES.get(why[0]), *why[1:]], [KF.ENC_CAUSES[want[0]], *want[1:]])
            assert out.value == 0x77, (what, form)                                # *out untouched: no handle is left
        with codec.Kept.decode(good) as ok:                                       # and a sound blob is taken right afterwards
            assert ok.info == codec.kept["nine"].info


def test_each_mutation_gets_the_references_verdict(codec):
    enc, cases = single_mutations()
    assert enc == codec.enc["nine"]                                               # the mutations are of the blob the device made too
    device_decided = [c for c in cases if c[2][0] >= 16]
    assert {c[2][0] for c in device_decided} == {KF.BAD_KEY_ORDER, KF.BAD_ZERO_COUNT, KF.BAD_SAMPLES} | set(range(32, 37))
    held_to_the_reference(codec, device_decided)
    held_to_the_reference(codec, [c for c in cases if c[2][0] < 16], forms=("device",))   # the header, once it has come over


def test_two_violations_report_the_lowest_row_then_index_then_cause(codec):
    held_to_the_reference(codec, two_violations(), forms=("host", "device"))
