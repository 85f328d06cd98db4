"""loghisto_amd.keptfile's statement of the ENCODED blob (lh_kept_encode* / lh_kept_decode*), on the CPU: encode and decode are
inverses byte for byte on rows crafted for every edge of the format -- the wave-step sizes, a row of all 65 536 bins, gaps of
exactly 256 (delta mode) and 257 (raw mode), counts at both sides of every width, bin 0 and bin 65 535 -- the size bound of
the format holds and an encoded blob is never longer than the verbatim one, and check_encoded names each single mutation with
the documented (cause, row, index), the lowest row / index / cause when two are present.  encode() is also held to
raw_encode() below, a second statement of the format written from the header's text with every width forced by the caller,
which is what the non-canonical blobs are made with.  tests/test_gpu_kept_encode.py holds the device to this module."""
import struct

import numpy as np
import pytest

from loghisto_amd import keptfile as KF

U64 = np.uint64
NK = 65536


# ---- the crafted rows: (bins, counts) -------------------------------------------------------------------------------------------
def row(bins, counts=None):
    bins = np.asarray(bins, dtype=np.int64)
    if counts is None:
        counts = 1 + np.arange(bins.size) % 5
    return bins, np.asarray(counts, dtype=U64)


def gap_row(at, gap, n=130):
    """n cells one bin apart, but cell `at` lies `gap` bins behind the one before"""
    steps = np.ones(n, dtype=np.int64)
    steps[at] = gap
    return row(1000 + np.cumsum(steps))


def big_row(big, at=66, n=70):
    """n small counts and ONE large one, behind the first step"""
    c = (1 + np.arange(n) % 5).astype(U64)
    c[at] = U64(big)
    return row(200 + 2 * np.arange(n), c)


SIZES = [0, 1, 2, 63, 64, 65, 128, 129]
BIGS = [255, 256, 65535, 65536, 2**32 - 1, 2**32, 2**64 - 1]


def crafted_rows():
    rows = [row(5000 + 3 * np.arange(n)) for n in SIZES]                           # 0 .. 7
    rows.append(row(np.arange(NK), 1 + np.arange(NK) % 200))                       # 8   every bin
    rows += [gap_row(1, 256), gap_row(1, 257), gap_row(129, 256), gap_row(129, 257)]   # 9 .. 12  first and last step
    rows += [row([0, 1, 2]), row([NK - 3, NK - 2, NK - 1]), row([0, NK - 1]), row([0]), row([NK - 1])]   # 13 .. 17
    rows += [big_row(b) for b in BIGS]                                             # 18 .. 24
    rows.append(row([7, 8], [2**63, 2**63 + 5]))                                   # 25  row_count wraps
    return rows


def blob_of(rows, first=0):
    off = np.concatenate([[0], np.cumsum([b.size for b, _ in rows])])
    bins = np.concatenate([b for b, _ in rows]) if rows else np.zeros(0, np.int64)
    counts = np.concatenate([c for _, c in rows]).astype(U64)
    return KF.pack(off, (bins.astype(np.uint16) ^ np.uint16(0x8000)).view(np.int16), counts, first=first)


def crafted_blobs():
    """name -> verbatim blob: nrows 1, 2, 3, 9 and all 26; first > 0; no cell at all"""
    R = crafted_rows()
    return {"all": blob_of(R), "one": blob_of([R[7]], first=5), "two": blob_of([R[10], R[3]], first=7), "three": blob_of(R[22:25]),
            "nine": blob_of(R[:8] + [R[12]], first=2**32 - 9), "every_bin": blob_of([R[8]]), "empty": blob_of([R[0]], first=3),
            "empty3": blob_of([R[0]] * 3)}


# ---- the format once more, from the header's text, with the widths in the caller's hand ---------------------------------------------
def up8(x):
    return (x + 7) // 8 * 8


def raw_encode(rows, first=0, force=None, samples=None):
    """The encoded blob of `rows`; force = {m: (cw, km)} overrides the canonical choice for row m"""
    force = force or {}
    desc, recs, total = [], [], 0
    for m, (bins, counts) in enumerate(rows):
        n = len(bins)
        total += sum(int(c) for c in counts)
        if n == 0:
            desc.append(0)
            continue
        top = max(int(c) for c in counts)
        cw = 0 if top < 2**8 else 1 if top < 2**16 else 2 if top < 2**32 else 3
        km = int(any(int(b) - int(a) > 256 for a, b in zip(bins[:-1], bins[1:])))
        cw, km = force.get(m, (cw, km))
        desc.append(n | cw << 20 | km << 24)
        part = b"".join(int(c).to_bytes(1 << cw, "little") for c in counts)
        rec = part + bytes(up8(len(part)) - len(part))
        if km:
            part = b"".join(struct.pack("<H", int(b)) for b in bins)
        else:
            part = struct.pack("<H", int(bins[0])) + bytes(int(b) - int(a) - 1 for a, b in zip(bins[:-1], bins[1:]))
        recs.append(rec + part + bytes(up8(len(part)) - len(part)))
    if len(desc) % 2:
        desc.append(0)
    body = struct.pack("<%dI" % len(desc), *desc) + b"".join(recs)
    cells = sum(len(b) for b, _ in rows)
    return struct.pack("<8sIIIIIIQQQ8s", b"LHKENC\x1a\n", 1, 64, NK, first, len(rows), 0, cells,
                       (total if samples is None else samples) % 2**64, len(body), bytes(8)) + body


def layout(enc):
    """[(n, cw, km, where the record starts, where its keys start)] per row of a blob whose directory is sound"""
    nrows = struct.unpack_from("<I", enc, 24)[0]
    at = 64 + KF.directory_bytes(nrows)
    out = []
    for d in struct.unpack_from("<%dI" % nrows, enc, 64):
        n, cw, km = d & 0x1ffff, d >> 20 & 3, d >> 24 & 1
        out.append((n, cw, km, at, at + up8(n << cw)))
        at += KF.record_bytes(n, cw, km)
    return out


def poke(enc, at, fmt, value):
    b = bytearray(enc)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


# ---- round trips and sizes --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    return crafted_blobs()


def holds_the_bounds(blob, enc):
    h = KF.parse_header(enc)
    assert len(enc) == 64 + h["bytes"] and h["bytes"] % 8 == 0
    assert len(enc) <= KF.encoded_bound(h["nrows"], h["cells"]) <= len(blob)      # the format's bound; never longer than verbatim
    assert KF.encoded_bound(h["nrows"], h["cells"]) == 64 + KF.directory_bytes(h["nrows"]) + 10 * h["cells"] + 6 * h["nrows"]


@pytest.mark.parametrize("name", ["all", "one", "two", "three", "nine", "every_bin", "empty", "empty3"])
def test_encode_and_decode_are_inverses(blobs, name):
    blob = blobs[name]
    assert KF.check(blob) is None
    enc = KF.encode(blob)
    assert KF.check_encoded(enc) is None
    assert KF.decode(enc) == blob and KF.encode(KF.decode(enc)) == enc
    holds_the_bounds(blob, enc)
    assert KF.check(enc) == (KF.BAD_MAGIC, 0, 0) and KF.check_encoded(blob) == (KF.BAD_MAGIC, 0, 0)   # neither reads the other


def test_encode_is_the_format_as_the_header_states_it(blobs):
    R = crafted_rows()
    assert KF.encode(blobs["all"]) == raw_encode(R)
    assert KF.encode(blobs["nine"]) == raw_encode(R[:8] + [R[12]], first=2**32 - 9)
    assert KF.encode(blobs["empty"]) == raw_encode([R[0]], first=3) and len(KF.encode(blobs["empty"])) == KF.ENC_MIN == 72
    lay = layout(KF.encode(blobs["all"]))
    assert [x[0] for x in lay[:9]] == SIZES + [NK]
    assert [x[2] for x in lay[9:13]] == [0, 1, 0, 1]                               # a gap of 256 stays in delta mode, 257 does not
    assert [x[2] for x in lay[13:18]] == [0, 0, 1, 0, 0]
    assert [x[1] for x in lay[18:25]] == [0, 1, 1, 2, 2, 3, 3]                     # the least width that holds the largest count
    assert lay[8][1:3] == (0, 0) and KF.record_bytes(NK, 0, 0) == NK + up8(NK + 1)


def random_rows(rng):
    rows = []
    for _ in range(int(rng.integers(1, 7))):
        n = int(rng.integers(0, 200)) if rng.random() < 0.8 else 0
        span = int(rng.choice([n + 1, 4 * n + 1, NK]))
        bins = np.sort(rng.choice(span, size=n, replace=False)) + int(rng.integers(0, NK - span + 1))
        top = int(rng.choice([2**8, 2**16, 2**32, 2**64]))
        counts = rng.integers(1, min(top, 2**63), size=n, dtype=np.uint64, endpoint=False)
        if n and rng.random() < 0.5:
            counts[int(rng.integers(0, n))] = U64(top - 1)
        rows.append(row(bins, counts))
    return rows


def test_the_size_bound_holds_on_random_handles():
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        rows = random_rows(rng)
        blob = blob_of(rows, first=int(rng.integers(0, 1000)))
        enc = KF.encode(blob)
        holds_the_bounds(blob, enc)
        assert KF.check_encoded(enc) is None and KF.decode(enc) == blob
        assert enc == raw_encode(rows, first=KF.parse_header(blob)["first"])


def test_decode_raises_on_what_check_encoded_refuses(blobs):
    enc = KF.encode(blobs["nine"])
    for bad in (enc[:-1], enc[:40], b"", poke(enc, 40, "<Q", 1), blobs["nine"]):
        assert KF.check_encoded(bad) is not None
        with pytest.raises(ValueError):
            KF.decode(bad)
    with pytest.raises(ValueError):
        KF.encode(enc)                                                            # not a verbatim blob
    assert set(KF.ENC_CAUSES) == set(KF.CAUSES) | {32, 33, 34, 35, 36}
    assert [KF.ENC_CAUSES[c] for c in range(32, 37)] == ["BAD_ENC_DESC", "BAD_ENC_TOTALS", "BAD_ENC_KEY_RANGE", "BAD_ENC_PAD",
                                                         "BAD_ENC_WIDTH"]


# ---- one mutation per cause -------------------------------------------------------------------------------------------------------
def mutation_rows():
    """nine rows: 0, 1, 2, 63, 64, 65, 128, 129 cells and the raw-mode row (a gap of 257 in its last step)"""
    R = crafted_rows()
    return R[:8] + [R[12]]


def single_mutations():
    """(enc, [(name, blob, verdict)]) over the nine rows above, first = 2^32 - 9"""
    rows = mutation_rows()
    enc = raw_encode(rows, first=2**32 - 9)
    lay = layout(enc)
    nrows, cells = 9, sum(SIZES) + 130
    n7, _, _, rec7, key7 = lay[7]                                                  # 129 cells, delta mode, 1-byte counts
    n8, _, _, rec8, key8 = lay[8]                                                  # 130 cells, raw mode
    top = mutation_rows()
    top[7] = row(NK - 1 - 3 * np.arange(129)[::-1])                                # the same row, ending at bin 65 535
    enc_top = raw_encode(top, first=2**32 - 9)
    cases = [
        # stage 0
        ("short", enc[:63], (KF.BAD_SHORT, 0, 0)),
        ("the verbatim magic", poke(enc, 0, "<8s", KF.MAGIC), (KF.BAD_MAGIC, 0, 0)),
        ("version 2", poke(enc, 8, "<I", 2), (KF.BAD_VERSION, 0, 0)),
        ("header size", poke(enc, 12, "<I", 72), (KF.BAD_HEADER_SIZE, 0, 0)),
        ("nkeys", poke(enc, 16, "<I", 65535), (KF.BAD_NKEYS, 0, 0)),
        ("no row", poke(enc, 24, "<I", 0), (KF.BAD_NROWS, 0, 0)),
        ("first + nrows past 2^32", poke(enc, 20, "<I", 2**32 - 8), (KF.BAD_FIRST, 0, 0)),
        ("cells beyond nrows * NKEYS", poke(enc, 32, "<Q", nrows * NK + 1), (KF.BAD_CELLS, 0, 0)),
        ("bytes not a multiple of 8", poke(enc, 48, "<Q", len(enc) - 64 + 4), (KF.BAD_BYTES, 0, 0)),
        ("bytes below the directory", poke(enc, 48, "<Q", 32), (KF.BAD_BYTES, 0, 0)),
        ("bytes above the bound", poke(enc, 48, "<Q", (40 + 10 * cells + 6 * nrows) // 8 * 8 + 8), (KF.BAD_BYTES, 0, 0)),
        ("bytes at the bound, not the length", poke(enc, 48, "<Q", (40 + 10 * cells + 6 * nrows) // 8 * 8), (KF.BAD_LENGTH, 0, 0)),
        ("a byte behind the end", enc + bytes(8), (KF.BAD_LENGTH, 0, 0)),
        ("reserved word", poke(enc, 28, "<I", 1), (KF.BAD_RESERVED, 0, 0)),
        ("reserved byte", poke(enc, 63, "<B", 1), (KF.BAD_RESERVED, 0, 0)),
        # stage 1
        ("a reserved bit of a descriptor", poke(enc, 64 + 4 * 3, "<I", 63 | 1 << 17), (KF.BAD_ENC_DESC, 3, 0)),
        ("bit 31 of a descriptor", poke(enc, 64 + 4 * 8, "<I", 130 | 1 << 24 | 1 << 31), (KF.BAD_ENC_DESC, 8, 0)),
        ("n = 65 537", poke(enc, 64 + 4 * 5, "<I", NK + 1), (KF.BAD_ENC_DESC, 5, 0)),
        ("an empty row with a width", poke(enc, 64, "<I", 1 << 20), (KF.BAD_ENC_DESC, 0, 0)),
        ("an empty row in raw mode", poke(enc, 64, "<I", 1 << 24), (KF.BAD_ENC_DESC, 0, 0)),
        ("the directory's pad word", poke(enc, 64 + 4 * nrows, "<I", 1), (KF.BAD_ENC_PAD, nrows, 0)),
        ("a cell fewer in a descriptor, the same S", poke(enc, 64 + 4 * 3, "<I", 62), (KF.BAD_ENC_TOTALS, nrows, 0)),
        ("the header's cells", poke(enc, 32, "<Q", cells + 1), (KF.BAD_ENC_TOTALS, nrows, 0)),
        ("a wider descriptor: more bytes than there are", poke(enc, 64 + 4 * 6, "<I", 128 | 3 << 20), (KF.BAD_ENC_TOTALS, nrows, 0)),
        ("n = 65 536 where 1 was", poke(enc, 64 + 4 * 1, "<I", NK), (KF.BAD_ENC_TOTALS, nrows, 0)),
        # stage 2
        ("a delta that carries the last bin to 65 536", poke(enc_top, layout(enc_top)[7][4] + 2 + 70, "<B", 3),
         (KF.BAD_ENC_KEY_RANGE, 7, 128)),
        ("a delta of 255 in the first step", poke(enc_top, layout(enc_top)[7][4] + 2 + 9, "<B", 255), (KF.BAD_ENC_KEY_RANGE, 7, 44)),
        ("two equal raw bins", poke(enc, key8 + 2 * 10, "<H", 1010), (KF.BAD_KEY_ORDER, 8, 10)),
        ("raw bins descending across the step", poke(enc, key8 + 2 * 64, "<H", 1063), (KF.BAD_KEY_ORDER, 8, 64)),
        ("... across the second step", poke(enc, key8 + 2 * 128, "<H", 5), (KF.BAD_KEY_ORDER, 8, 128)),
        ("a zero count", poke(enc, rec7 + 64, "<B", 0), (KF.BAD_ZERO_COUNT, 7, 64)),
        ("a zero count in the one-cell row", poke(enc, lay[1][3], "<B", 0), (KF.BAD_ZERO_COUNT, 1, 0)),
        ("a pad byte behind the counts", poke(enc, rec7 + 129, "<B", 1), (KF.BAD_ENC_PAD, 7, 129)),
        ("the last pad byte behind the counts", poke(enc, key7 - 1, "<B", 0x80), (KF.BAD_ENC_PAD, 7, 129)),
        ("a pad byte behind the keys", poke(enc, key7 + 130, "<B", 1), (KF.BAD_ENC_PAD, 7, 129)),
        ("a pad byte behind raw keys", poke(enc, key8 + 2 * 130 + 3, "<B", 9), (KF.BAD_ENC_PAD, 8, 130)),
        ("counts wider than they need be", raw_encode(rows, 2**32 - 9, {4: (1, 0)}), (KF.BAD_ENC_WIDTH, 4, 64)),
        ("8-byte counts for small ones", raw_encode(rows, 2**32 - 9, {7: (3, 0)}), (KF.BAD_ENC_WIDTH, 7, 129)),
        ("raw mode without a wide gap", raw_encode(rows, 2**32 - 9, {5: (0, 1)}), (KF.BAD_ENC_WIDTH, 5, 65)),
        ("raw mode for one cell", raw_encode(rows, 2**32 - 9, {1: (0, 1)}), (KF.BAD_ENC_WIDTH, 1, 1)),
        ("samples off by one", raw_encode(rows, 2**32 - 9, samples=sum(int(c.sum()) for _, c in rows) + 1), (KF.BAD_SAMPLES, nrows, 0)),
    ]
    return enc, cases


def two_violations():
    """[(name, blob, verdict)]: the lowest row, in it the lowest index, there the lowest cause; a stage-1 refusal is final"""
    rows = mutation_rows()
    enc = raw_encode(rows, first=2**32 - 9)
    lay = layout(enc)
    rec = lambda m: lay[m][3]                                                     # noqa: E731
    key = lambda m: lay[m][4]                                                     # noqa: E731
    z = lambda b, m, i: poke(b, rec(m) + i, "<B", 0)                              # noqa: E731
    return [
        ("two rows", z(z(enc, 7, 3), 3, 40), (KF.BAD_ZERO_COUNT, 3, 40)),
        ("two steps of a row", z(z(enc, 7, 100), 7, 9), (KF.BAD_ZERO_COUNT, 7, 9)),
        ("one cell, two causes", poke(z(enc, 8, 9), key(8) + 18, "<H", 1009), (KF.BAD_KEY_ORDER, 8, 9)),
        ("a cell before the row's pads", poke(z(enc, 7, 128), rec(7) + 130, "<B", 1), (KF.BAD_ZERO_COUNT, 7, 128)),
        ("a pad and a width", poke(raw_encode(rows, 2**32 - 9, {5: (0, 1)}), layout(raw_encode(rows, 2**32 - 9, {5: (0, 1)}))[5][3] + 66,
                                   "<B", 1), (KF.BAD_ENC_PAD, 5, 65)),
        ("a row before the samples", poke(z(enc, 8, 129), 40, "<Q", 0), (KF.BAD_ZERO_COUNT, 8, 129)),
        ("two descriptors", poke(poke(enc, 64 + 4 * 6, "<I", 1 << 31), 64 + 4 * 2, "<I", 2 | 1 << 18), (KF.BAD_ENC_DESC, 2, 0)),
        ("a descriptor before the totals", poke(poke(enc, 32, "<Q", 583), 64 + 4 * 8, "<I", 130 | 1 << 25), (KF.BAD_ENC_DESC, 8, 0)),
        ("the totals before the pad word", poke(poke(enc, 32, "<Q", 583), 64 + 36, "<I", 7), (KF.BAD_ENC_TOTALS, 9, 0)),
        ("the directory before any record", z(poke(enc, 64 + 4 * 8, "<I", 130 | 1 << 24 | 1 << 30), 1, 0), (KF.BAD_ENC_DESC, 8, 0)),
    ]


def test_check_encoded_names_each_single_mutation():
    enc, cases = single_mutations()
    assert KF.check_encoded(enc) is None
    seen = set()
    for name, bad, want in cases:
        assert KF.check_encoded(bad) == want, (name, KF.check_encoded(bad), want)
        seen.add(want[0])
    assert seen == set(range(2, 13)) | {KF.BAD_KEY_ORDER, KF.BAD_ZERO_COUNT, KF.BAD_SAMPLES} | set(range(32, 37))   # every cause but BAD_ARG


def test_two_violations_report_the_lowest_row_then_index_then_cause():
    for name, bad, want in two_violations():
        assert KF.check_encoded(bad) == want, (name, KF.check_encoded(bad), want)
