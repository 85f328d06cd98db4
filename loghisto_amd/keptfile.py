"""The blob of a kept interval (lh_kept_save* / lh_kept_load*, include/loghisto_gpu.h) in pure NumPy: no GPU, no library.

A 64-byte little-endian header, then the handle's single allocation verbatim:
    offsets uint64[nrows + 1] | row_count uint64[nrows] | counts uint64[cells] | keys int16[cells]

pack() makes a blob from CSR arrays, unpack() takes one apart, and check() restates every rule lh_kept_load* holds a blob
to -- the header's on the host, the block's on the device -- with the same verdict: of all violations the one of the lowest
row, in it the lowest index, there the lowest cause code.  The device's check is held to check() by the tests.
combine() states lh_kept_slide on blobs -- per row and bin the add side's sum minus the sub side's, KeptUnderflow for a cell that
would go below zero -- and is the reference the device's slide is held to.  gather() states lh_kept_gather* the same way: rows
re-mapped per blob and summed; group() states lh_kept_group*: many rows summed into one, by group.  pack_names() / unpack_names() are a sidecar for the names of a handle's rows (the blob itself
carries row numbers only and its format does not change).

encode() / decode() / check_encoded() state the COMPACT blob the same way (lh_kept_encode* / lh_kept_decode*): the same handle in
a per-row encoding -- a directory of row descriptors, then per row the counts at the narrowest width that holds the row's largest
and the bins as byte deltas (or raw uint16 where a gap exceeds 256).  One handle has exactly one encoding, decode(encode(b)) == b
byte for byte, and check_encoded() gives the library's verdict on untrusted bytes.
"""
from __future__ import annotations

import struct

import numpy as np

NKEYS = 65536
MAGIC = b"LHKEPT\x1a\n"
VERSION = 1
HEADER = 64
BLOB_MIN = HEADER + 24
_HEAD = struct.Struct("<8sIIIIIIQQQ8s")
assert _HEAD.size == HEADER

# lh_kept_check.cause (LH_KEPT_BAD_*)
(BAD_ARG, BAD_SHORT, BAD_MAGIC, BAD_VERSION, BAD_HEADER_SIZE, BAD_NKEYS, BAD_NROWS, BAD_FIRST, BAD_CELLS, BAD_BYTES, BAD_LENGTH,
 BAD_RESERVED) = range(1, 13)
(BAD_OFFSET_FIRST, BAD_OFFSET_ORDER, BAD_ROW_LENGTH, BAD_OFFSET_LAST, BAD_KEY_ORDER, BAD_ZERO_COUNT, BAD_ROW_COUNT,
 BAD_SAMPLES) = range(16, 24)
CAUSES = {v: k for k, v in list(globals().items()) if k.startswith("BAD_")}

# the verbatim blob's causes are CAUSES (above: the header's enum, name for name); an encoded blob reuses most of them and adds
(BAD_ENC_DESC, BAD_ENC_TOTALS, BAD_ENC_KEY_RANGE, BAD_ENC_PAD, BAD_ENC_WIDTH) = range(32, 37)
ENC_CAUSES = dict(CAUSES)                # every cause lh_kept_decode* can report
ENC_CAUSES.update({v: k for k, v in list(globals().items()) if k.startswith("BAD_ENC_")})

_M64 = (1 << 64) - 1


def block_bytes(nrows: int, cells: int) -> int:
    return (2 * nrows + 1) * 8 + cells * 10


def header(first: int, nrows: int, cells: int, samples: int) -> bytes:
    return _HEAD.pack(MAGIC, VERSION, HEADER, NKEYS, first, nrows, 0, cells, samples, block_bytes(nrows, cells), bytes(8))


def pack(offsets, keys, counts, first: int = 0) -> bytes:
    """The blob of rows [first, first + nrows) with CSR arrays offsets[nrows + 1], keys[cells] (int16), counts[cells] (uint64):
    row_count and samples are computed here (wrapping sums).  Nothing is checked: check() does that."""
    off = np.ascontiguousarray(offsets, dtype="<u8").ravel()
    k = np.ascontiguousarray(keys, dtype="<i2").ravel()
    c = np.ascontiguousarray(counts, dtype="<u8").ravel()
    nrows = off.size - 1
    if nrows < 1 or k.size != c.size:
        raise ValueError("offsets has nrows + 1 >= 2 entries, keys and counts one entry per cell")
    with np.errstate(over="ignore"):
        row_count = np.array([c[int(a):int(b)].sum(dtype=np.uint64) for a, b in zip(off[:-1], off[1:])], dtype="<u8")
        samples = int(row_count.sum(dtype=np.uint64))
    return header(first, nrows, c.size, samples) + off.tobytes() + row_count.tobytes() + c.tobytes() + k.tobytes()


def parse_header(blob) -> dict:
    b = bytes(memoryview(blob)[:HEADER])
    f = _HEAD.unpack(b)
    return dict(zip(("magic", "version", "header_size", "nkeys", "first", "nrows", "reserved0", "cells", "samples", "bytes",
                     "reserved1"), f))


def _header_cause(h: dict, length: int):
    if h["magic"] != MAGIC:
        return BAD_MAGIC
    if h["version"] != VERSION:
        return BAD_VERSION
    if h["header_size"] != HEADER:
        return BAD_HEADER_SIZE
    if h["nkeys"] != NKEYS:
        return BAD_NKEYS
    if h["nrows"] == 0:
        return BAD_NROWS
    if h["first"] + h["nrows"] > 1 << 32:
        return BAD_FIRST
    if h["cells"] > h["nrows"] * NKEYS:
        return BAD_CELLS
    if h["bytes"] != block_bytes(h["nrows"], h["cells"]):
        return BAD_BYTES
    if length != HEADER + h["bytes"]:
        return BAD_LENGTH
    if h["reserved0"] != 0 or any(h["reserved1"]):
        return BAD_RESERVED
    return None


def _arrays(blob, h):
    nrows, cells = h["nrows"], h["cells"]
    buf = memoryview(blob)
    at = HEADER
    off = np.frombuffer(buf, dtype="<u8", count=nrows + 1, offset=at)
    at += 8 * (nrows + 1)
    row_count = np.frombuffer(buf, dtype="<u8", count=nrows, offset=at)
    at += 8 * nrows
    counts = np.frombuffer(buf, dtype="<u8", count=cells, offset=at)
    at += 8 * cells
    keys = np.frombuffer(buf, dtype="<i2", count=cells, offset=at)
    return off, row_count, counts, keys


def unpack(blob) -> dict:
    """dict(first, nrows, cells, samples, bytes, offsets, keys, counts, row_count) of a blob whose HEADER is sound (ValueError
    otherwise); the arrays view the blob.  The block is not checked: check() does that."""
    if len(blob) < HEADER:
        raise ValueError("shorter than a header")
    h = parse_header(blob)
    cause = _header_cause(h, len(blob))
    if cause:
        raise ValueError("not a kept blob: " + CAUSES[cause])
    off, row_count, counts, keys = _arrays(blob, h)
    return dict(first=h["first"], nrows=h["nrows"], cells=h["cells"], samples=h["samples"], bytes=h["bytes"], offsets=off, keys=keys,
                counts=counts, row_count=row_count)


def check(blob):
    """None for a blob lh_kept_load* takes, else (cause, row, index) as lh_kept_check reports it: the header's causes in
    their documented order with row = index = 0, then -- over the block -- the violation of the lowest row, in it the lowest
    index, there the lowest cause code.  A row whose offsets are bad is not walked (index 0); a cell's causes carry the cell's
    index within the row; a bad row_count has index = the row's number of cells; bad samples has row = nrows."""
    if len(blob) < HEADER:
        return (BAD_SHORT, 0, 0)
    h = parse_header(blob)
    cause = _header_cause(h, len(blob))
    if cause:
        return (cause, 0, 0)
    off, row_count, counts, keys = _arrays(blob, h)
    nrows, cells = h["nrows"], h["cells"]
    bins = (keys.view("<u2") ^ np.uint16(0x8000)).astype(np.int64)
    for m in range(nrows):
        a, b = int(off[m]), int(off[m + 1])
        bad = []
        if m == 0 and a != 0:
            bad.append(BAD_OFFSET_FIRST)
        if not a <= b <= cells:
            bad.append(BAD_OFFSET_ORDER)
        elif b - a > NKEYS:
            bad.append(BAD_ROW_LENGTH)
        if m == nrows - 1 and b != cells:
            bad.append(BAD_OFFSET_LAST)
        if bad:
            return (min(bad), m, 0)
        rb, rc = bins[a:b], counts[a:b]
        found = []                                       # (index, cause)
        down = np.flatnonzero(rb[1:] <= rb[:-1])
        if down.size:
            found.append((int(down[0]) + 1, BAD_KEY_ORDER))
        zero = np.flatnonzero(rc == 0)
        if zero.size:
            found.append((int(zero[0]), BAD_ZERO_COUNT))
        if found:
            index, cause = min(found)
            return (cause, m, index)
        if sum(int(c) for c in rc) & _M64 != int(row_count[m]):
            return (BAD_ROW_COUNT, m, b - a)
    if sum(int(c) for c in row_count) & _M64 != h["samples"]:
        return (BAD_SAMPLES, nrows, 0)
    return None


# ---- the compact blob (lh_kept_encode* / lh_kept_decode*; include/loghisto_gpu.h has the format) -------------------------------
ENC_MAGIC = b"LHKENC\x1a\n"
ENC_VERSION = 1
ENC_MIN = HEADER + 8                     # one row, no cell: the header and a directory of one descriptor and its pad word
_DESC_BITS = 0x1ffff | 3 << 20 | 1 << 24


def _up8(x: int) -> int:
    return (x + 7) & ~7


def directory_bytes(nrows: int) -> int:
    return 8 * ((nrows + 1) // 2)


def record_bytes(n: int, cw: int, km: int) -> int:
    """S(m): the length of the record of a row of n >= 1 cells with count width 1 << cw and key mode km; 0 for n == 0"""
    return _up8(n << cw) + _up8(2 * n if km else n + 1) if n else 0


def encoded_bound(nrows: int, cells: int) -> int:
    """The capacity that always suffices for the encoded blob of a handle of nrows rows and `cells` cells, header included
    (LH_KEPT_ENC_BOUND): 64 + D + 10 * cells + 6 * nrows, never above the verbatim blob's 64 + 10 * cells + 16 * nrows + 8."""
    return HEADER + directory_bytes(nrows) + 10 * cells + 6 * nrows


def _enc_header(first, nrows, cells, samples, nbytes) -> bytes:
    return _HEAD.pack(ENC_MAGIC, ENC_VERSION, HEADER, NKEYS, first, nrows, 0, cells, samples, nbytes, bytes(8))


def _width_class(c) -> int:
    """cw: the least of 0 .. 3 with max(c) < 2^(8 << cw) (c: a non-empty uint64 array)"""
    top = int(c.max())
    return 0 if top <= 0xff else 1 if top <= 0xffff else 2 if top <= 0xffffffff else 3


_COUNT_TYPES = ("u1", "<u2", "<u4", "<u8")


def encode(blob) -> bytes:
    """The encoded blob of a verbatim one, as lh_kept_encode writes it for the handle lh_kept_load makes of `blob`.  ValueError
    for a blob check() refuses."""
    blob = bytes(blob)
    bad = check(blob)
    if bad:
        raise ValueError(f"not a kept blob: {CAUSES[bad[0]]} (row {bad[1]}, index {bad[2]})")
    u = unpack(blob)
    nrows, off = u["nrows"], u["offsets"].astype(np.int64)
    bins_all = (u["keys"].view("<u2") ^ np.uint16(0x8000)).astype(np.int64)
    desc = np.zeros(nrows + (nrows & 1), dtype="<u4")
    records = []
    for m in range(nrows):
        a, b = int(off[m]), int(off[m + 1])
        n = b - a
        if not n:
            continue
        c, bins = u["counts"][a:b], bins_all[a:b]
        cw = _width_class(c)
        gaps = np.diff(bins)
        km = int(gaps.size > 0 and int(gaps.max()) > 256)
        desc[m] = n | cw << 20 | km << 24
        cb = c.astype(_COUNT_TYPES[cw]).tobytes()
        kb = bins.astype("<u2").tobytes() if km else bins[:1].astype("<u2").tobytes() + (gaps - 1).astype("u1").tobytes()
        records.append(cb + bytes(_up8(len(cb)) - len(cb)) + kb + bytes(_up8(len(kb)) - len(kb)))
    body = desc.tobytes() + b"".join(records)
    return _enc_header(u["first"], nrows, u["cells"], u["samples"], len(body)) + body


def _enc_header_cause(h: dict, length: int):
    if h["magic"] != ENC_MAGIC:
        return BAD_MAGIC
    if h["version"] != ENC_VERSION:
        return BAD_VERSION
    if h["header_size"] != HEADER:
        return BAD_HEADER_SIZE
    if h["nkeys"] != NKEYS:
        return BAD_NKEYS
    if h["nrows"] == 0:
        return BAD_NROWS
    if h["first"] + h["nrows"] > 1 << 32:
        return BAD_FIRST
    if h["cells"] > h["nrows"] * NKEYS:
        return BAD_CELLS
    D = directory_bytes(h["nrows"])
    if h["bytes"] % 8 or h["bytes"] < D or h["bytes"] > D + 10 * h["cells"] + 6 * h["nrows"]:
        return BAD_BYTES
    if length != HEADER + h["bytes"]:
        return BAD_LENGTH
    if h["reserved0"] != 0 or any(h["reserved1"]):
        return BAD_RESERVED
    return None


def _walk_encoded(enc, want_arrays: bool):
    """(verdict, arrays): check_encoded's verdict, and for a sound blob with want_arrays (first, offsets, keys, counts)"""
    if len(enc) < HEADER:
        return (BAD_SHORT, 0, 0), None
    h = parse_header(enc)
    cause = _enc_header_cause(h, len(enc))
    if cause:
        return (cause, 0, 0), None
    nrows, cells = h["nrows"], h["cells"]
    buf = np.frombuffer(enc, dtype=np.uint8)
    D = directory_bytes(nrows)
    desc = np.frombuffer(enc, dtype="<u4", count=D // 4, offset=HEADER).astype(np.int64)
    # ---- stage 1: the directory alone
    d = desc[:nrows]
    n = d & 0x1ffff
    bad = np.flatnonzero(((d & ~_DESC_BITS) != 0) | (n > NKEYS) | ((n == 0) & (d != 0)))
    if bad.size:
        return (BAD_ENC_DESC, int(bad[0]), 0), None
    cw, km = (d >> 20) & 3, (d >> 24) & 1
    S = np.where(n > 0, ((n << cw) + 7 & ~7) + (np.where(km == 1, 2 * n, n + 1) + 7 & ~7), 0)
    if int(n.sum()) != cells or D + int(S.sum()) != h["bytes"]:
        return (BAD_ENC_TOTALS, nrows, 0), None
    if nrows & 1 and desc[nrows] != 0:
        return (BAD_ENC_PAD, nrows, 0), None
    # ---- stage 2: the records
    off = np.concatenate(([0], np.cumsum(n)))
    at = HEADER + D
    keys = np.zeros(cells, dtype="<u2")
    counts = np.zeros(cells, dtype="<u8")
    samples = 0
    for m in range(nrows):
        nm = int(n[m])
        if not nm:
            continue
        w, raw = 1 << int(cw[m]), int(km[m])
        cb, kb = nm * w, 2 * nm if raw else nm + 1
        c = np.frombuffer(enc, dtype=_COUNT_TYPES[int(cw[m])], count=nm, offset=at).astype(np.uint64)
        kat = at + _up8(cb)
        pads = np.concatenate((buf[at + cb:kat], buf[kat + kb:kat + _up8(kb)]))
        found = []                                       # (index, cause)
        if raw:
            bins = np.frombuffer(enc, dtype="<u2", count=nm, offset=kat).astype(np.int64)
            down = np.flatnonzero(bins[1:] <= bins[:-1])
            if down.size:
                found.append((int(down[0]) + 1, BAD_KEY_ORDER))
        else:
            first_bin = int(np.frombuffer(enc, dtype="<u2", count=1, offset=kat)[0])
            bins = first_bin + np.concatenate(([0], np.cumsum(buf[kat + 2:kat + kb].astype(np.int64) + 1)))
            over = np.flatnonzero(bins > NKEYS - 1)
            if over.size:
                found.append((int(over[0]), BAD_ENC_KEY_RANGE))
        zero = np.flatnonzero(c == 0)
        if zero.size:
            found.append((int(zero[0]), BAD_ZERO_COUNT))
        if not found and pads.any():
            found.append((nm, BAD_ENC_PAD))
        if not found and (_width_class(c) != int(cw[m]) or (raw and not (nm > 1 and int(np.diff(bins).max()) > 256))):
            found.append((nm, BAD_ENC_WIDTH))
        if found:
            index, cause = min(found)
            return (cause, m, index), None
        a = int(off[m])
        keys[a:a + nm] = bins.astype("<u2") ^ np.uint16(0x8000)
        counts[a:a + nm] = c
        with np.errstate(over="ignore"):
            samples = (samples + int(c.sum(dtype=np.uint64))) & _M64
        at = kat + _up8(kb)
    if samples != h["samples"]:
        return (BAD_SAMPLES, nrows, 0), None
    return None, (h["first"], off, keys.view("<i2"), counts)


def check_encoded(enc):
    """None for an encoded blob lh_kept_decode* takes, else (cause, row, index) as lh_kept_check reports it.  The header's causes
    in their documented order with row = index = 0.  Then the directory: a descriptor with a reserved bit, more than NKEYS
    cells, or no cell and another bit (BAD_ENC_DESC: row m, index 0); cells or bytes that the directory does not add up to
    (BAD_ENC_TOTALS: row nrows, index 0); a non-zero pad word behind an odd number of descriptors (BAD_ENC_PAD: row nrows,
    index 0) -- the lowest row, there the lowest cause code, and a refusal of the directory is final.  Then the records: per
    cell i a bin above 65 535 in delta mode (BAD_ENC_KEY_RANGE), raw bins that do not ascend (BAD_KEY_ORDER), a zero count
    (BAD_ZERO_COUNT); behind the row's cells (index n) a non-zero pad byte (BAD_ENC_PAD), then a count width or key mode that
    is not the canonical one (BAD_ENC_WIDTH); behind every row (row nrows) BAD_SAMPLES.  Of all violations the one of the lowest
    row, in it the lowest index, there the lowest cause code."""
    return _walk_encoded(bytes(enc), False)[0]


def decode(enc) -> bytes:
    """The verbatim blob of an encoded one: encode() back, byte for byte.  ValueError for anything check_encoded refuses."""
    bad, arrays = _walk_encoded(bytes(enc), True)
    if bad:
        raise ValueError(f"not an encoded kept blob: {ENC_CAUSES[bad[0]]} (row {bad[1]}, index {bad[2]})")
    first, off, keys, counts = arrays
    return pack(off, keys, counts, first=first)


class KeptUnderflow(ArithmeticError):
    """lh_kept_slide / combine() refused a window: the cell (row, key) -- row an ABSOLUTE metric id, key its bucket key; of all
    such cells the one of the lowest row, in it the lowest bin -- would go below zero."""

    def __init__(self, row: int, key: int):
        super().__init__(f"kept slide: the cell of metric {row}, key {key}, would go below zero")
        self.row, self.key = row, key


def _side(blobs, first, nrows):
    """Per row of [first, first + nrows): {bin: the sum mod 2^64 of the blobs' cells}, and the sum mod 2^64 of their row_count."""
    cells, rcs = [{} for _ in range(nrows)], [0] * nrows
    for u in blobs:
        at = first - u["first"]
        bins = u["keys"].view("<u2") ^ np.uint16(0x8000)
        for m in range(nrows):
            a, b = int(u["offsets"][at + m]), int(u["offsets"][at + m + 1])
            row = cells[m]
            for j, c in zip(bins[a:b].tolist(), u["counts"][a:b].tolist()):
                row[j] = (row.get(j, 0) + c) & _M64
            rcs[m] = (rcs[m] + int(u["row_count"][at + m])) & _M64
    return cells, rcs


def combine(add_blobs, sub_blobs=(), first=None, nrows=None) -> bytes:
    """The blob lh_kept_save writes for lh_kept_slide(add, sub) of rows [first, first + nrows): per row and bin A - S, with A / S
    the sums mod 2^64 of the add / sub blobs' cells; a difference of 0 is not listed; row_count is the add side's sum of
    row_count minus the sub side's, mod 2^64, samples the sum of those.  first=None: the first add blob's; nrows=None: up to
    the end of its block.  KeptUnderflow for a cell with S > A (decided on the wrapped sums): the lowest row, then the lowest
    bin.  ValueError for a blob that is not sound (check()), no add blob, or rows outside some blob's block."""
    add, sub = [bytes(b) for b in add_blobs], [bytes(b) for b in sub_blobs]
    if not add:
        raise ValueError("at least one add blob")
    for b in add + sub:
        bad = check(b)
        if bad:
            raise ValueError(f"not a kept blob: {CAUSES[bad[0]]} (row {bad[1]}, index {bad[2]})")
    A, S = [unpack(b) for b in add], [unpack(b) for b in sub]
    if first is None:
        first = A[0]["first"]
    if nrows is None:
        nrows = A[0]["first"] + A[0]["nrows"] - first
    if nrows < 1 or any(first < u["first"] or first + nrows > u["first"] + u["nrows"] for u in A + S):
        raise ValueError("rows [first, first + nrows) lie inside every blob's block, and there is at least one")
    (ca, ra), (cs, rs) = _side(A, first, nrows), _side(S, first, nrows)
    offsets, keys, counts, row_count = [0], [], [], []
    for m in range(nrows):
        under = [j for j, c in cs[m].items() if c > ca[m].get(j, 0)]        # (a bin the add side lacks counts as 0)
        if under:
            raise KeptUnderflow(first + m, ((min(under) ^ 0x8000) + 0x8000) % NKEYS - 0x8000)
        for j in sorted(ca[m]):
            d = ca[m][j] - cs[m].get(j, 0)
            if d:
                keys.append(j ^ 0x8000)
                counts.append(d)
        offsets.append(len(keys))
        row_count.append((ra[m] - rs[m]) & _M64)
    off, rc, c = np.array(offsets, dtype="<u8"), np.array(row_count, dtype="<u8"), np.array(counts, dtype="<u8")
    k = np.array(keys, dtype="<u2").view("<i2")
    return header(first, nrows, len(keys), sum(row_count) & _M64) + off.tobytes() + rc.tobytes() + c.tobytes() + k.tobytes()


NO_ROW = 0xffffffff                      # LH_KEPT_NO_ROW


def _permuted(u, line, first_out):
    """gather() of ONE blob, in whole-array NumPy: no cell changes, the rows' runs are copied (what a host did before
    lh_kept_gather: a permutation of the CSR arrays)."""
    r = np.asarray(line, dtype=np.int64)
    has = r != NO_ROW
    at = np.where(has, r - u["first"], 0)
    if ((at < 0) | (at >= u["nrows"])).any():
        raise ValueError("a row is neither NO_ROW nor inside its blob's block")
    off = u["offsets"].astype(np.int64)
    lo, ln = off[at], np.where(has, off[at + 1] - off[at], 0)
    new_off = np.concatenate(([0], np.cumsum(ln)))
    idx = np.repeat(lo - new_off[:-1], ln) + np.arange(int(new_off[-1]), dtype=np.int64)
    rc = np.where(has, u["row_count"][at], np.uint64(0)).astype("<u8")
    with np.errstate(over="ignore"):
        samples = int(rc.sum(dtype=np.uint64))
    return (header(first_out, r.size, idx.size, samples) + new_off.astype("<u8").tobytes() + rc.tobytes()
            + u["counts"][idx].astype("<u8").tobytes() + u["keys"][idx].astype("<i2").tobytes())


def gather(blobs, src, first_out: int = 0, *, checked: bool = True) -> bytes:
    """The blob lh_kept_save writes for lh_kept_gather(blobs, src, first_out): src is [len(blobs), n] (a 1-D map belongs to a single
    blob), src[i][j] the ABSOLUTE row of blob i that feeds output row first_out + j, NO_ROW: none.  Per output row and bin the sum
    mod 2^64 of the source rows' cells, a sum of 0 not listed, bins ascending; row_count the sum mod 2^64 of the source rows'
    row_count entries, samples the sum of those.  The same source row may feed several output rows and a blob may be listed
    several times.  ValueError for a blob that is not sound (check(); checked=False trusts blobs of one's own), no blob, a map of
    another shape or without a column, a row that is neither NO_ROW nor inside its blob's block, or first_out + n > 2^32.
    One blob is a permutation of rows and is done in whole arrays; several are summed cell by cell in Python integers."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("at least one blob")
    for b in blobs:
        bad = check(b) if checked else None
        if bad:
            raise ValueError(f"not a kept blob: {CAUSES[bad[0]]} (row {bad[1]}, index {bad[2]})")
    U = [unpack(b) for b in blobs]
    a = np.asarray(src)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[0] != len(U) or a.shape[1] < 1:
        raise ValueError("the map is [len(blobs), n] with n >= 1")
    n = a.shape[1]
    if first_out < 0 or first_out + n > 1 << 32:
        raise ValueError("rows [first_out, first_out + n) end at 2^32 at most")
    if len(U) == 1:
        return _permuted(U[0], a[0], first_out)
    rows = [[int(r) for r in line] for line in a.tolist()]
    offsets, keys, counts, row_count = [0], [], [], []
    for j in range(n):
        cells, rc = {}, 0
        for u, line in zip(U, rows):
            r = line[j]
            if r == NO_ROW:
                continue
            if not u["first"] <= r < u["first"] + u["nrows"]:
                raise ValueError(f"row {r} is neither NO_ROW nor inside its blob's block")
            at = r - u["first"]
            lo, hi = int(u["offsets"][at]), int(u["offsets"][at + 1])
            bins = (u["keys"][lo:hi].view("<u2") ^ np.uint16(0x8000)).tolist()
            for b, c in zip(bins, u["counts"][lo:hi].tolist()):
                cells[b] = (cells.get(b, 0) + c) & _M64
            rc = (rc + int(u["row_count"][at])) & _M64
        for b in sorted(cells):
            if cells[b]:
                keys.append(b ^ 0x8000)
                counts.append(cells[b])
        offsets.append(len(keys))
        row_count.append(rc)
    off, rcs, c = np.array(offsets, dtype="<u8"), np.array(row_count, dtype="<u8"), np.array(counts, dtype="<u8")
    k = np.array(keys, dtype="<u2").view("<i2")
    return header(first_out, n, len(keys), sum(row_count) & _M64) + off.tobytes() + rcs.tobytes() + c.tobytes() + k.tobytes()


def group(blobs, goff, members, first_out: int = 0, *, checked: bool = True) -> bytes:
    """The blob lh_kept_save writes for lh_kept_group(blobs, goff, members, first_out): a CSR of groups over ABSOLUTE row numbers,
    group g = members[goff[g]:goff[g + 1]], NO_ROW: nothing.  Output row first_out + g holds, per bin, the sum mod 2^64 over the
    blobs and over the group's members of the source rows' cells, a sum of 0 not listed, bins ascending; row_count the sum mod
    2^64 of the source rows' row_count entries, samples the sum of those.  A row may stand in several groups, and several times in
    one (it counts that often); a blob may be listed several times; an empty group gives an empty row.  ValueError for what the
    host form refuses: a blob that is not sound (check(); checked=False trusts blobs of one's own), no blob, no group, a goff
    that does not start at 0, decreases or does not end at len(members), a member that is neither NO_ROW nor inside EVERY blob's
    block, or first_out + ngroups > 2^32.  Summed cell by cell in Python integers."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("at least one blob")
    for b in blobs:
        bad = check(b) if checked else None
        if bad:
            raise ValueError(f"not a kept blob: {CAUSES[bad[0]]} (row {bad[1]}, index {bad[2]})")
    U = [unpack(b) for b in blobs]
    off = [int(x) for x in np.asarray(goff).ravel().tolist()]
    mem = [int(x) for x in np.asarray(members).ravel().tolist()]
    ngroups = len(off) - 1
    if ngroups < 1:
        raise ValueError("goff has ngroups + 1 >= 2 entries")
    if off[0] != 0 or off[-1] != len(mem) or any(b < a for a, b in zip(off[:-1], off[1:])):
        raise ValueError("goff starts at 0, never decreases and ends at len(members)")
    if first_out < 0 or first_out + ngroups > 1 << 32:
        raise ValueError("rows [first_out, first_out + ngroups) end at 2^32 at most")
    lo, end = max(u["first"] for u in U), min(u["first"] + u["nrows"] for u in U)
    for r in mem:
        if r != NO_ROW and not lo <= r < end:
            raise ValueError(f"row {r} is neither NO_ROW nor inside every blob's block")
    rows = {}                                            # (blob, row) -> (bins, counts, row_count), taken apart once

    def source(i, r):
        if (i, r) not in rows:
            u, at = U[i], r - U[i]["first"]
            a, b = int(u["offsets"][at]), int(u["offsets"][at + 1])
            rows[i, r] = ((u["keys"][a:b].view("<u2") ^ np.uint16(0x8000)).tolist(), u["counts"][a:b].tolist(), int(u["row_count"][at]))
        return rows[i, r]

    offsets, keys, counts, row_count = [0], [], [], []
    for g in range(ngroups):
        cells, rc = {}, 0
        for i in range(len(U)):
            for r in mem[off[g]:off[g + 1]]:
                if r == NO_ROW:
                    continue
                bins, cs, n = source(i, r)
                for b, c in zip(bins, cs):
                    cells[b] = (cells.get(b, 0) + c) & _M64
                rc = (rc + n) & _M64
        for b in sorted(cells):
            if cells[b]:
                keys.append(b ^ 0x8000)
                counts.append(cells[b])
        offsets.append(len(keys))
        row_count.append(rc)
    o, rcs, c = np.array(offsets, dtype="<u8"), np.array(row_count, dtype="<u8"), np.array(counts, dtype="<u8")
    k = np.array(keys, dtype="<u2").view("<i2")
    return header(first_out, ngroups, len(keys), sum(row_count) & _M64) + o.tobytes() + rcs.tobytes() + c.tobytes() + k.tobytes()


# ---- the names of a handle's rows: a sidecar beside the blob, whose format does not change --------------------------------------
NAMES_MAGIC = b"LHNAMES\n"
NAMES_VERSION = 1
_NAMES_HEAD = struct.Struct("<8sIIII")   # magic, version, first, count, reserved (0); then per name uint32 length + UTF-8 bytes


def pack_names(names, first: int = 0) -> bytes:
    """The names of rows [first, first + len(names)) of a handle -- Engine.metric_name's output, in row order -- as bytes to store
    beside its blob: a 24-byte little-endian header (magic, version, first, count, 0), then each name as a uint32 length and its
    UTF-8 bytes.  Pure data: nothing in the blob refers to it."""
    names = list(names)
    if not 0 <= first <= 0xffffffff or first + len(names) > 1 << 32:
        raise ValueError("rows [first, first + len(names)) end at 2^32 at most")
    out = [_NAMES_HEAD.pack(NAMES_MAGIC, NAMES_VERSION, first, len(names), 0)]
    for name in names:
        raw = name.encode("utf-8")
        out.append(struct.pack("<I", len(raw)) + raw)
    return b"".join(out)


def unpack_names(blob, with_first: bool = False):
    """pack_names back: the list of names (with_first: (names, first)).  ValueError for anything else: a wrong magic or version, a
    non-zero reserved word, a truncated or over-long blob, bytes that are not UTF-8."""
    b = bytes(blob)
    if len(b) < _NAMES_HEAD.size:
        raise ValueError("not a names sidecar: shorter than its header")
    magic, version, first, count, reserved = _NAMES_HEAD.unpack_from(b)
    if magic != NAMES_MAGIC:
        raise ValueError("not a names sidecar: bad magic")
    if version != NAMES_VERSION or reserved != 0 or first + count > 1 << 32:
        raise ValueError("not a names sidecar of version 1")
    at, names = _NAMES_HEAD.size, []
    for _ in range(count):
        if at + 4 > len(b):
            raise ValueError("names sidecar truncated")
        (ln,) = struct.unpack_from("<I", b, at)
        at += 4
        if at + ln > len(b):
            raise ValueError("names sidecar truncated")
        try:
            names.append(b[at:at + ln].decode("utf-8"))
        except UnicodeDecodeError as exc:
            raise ValueError("names sidecar: a name is not UTF-8") from exc
        at += ln
    if at != len(b):
        raise ValueError("names sidecar: bytes behind the last name")
    return (names, first) if with_first else names
