"""The blob of a kept interval (lh_kept_save* / lh_kept_load*, include/loghisto_gpu.h) in pure NumPy: no GPU, no library.

A 64-byte little-endian header, then the handle's single allocation verbatim:
    offsets uint64[nrows + 1] | row_count uint64[nrows] | counts uint64[cells] | keys int16[cells]

pack() makes a blob from CSR arrays, unpack() takes one apart, and check() restates every rule lh_kept_load* holds a blob
to -- the header's on the host, the block's on the device -- with the same verdict: of all violations the one of the lowest
row, in it the lowest index, there the lowest cause code.  The device's check is held to check() by the tests.
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
