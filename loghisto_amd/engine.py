"""Thin object wrapper over the C ABI: Engine (lh_engine) and Snapshot (lh_snapshot).

Nothing is computed here; every method is one or two calls into liblhgpu.so.
Reference counterparts are cited on the C declarations in include/loghisto_gpu.h.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _native as N


def _ptr(x) -> int:
    """Raw address of a torch tensor / numpy array / int."""
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    if isinstance(x, np.ndarray):
        return int(x.ctypes.data)
    raise TypeError(f"cannot take the address of {type(x)!r}")


def _stream_handle(stream) -> int:
    if stream is None:
        return 0
    if isinstance(stream, int):
        return stream
    if hasattr(stream, "cuda_stream"):  # torch.cuda.Stream
        return int(stream.cuda_stream)
    raise TypeError(f"not a stream: {type(stream)!r}")


def _out_arrays(out: dict, spec):
    """out= of _dict_call, a dict of per-name output arrays, against spec = (key, element width, elements or None:
    not measured) per output in the library's order -> (the library's pointer arguments, device form?)."""
    if not out or set(out) - {k for k, _, _ in spec}:
        raise ValueError("out holds some of " + ", ".join(k for k, _, _ in spec))
    device = [hasattr(t, "data_ptr") and getattr(t, "is_cuda", False) for t in out.values()]
    if any(device) != all(device):
        raise ValueError("out holds device tensors or host arrays, not both")
    args = []
    for k, width, n in spec:
        t = out.get(k)
        if t is not None and n is not None:
            if hasattr(t, "data_ptr"):
                ok = t.element_size() == width and int(t.numel()) == n and t.is_contiguous()
            else:
                ok = isinstance(t, np.ndarray) and t.itemsize == width and t.size == n and t.flags.c_contiguous
            if not ok:
                raise ValueError(f"out[{k!r}] holds {n} contiguous elements of {width} bytes")
        args.append(_ptr(t))
    return args, all(device)


def _id_list(ids):
    """ids of an *_ids call -> (what keeps the array alive, its address, n, device array?): a torch device tensor of 4-byte
    elements is handed over as it is, anything else becomes a contiguous uint32 host array."""
    if hasattr(ids, "data_ptr") and getattr(ids, "is_cuda", False):
        if ids.element_size() != 4 or not ids.is_contiguous():
            raise ValueError("device ids are contiguous 4-byte elements")
        return ids, int(ids.data_ptr()), int(ids.numel()), True
    a = np.asarray(ids.numpy() if hasattr(ids, "data_ptr") else ids)
    if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xffffffff):
        raise ValueError("ids are unsigned 32-bit integers")
    a = np.ascontiguousarray(a, dtype=np.uint32).ravel()
    return a, int(a.ctypes.data), int(a.size), False


# The outputs of a reader that returns a dict of per-name arrays, in the library's order: (key, element width, an element per
# name AND percentile -- or bound -- rather than one per name?, numpy dtype)
_SPREAD_OUT = (("count", 8, 0, np.uint64), ("sum", 8, 0, np.float64), ("m2", 8, 0, np.float64), ("pkeys", 2, 1, np.int16),
               ("pvalid", 1, 1, np.uint8), ("count_le", 8, 1, np.uint64), ("sum_le", 8, 1, np.float64))
_COMPARE_OUT = (("count_a", 8, 0, np.uint64), ("count_b", 8, 0, np.uint64), ("ks", 8, 0, np.float64), ("key", 2, 0, np.int16),
                ("below_a", 8, 0, np.uint64), ("below_b", 8, 0, np.uint64), ("w1", 8, 0, np.float64), ("shift", 8, 0, np.float64))
_KEPT_COUNT_LE_OUT = (("cum", 8, 1, np.uint64), ("total", 8, 0, np.uint64))


def _dict_call(fn, lead, spec, nmetrics, np_, out, device_ids=None, derive=None, table=None):
    """The out= protocol of the readers that return a dict of per-name arrays: library call `fn` (host form) or fn + "_device"
    with `lead`, every argument ahead of the outputs `spec` lists, for nmetrics names and np_ percentiles (or bounds).
    out: None (pinned arrays of this call's own), or a dict with some of spec's keys -> numpy arrays (the host form into them)
    or torch device tensors (the device form: returned as they are, dict(out)).  device_ids: whether an id list lies on the
    device, which the outputs then do too (None: there is none).  derive(res, table), if given, adds a host form's derived fields;
    table(): decompress() by bin."""
    L = N.lib()
    per_p = {k: c for k, _, c, _ in spec}
    if device_ids and out is None:
        raise ValueError("device ids go with an out= of device tensors")
    if out is not None:                                # (without percentiles the per-percentile arrays are not measured)
        args, device = _out_arrays(out, [(k, width, (nmetrics * np_ if np_ else None) if per_p[k] else nmetrics)
                                         for k, width, *_ in spec])
        if device_ids is not None and device != device_ids:
            raise ValueError("ids and out are both on the device or both on the host")
        if device:
            N.check(getattr(L, fn + "_device")(*lead, *args), fn + "_device")
            return dict(out)
        N.check(getattr(L, fn)(*lead, *args), fn)
        res = {k: (np.asarray(v) if not hasattr(v, "data_ptr") else v.numpy()) for k, v in out.items()
               if v is not None and (np_ or not per_p[k])}                                  # (... and not returned)
    else:
        import torch
        res = {}
        for k, width, _, dt in spec:                   # (a row more than an empty call needs: the arrays have addresses)
            n = max(nmetrics, 1) * (np_ if per_p[k] else 1)
            res[k] = torch.zeros((n * width,), dtype=torch.uint8, pin_memory=True).numpy().view(dt)
        N.check(getattr(L, fn)(*lead, *[res[k].ctypes.data if res[k].size else 0 for k, *_ in spec]), fn)
        res = {k: v[:nmetrics * (np_ if per_p[k] else 1)] for k, v in res.items()}
    res = {k: v.reshape((nmetrics, np_) if per_p[k] else (nmetrics,)) for k, v in res.items()}
    return derive(res, table) if derive else res


def _key_values(keys, table):
    """decompress(key) for an array of int16 keys; table(): decompress() by bin."""
    return table()[keys.view(np.int16).astype(np.int64) & 0xffff ^ 0x8000]


def _across_derived(res, table):
    """avg and pvals of across, where the arrays they come from were asked for."""
    if "sum" in res and "count" in res:
        with np.errstate(divide="ignore", invalid="ignore"):
            res["avg"] = res["sum"] / res["count"].view(np.uint64).astype(np.float64)
    if "pkeys" in res and "pvalid" in res:
        res["pvals"] = np.where(res["pvalid"] != 0, _key_values(res["pkeys"], table), np.nan)
    return res


def _spread_derived(res, table):
    """std, mean_le and upper of spread, where the arrays they come from were asked for."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if "m2" in res and "count" in res:
            res["std"] = np.sqrt(res["m2"] / res["count"].view(np.uint64).astype(np.float64))
        if "sum_le" in res and "count_le" in res:
            res["mean_le"] = res["sum_le"] / res["count_le"].view(np.uint64).astype(np.float64)
    if "pkeys" in res and "pvalid" in res:
        res["upper"] = np.where(res["pvalid"] != 0, _key_values(res["pkeys"], table), np.nan)
    return res


def _compare_derived(res, table):
    """ks_value of compare, where key was asked for."""
    if "key" in res:
        value = _key_values(res["key"], table)
        res["ks_value"] = np.where(np.isnan(res["ks"]), np.nan, value) if "ks" in res else value
    return res


class Snapshot:
    """One interval's cells, stolen at the epoch flip (metrics.go:460-463)."""

    def __init__(self, engine: "Engine", handle: int):
        self.engine = engine
        self._h = C.c_void_p(handle)

    def extract(self, percentiles: Sequence[float], nmetrics: Optional[int] = None, first: int = 0):
        """processHistograms for metrics [first, first+nmetrics) -> dict of numpy arrays."""
        L = N.lib()
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        p = np.ascontiguousarray(percentiles, dtype=np.float64)
        np_ = int(p.size)
        stats = (N.LhStats * max(nmetrics, 1))()
        pvals = np.zeros((nmetrics, np_), dtype=np.float64)
        pkeys = np.zeros((nmetrics, np_), dtype=np.int16)
        pvalid = np.zeros((nmetrics, np_), dtype=np.uint8)
        N.check(L.lh_extract_rows(self._h, first, nmetrics, p.ctypes.data_as(C.POINTER(C.c_double)), np_, stats,
                                  pvals.ctypes.data_as(C.POINTER(C.c_double)),
                                  pkeys.ctypes.data_as(C.POINTER(C.c_int16)),
                                  pvalid.ctypes.data_as(C.POINTER(C.c_uint8))), "lh_extract_rows")
        raw = np.frombuffer(stats, dtype=np.dtype([("count", "<u8"), ("sum", "<f8"), ("avg", "<f8"),
                                                   ("agg_sum_add", "<u8"), ("nbuckets", "<u4"),
                                                   ("present", "<u4")]), count=nmetrics).copy()
        return dict(count=raw["count"], sum=raw["sum"], avg=raw["avg"], agg_sum_add=raw["agg_sum_add"],
                    nbuckets=raw["nbuckets"], present=raw["present"], pvals=pvals, pkeys=pkeys, pvalid=pvalid)

    def extract_view(self, percentiles: Sequence[float], nmetrics: Optional[int] = None, first: int = 0):
        """extract() without the last copy: numpy views of the engine's pinned result buffer (lh_extract_rows_view).
        Valid until the next call that produces results on this engine, or release()."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        p = np.ascontiguousarray(percentiles, dtype=np.float64)
        v = N.LhExtractView()
        N.check(N.lib().lh_extract_rows_view(self._h, first, nmetrics, p.ctypes.data_as(C.POINTER(C.c_double)), int(p.size),
                                             C.byref(v)), "lh_extract_rows_view")
        dt = np.dtype([("count", "<u8"), ("sum", "<f8"), ("avg", "<f8"), ("agg_sum_add", "<u8"), ("nbuckets", "<u4"),
                       ("present", "<u4")])
        np_ = int(p.size)

        def arr(ptr, ctype, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((ctype * count).from_address(ptr), dtype=dtype, count=count)

        raw = arr(v.stats, C.c_uint8 * 40, nmetrics, dt)
        return dict(count=raw["count"], sum=raw["sum"], avg=raw["avg"], agg_sum_add=raw["agg_sum_add"],
                    nbuckets=raw["nbuckets"], present=raw["present"],
                    pvals=arr(v.pvals, C.c_double, nmetrics * np_, np.float64).reshape(nmetrics, np_),
                    pkeys=arr(v.pkeys, C.c_int16, nmetrics * np_, np.int16).reshape(nmetrics, np_),
                    pvalid=arr(v.pvalid, C.c_uint8, nmetrics * np_, np.uint8).reshape(nmetrics, np_))

    def extract_compact(self, percentiles: Sequence[float], nmetrics: Optional[int] = None, first: int = 0):
        """The compact form of extract_view (lh_extract_rows_compact): count, sum, nbuckets, the selected keys and one
        word of valid bits per metric -- 42 B per name at nine percentiles instead of 139 B.  numpy views of the engine's
        pinned result buffer, valid until the next call that produces results on this engine, or release().
        expand_compact() derives the full form on the host."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        p = np.ascontiguousarray(percentiles, dtype=np.float64)
        v = N.LhExtractCompact()
        N.check(N.lib().lh_extract_rows_compact(self._h, first, nmetrics, p.ctypes.data_as(C.POINTER(C.c_double)),
                                                int(p.size), C.byref(v)), "lh_extract_rows_compact")
        np_ = int(p.size)

        def arr(ptr, ctype, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((ctype * count).from_address(ptr), dtype=dtype, count=count)

        return dict(count=arr(v.count, C.c_uint64, nmetrics, np.uint64), sum=arr(v.sum, C.c_double, nmetrics, np.float64),
                    nbuckets=arr(v.nbuckets, C.c_uint32, nmetrics, np.uint32),
                    pvalid_bits=arr(v.pvalid_bits, C.c_uint32, nmetrics, np.uint32),
                    pkeys=arr(v.pkeys, C.c_int16, nmetrics * np_, np.int16).reshape(nmetrics, np_), _view=v)

    def expand_compact(self, compact: dict):
        """extract()'s dict from extract_compact()'s, derived on the host by lh_expand_compact (bit for bit what
        lh_extract_rows returns for the same snapshot)."""
        v = compact["_view"]
        n, np_ = int(v.nmetrics), int(v.np)
        stats = (N.LhStats * max(n, 1))()
        pvals = np.zeros((n, np_), dtype=np.float64)
        pkeys = np.zeros((n, np_), dtype=np.int16)
        pvalid = np.zeros((n, np_), dtype=np.uint8)
        N.check(N.lib().lh_expand_compact(self.engine._h, C.byref(v), stats, pvals.ctypes.data_as(C.POINTER(C.c_double)),
                                          pkeys.ctypes.data_as(C.POINTER(C.c_int16)),
                                          pvalid.ctypes.data_as(C.POINTER(C.c_uint8))), "lh_expand_compact")
        raw = np.frombuffer(stats, dtype=np.dtype([("count", "<u8"), ("sum", "<f8"), ("avg", "<f8"),
                                                   ("agg_sum_add", "<u8"), ("nbuckets", "<u4"),
                                                   ("present", "<u4")]), count=n).copy()
        return dict(count=raw["count"], sum=raw["sum"], avg=raw["avg"], agg_sum_add=raw["agg_sum_add"],
                    nbuckets=raw["nbuckets"], present=raw["present"], pvals=pvals, pkeys=pkeys, pvalid=pvalid)

    def buckets(self, metric_id: int):
        """Occupied (key, count) cells of one metric, ascending key."""
        L = N.lib()
        n = C.c_size_t(0)
        N.check(L.lh_buckets(self._h, metric_id, None, None, 0, C.byref(n)), "lh_buckets")
        keys = np.zeros(n.value, dtype=np.int16)
        counts = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            N.check(L.lh_buckets(self._h, metric_id, keys.ctypes.data_as(C.POINTER(C.c_int16)),
                                 counts.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)), "lh_buckets")
        return keys, counts

    def buckets_all(self, nmetrics: int, first: int = 0):
        """CSR listing of the occupied cells of metrics [first, first+nmetrics): (offsets, keys, counts)."""
        L = N.lib()
        offsets = np.zeros(nmetrics + 1, dtype=np.uint64)
        total = C.c_size_t(0)
        op = offsets.ctypes.data_as(C.POINTER(C.c_uint64))
        N.check(L.lh_buckets_all(self._h, first, nmetrics, op, None, None, 0, C.byref(total)), "lh_buckets_all")
        keys = np.zeros(total.value, dtype=np.int16)
        counts = np.zeros(total.value, dtype=np.uint64)
        if total.value:
            N.check(L.lh_buckets_all(self._h, first, nmetrics, op, keys.ctypes.data_as(C.POINTER(C.c_int16)),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint64)), total.value, C.byref(total)),
                    "lh_buckets_all")
        return offsets, keys, counts

    def serialize(self, percentiles, prefix: str, sep: str, suffix: str, underscore_to_dot: bool = False,
                  aggregates: bool = False, nmetrics: Optional[int] = None, first: int = 0) -> bytes:
        """K6: the interval's histogram keys as wire text, formatted on the device (lh_serialize).
        `percentiles` is the reference's label -> p mapping ({"%s_50": .5, ...}), in the order the keys
        should appear."""
        L = N.lib()
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        labels = list(percentiles.keys())
        p = np.ascontiguousarray([percentiles[k] for k in labels], dtype=np.float64)
        lab = (C.c_char_p * max(1, len(labels)))(*[k.encode() for k in labels])
        fmt = N.LhLineFormat(prefix.encode(), sep.encode(), suffix.encode(),
                             N.FMT_UNDERSCORE_TO_DOT if underscore_to_dot else 0, 0)
        flags = N.SER_AGGREGATES if aggregates else 0
        n = C.c_size_t(0)
        pp = p.ctypes.data_as(C.POINTER(C.c_double))
        rc = L.lh_serialize(self._h, first, nmetrics, pp, lab, len(labels), C.byref(fmt), flags, None, 0, C.byref(n))
        if rc != N.ERANGE:
            N.check(rc, "lh_serialize")
        if n.value == 0:
            return b""
        buf = C.create_string_buffer(n.value)
        rc = L.lh_serialize(self._h, first, nmetrics, pp, lab, len(labels), C.byref(fmt), flags, buf, n.value,
                            C.byref(n))
        if rc != N.ERANGE:
            N.check(rc, "lh_serialize")
        return buf.raw[:n.value]

    def counter_values(self, n: Optional[int] = None, first: int = 0):
        """Counters [first, first+n) of the interval (lh_counters_collect): dict(rate, present, total, known).
        rate = the interval's amounts of the names touched (metrics.go:430-433), total = lifetime store
        after the fold (metrics.go:435-458)."""
        if n is None:
            n = self.engine.num_counters() - first
        rate, total = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        present, known = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
        N.check(N.lib().lh_counters_collect(self._h, first, n, rate.ctypes.data_as(u64p), present.ctypes.data_as(u8p),
                                            total.ctypes.data_as(u64p), known.ctypes.data_as(u8p)), "lh_counters_collect")
        return dict(rate=rate, present=present.astype(bool), total=total, known=known.astype(bool))

    def serialize_counters(self, prefix: str, sep: str, suffix: str, underscore_to_dot: bool = False,
                           n: Optional[int] = None, first: int = 0) -> bytes:
        """"<name>" / "<name>_rate" wire lines of the counters, formatted on the device (lh_serialize_counters)."""
        L = N.lib()
        if n is None:
            n = self.engine.num_counters() - first
        fmt = N.LhLineFormat(prefix.encode(), sep.encode(), suffix.encode(),
                             N.FMT_UNDERSCORE_TO_DOT if underscore_to_dot else 0, 0)
        ln = C.c_size_t(0)
        N.check(L.lh_serialize_counters(self._h, first, n, C.byref(fmt), None, 0, C.byref(ln)), "lh_serialize_counters")
        if ln.value == 0:
            return b""
        buf = C.create_string_buffer(ln.value)
        N.check(L.lh_serialize_counters(self._h, first, n, C.byref(fmt), buf, ln.value, C.byref(ln)),
                "lh_serialize_counters")
        return buf.raw[:ln.value]

    def accumulate(self):
        """processHistograms' lifetime side effect (metrics.go:359-376), once per snapshot, in HBM."""
        N.check(N.lib().lh_snapshot_accumulate(self._h), "lh_snapshot_accumulate")

    def dense_row(self, metric_id: int) -> np.ndarray:
        """Dense uint64[65536] row (bin = key ^ 0x8000) rebuilt from lh_buckets."""
        keys, counts = self.buckets(metric_id)
        row = np.zeros(N.NKEYS, dtype=np.uint64)
        row[(keys.astype(np.int64) & 0xFFFF) ^ 0x8000] = counts
        return row

    @staticmethod
    def row_stride() -> int:
        """Cells from one device row to the next (lh_row_stride: more than 65 536)."""
        return int(N.lib().lh_row_stride())

    def device_rows(self):
        """(device pointer of row 0, nrows); row r starts row_stride() uint64 cells after row r - 1 and is 65 536 cells long."""
        p, n = C.c_void_p(0), C.c_uint32(0)
        N.check(N.lib().lh_snapshot_rows(self._h, C.byref(p), C.byref(n)), "lh_snapshot_rows")
        return int(p.value), int(n.value)

    def device_cells(self):
        """(device pointer of row 0, nrows, cell_bytes): the cells as they are (lh_snapshot_cells) -- uint32 on an engine of
        32-bit cells whose interval stayed below 2^32 samples; row r starts row_stride() * cell_bytes bytes after row r - 1."""
        p, n, cb = C.c_void_p(0), C.c_uint32(0), C.c_uint32(0)
        N.check(N.lib().lh_snapshot_cells(self._h, C.byref(p), C.byref(n), C.byref(cb)), "lh_snapshot_cells")
        return int(p.value), int(n.value), int(cb.value)

    def device_ranges(self) -> int:
        p = C.c_void_p(0)
        N.check(N.lib().lh_snapshot_ranges(self._h, C.byref(p)), "lh_snapshot_ranges")
        return int(p.value)

    def mark_dirty(self, first_row: int, nrows: int, lo_bin: int = 0, hi_bin: int = N.NKEYS - 1):
        N.check(N.lib().lh_snapshot_mark_dirty(self._h, first_row, nrows, lo_bin, hi_bin), "lh_snapshot_mark_dirty")

    # -- cells back in (RawMetricSet.Histograms, metrics.go:54-60; cells are an integer sum, metrics.go:278, 292) --------
    def add_buckets(self, ids, keys, counts):
        """snapshot[ids[i]][keys[i]] += counts[i] (lh_snapshot_add_buckets*): any order, duplicates add up, count 0 is
        skipped, all or nothing.  numpy arrays / sequences take the host form (copied before the call returns); torch
        device tensors (ids 4-byte, keys torch.int16, counts 8-byte) the device form, enqueued on the snapshot's stream."""
        L = N.lib()
        if hasattr(counts, "data_ptr"):
            if ids.element_size() != 4 or keys.element_size() != 2 or counts.element_size() != 8:
                raise TypeError("device form: ids are 4-byte, keys 2-byte and counts 8-byte tensors")
            n = int(counts.numel())
            if int(ids.numel()) != n or int(keys.numel()) != n:
                raise ValueError("ids, keys and counts differ in length")
            if not (ids.is_contiguous() and keys.is_contiguous() and counts.is_contiguous()):
                raise ValueError("device form: the tensors must be contiguous")
            N.check(L.lh_snapshot_add_buckets_device(self._h, _ptr(ids), _ptr(keys), _ptr(counts), n),
                    "lh_snapshot_add_buckets_device")
            return
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        k = np.ascontiguousarray(keys, dtype=np.int16)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if not (i.size == k.size == c.size):
            raise ValueError("ids, keys and counts differ in length")
        N.check(L.lh_snapshot_add_buckets(self._h, i.ctypes.data, k.ctypes.data, c.ctypes.data, c.size),
                "lh_snapshot_add_buckets")

    def add_buckets_csr(self, offsets, keys, counts, first: int = 0):
        """The inverse of buckets_all(): metric first + i gets keys / counts[offsets[i] .. offsets[i + 1])
        (lh_snapshot_add_buckets_csr*).  Accepts exactly what buckets_all() returns; torch device tensors (offsets and
        counts 8-byte, keys torch.int16) take the device form."""
        L = N.lib()
        if hasattr(counts, "data_ptr"):
            if offsets.element_size() != 8 or keys.element_size() != 2 or counts.element_size() != 8:
                raise TypeError("device form: offsets and counts are 8-byte tensors, keys 2-byte")
            if int(offsets.numel()) < 1 or int(keys.numel()) != int(counts.numel()):
                raise ValueError("offsets holds nmetrics + 1 entries; keys and counts are equally long")
            if not (offsets.is_contiguous() and keys.is_contiguous() and counts.is_contiguous()):
                raise ValueError("device form: the tensors must be contiguous")
            N.check(L.lh_snapshot_add_buckets_csr_device(self._h, first, int(offsets.numel()) - 1, _ptr(offsets), _ptr(keys),
                                                         _ptr(counts)), "lh_snapshot_add_buckets_csr_device")
            return
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        k = np.ascontiguousarray(keys, dtype=np.int16)
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if o.size < 1 or k.size != c.size:
            raise ValueError("offsets holds nmetrics + 1 entries; keys and counts are equally long")
        if o.size > 1 and int(o.max()) > c.size:
            raise ValueError("offsets point past the end of keys / counts")
        N.check(L.lh_snapshot_add_buckets_csr(self._h, first, o.size - 1, o.ctypes.data, k.ctypes.data, c.ctypes.data),
                "lh_snapshot_add_buckets_csr")

    def add_raw(self, raw):
        """A RawMetricSet.Histograms-shaped mapping, name -> (keys, counts): interns the names on the engine and adds
        the cells (add_buckets)."""
        ids, keys, counts = [], [], []
        for name, (k, c) in raw.items():
            k = np.ascontiguousarray(k, dtype=np.int16).ravel()
            c = np.ascontiguousarray(c, dtype=np.uint64).ravel()
            if k.size != c.size:
                raise ValueError(f"{name}: keys and counts differ in length")
            ids.append(np.full(k.size, self.engine.intern(name), dtype=np.uint32))
            keys.append(k)
            counts.append(c)
        if ids:
            self.add_buckets(np.concatenate(ids), np.concatenate(keys), np.concatenate(counts))

    # -- counts at or below given values (the running count of percentile()'s bucket walk, metrics.go:389-418) -----------
    def count_le(self, bounds, nmetrics: Optional[int] = None, first: int = 0, out=None):
        """dict(cum=uint64[nmetrics, nb], total=uint64[nmetrics]) for metrics [first, first+nmetrics) (lh_count_le*):
        cum[m, j] = samples of metric first + m whose bucket key is <= the key of bound j (bucket resolution), total[m] =
        all of them.  A 1-D `bounds` is shared by all names, a 2-D [nmetrics, nb] one holds a row per metric; every row is
        non-decreasing.  out=(cum, total) of contiguous 8-byte torch device tensors (either may be None) takes the device
        form: enqueued on the snapshot's stream, the tensors are returned as they are.  The host form's arrays are pinned
        host memory, so that the results arrive by one copy."""
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        if nmetrics is None:
            nmetrics = int(b.shape[0]) if b.ndim == 2 else self.engine.num_metrics() - first
        return self._count_le("lh_count_le", (first, nmetrics), nmetrics, b, out)

    def count_le_ids(self, ids, bounds, out=None):
        """count_le for the metrics `ids`, in that order (lh_count_le_ids*): row m of cum / total describes metric ids[m],
        and a 2-D `bounds` holds a row per entry of ids.  ids may repeat and come in any order.  A host list (anything
        numpy takes) is checked: an id the snapshot has no row for raises.  A torch device tensor of 4-byte ids goes with
        out=(cum, total) of device tensors (the device form): nothing comes back to the host, and an entry whose id is
        beyond the rows comes out as zeros."""
        keep, addr, n, device_ids = _id_list(ids)
        if device_ids != (out is not None):
            raise ValueError("device ids go with out= device tensors, host ids without out=")
        return self._count_le("lh_count_le_ids", (addr, n), n, np.ascontiguousarray(bounds, dtype=np.float64), out)

    def _count_le(self, fn, rows, nmetrics, b, out):
        """count_le / count_le_ids: library call `fn` (host form) or fn + "_device" over `rows`, its row arguments."""
        L = N.lib()
        if b.ndim == 2:
            flags, nb = N.LE_PER_METRIC, int(b.shape[1])
            if int(b.shape[0]) != nmetrics:
                raise ValueError("per-metric bounds hold one row per metric")
        elif b.ndim == 1:
            flags, nb = 0, int(b.size)
        else:
            raise ValueError("bounds are 1-D (shared) or 2-D [nmetrics, nb]")
        if out is not None:
            cum, total = out
            for t, n in ((cum, nmetrics * nb), (total, nmetrics)):
                if t is not None and (t.element_size() != 8 or int(t.numel()) != n or not t.is_contiguous()):
                    raise ValueError("device form: cum holds nmetrics * nb and total nmetrics contiguous 8-byte elements")
            N.check(getattr(L, fn + "_device")(self._h, *rows, b.ctypes.data, nb, flags, _ptr(cum), _ptr(total)), fn + "_device")
            return dict(cum=cum, total=total)
        import torch
        cum = torch.empty((nmetrics, nb), dtype=torch.int64, pin_memory=True).numpy().view(np.uint64)
        total = torch.empty((nmetrics,), dtype=torch.int64, pin_memory=True).numpy().view(np.uint64)
        N.check(getattr(L, fn)(self._h, *rows, b.ctypes.data, nb, flags, cum.ctypes.data, total.ctypes.data), fn)
        return dict(cum=cum, total=total)

    # -- spread and percentile-trimmed sums (the weighted walk of metrics.go:342-346, cut where percentile() cuts) --------
    _SPREAD_OUT = _SPREAD_OUT

    def spread(self, percentiles, nmetrics: Optional[int] = None, first: int = 0, out=None):
        """dict(count, sum, m2, std, pkeys, pvalid, count_le, sum_le, mean_le, upper) for metrics [first, first+nmetrics)
        (lh_spread*): count / sum as extract() has them, m2 = sum of count * (value - mean)^2 over the buckets, std =
        sqrt(m2 / count); per percentile the key lh_extract_rows selects, the samples (count_le) and their sum (sum_le) up to
        and including that bucket, mean_le = sum_le / count_le (statsd's mean_90) and upper = decompress(key) (upper_90).
        Bucket resolution, like count_le.  The mean of the tail above a percentile is (sum - sum_le) / (count - count_le).
        std, mean_le and upper are NaN where there is nothing to divide (an empty name, a percentile without a bucket).
        `percentiles` may be empty: moments only.
        out = a dict with any of count, sum, m2, pkeys, pvalid, count_le, sum_le -> contiguous arrays of nmetrics
        (the first three) or nmetrics * np elements of 8, 8, 8, 2, 1, 8, 8 bytes; outputs left out are not computed.
        torch device tensors take the device form: enqueued on the snapshot's stream, the tensors are returned as they are
        and nothing is derived.  numpy arrays (pinned ones receive their results by one copy) take the host form."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        return self._spread("lh_spread", (first, nmetrics), nmetrics, percentiles, out)

    def spread_ids(self, ids, percentiles, out=None):
        """spread for the metrics `ids`, in that order (lh_spread_ids*): row m of every array describes metric ids[m].  ids
        may repeat and come in any order.  A host list (anything numpy takes) is checked: an id the snapshot has no row
        for raises.  A torch device tensor of 4-byte ids goes with an `out` of device tensors (the device form): nothing
        comes back to the host, and an entry whose id is beyond the rows comes out as zeros."""
        keep, addr, n, device_ids = _id_list(ids)
        return self._spread("lh_spread_ids", (addr, n), n, percentiles, out, device_ids)

    def _spread(self, fn, rows, nmetrics, percentiles, out, device_ids=None):
        """spread / spread_ids: library call `fn` (host form) or fn + "_device" over `rows`, its row arguments.
        device_ids: whether an id list lies on the device, which the outputs then do too (None: there is none)."""
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        return _dict_call(fn, (self._h, *rows, p.ctypes.data, int(p.size)), _SPREAD_OUT, nmetrics, int(p.size), out, device_ids,
                          _spread_derived, self._decompress_table)

    def _decompress_table(self) -> np.ndarray:
        """decompress() by bin (the engine's codec_tables), fetched once per engine."""
        if getattr(self.engine, "_decompress_table", None) is None:
            self.engine._decompress_table = self.engine.codec_tables()[1]
        return self.engine._decompress_table

    def spread_lines(self, names: "Names", percentiles, prefix: str, sep: str, suffix: str, underscore_to_dot: bool = False,
                     nmetrics: Optional[int] = None, first: int = 0) -> bytes:
        """What statsd emits per name, as wire text formatted on the device: lh_spread_device into device tensors, then
        Names.lines over them on the snapshot's stream -- nothing but the text comes back to the host.  Per name with samples
        <name>_std = sqrt(m2 / count), then per percentile that has a bucket <name>_mean_<p> = sum_le / count_le,
        <name>_upper_<p> = decompress(key), <name>_count_<p> = count_le and <name>_sum_<p> = sum_le.  `percentiles` is a
        sequence of p (<p> is then 100 * p as %.10g prints it: 0.999 -> "99.9") or a mapping <p> text -> p."""
        import torch
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        tags = list(percentiles.keys()) if hasattr(percentiles, "keys") else ["%.10g" % (100.0 * float(p)) for p in percentiles]
        ps = [float(percentiles[t]) for t in tags] if hasattr(percentiles, "keys") else [float(p) for p in percentiles]
        np_ = len(ps)
        dev = torch.device("cuda", self.engine.device)
        if nmetrics == 0:
            return b""
        t = dict(count=torch.empty(nmetrics, dtype=torch.int64, device=dev), m2=torch.empty(nmetrics, dtype=torch.float64, device=dev))
        if np_:                                            # (lh_spread_device writes every element: nothing to clear)
            shape = (nmetrics, np_)
            t.update(pkeys=torch.empty(shape, dtype=torch.int16, device=dev), pvalid=torch.empty(shape, dtype=torch.uint8, device=dev),
                     count_le=torch.empty(shape, dtype=torch.int64, device=dev), sum_le=torch.empty(shape, dtype=torch.float64, device=dev))
        self._spread("lh_spread", (first, nmetrics), nmetrics, ps, t)
        cols = [dict(label="%s_std", a=t["m2"], b=t["count"], op="sqrt_ratio")]
        for i, tag in enumerate(tags):
            tag = tag.replace("%", "%%")
            v = t["pvalid"][:, i]
            cols += [dict(label="%s_mean_" + tag, a=t["sum_le"][:, i], b=t["count_le"][:, i], op="ratio", valid=v),
                     dict(label="%s_upper_" + tag, a=t["pkeys"][:, i], key=True, valid=v),
                     dict(label="%s_count_" + tag, a=t["count_le"][:, i], valid=v),
                     dict(label="%s_sum_" + tag, a=t["sum_le"][:, i], valid=v)]
        return names.lines(cols, n=nmetrics, first=first, row_count=t["count"], prefix=prefix, sep=sep, suffix=suffix,
                           underscore_to_dot=underscore_to_dot, stream=self.stream())

    # -- the k names that lead (a selection across names; what is ranked is what extract / count_le return) ---------------
    _TOP_BY = {"count": N.TOP_BY_COUNT, "sum": N.TOP_BY_SUM, "percentile": N.TOP_BY_PERCENTILE,
               "count_above": N.TOP_BY_COUNT_ABOVE}

    def top(self, k: int, by: str = "count", arg: Optional[float] = None, ascending: bool = False,
            nmetrics: Optional[int] = None, first: int = 0, out=None):
        """The k names of [first, first+nmetrics) that lead (lh_top*), as a structured array (dtype N.TOP_ENTRY: id, pkey,
        reserved, count, sum, above) of n_out = min(k, names with samples) entries, the leader first.  by = "count", "sum",
        "percentile" (arg = p in [0, 1]: ranked by the bucket extract() selects, whose key is `pkey`) or "count_above" (arg =
        a value: ranked by the samples in buckets above that value's, `above` -- count minus count_le's answer).  Descending
        score, or ascending with ascending=True; equal scores go lowest id first either way.  ids are absolute.
        out = a contiguous numpy array of at least k TOP_ENTRY elements takes the host form into it (its first n_out
        entries are written and returned as a view); out = (entries, n) of contiguous torch device tensors of at least
        k * 32 and 4 bytes takes the device form: enqueued on the snapshot's stream, the pair is returned as it is."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        return self._leaders("lh_top", (self._h,), self._TOP_BY, ("percentile", "count_above"), "TOP_ENTRY", k, by, arg,
                             N.TOP_ASCENDING if ascending else 0, nmetrics, first, out)

    @staticmethod
    def _leaders(fn, handles, by_codes, takes_arg, entry, k, by, arg, flags, nmetrics, first, out, stream=(), nwin=None):
        """top / movers, of a Snapshot or of a Kept: the k leaders of [first, first+nmetrics) from library call `fn` (host form)
        or fn + "_device", whose arguments begin with `handles` (a snapshot's handle or two; a list of kept handles and its
        length, or two; the per-window forms' list, length, windows and their number) and -- the kept readers' -- have `stream`
        = (its handle,) in front of the outputs.  by_codes: the names `by` takes -> the library's; takes_arg: those that need an
        arg; entry: the name of the entry dtype in N.  nwin: the windows of a per-window form, whose outputs hold nwin blocks of
        k entries and nwin counts and whose host form returns a list of nwin arrays, window w's of length n_out[w]."""
        L = N.lib()
        if by not in by_codes:
            raise ValueError("by is one of " + ", ".join(by_codes))
        if arg is None:
            if by in takes_arg:
                raise ValueError(f"by={by!r} takes an arg")
            arg = 0.0
        dtype = getattr(N, entry)
        blocks, per = (1, "") if nwin is None else (nwin, ", per window")
        lead = (*handles, first, nmetrics, by_codes[by], float(arg), k, flags, *stream)
        if isinstance(out, tuple):
            entries, n = out
            for t, need in ((entries, blocks * k * dtype.itemsize), (n, 4 * blocks)):
                if not t.is_contiguous() or t.element_size() * int(t.numel()) < need:
                    raise ValueError("device form: entries holds k * 32 contiguous bytes and n 4" + per)
            N.check(getattr(L, fn + "_device")(*lead, _ptr(entries), _ptr(n)), fn + "_device")
            return out
        if out is None:
            out = np.zeros(max(blocks * k, 1), dtype=dtype)
        elif not (isinstance(out, np.ndarray) and out.dtype == dtype and out.size >= blocks * k and out.flags.c_contiguous):
            raise ValueError(f"out holds at least k contiguous {entry} elements" + per)
        n = (C.c_size_t * max(blocks, 1))()
        N.check(getattr(L, fn)(*lead, out.ctypes.data, C.addressof(n)), fn)
        if nwin is None:
            return out.reshape(-1)[:n[0]]
        return [out.reshape(-1)[w * k:w * k + n[w]] for w in range(nwin)]

    # -- distribution shift against another snapshot (percentile()'s bucket walk, metrics.go:389-418, over two rows at once) --
    _COMPARE_OUT = _COMPARE_OUT

    def compare(self, base: "Snapshot", nmetrics: Optional[int] = None, first: int = 0, out=None):
        """How metrics [first, first+nmetrics) of THIS snapshot differ from the same names of `base` (lh_compare*), as a
        dict of numpy arrays: count_a / count_b (the totals in base / here), ks (the Kolmogorov-Smirnov distance of the two
        normalised distributions, its bin chosen in exact integers), key (the int16 key of that bin: the lowest at which
        the distance is reached), below_a / below_b (the inclusive prefix counts there), ks_value = decompress(key) from the
        engine's codec_tables, w1 (earth mover's distance in buckets: 100 buckets are one e-fold) and shift (the signed
        form: positive when this snapshot sits higher).  ks, w1, shift and ks_value are NaN for a name that is empty on
        either side; identical distributions give ks = 0 with key 0.  `base` may belong to another engine on the same
        device, and may be this snapshot.
        out = a dict with any of count_a, count_b, ks, key, below_a, below_b, w1, shift -> contiguous arrays of nmetrics
        elements of 8 bytes (key: 2); outputs left out are not computed.  torch device tensors take the device form:
        enqueued on this snapshot's stream (`base` must stay unreleased until that stream has passed the call), the
        tensors are returned as they are and nothing is derived.  numpy arrays take the host form."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        return _dict_call("lh_compare", (base._h, self._h, first, nmetrics, 0), _COMPARE_OUT, nmetrics, 0, out,
                          derive=_compare_derived, table=self._decompress_table)

    # -- the k names whose distribution moved most against another snapshot (compare's scores, top's selection) ------------
    _MOVERS_BY = {"ks": N.MOVERS_BY_KS, "w1": N.MOVERS_BY_W1, "shift": N.MOVERS_BY_SHIFT, "percentile": N.MOVERS_BY_PERCENTILE}

    def movers(self, base: "Snapshot", k: int, by: str = "ks", arg: Optional[float] = None, ascending: bool = False,
               nmetrics: Optional[int] = None, first: int = 0, out=None):
        """The k names of [first, first+nmetrics) whose distribution in THIS snapshot moved most against the same names of
        `base` (lh_movers*), as a structured array (dtype N.MOVER_ENTRY: id, key, key_base, count_a, count_b, score) of
        n_out = min(k, names with samples on both sides) entries, the leader first.  by = "ks", "w1" or "shift" (score = that
        output of compare(); for "ks" `key` is compare's key; "shift" ranks the signed value: descending gives the names
        that moved up most, ascending=True those that moved down most) or "percentile" (arg = p in [0, 1]: score = the
        number of buckets the bucket extract() selects for p moved, bin here minus bin in base -- 100 buckets are one e-fold;
        `key` / `key_base` are the two selected keys).  Equal scores go lowest id first either way.  ids are absolute.
        `base` may belong to another engine on the same device, and may be this snapshot.
        out = a contiguous numpy array of at least k MOVER_ENTRY elements takes the host form into it (its first n_out
        entries are written and returned as a view); out = (entries, n) of contiguous torch device tensors of at least
        k * 32 and 4 bytes takes the device form: enqueued on this snapshot's stream (`base` must stay unreleased until
        that stream has passed the call), the pair is returned as it is."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        return self._leaders("lh_movers", (base._h, self._h), self._MOVERS_BY, ("percentile",), "MOVER_ENTRY", k, by, arg,
                             N.MOVERS_ASCENDING if ascending else 0, nmetrics, first, out)

    # -- one name over several snapshots (the cells added up, then processHistograms' walks, metrics.go:342-346, 389-418) ---
    _ACROSS_OUT = (("count", 8, 0, np.uint64), ("sum", 8, 0, np.float64), ("nbuckets", 4, 0, np.uint32),
                   ("present_bits", 4, 0, np.uint32), ("pkeys", 2, 1, np.int16), ("pvalid", 1, 1, np.uint8))

    def across(self, earlier, percentiles, nmetrics: Optional[int] = None, first: int = 0, out=None):
        """dict(count, sum, avg, nbuckets, present_bits, pkeys, pvalid, pvals) for metrics [first, first+nmetrics) over the
        snapshots list(earlier) + [self] taken together (lh_across*, at most N.MAX_ACROSS of them): per name the cells of
        all of them are added up in 64 bits, and count, sum, nbuckets and the percentile keys are what extract() returns
        for a snapshot that holds those sums -- p99 over the last 10 intervals while emitting every interval.
        present_bits has bit i set where snapshot i of the list holds a sample of the name; avg = sum / count (NaN at 0);
        pvals = decompress(pkey) from the engine's codec_tables, NaN where the percentile has no bucket.  A snapshot may
        appear more than once and counts that often; the snapshots may belong to other engines on the same device.
        `percentiles` may be empty.  No snapshot is changed.
        out = a dict with any of count, sum, nbuckets, present_bits, pkeys, pvalid -> contiguous arrays of nmetrics (the
        first four) or nmetrics * np elements of 8, 8, 4, 4, 2, 1 bytes; outputs left out are not computed.  torch device
        tensors take the device form: enqueued on this snapshot's stream (the others must stay unreleased until that stream
        has passed the call), the tensors are returned as they are and nothing is derived.  numpy arrays (pinned ones
        receive their results by one copy) take the host form."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        return self._across("lh_across", earlier, (first, nmetrics), nmetrics, percentiles, out)

    def across_ids(self, ids, earlier, percentiles, out=None):
        """across for the metrics `ids`, in that order (lh_across_ids*): row m of every array describes metric ids[m] over
        list(earlier) + [self]; with earlier=() this is the compact extract of chosen names.  ids may repeat and come in
        any order.  A host list (anything numpy takes) is checked: an id that some snapshot of the list has no row for
        raises.  A torch device tensor of 4-byte ids -- the ids top(..., out=...) has just written, on the same stream --
        goes with an `out` of device tensors (the device form): nothing comes back to the host, and an entry whose id is
        beyond the rows of the shortest snapshot comes out as zeros."""
        keep, addr, n, device_ids = _id_list(ids)
        return self._across("lh_across_ids", earlier, (addr, n), n, percentiles, out, device_ids)

    def _across(self, fn, earlier, rows, nmetrics, percentiles, out, device_ids=None):
        """across / across_ids: library call `fn` (host form) or fn + "_device" over `rows`, its row arguments.
        device_ids: whether an id list lies on the device, which the outputs then do too (None: there is none)."""
        snaps = list(earlier) + [self]
        handles = (C.c_void_p * len(snaps))(*[s._h.value for s in snaps])
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        lead = (C.addressof(handles), len(snaps), *rows, p.ctypes.data, int(p.size), 0)
        return _dict_call(fn, lead, self._ACROSS_OUT, nmetrics, int(p.size), out, device_ids,
                          _across_derived, self._decompress_table)

    def keep(self, nmetrics: Optional[int] = None, first: int = 0) -> "Kept":
        """The occupied cells of metrics [first, first+nmetrics) in compact form, in device memory of their own (lh_keep): a
        Kept, which outlives this snapshot and the engine.  The snapshot is not changed."""
        if nmetrics is None:
            nmetrics = self.engine.num_metrics() - first
        h = C.c_void_p(0)
        N.check(N.lib().lh_keep(self._h, first, nmetrics, 0, C.byref(h)), "lh_keep")
        return Kept(h, self._decompress_table())

    def merge_rccl(self, comm: int, nranks: int, rank: int, nrows: int, plan: str = "allreduce"):
        """K4 through the C ABI: RCCL merge on the snapshot's stream (comm = ncclComm_t as int).
        Returns the [first, last) rows that hold merged data on this rank."""
        first, last = C.c_uint32(0), C.c_uint32(0)
        N.check(N.lib().lh_snapshot_merge(self._h, C.c_void_p(comm), nranks, rank,
                                          0 if plan == "allreduce" else 1, nrows, C.byref(first), C.byref(last)),
                "lh_snapshot_merge")
        return int(first.value), int(last.value)

    def merge_info(self) -> dict:
        """What the last merge moved (lh_snapshot_merge_info)."""
        mi = N.LhMergeInfo()
        N.check(N.lib().lh_snapshot_merge_info(self._h, C.byref(mi)), "lh_snapshot_merge_info")
        return {k: (float(getattr(mi, k)) if k.endswith("_ms") else int(getattr(mi, k)))
                for k, _ in N.LhMergeInfo._fields_ if k != "reserved"}

    def stream(self) -> int:
        p = C.c_void_p(0)
        N.check(N.lib().lh_snapshot_stream(self._h, C.byref(p)), "lh_snapshot_stream")
        return int(p.value or 0)

    def release(self):
        if self._h is not None and self._h.value:
            N.check(N.lib().lh_release(self._h), "lh_release")
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()


class Kept:
    """One interval's occupied cells of metrics [first, first + nrows), kept in compact form on the device (lh_kept):
    Snapshot.keep(), Kept.merge(), Kept.gather(), Kept.slide(), or -- with no engine at all -- Kept.from_bytes / load / from_device_blob of a saved one.  It
    depends on neither its snapshot nor its engine, and never changes."""

    _OUT = (("count", 8, 0, np.uint64), ("sum", 8, 0, np.float64), ("nbuckets", 4, 0, np.uint32),
            ("present_bits", 8, 0, np.uint64), ("pkeys", 2, 1, np.int16), ("pvalid", 1, 1, np.uint8))

    def __init__(self, handle: C.c_void_p, decompress_table: np.ndarray):
        self._h = handle
        self._table = decompress_table
        self.info = self._info()

    def _info(self) -> dict:
        ki = N.LhKeptInfo(struct_size=C.sizeof(N.LhKeptInfo))
        N.check(N.lib().lh_kept_info_get(self._h, C.byref(ki)), "lh_kept_info_get")
        return {k: int(getattr(ki, k)) for k, _ in N.LhKeptInfo._fields_ if k != "struct_size"}

    def arrays(self):
        """(offsets uint64[nrows + 1], keys int16[cells], counts uint64[cells], row_count uint64[nrows]) as torch device
        tensors that VIEW the handle's memory (8-byte integers come as torch.int64): no copy, valid until close().
        Exactly buckets_all() of the same rows, and each row's sum of cells."""
        import torch
        from .merge import _DeviceArray
        ptrs = [C.c_void_p(0) for _ in range(4)]
        N.check(N.lib().lh_kept_arrays(self._h, *[C.byref(p) for p in ptrs]), "lh_kept_arrays")
        dev = torch.device("cuda", self.info["device"])
        nrows, cells = self.info["nrows"], self.info["cells"]

        def view(p, n, typestr, dtype):
            if n == 0:
                return torch.empty(0, dtype=dtype, device=dev)
            return torch.as_tensor(_DeviceArray(int(p.value), (n,), typestr), device=dev)

        return (view(ptrs[0], nrows + 1, "<i8", torch.int64), view(ptrs[1], cells, "<i2", torch.int16),
                view(ptrs[2], cells, "<i8", torch.int64), view(ptrs[3], nrows, "<i8", torch.int64))

    def add_to(self, snapshot: Snapshot):
        """The kept cells added to `snapshot` (rows first .. first + nrows), on its stream: lh_snapshot_add_buckets_csr_device
        with the handle's own arrays.  The handle may be closed at once: close() waits for the import (lh_kept_hold)."""
        offsets, keys, counts, _ = self.arrays()
        snapshot.add_buckets_csr(offsets, keys, counts, first=self.info["first"])
        N.check(N.lib().lh_kept_hold(self._h, snapshot.stream()), "lh_kept_hold")

    # -- what the readers and merge share: the handle lists, the block's defaults, the leading arguments ----------------------
    @staticmethod
    def _handles(kept):
        """-> (the handles of `kept` as the library takes a list, its length).  The caller holds on to the array until the
        library call has returned."""
        return (C.c_void_p * max(len(kept), 1))(*[k._h.value for k in kept]), len(kept)

    def _list(self, earlier):
        """list(earlier) + [self] -> (list, nkept)"""
        return self._handles(list(earlier) + [self])

    def _pair(self, base, earlier):
        """`base`, a Kept or a sequence of them, and list(earlier) + [self] -> (base, nbase, cur, ncur)"""
        return (*self._handles([base] if isinstance(base, Kept) else list(base)), *self._list(earlier))

    def _block(self, nmetrics, first):
        """first=None: this handle's first; nmetrics=None: up to the end of this handle's block."""
        if first is None:
            first = self.info["first"]
        if nmetrics is None:
            nmetrics = self.info["first"] + self.info["nrows"] - first
        return nmetrics, first

    def _decompress_table(self) -> np.ndarray:
        return self._table

    def _list_rows(self, lists, fn, nmetrics, first, ids):
        """The leading arguments of a reader over `lists`, _list's or _pair's: -> (what keeps the arrays alive, library call,
        (list, nkept, [list, nkept,] rows ...), nmetrics, device ids? or None)."""
        heads = tuple(x if isinstance(x, int) else C.addressof(x) for x in lists)
        if ids is not None:
            keep, addr, nmetrics, device_ids = _id_list(ids)
            return (lists, keep), fn + "_ids", (*heads, addr, nmetrics), nmetrics, device_ids
        nmetrics, first = self._block(nmetrics, first)
        return (lists,), fn, (*heads, first, nmetrics), nmetrics, None

    def across(self, earlier, percentiles, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Snapshot.across over kept intervals: dict(count, sum, avg, nbuckets, present_bits, pkeys, pvalid, pvals) for metrics
        [first, first+nmetrics) -- or, with ids=, for the metrics `ids` in that order -- over list(earlier) + [self] taken
        together (lh_kept_across*, at most N.MAX_KEPT handles; one may appear more than once and counts that often).  first
        and ids are metric ids; every handle of the list must hold them.  nmetrics=None: up to the end of this handle's block.
        present_bits is uint64.  out= as for Snapshot.across (present_bits 8 bytes); torch device tensors take the device form,
        enqueued on `stream` (a torch stream or a raw handle; None: the null stream), and device ids go with them."""
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        alive, fn, rows, nmetrics, device_ids = self._list_rows(self._list(earlier), "lh_kept_across", nmetrics, first, ids)
        lead = (*rows, p.ctypes.data, int(p.size), 0, _stream_handle(stream))
        return _dict_call(fn, lead, self._OUT, nmetrics, int(p.size), out, device_ids,
                          _across_derived, self._decompress_table)

    def merge(self, earlier=(), nmetrics: Optional[int] = None, first: Optional[int] = None, stream=None) -> "Kept":
        """list(earlier) + [self] rolled up into ONE new Kept of metrics [first, first+nmetrics) (lh_kept_merge): per metric the
        union of the handles' bins with their counts summed in 64 bits -- what Snapshot.keep would give had the samples arrived
        in one interval.  A handle listed twice counts twice; every handle of the list must hold the block.  first=None: this
        handle's first; nmetrics=None: up to the end of this handle's block.  The work goes on `stream` (a torch stream or a
        raw handle; None: the null stream) and is complete on return; the new handle depends on none of the listed ones."""
        nmetrics, first = self._block(nmetrics, first)
        handles, nkept = self._list(earlier)
        h = C.c_void_p(0)
        N.check(N.lib().lh_kept_merge(C.addressof(handles), nkept, first, nmetrics, 0, _stream_handle(stream), C.byref(h)),
                "lh_kept_merge")
        return Kept(h, self._table)

    def gather(self, src, earlier=(), first: int = 0, stream=None) -> "Kept":
        """Rows re-mapped per handle and summed into ONE new Kept of metrics [first, first + n) (lh_kept_gather*): over
        list(earlier) + [self], `src` is [nkept, n] and src[i, j] is the metric id (absolute, as ids are everywhere) of handle i
        that feeds metric first + j of the result; N.KEPT_NO_ROW: handle i has nothing for it.  Per metric and bin the counts are
        summed in 64 bits -- what merge() gives once every handle speaks of the same names: handles of other processes, of the
        time before a restart (loghisto_amd.fleet.union_names builds src from their name lists).  A source metric may feed
        several results and a handle may be listed several times.  A uint32 host array (a 1-D one is the map of a single handle)
        takes the host form, where a metric outside its handle's block is LH_ERANGE; a torch device tensor of 4-byte elements the
        device form, where such a metric counts as KEPT_NO_ROW.  The work goes on `stream` (a torch stream or a raw handle; None:
        the null stream) and is complete on return; the new handle depends on none of the listed ones."""
        handles, nkept = self._list(earlier)
        if hasattr(src, "data_ptr") and getattr(src, "is_cuda", False):
            if src.element_size() != 4 or not src.is_contiguous():
                raise ValueError("a device map holds contiguous 4-byte elements")
            shape, addr, fn = tuple(src.shape), int(src.data_ptr()), "lh_kept_gather_device"
        else:
            a = np.asarray(src.numpy() if hasattr(src, "data_ptr") else src)
            if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xffffffff):
                raise ValueError("the map holds unsigned 32-bit integers")
            src = np.ascontiguousarray(a, dtype=np.uint32)
            shape, addr, fn = src.shape, int(src.ctypes.data), "lh_kept_gather"
        if len(shape) == 1:
            shape = (1, shape[0])
        if len(shape) != 2 or shape[0] != nkept:
            raise ValueError(f"the map is [{nkept}, n]: a row per listed handle")
        h = C.c_void_p(0)
        N.check(getattr(N.lib(), fn)(C.addressof(handles), nkept, addr, shape[1], first, 0, _stream_handle(stream), C.byref(h)), fn)
        return Kept(h, self._table)

    def group(self, groups, earlier=(), first: int = 0, stream=None) -> "Kept":
        """Many metrics summed into one, by group (lh_kept_group*): ONE new Kept of metrics [first, first + ngroups) whose metric
        first + g holds, per bin, the 64-bit sum over list(earlier) + [self] and over the members of group g -- the roll-up of a
        service over its endpoints, of "everything" beside them (loghisto_amd.fleet.group_names builds the groups from names).
        `groups` is a sequence of sequences of metric ids (absolute, as ids are everywhere; N.KEPT_NO_ROW: nothing), or a
        (goff, members) pair of arrays, a CSR: group g has members[goff[g]:goff[g + 1]].  A metric may stand in several groups,
        and several times in one: it counts that often.  There is no limit on a group's size.  Host arrays take the host form,
        where a member outside some handle's block is LH_ERANGE and a goff that is no CSR over members LH_EINVAL; a pair of torch
        device tensors (goff of 8-byte, members of 4-byte elements) the device form, where goff is clamped to the members and a
        member outside a handle's block counts as nothing for that handle alone.  The work goes on `stream` and is complete on
        return; the new handle depends on none of the listed ones."""
        handles, nkept = self._list(earlier)
        pair = isinstance(groups, tuple) and len(groups) == 2 and all(hasattr(x, "shape") for x in groups)
        if pair and any(hasattr(x, "data_ptr") and getattr(x, "is_cuda", False) for x in groups):
            goff, members = groups
            if not all(hasattr(x, "data_ptr") and x.is_cuda and x.is_contiguous() and x.dim() == 1 for x in groups):
                raise ValueError("the device form takes two contiguous 1-D device tensors")
            if goff.element_size() != 8 or members.element_size() != 4 or goff.numel() < 2:
                raise ValueError("goff holds ngroups + 1 >= 2 8-byte elements, members 4-byte elements")
            ngroups, nmembers, fn = goff.numel() - 1, members.numel(), "lh_kept_group_device"
            addrs = (int(goff.data_ptr()), int(members.data_ptr()) if nmembers else 0)
        else:
            if pair:
                goff, members = (np.asarray(x.numpy() if hasattr(x, "data_ptr") else x).ravel() for x in groups)
            else:
                rows = [np.asarray(g).ravel() for g in groups]
                rows = [r if r.size else r.astype(np.uint32) for r in rows]   # (an empty group has no integers to show)
                goff = np.cumsum([0] + [r.size for r in rows])
                members = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint32)
            for a, top, what in ((goff, (1 << 64) - 1, "goff holds unsigned 64-bit integers"),
                                 (members, 0xffffffff, "members are unsigned 32-bit integers")):
                if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > top):
                    raise ValueError(what)
            if goff.size < 2:
                raise ValueError("at least one group")
            goff, members = np.ascontiguousarray(goff, dtype=np.uint64), np.ascontiguousarray(members, dtype=np.uint32)
            ngroups, nmembers, fn = goff.size - 1, members.size, "lh_kept_group"
            addrs = (int(goff.ctypes.data), int(members.ctypes.data) if nmembers else 0)
        h = C.c_void_p(0)
        N.check(getattr(N.lib(), fn)(C.addressof(handles), nkept, *addrs, nmembers, ngroups, first, 0, _stream_handle(stream), C.byref(h)), fn)
        return Kept(h, self._table)

    def slide(self, add=(), sub=(), nmetrics: Optional[int] = None, first: Optional[int] = None, stream=None) -> "Kept":
        """A rolling window advanced exactly (lh_kept_slide): ONE new Kept of metrics [first, first+nmetrics) that holds, per
        metric and bin, the 64-bit sum over [self] + list(add) minus the sum over list(sub) -- with self the window so far,
        add the newest interval and sub the oldest, bit for bit what merge() of the new window's intervals gives.  sub=(): plain
        merge.  A handle may appear several times and on both sides; at most N.MAX_KEPT in the two lists together; every one
        must hold the block.  A cell that would go below zero raises loghisto_amd.KeptUnderflow with the row (a metric id) and
        key of the lowest such row's lowest bin, and nothing is made.  first / nmetrics / stream as for merge; complete on
        return, and the new handle depends on none of the listed ones."""
        from .keptfile import KeptUnderflow
        nmetrics, first = self._block(nmetrics, first)
        plus, nadd = self._handles([self] + list(add))
        minus, nsub = self._handles(list(sub))
        why = N.LhKeptUnder(struct_size=C.sizeof(N.LhKeptUnder), reserved1=1)
        h = C.c_void_p(0)
        rc = N.lib().lh_kept_slide(C.addressof(plus), nadd, C.addressof(minus) if nsub else None, nsub, first, nmetrics, 0,
                                   _stream_handle(stream), C.byref(why), C.byref(h))
        if rc == N.ERANGE and why.reserved1 == 0:      # written, as 0, by an underflow refusal only
            raise KeptUnderflow(int(why.row), int(why.key))
        N.check(rc, "lh_kept_slide")
        return Kept(h, self._table)

    def compare(self, base, nmetrics: Optional[int] = None, first: int = 0, earlier=(), ids=None, stream=None, out=None):
        """Snapshot.compare over kept intervals (lh_kept_compare*): how metrics [first, first+nmetrics) -- or, with ids=, the
        metrics `ids` in that order -- of list(earlier) + [self] taken together differ from the same names of `base`, a Kept or
        a sequence of them taken together.  The same dict: count_a / count_b (base / here), ks, key, below_a, below_b,
        ks_value, w1, shift, with NaN for a name that is empty on either side.  At most N.MAX_KEPT handles in the two lists
        together; one may appear more than once, and in both lists.  first and ids are metric ids; every handle must hold
        them.  nmetrics=None: up to the end of this handle's block.  out= as for Snapshot.compare; torch device tensors take
        the device form, enqueued on `stream` (a torch stream or a raw handle; None: the null stream), and device ids go with
        them.  Every handle may be closed right afterwards: close() waits."""
        alive, fn, rows, nmetrics, device_ids = self._list_rows(self._pair(base, earlier), "lh_kept_compare", nmetrics, first, ids)
        return _dict_call(fn, (*rows, 0, _stream_handle(stream)), _COMPARE_OUT, nmetrics, 0, out, device_ids,
                          _compare_derived, self._decompress_table)

    def count_le(self, bounds, earlier=(), nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Snapshot.count_le over kept intervals (lh_kept_count_le*): dict(cum=uint64[nmetrics, nb], total=uint64[nmetrics]) for
        metrics [first, first+nmetrics) -- or, with ids=, for the metrics `ids` in that order -- over list(earlier) + [self] taken
        together: cum[m, j] = the samples whose bucket key is <= the key of bound j, total[m] = all of them, both exact and
        wrapping past 2^64.  `bounds` is 1-D, non-decreasing and shared by all names (a row per name is not supported over
        handles).  first and ids are metric ids; every handle must hold them.  out= a dict with cum and / or total, as for
        Kept.across: torch device tensors take the device form, enqueued on `stream` (a torch stream or a raw handle; None: the
        null stream), and device ids go with them; every handle may be closed right afterwards: close() waits."""
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        if b.ndim != 1:
            raise ValueError("bounds over kept intervals are 1-D: one row shared by all names")
        alive, fn, rows, nmetrics, device_ids = self._list_rows(self._list(earlier), "lh_kept_count_le", nmetrics, first, ids)
        lead = (*rows, b.ctypes.data, int(b.size), 0, _stream_handle(stream))
        return _dict_call(fn, lead, _KEPT_COUNT_LE_OUT, nmetrics, int(b.size), out, device_ids)

    def spread(self, percentiles, earlier=(), nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None, stream=None):
        """Snapshot.spread over kept intervals (lh_kept_spread*): the same dict -- count, sum, m2, std, pkeys, pvalid, count_le,
        sum_le, mean_le, upper -- for metrics [first, first+nmetrics) -- or, with ids=, for the metrics `ids` in that order --
        over list(earlier) + [self] taken together.  `percentiles` may be empty: moments only.  first and ids are metric ids;
        every handle must hold them.  out= as for Snapshot.spread; torch device tensors take the device form, enqueued on
        `stream` (a torch stream or a raw handle; None: the null stream), nothing is derived, and device ids go with them;
        every handle may be closed right afterwards: close() waits."""
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        alive, fn, rows, nmetrics, device_ids = self._list_rows(self._list(earlier), "lh_kept_spread", nmetrics, first, ids)
        lead = (*rows, p.ctypes.data, int(p.size), 0, _stream_handle(stream))
        return _dict_call(fn, lead, _SPREAD_OUT, nmetrics, int(p.size), out, device_ids,
                          _spread_derived, self._decompress_table)

    # -- across and count_le per WINDOW of the list, in one call (lh_kept_series* / lh_kept_heat*) ---------------------------------
    @staticmethod
    def _windows(windows, nkept):
        """windows of series / heat -> (the library's array of 2 * nwin uint32, nwin); None: one window per handle."""
        pairs = [(i, i + 1) for i in range(nkept)] if windows is None else [(int(lo), int(hi)) for lo, hi in windows]
        if any(not 0 <= v <= 0xffffffff for pair in pairs for v in pair):
            raise ValueError("a window is a pair (lo, hi) of list positions")
        return (C.c_uint32 * max(2 * len(pairs), 1))(*[v for pair in pairs for v in pair]), len(pairs)

    def _windowed(self, fn, earlier, windows, nmetrics, first, ids, tail, spec, per, out, derive=None, make=None):
        """The call of a per-window reader through _list_rows / _dict_call: nwin * n entries, window-major, which a host form's
        arrays then show as a leading window axis.  make(windows, nkept) -> (the library's array, nwin); None: _windows."""
        handles, nkept = self._list(earlier)
        win, nwin = (make or self._windows)(windows, nkept)
        alive, fn, rows, n, device_ids = self._list_rows((handles, nkept, win, nwin), fn, nmetrics, first, ids)
        res = _dict_call(fn, (*rows, *tail), spec, nwin * n, per, out, device_ids, derive, self._decompress_table)
        if out is not None and any(hasattr(t, "data_ptr") and getattr(t, "is_cuda", False) for t in out.values()):
            return res                                 # the device form: the caller's tensors as they are
        return {k: v.reshape((nwin, n) + v.shape[1:]) for k, v in res.items()}

    def series(self, percentiles, earlier=(), windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None,
               stream=None):
        """Kept.across per WINDOW of list(earlier) + [self], in one call (lh_kept_series*): `windows` is a sequence of (lo, hi)
        pairs, window w the handles [lo, hi) of the list (0 <= lo < hi <= its length; they may overlap, repeat and come in any
        order; at most N.MAX_WINDOWS), None: one window per handle -- the p99 of each of the last 60 seconds.  Returns
        Kept.across's dict with a leading window axis -- count[nwin, n], pkeys[nwin, n, np], and the derived avg / pvals --
        where block w is byte for byte what across() over that slice returns, but for present_bits, whose bit i means handle i
        of the WHOLE list.  out= and device tensors follow Kept.across's rules, with nwin * n (* np) elements, window-major."""
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        tail = (p.ctypes.data, int(p.size), 0, _stream_handle(stream))
        return self._windowed("lh_kept_series", earlier, windows, nmetrics, first, ids, tail, self._OUT, int(p.size), out,
                              _across_derived)

    def heat(self, bounds, earlier=(), windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None,
             stream=None):
        """Kept.count_le per WINDOW of list(earlier) + [self], in one call (lh_kept_heat*): dict(cum=uint64[nwin, n, nb],
        total=uint64[nwin, n]), block w byte for byte what count_le() over the handles [lo, hi) of window w returns -- a
        latency heat map, counts per `le` band per second.  windows, out= and device tensors as for Kept.series."""
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        if b.ndim != 1:
            raise ValueError("bounds over kept intervals are 1-D: one row shared by all names")
        tail = (b.ctypes.data, int(b.size), 0, _stream_handle(stream))
        return self._windowed("lh_kept_heat", earlier, windows, nmetrics, first, ids, tail, _KEPT_COUNT_LE_OUT, int(b.size), out)

    # -- bounds PER NAME per window, and the burn-rate alert over them (lh_kept_slo* / lh_kept_burn*) --------------------------------
    def _entries(self, nmetrics, first, ids):
        """the entries of a call: len(ids), or nmetrics (None: up to the end of this handle's block)"""
        if ids is not None:
            return int(ids.numel()) if hasattr(ids, "numel") else int(np.asarray(ids).size)
        return self._block(nmetrics, first)[0]

    @staticmethod
    def _per_entry(arrays, n, width_of):
        """The per-entry float64 arrays of slo / burn, name -> array, n entries each -> (what keeps them alive, their addresses,
        the trailing width of the first, device arrays?).  Torch device tensors are handed over as they are (all of them or none),
        anything else becomes a contiguous float64 host array.  width_of(shape) -> the elements an entry has, or None: refused."""
        device = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in arrays.values()]
        if any(device) != all(device):
            raise ValueError(" and ".join(arrays) + " are device tensors or host arrays, not both")
        keep, widths = [], []
        for name, a in arrays.items():
            if not device[0]:
                a = np.ascontiguousarray(a.numpy() if hasattr(a, "data_ptr") else a, dtype=np.float64)
            elif a.element_size() != 8 or not a.is_floating_point() or not a.is_contiguous():
                raise ValueError(f"device {name} are contiguous float64")
            width = width_of(tuple(a.shape))
            if width is None or (len(a.shape) and int(a.shape[0]) != n) or (not len(a.shape)):
                raise ValueError(f"{name} holds one entry per name: {n}")
            keep.append(a)
            widths.append(width)
        return keep, [_ptr(a) for a in keep], widths[0], device[0]

    def slo(self, bounds, earlier=(), windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None,
            stream=None):
        """Kept.heat with a row of bounds PER NAME, in one call (lh_kept_slo*) -- every endpoint's own SLO threshold over each
        window of the history: `bounds` has shape (n,) or (n, nb), row m for metric first + m or ids[m].  Returns
        dict(cum=uint64[nwin, n, nb], total=uint64[nwin, n]), entry (w, m) byte for byte what heat(ids=[id of m], bounds=row m)
        returns for window w.  Host rows are non-decreasing and free of NaN.  A torch device tensor for `bounds` takes the device
        form, which goes with an out= of device tensors (and device ids, if any): a device row is answered bound by bound, a NaN
        takes in nothing.  windows, nmetrics, first, ids, out= and stream as for Kept.heat."""
        n = self._entries(nmetrics, first, ids)
        keep, (addr,), nb, device = self._per_entry({"bounds": bounds}, n, lambda s: 1 if len(s) == 1 else s[1] if len(s) == 2 else None)
        if device and out is None:
            raise ValueError("device bounds go with an out= of device tensors")
        if out is not None and device != any(getattr(t, "is_cuda", False) for t in out.values()):
            raise ValueError("bounds and out are both on the device or both on the host")
        tail = (addr, nb, 0, _stream_handle(stream))
        return self._windowed("lh_kept_slo", earlier, windows, nmetrics, first, ids, tail, _KEPT_COUNT_LE_OUT, nb, out)

    def burn(self, bounds, budget, rates, k: int, earlier=(), windows=None, nmetrics: Optional[int] = None, first: int = 0,
             ids=None, counts: bool = False, out=None, stream=None):
        """The multi-window burn-rate alert over kept intervals (lh_kept_burn*): the names whose bad fraction -- the samples above
        their own bound, `bounds[m]`, over all their samples -- exceeds rates[w] * budget[m] in EVERY window w of the call
        (loghisto_amd.burn_fires is the rule; strictly above, a name with no sample in a window does not fire).  `windows` as for
        Kept.series, `rates` one per window.  Returns dict(entry=uint32[min(n, k)], row=uint32[...], n=int): the reported entries
        in ascending m -- entry m, row its metric id -- the first k of them, and how many there are whatever k is (k=0 only
        counts).  counts=True adds cum=uint64[nwin, n] and total=uint64[nwin, n], Kept.slo's for the one bound a name.
        Torch device tensors for `bounds` and `budget` take the device form, enqueued on `stream`: out= is then a dict of device
        tensors -- hits (at least k * 8 bytes), n (8 bytes), and optionally cum and total (nwin * n * 8 bytes each) -- which is
        returned as it is; device ids go with it."""
        L = N.lib()
        k = int(k)
        n = self._entries(nmetrics, first, ids)
        keep, (b_addr, g_addr), _, device = self._per_entry({"bounds": bounds, "budget": budget}, n, lambda s: 1 if len(s) == 1 else None)
        handles, nkept = self._list(earlier)
        win, nwin = self._windows(windows, nkept)
        r = np.ascontiguousarray(rates, dtype=np.float64).ravel()
        if int(r.size) != nwin:
            raise ValueError(f"rates holds one rate per window: {nwin}")
        alive, fn, rows, n, device_ids = self._list_rows((handles, nkept, win, nwin), "lh_kept_burn", nmetrics, first, ids)
        if device_ids is not None and device_ids != device:
            raise ValueError("ids, bounds and budget are all on the device or all on the host")
        lead = (*rows, r.ctypes.data, b_addr, g_addr, k, 0, _stream_handle(stream))
        if device:
            if not isinstance(out, dict) or set(out) - {"hits", "n", "cum", "total"} or "n" not in out or (k and "hits" not in out):
                raise ValueError("device form: out holds device tensors hits, n and optionally cum, total")
            need = {"hits": k * 8, "n": 8, "cum": nwin * n * 8, "total": nwin * n * 8}
            for key, t in out.items():
                if not getattr(t, "is_cuda", False) or not t.is_contiguous() or t.element_size() * int(t.numel()) < need[key]:
                    raise ValueError(f"device form: out[{key!r}] is a contiguous device tensor of at least {need[key]} bytes")
            N.check(getattr(L, fn + "_device")(*lead, _ptr(out.get("hits")), _ptr(out["n"]), _ptr(out.get("cum")),
                                               _ptr(out.get("total"))), fn + "_device")
            return out
        if out is not None:
            raise ValueError("out= goes with the device form")
        hits = np.zeros(max(min(k, n), 1), dtype=N.BURN_HIT)
        n_out = C.c_uint64(0)
        blocks = [np.zeros(max(nwin * n, 1), dtype=np.uint64) for _ in range(2)] if counts else [None, None]
        N.check(getattr(L, fn)(*lead, hits.ctypes.data if k else None, C.addressof(n_out), *[_ptr(b) for b in blocks]), fn)
        hits = hits[:min(int(n_out.value), k)]
        res = {"entry": hits["entry"].copy(), "row": hits["row"].copy(), "n": int(n_out.value)}
        if counts:
            res["cum"], res["total"] = (b[:nwin * n].reshape(nwin, n) for b in blocks)
        return res

    # -- spread and compare per WINDOW of the list, in one call (lh_kept_spread_series* / lh_kept_drift*) ---------------------------
    def spread_series(self, percentiles, earlier=(), windows=None, nmetrics: Optional[int] = None, first: int = 0, ids=None,
                      out=None, stream=None):
        """Kept.spread per WINDOW of list(earlier) + [self], in one call (lh_kept_spread_series*): the std, mean_le, sum_le and
        upper of each of the last 60 seconds, or of the minute at 10 s resolution.  Returns Kept.spread's dict, derived fields
        included, with a leading window axis -- count[nwin, n], sum_le[nwin, n, np] -- where block w is byte for byte what
        spread() over the handles [lo, hi) of window w returns.  `percentiles` may be empty.  windows, out= and device tensors
        as for Kept.series."""
        p = np.ascontiguousarray(percentiles, dtype=np.float64).ravel()
        tail = (p.ctypes.data, int(p.size), 0, _stream_handle(stream))
        return self._windowed("lh_kept_spread_series", earlier, windows, nmetrics, first, ids, tail, _SPREAD_OUT, int(p.size), out,
                              _spread_derived)

    @staticmethod
    def _drift_windows(against):
        """-> make(windows, nkept) for _windowed: the library's array of 4 * nwin uint32 {base_lo, base_hi, cur_lo, cur_hi}."""
        def make(windows, nkept):
            if against is not None:
                cur = [(i, i + 1) for i in range(nkept)] if windows is None else list(windows)
                quads = [(*against, *c) for c in cur]
            elif windows is None:
                if nkept < 2:
                    raise ValueError("drift of each handle against the one before it needs two handles")
                quads = [(i, i + 1, i + 1, i + 2) for i in range(nkept - 1)]
            else:
                quads = [(*base, *cur) for base, cur in windows]
            quads = [tuple(int(v) for v in q) for q in quads]
            if any(len(q) != 4 or not 0 <= v <= 0xffffffff for q in quads for v in q):
                raise ValueError("a drift window is ((base_lo, base_hi), (cur_lo, cur_hi)) in list positions")
            return (C.c_uint32 * max(4 * len(quads), 1))(*[v for q in quads for v in q]), len(quads)
        return make

    def drift(self, windows=None, earlier=(), against=None, nmetrics: Optional[int] = None, first: int = 0, ids=None, out=None,
              stream=None):
        """Kept.compare per WINDOW of list(earlier) + [self], in one call (lh_kept_drift*) -- "when did it start": `windows`
        is a sequence of ((base_lo, base_hi), (cur_lo, cur_hi)), window w comparing the handles [cur_lo, cur_hi) of the list with
        the handles [base_lo, base_hi) of the same list (each 0 <= lo < hi <= its length, at most N.MAX_KEPT handles in the two
        together; the slices may overlap, coincide and stand in either order; at most N.MAX_WINDOWS windows).  With
        against=(lo, hi), a fixed baseline, `windows` are (cur_lo, cur_hi) slices only, None: one per handle of the list.  With
        neither, each handle is compared with the one before it: len(list) - 1 windows.  Returns Kept.compare's dict with a
        leading window axis, block w byte for byte what compare() of the two slices returns (count_a: the base slice).  out=
        and device tensors as for Kept.series."""
        return self._windowed("lh_kept_drift", earlier, windows, nmetrics, first, ids, (0, _stream_handle(stream)), _COMPARE_OUT,
                              0, out, _compare_derived, self._drift_windows(against))

    # -- the two readers that select across names (lh_top's / lh_movers' entries; what is ranked is what across / count_le /
    #    compare return for the same lists) ------------------------------------------------------------------------------------
    def top(self, k: int, by: str = "count", arg: Optional[float] = None, ascending: bool = False, earlier=(),
            nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Snapshot.top over kept intervals (lh_kept_top*): the k names of [first, first+nmetrics) that lead over
        list(earlier) + [self] taken together, as TOP_ENTRY records, the leader first -- by "count", "sum", "percentile" (arg = p)
        or "count_above" (arg = a value), as there.  count, sum and pkey are what Kept.across returns for the same list (sum bit
        for bit), above is count minus Kept.count_le's answer.  first and ids are metric ids; every handle must hold the range;
        first=None / nmetrics=None: this handle's block.  out= as for Snapshot.top: a numpy array of TOP_ENTRY takes the host
        form, an (entries, n) pair of torch device tensors the device form, enqueued on `stream` (a torch stream or a raw handle;
        None: the null stream); every handle may be closed right afterwards: close() waits."""
        nmetrics, first = self._block(nmetrics, first)
        handles, nkept = self._list(earlier)
        return Snapshot._leaders("lh_kept_top", (C.addressof(handles), nkept), Snapshot._TOP_BY, ("percentile", "count_above"),
                                 "TOP_ENTRY", k, by, arg, N.TOP_ASCENDING if ascending else 0, nmetrics, first, out,
                                 (_stream_handle(stream),))

    def movers(self, base, k: int, by: str = "ks", arg: Optional[float] = None, ascending: bool = False, earlier=(),
               nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Snapshot.movers over kept intervals (lh_kept_movers*): the k names of [first, first+nmetrics) whose distribution over
        list(earlier) + [self] taken together moved most against the same names of `base`, a Kept or a sequence of them taken
        together, as MOVER_ENTRY records, the leader first -- by "ks", "w1", "shift" (the bits Kept.compare returns for the same
        lists) or "percentile" (arg = p: the buckets Kept.across selects on either side).  At most N.MAX_KEPT handles in the
        two lists together.  first / nmetrics / out / stream as for Kept.top."""
        nmetrics, first = self._block(nmetrics, first)
        lists = self._pair(base, earlier)
        return Snapshot._leaders("lh_kept_movers", (C.addressof(lists[0]), lists[1], C.addressof(lists[2]), lists[3]),
                                 Snapshot._MOVERS_BY, ("percentile",), "MOVER_ENTRY", k, by, arg,
                                 N.MOVERS_ASCENDING if ascending else 0, nmetrics, first, out, (_stream_handle(stream),))

    # -- top and movers per WINDOW of the list, in one call (lh_kept_top_series* / lh_kept_movers_series*) ---------------------------
    _TOP_SERIES, _MOVERS_SERIES = "lh_kept_top_series", "lh_kept_movers_series"

    def _leaders_series(self, fn, make, windows, earlier, by_codes, takes_arg, entry, k, by, arg, flags, nmetrics, first, out, stream):
        """The call of a per-window selecting reader through Snapshot._leaders: the list, the windows make(windows, nkept) gives."""
        nmetrics, first = self._block(nmetrics, first)
        handles, nkept = self._list(earlier)
        win, nwin = make(windows, nkept)
        return Snapshot._leaders(fn, (C.addressof(handles), nkept, C.addressof(win), nwin), by_codes, takes_arg, entry, k, by, arg,
                                 flags, nmetrics, first, out, (_stream_handle(stream),), nwin)

    def top_series(self, k: int, by: str = "count", arg: Optional[float] = None, ascending: bool = False, earlier=(), windows=None,
                   nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Kept.top per WINDOW of list(earlier) + [self], in one call (lh_kept_top_series*) -- which k names led in each of the
        last 60 seconds: `windows` as for Kept.series ((lo, hi) pairs of list positions; None: one window per handle).  Returns a
        list of nwin TOP_ENTRY arrays, window w's byte for byte what top() over the handles [lo, hi) returns, of its length.
        out= follows Kept.top's forms: a numpy array of nwin * k TOP_ENTRY takes the host form (window w's entries at
        out[w * k:], the returned arrays view it); an (entries, n) pair of torch device tensors, of nwin * k * 32 bytes and nwin
        uint32, takes the device form on `stream` and is returned as it is."""
        return self._leaders_series(self._TOP_SERIES, self._windows, windows, earlier, Snapshot._TOP_BY, ("percentile", "count_above"),
                                    "TOP_ENTRY", k, by, arg, N.TOP_ASCENDING if ascending else 0, nmetrics, first, out, stream)

    def movers_series(self, k: int, by: str = "ks", arg: Optional[float] = None, ascending: bool = False, earlier=(), windows=None,
                      against=None, nmetrics: Optional[int] = None, first: Optional[int] = None, out=None, stream=None):
        """Kept.movers per WINDOW of list(earlier) + [self], in one call (lh_kept_movers_series*) -- which k names moved most in
        each second against the minute before the deploy: `windows` / `against` exactly as Kept.drift takes them.  Returns a
        list of nwin MOVER_ENTRY arrays, window w's byte for byte what movers() of the two slices returns (count_a: the base
        slice).  out= as for Kept.top_series."""
        return self._leaders_series(self._MOVERS_SERIES, self._drift_windows(against), windows, earlier, Snapshot._MOVERS_BY,
                                    ("percentile",), "MOVER_ENTRY", k, by, arg, N.MOVERS_ASCENDING if ascending else 0, nmetrics,
                                    first, out, stream)

    # -- save and load (lh_kept_save* / lh_kept_load*; loghisto_amd.keptfile has the blob's format in NumPy) ------------------------
    def _save_size(self) -> int:
        n = C.c_size_t(0)
        N.check(N.lib().lh_kept_save_size(self._h, C.byref(n)), "lh_kept_save_size")
        return int(n.value)

    def to_bytes(self, stream=None) -> bytes:
        """The handle as a blob (lh_kept_save): a 64-byte header and the four arrays verbatim.  Kept.from_bytes takes it back, in
        this process or another, on this device or another, with no engine."""
        n = self._save_size()
        buf = np.empty(n, dtype=np.uint8)
        written = C.c_size_t(0)
        N.check(N.lib().lh_kept_save(self._h, buf.ctypes.data, n, _stream_handle(stream), C.byref(written)), "lh_kept_save")
        return buf[:int(written.value)].tobytes()

    def save(self, path, stream=None, encoded: bool = False):
        """to_bytes() written to the file `path` -- encoded=True: encode(), the compact blob.  The names that belong to the ids are
        not part of it."""
        with open(path, "wb") as f:
            f.write(self.encode(stream).tobytes() if encoded else self.to_bytes(stream))

    # -- the compact blob (lh_kept_encode* / lh_kept_decode*; loghisto_amd.keptfile.encode is its NumPy statement) ---------------------
    def encoded_size(self, stream=None) -> int:
        """The exact length of encode()'s result (lh_kept_encode_size: the encoder's first pass alone)."""
        n = C.c_size_t(0)
        N.check(N.lib().lh_kept_encode_size(self._h, _stream_handle(stream), C.byref(n)), "lh_kept_encode_size")
        return int(n.value)

    def _encode_bound(self) -> int:
        from . import keptfile
        return keptfile.encoded_bound(self.info["nrows"], self.info["cells"])

    def encode(self, stream=None) -> np.ndarray:
        """The handle as an ENCODED blob (lh_kept_encode), uint8: counts at the narrowest width per row, bins as byte deltas, made on
        the device and brought over in one copy.  Kept.decode takes it back into a handle with the same bytes as this one."""
        buf = np.empty(self._encode_bound(), dtype=np.uint8)
        written = C.c_size_t(0)
        N.check(N.lib().lh_kept_encode(self._h, buf.ctypes.data, buf.size, _stream_handle(stream), C.byref(written)), "lh_kept_encode")
        return buf[:int(written.value)].copy()

    def encode_device(self, stream=None):
        """The same blob as a torch uint8 tensor on the handle's device (lh_kept_encode_device): what a rank hands to a collective.
        Kept.decode_device takes it back."""
        import torch
        n = self.encoded_size(stream)
        t = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", self.info["device"]))
        N.check(N.lib().lh_kept_encode_device(self._h, int(t.data_ptr()), n, _stream_handle(stream), None), "lh_kept_encode_device")
        return t

    def to_device_blob(self, stream=None):
        """The same blob as a torch uint8 tensor on the handle's device (lh_kept_save_device): what a rank hands to a
        collective.  Kept.from_device_blob takes it back."""
        import torch
        n = self._save_size()
        t = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", self.info["device"]))
        N.check(N.lib().lh_kept_save_device(self._h, int(t.data_ptr()), n, _stream_handle(stream), None), "lh_kept_save_device")
        return t

    @staticmethod
    def values(device: int = 0) -> np.ndarray:
        """decompress() by bin, float64[N.NKEYS], as the kept readers weigh cells with on `device` (lh_kept_values): bit-equal to
        Engine.codec_tables()' D, and there for a process that has no engine."""
        D = Kept._values.get(device)
        if D is None:                                  # fetched once per device: the table never changes
            D = np.empty(N.NKEYS, dtype=np.float64)
            N.check(N.lib().lh_kept_values(device, D.ctypes.data_as(C.POINTER(C.c_double))), "lh_kept_values")
            D.flags.writeable = False
            Kept._values[device] = D
        return D

    _values: dict = {}

    @classmethod
    def _load(cls, fn, device, addr, n, stream):
        table = cls.values(device)                     # before the handle exists: a failure here leaves nothing behind
        why = N.LhKeptCheck(struct_size=C.sizeof(N.LhKeptCheck))
        h = C.c_void_p(0)
        rc = getattr(N.lib(), fn)(device, addr, n, 0, _stream_handle(stream), C.byref(why), C.byref(h))
        if rc == N.EINVAL:
            from . import keptfile
            raise ValueError(f"{fn}: not a kept blob: {keptfile.ENC_CAUSES.get(why.cause, why.cause)} (row {why.row}, index {why.index})")
        N.check(rc, fn)
        return cls(h, table)

    @classmethod
    def from_bytes(cls, blob, device: int = 0, stream=None) -> "Kept":
        """A new Kept on `device` from a blob (lh_kept_load): every reader, merge, arrays and close take it like one made by
        Snapshot.keep.  No engine is needed.  The blob is untrusted: it is checked on the device before the handle exists, and
        ValueError says what is wrong with one that is refused."""
        a = np.frombuffer(blob, dtype=np.uint8)
        keep = a if a.size else np.zeros(1, dtype=np.uint8)   # an empty blob is a SHORT one, as keptfile.check has it: a valid address
        return cls._load("lh_kept_load", device, keep.ctypes.data, int(a.size), stream)

    @classmethod
    def load(cls, path, device: int = 0, stream=None, encoded: bool = False) -> "Kept":
        """from_bytes() of the file `path` -- encoded=True: decode() of it, a file save(path, encoded=True) wrote."""
        with open(path, "rb") as f:
            data = f.read()
        return cls.decode(data, device, stream) if encoded else cls.from_bytes(data, device, stream)

    @classmethod
    def decode(cls, data, device: int = 0, stream=None) -> "Kept":
        """A new Kept on `device` from an ENCODED blob (lh_kept_decode; bytes or a uint8 array): the handle that was encoded, byte
        for byte.  Untrusted like from_bytes' blob: checked on the device before the handle exists, ValueError says what is wrong."""
        a = np.frombuffer(data, dtype=np.uint8)
        keep = a if a.size else np.zeros(1, dtype=np.uint8)
        return cls._load("lh_kept_decode", device, keep.ctypes.data, int(a.size), stream)

    @classmethod
    def decode_device(cls, t, stream=None) -> "Kept":
        """The same from a contiguous torch uint8 device tensor that holds an encoded blob (lh_kept_decode_device), at any
        alignment: only its 64 header bytes come to the host."""
        if not (getattr(t, "is_cuda", False) and t.element_size() == 1 and t.is_contiguous()):
            raise ValueError("a contiguous torch uint8 device tensor")
        return cls._load("lh_kept_decode_device", t.device.index, int(t.data_ptr()), int(t.numel()), stream)

    @classmethod
    def from_device_blob(cls, t, stream=None) -> "Kept":
        """A new Kept on the device of `t`, a contiguous torch uint8 device tensor that holds a blob (lh_kept_load_device): only
        its 64 header bytes come to the host."""
        if not (getattr(t, "is_cuda", False) and t.element_size() == 1 and t.is_contiguous()):
            raise ValueError("a contiguous torch uint8 device tensor")
        return cls._load("lh_kept_load_device", t.device.index, int(t.data_ptr()), int(t.numel()), stream)

    def close(self):
        """Frees the device memory (lh_kept_release); waits first for enqueued device-form work that still reads it."""
        if self._h is not None and self._h.value:
            N.check(N.lib().lh_kept_release(self._h), "lh_kept_release")
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _device_column(t, what, widths):
    """A 1-D (possibly strided) torch device tensor whose (element width, "f" | "i") is in `widths` -> (address, byte stride,
    element width, elements).  Host memory is refused: every data-shaped argument of lh_lines* is device memory."""
    if not (hasattr(t, "data_ptr") and getattr(t, "is_cuda", False)):
        raise ValueError(f"{what} is a torch device tensor (lh_lines* reads device memory only)")
    if t.dim() != 1:
        raise ValueError(f"{what} is 1-D (a strided view such as t[:, i] is fine)")
    width = t.element_size()
    if (width, "f" if t.is_floating_point() else "i") not in widths:
        raise ValueError(f"{what} has an element type lh_lines* does not take")
    return int(t.data_ptr()), int(t.stride(0)) * width if t.numel() > 1 else width, width, int(t.numel())


class Names:
    """A device copy of an engine's metric names (lh_names): what lh_lines* prints keys from.  Engine.device_names()."""

    _OPS = {"value": N.OP_VALUE, "ratio": N.OP_RATIO, "sqrt_ratio": N.OP_SQRT_RATIO, "diff": N.OP_DIFF}

    def __init__(self, engine: "Engine"):
        h = C.c_void_p(0)
        N.check(N.lib().lh_names_create(engine._h, engine.device, C.byref(h)), "lh_names_create")
        self._h = h
        self.engine = engine
        self._buf = None
        self.count = self.refresh()

    def refresh(self) -> int:
        """Appends the names interned since (lh_names_refresh) -> the number of names held."""
        n = C.c_uint32(0)
        N.check(N.lib().lh_names_refresh(self._h, C.byref(n)), "lh_names_refresh")
        self.count = int(n.value)
        return self.count

    def _column(self, c: dict, n: int) -> N.LhColumn:
        if set(c) - {"label", "a", "b", "op", "valid", "key"}:
            raise ValueError("a column holds label, a and optionally b, op, valid, key")
        op = c.get("op", "value")
        if op not in self._OPS:
            raise ValueError("op is one of " + ", ".join(self._OPS))
        col = N.LhColumn()
        col.label = c["label"].encode()
        col.op = self._OPS[op]
        for side in ("a", "b"):
            t = c.get(side)
            if t is None:
                continue
            key = side == "a" and bool(c.get("key"))
            addr, stride, width, numel = _device_column(t, f"column {c['label']!r}: {side}",
                                                        ((2, "i"),) if key else ((8, "f"), (8, "i"), (4, "i")))
            if numel < n:
                raise ValueError(f"column {c['label']!r}: {side} holds fewer than n elements")
            kind = N.COL_KEY if key else N.COL_F64 if t.is_floating_point() else N.COL_U64 if width == 8 else N.COL_U32
            setattr(col, side, addr)
            setattr(col, side + "_stride", stride)
            setattr(col, side + "_type", kind)
        if c.get("key") and op != "value":
            raise ValueError("key=True goes with op='value'")
        if c.get("valid") is not None:
            addr, stride, _, numel = _device_column(c["valid"], f"column {c['label']!r}: valid", ((1, "i"),))
            if numel < n:
                raise ValueError(f"column {c['label']!r}: valid holds fewer than n elements")
            col.valid, col.valid_stride = addr, stride
        return col

    def lines(self, columns, n: Optional[int] = None, first: int = 0, ids=None, row_count=None, prefix: str = "", sep: str = " ",
              suffix: str = "\n", underscore_to_dot: bool = False, skip_nan: bool = False, stream=None, out=None):
        """One wire line per (entry, column), formatted on the device (lh_lines*): prefix key sep %f suffix with key =
        label % name.  Each column is a dict: label (a Go format with one %s), a, optionally b, op ("value", "ratio" = a / b,
        "sqrt_ratio" = sqrt(a / b), "diff" = a - b), valid (uint8: 0 omits the line) and key=True (a holds int16 bucket keys,
        printed as their values).  a, b, valid, ids and row_count are 1-D torch DEVICE tensors, possibly strided views
        (t[:, i] of an [n, np] tensor); the element type comes from the dtype (float64; 8- and 4-byte integers as unsigned).
        Entry m's name is first + m, or ids[m] (4-byte integers; an id beyond the names held emits nothing); an entry whose
        row_count is 0 emits nothing.  The work goes on `stream` (an int handle or a torch stream; usually
        snapshot.stream()); None: the null stream.  Returns the text as bytes -- or, with out=(uint8 tensor, 8-byte length
        tensor) on the device, takes the device form and returns `out`: the length always arrives, the text only if it
        fits."""
        L = N.lib()
        id_addr = id_stride = 0
        if ids is not None:
            id_addr, id_stride, _, numel = _device_column(ids, "ids", ((4, "i"),))
            n = numel if n is None else n
            if numel < n:
                raise ValueError("ids holds fewer than n elements")
        elif n is None:
            n = self.count - first
        if n == 0 and out is None:                        # (an empty tensor has no address to hand over)
            return b""
        cols = (N.LhColumn * max(1, len(columns)))(*[self._column(c, n) for c in columns])
        rc_addr = rc_stride = 0
        if row_count is not None:
            rc_addr, rc_stride, _, numel = _device_column(row_count, "row_count", ((8, "i"),))
            if numel < n:
                raise ValueError("row_count holds fewer than n elements")
        fmt = N.LhLineFormat(prefix.encode(), sep.encode(), suffix.encode(), N.FMT_UNDERSCORE_TO_DOT if underscore_to_dot else 0, 0)
        flags = N.LINES_SKIP_NAN if skip_nan else 0
        rows = (id_addr, id_stride, n) if ids is not None else (first, n)
        fn = "lh_lines_ids" if ids is not None else "lh_lines"
        lead = (self._h, *rows, rc_addr, rc_stride, cols, len(columns), C.byref(fmt), flags, _stream_handle(stream))
        if out is not None:
            text, length = out
            for t, what in ((text, "text"), (length, "length")):
                if not (hasattr(t, "data_ptr") and getattr(t, "is_cuda", False) and t.is_contiguous()):
                    raise ValueError(f"device form: {what} is a contiguous torch device tensor")
            if length.element_size() * int(length.numel()) < 8:
                raise ValueError("device form: length holds 8 bytes")
            N.check(getattr(L, fn + "_device")(*lead, _ptr(text), text.element_size() * int(text.numel()), _ptr(length)),
                    fn + "_device")
            return out
        need = C.c_size_t(0)
        if self._buf is None:
            self._buf = C.create_string_buffer(1 << 20)
        N.check(getattr(L, fn)(*lead, self._buf, len(self._buf), C.byref(need)), fn)
        if need.value > len(self._buf):                 # size-then-call: the buffer only grows
            self._buf = C.create_string_buffer(1 << max(20, int(need.value - 1).bit_length()))
            N.check(getattr(L, fn)(*lead, self._buf, len(self._buf), C.byref(need)), fn)
        return C.string_at(self._buf, need.value)

    def close(self):
        if self._h is not None and self._h.value:
            N.check(N.lib().lh_names_destroy(self._h), "lh_names_destroy")
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Engine:
    def __init__(self, device: int = 0, max_metrics: int = 1024, num_buffers: int = 2, num_lanes: int = 4,
                 lane_samples: int = 1 << 20, max_counters: int = 1024, cell_bits: Optional[int] = None):
        """cell_bits: 0 = the library's default (uint64 cells up to 8 192 names, uint32 above), 32, 64.  None reads the TEST
        HARNESS's knobs -- this wrapper's, not the library's (liblhgpu.so never reads the environment): LH_TEST_CELL_BITS, and
        LH_TEST_WIDEN_AT (LH_OPT_WIDEN_AT_SAMPLES), so that the whole GPU suite can be run on engines of 32-bit cells, and on
        ones that move to uint64 cells in the middle of every test (tools/round.sh cells32)."""
        L = N.lib()
        cfg = N.LhConfig()
        N.check(L.lh_default_config(C.byref(cfg)), "lh_default_config")
        cfg.device, cfg.max_metrics, cfg.num_buffers = device, max_metrics, num_buffers
        cfg.num_lanes, cfg.lane_samples, cfg.max_counters = num_lanes, lane_samples, max_counters
        widen_at = 0
        if cell_bits is None:
            cell_bits = int(os.environ.get("LH_TEST_CELL_BITS", "0"))
            widen_at = int(os.environ.get("LH_TEST_WIDEN_AT", "0"))
        cfg.cell_bits = cell_bits
        h = C.c_void_p(0)
        N.check(L.lh_create(C.byref(cfg), C.byref(h)), "lh_create")
        self._h = h
        self.device = device
        self.max_metrics = max_metrics
        if widen_at:
            N.check(L.lh_set_option(h, N.OPT_WIDEN_AT_SAMPLES, widen_at), "lh_set_option")

    # -- names -------------------------------------------------------------
    def intern(self, name: str) -> int:
        b = name.encode()
        out = C.c_uint32(0)
        N.check(N.lib().lh_intern(self._h, b, len(b), C.byref(out)), "lh_intern")
        return int(out.value)

    def lookup(self, name: str) -> Optional[int]:
        b = name.encode()
        out = C.c_uint32(0)
        rc = N.lib().lh_lookup(self._h, b, len(b), C.byref(out))
        if rc == N.ERANGE:
            return None
        N.check(rc, "lh_lookup")
        return int(out.value)

    def num_metrics(self) -> int:
        out = C.c_uint32(0)
        N.check(N.lib().lh_num_metrics(self._h, C.byref(out)), "lh_num_metrics")
        return int(out.value)

    def device_names(self) -> "Names":
        """A device copy of the names interned so far (lh_names_create), for Names.lines / Snapshot.spread_lines."""
        return Names(self)

    def metric_name(self, metric_id: int) -> str:
        ln = C.c_size_t(0)
        buf = C.create_string_buffer(4096)
        N.check(N.lib().lh_metric_name(self._h, metric_id, buf, 4096, C.byref(ln)), "lh_metric_name")
        return buf.raw[:min(ln.value, 4096)].decode()

    # -- ingest ------------------------------------------------------------
    def submit(self, metric_id: int, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        N.check(N.lib().lh_submit(self._h, metric_id, v.ctypes.data, v.size), "lh_submit")

    def submit_pairs(self, ids, values):
        """(id, value) pairs from host arrays (copied before the call returns).  uint16 ids take the 10-byte form
        (lh_submit_pairs16: legal for <= 65 536 names), anything else is sent as uint32 (lh_submit_pairs)."""
        narrow = isinstance(ids, np.ndarray) and ids.dtype == np.uint16
        i = np.ascontiguousarray(ids, dtype=np.uint16 if narrow else np.uint32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if i.size != v.size:
            raise ValueError("ids and values differ in length")
        if narrow:
            N.check(N.lib().lh_submit_pairs16(self._h, i.ctypes.data, v.ctypes.data, v.size), "lh_submit_pairs16")
        else:
            N.check(N.lib().lh_submit_pairs(self._h, i.ctypes.data, v.ctypes.data, v.size), "lh_submit_pairs")

    def reserve_pairs(self, want: int, id_bits: int = 32):
        """(ids uint32[granted] or uint16[granted], values float64[granted], token): views of a pinned staging buffer
        to fill in place (lh_reserve_pairs / lh_reserve_pairs16); publish the first n with commit_pairs(token, n)."""
        pi, pv, g, tok = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_uint32(0)
        fn, ct = (N.lib().lh_reserve_pairs16, C.c_uint16) if id_bits == 16 else (N.lib().lh_reserve_pairs, C.c_uint32)
        N.check(fn(self._h, want, C.byref(pi), C.byref(pv), C.byref(g), C.byref(tok)), "lh_reserve_pairs")
        ids = np.ctypeslib.as_array(C.cast(pi, C.POINTER(ct)), shape=(g.value,))
        vals = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_double)), shape=(g.value,))
        return ids, vals, tok.value

    def commit_pairs(self, token: int, n: int):
        N.check(N.lib().lh_commit_pairs(self._h, token, n), "lh_commit_pairs")

    def submit_pairs_in_place(self, ids, values):
        """The same stream as submit_pairs through reserve / fill / commit: one host-side copy, no id scan.  uint16 ids
        are staged as uint16 (10 bytes per pair over PCIe)."""
        narrow = isinstance(ids, np.ndarray) and ids.dtype == np.uint16
        i = np.ascontiguousarray(ids, dtype=np.uint16 if narrow else np.uint32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if i.size != v.size:
            raise ValueError("ids and values differ in length")
        done = 0
        while done < v.size:
            di, dv, tok = self.reserve_pairs(v.size - done, 16 if narrow else 32)
            k = di.size
            np.copyto(di, i[done:done + k])
            np.copyto(dv, v[done:done + k])
            self.commit_pairs(tok, k)
            done += k

    def submit_device(self, metric_id: int, d_values, n: Optional[int] = None, stream=None):
        n = int(d_values.numel()) if n is None else n
        N.check(N.lib().lh_submit_device(self._h, metric_id, _ptr(d_values), n, _stream_handle(stream)),
                "lh_submit_device")

    def submit_pairs_device(self, d_ids, d_values, n: Optional[int] = None, stream=None):
        """Device-resident (id, value) pairs.  A 2-byte id tensor (torch.int16 / torch.uint16: the bits of uint16 ids)
        takes lh_submit_pairs16_device, a 4-byte one lh_submit_pairs_device."""
        n = int(d_values.numel()) if n is None else n
        if getattr(d_ids, "element_size", lambda: 4)() == 2:
            N.check(N.lib().lh_submit_pairs16_device(self._h, _ptr(d_ids), _ptr(d_values), n, _stream_handle(stream)),
                    "lh_submit_pairs16_device")
            return
        N.check(N.lib().lh_submit_pairs_device(self._h, _ptr(d_ids), _ptr(d_values), n, _stream_handle(stream)),
                "lh_submit_pairs_device")

    # -- counters (metrics.go:251-269) -----------------------------------------
    def intern_counter(self, name: str) -> int:
        b = name.encode()
        out = C.c_uint32(0)
        N.check(N.lib().lh_intern_counter(self._h, b, len(b), C.byref(out)), "lh_intern_counter")
        return int(out.value)

    def num_counters(self) -> int:
        out = C.c_uint32(0)
        N.check(N.lib().lh_num_counters(self._h, C.byref(out)), "lh_num_counters")
        return int(out.value)

    def counter_name(self, cid: int) -> str:
        ln = C.c_size_t(0)
        buf = C.create_string_buffer(4096)
        N.check(N.lib().lh_counter_name(self._h, cid, buf, 4096, C.byref(ln)), "lh_counter_name")
        return buf.raw[:min(ln.value, 4096)].decode()

    def submit_counts(self, ids, amounts):
        i = np.ascontiguousarray(ids, dtype=np.uint32)
        a = np.ascontiguousarray(amounts, dtype=np.uint64)
        if i.size != a.size:
            raise ValueError("ids and amounts differ in length")
        N.check(N.lib().lh_submit_counts(self._h, i.ctypes.data, a.ctypes.data, a.size), "lh_submit_counts")

    def submit_counts_device(self, d_ids, d_amounts, n: Optional[int] = None, stream=None):
        n = int(d_amounts.numel()) if n is None else n
        N.check(N.lib().lh_submit_counts_device(self._h, _ptr(d_ids), _ptr(d_amounts), n, _stream_handle(stream)),
                "lh_submit_counts_device")

    def flush(self):
        N.check(N.lib().lh_flush(self._h), "lh_flush")

    def sync(self):
        N.check(N.lib().lh_sync(self._h), "lh_sync")

    # -- epoch -------------------------------------------------------------
    def flip(self) -> Snapshot:
        h = C.c_void_p(0)
        N.check(N.lib().lh_flip(self._h, C.byref(h)), "lh_flip")
        return Snapshot(self, h.value)

    # -- codec (parity tests) -----------------------------------------------
    def compress_device(self, d_values, d_keys, n: int, golog: bool = False, stream=None):
        fn = N.lib().lh_compress_device_golog if golog else N.lib().lh_compress_device
        N.check(fn(self._h, _ptr(d_values), _ptr(d_keys), n, _stream_handle(stream)), "lh_compress_device")

    def codec_tables(self):
        tx = np.zeros(N.NTHRESH, dtype=np.float64)
        d = np.zeros(N.NKEYS, dtype=np.float64)
        N.check(N.lib().lh_codec_tables(self._h, tx.ctypes.data_as(C.POINTER(C.c_double)),
                                        d.ctypes.data_as(C.POINTER(C.c_double))), "lh_codec_tables")
        return tx, d

    def selftest_vlog(self) -> float:
        out = C.c_double(0)
        N.check(N.lib().lh_selftest_vlog(self._h, C.byref(out)), "lh_selftest_vlog")
        return float(out.value)

    def lifetime(self, n: Optional[int] = None, first: int = 0):
        """(count, sum) lifetime stores of metrics [first, first+n) (histogramCountStore, metrics.go:127)."""
        if n is None:
            n = self.num_metrics() - first
        cnt = np.zeros(n, dtype=np.uint64)
        sm = np.zeros(n, dtype=np.uint64)
        if n:
            N.check(N.lib().lh_lifetime(self._h, first, n, cnt.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        sm.ctypes.data_as(C.POINTER(C.c_uint64))), "lh_lifetime")
        return cnt, sm

    def format_f(self, values) -> list:
        """Go's %f of each float64, formatted by the device formatter (lh_format_f)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        out: list = []
        step = 1 << 16
        for i in range(0, v.size, step):
            part = v[i:i + step]
            buf = C.create_string_buffer(part.size * N.FMT_SLOT)
            lens = np.zeros(part.size, dtype=np.uint32)
            N.check(N.lib().lh_format_f(self._h, part.ctypes.data_as(C.POINTER(C.c_double)), part.size, buf,
                                        N.FMT_SLOT, lens.ctypes.data_as(C.POINTER(C.c_uint32))), "lh_format_f")
            raw = buf.raw
            out.extend(raw[k * N.FMT_SLOT:k * N.FMT_SLOT + int(lens[k])].decode() for k in range(part.size))
        return out

    def counters(self) -> dict:
        """Self-metrics of the engine (lh_get_counters)."""
        c = N.LhCounters()
        N.check(N.lib().lh_get_counters(self._h, C.byref(c)), "lh_get_counters")
        return {k: int(getattr(c, k)) for k, _ in N.LhCounters._fields_ if k != "reserved"}

    def set_option(self, option: int, value: int):
        """Dispatch settings (lh_set_option): they choose among exact kernel paths, never a result."""
        N.check(N.lib().lh_set_option(self._h, int(option), int(value)), "lh_set_option")

    def close(self):
        if self._h is not None and self._h.value:
            N.check(N.lib().lh_destroy(self._h), "lh_destroy")
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
