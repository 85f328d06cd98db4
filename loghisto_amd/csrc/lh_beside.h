// lh_beside.h -- host-only plumbing of the units built BESIDE the engine (lh_import.hip, lh_count.hip, lh_spread.hip, lh_top.hip,
// lh_compare.hip, lh_movers.hip, lh_across.hip; a new reader of a snapshot starts here and in lh_wave.h).  Such a unit sees
// the engine through its public C ABI only (include/loghisto_gpu.h: it cannot see struct lh_engine / lh_snapshot):
//   lh_snapshot_cells    the cells AS THEY ARE, 4 or 8 bytes wide (nothing moves: a narrow snapshot stays narrow), and the
//                        number of rows
//   lh_snapshot_ranges   the rows' dirty spans [lo, hi] -- cells outside are zero; their address also names the device
//   lh_snapshot_stream   the stream the snapshot's extract / clear work is ordered on: the unit's kernels go there
//   lh_row_stride        >= LH_NKEYS + 4, so that whole 4-bin groups are readable up to bin 65 535
// A reader is read-only: no store goes to a cell, a span or the engine.  (lh_import.hip writes, and says how.)
//
// What is here: the HIP error check, pointer tests, one context slot per (unit, device), the opener, growing blocks, the
// way a host form's results travel back, the event that guards a block across streams, and the measurement switch's
// exchange.  For the readers, which all walk rows [first, first + nmetrics) or a list of row ids (RowSel, rows_in; stage_ids
// brings a host list to the device, stage_doubles per-entry host arrays of doubles): their source record and its two-step opener
// (Source, source_cells, source_open), the same two steps for a reader of a list of snapshots (list_cells, list_open: two
// for lh_compare.hip and lh_movers.hip, up to 16 for lh_across.hip) with the events that put the last snapshot's stream
// behind the others' (order_behind), the launch shape (row_shape), the dispatch on the cells' width (with_cells) and the
// value table's set-up (ensure_table).  A reader itself has its context, its argument checks, its kernels and its entry
// points; one that selects k names has the rest of its host side in lh_select.h.
#pragma once

#include "../../include/loghisto_gpu.h"
#include "lh_wave.h" // the launch geometry (row_shape)

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <type_traits>

namespace lh {
namespace beside {

// clears the sticky error; for functions that return an lh status
#define LH_BESIDE_CHK(expr)                                                                    \
    do {                                                                                       \
        const hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                                \
            (void)hipGetLastError();                                                           \
            return _e == hipErrorOutOfMemory ? LH_ENOMEM : LH_EDEVICE;                         \
        }                                                                                      \
    } while (0)

inline bool misaligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// pinned host memory the copy engine can write directly (hipHostMalloc'ed or registered by the caller)
inline bool is_pinned(const void *p)
{
    if (!p) return true;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// Per-device state of a unit, allocated on first use and kept for the life of the process (the engine's own pinned
// blocks are not reachable through the ABI).  One array per context TYPE: each unit has its own slots, and its own
// mutex in them -- units never wait for each other.  nullptr: no such slot.
constexpr int MAX_DEVICES = 64;
template <class Ctx> Ctx *device_ctx(int device)
{
    static Ctx slots[MAX_DEVICES];
    return device < 0 || device >= MAX_DEVICES ? nullptr : &slots[device];
}

struct Opened {
    uint32_t *ranges = nullptr;
    int device = -1;
    hipStream_t stream = nullptr;
    size_t stride = 0;
};

// spans, device (made current), the unit's context there, stream, stride.  Moves nothing.
template <class Ctx> int open_snapshot(lh_snapshot *s, Opened &o, Ctx *&cx)
{
    void *p = nullptr;
    int rc = lh_snapshot_ranges(s, &p);
    if (rc) return rc;
    o.ranges = static_cast<uint32_t *>(p);
    hipPointerAttribute_t attr;
    LH_BESIDE_CHK(hipPointerGetAttributes(&attr, p));
    cx = device_ctx<Ctx>(attr.device);
    if (!cx) return LH_EDEVICE;
    o.device = attr.device;
    LH_BESIDE_CHK(hipSetDevice(attr.device));
    rc = lh_snapshot_stream(s, &p);
    if (rc) return rc;
    o.stream = static_cast<hipStream_t>(p);
    o.stride = lh_row_stride();
    return LH_OK;
}

// A block that only grows: below `need` elements it is freed and allocated again at `floor` doubled until it fits.
// After a failure the pointer is null and the capacity 0.
inline size_t grown(size_t need, size_t floor)
{
    while (floor < need) floor <<= 1;
    return floor;
}
template <class T> int grow_device(T *&ptr, size_t &cap, size_t need, size_t floor, size_t elem_bytes = sizeof(T))
{
    if (cap >= need) return LH_OK;
    if (ptr) LH_BESIDE_CHK(hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    const size_t n = grown(need, floor);
    LH_BESIDE_CHK(hipMalloc((void **)&ptr, n * elem_bytes));
    cap = n;
    return LH_OK;
}
template <class T> int grow_pinned(T *&ptr, size_t &cap, size_t need, size_t floor, size_t elem_bytes = sizeof(T))
{
    if (cap >= need) return LH_OK;
    if (ptr) LH_BESIDE_CHK(hipHostFree(ptr));
    ptr = nullptr;
    cap = 0;
    const size_t n = grown(need, floor);
    LH_BESIDE_CHK(hipHostMalloc((void **)&ptr, n * elem_bytes, hipHostMallocDefault));
    cap = n;
    return LH_OK;
}

// The host form's results: the kernel's output in HBM / its pinned landing block (in bytes; part of the unit's context)
struct ResultBlocks {
    unsigned char *d_res = nullptr, *h_res = nullptr;
    size_t d_cap = 0, h_cap = 0;
};
constexpr size_t RESULT_FLOOR = 32768;
struct HostOut {
    void *host; // the caller's array, or null: not asked for
    size_t bytes;
};

// (the context's mutex held)  Lays the arrays that were asked for out in the device block, each at a multiple of 8 bytes,
// has `enqueue(dev)` put the work that fills them on `st` (dev[k]: where array k goes, null with out[k].host), then
// brings them back -- one copy per array straight into the caller's arrays when all of those are pinned, one copy through
// the pinned block otherwise -- and waits for `st`.
template <size_t N, class Enqueue> int host_results(ResultBlocks &rb, hipStream_t st, const HostOut (&out)[N], Enqueue enqueue)
{
    size_t at[N], need = 0;
    bool direct = true;
    for (size_t k = 0; k < N; k++) {
        at[k] = need;
        need += ((out[k].host ? out[k].bytes : 0) + 7) & ~(size_t)7;
    }
    int rc = grow_device(rb.d_res, rb.d_cap, need, RESULT_FLOOR);
    if (rc) return rc;
    for (size_t k = 0; k < N; k++) direct = direct && is_pinned(out[k].host);
    if (!direct) {
        rc = grow_pinned(rb.h_res, rb.h_cap, need, RESULT_FLOOR);
        if (rc) return rc;
    }
    unsigned char *dev[N];
    for (size_t k = 0; k < N; k++) dev[k] = out[k].host ? rb.d_res + at[k] : nullptr;
    rc = enqueue(dev);
    if (rc) return rc;
    if (direct) {
        for (size_t k = 0; k < N; k++)
            if (out[k].host) LH_BESIDE_CHK(hipMemcpyAsync(out[k].host, dev[k], out[k].bytes, hipMemcpyDeviceToHost, st));
        LH_BESIDE_CHK(hipStreamSynchronize(st));
    } else {
        LH_BESIDE_CHK(hipMemcpyAsync(rb.h_res, rb.d_res, need, hipMemcpyDeviceToHost, st));
        LH_BESIDE_CHK(hipStreamSynchronize(st));
        for (size_t k = 0; k < N; k++)
            if (out[k].host) std::memcpy(out[k].host, rb.h_res + at[k], out[k].bytes);
    }
    return LH_OK;
}

// A block that outlives a device-form call, while snapshots of different engines run on different streams: it is guarded
// by an event, not by stream order.  `pending` is cleared only after a wait that covers the event itself (host_wait, or the
// caller's synchronize of the very stream it was last recorded on: covered()) -- another stream's sync says nothing.
struct __attribute__((visibility("hidden"))) EventGuard { // (hidden: the library exports nothing of this header)
    hipEvent_t ev = nullptr; // behind the last work that uses the block, on whichever stream that was
    bool pending = false;
    int create()
    {
        if (!ev) LH_BESIDE_CHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        return LH_OK;
    }
    int host_wait() // before the host frees or rewrites the block
    {
        if (pending) {
            LH_BESIDE_CHK(hipEventSynchronize(ev));
            pending = false;
        }
        return LH_OK;
    }
    int stream_wait(hipStream_t st) // before work on `st` uses the block: on the device, not on the host
    {
        if (pending) LH_BESIDE_CHK(hipStreamWaitEvent(st, ev, 0));
        return LH_OK;
    }
    int record(hipStream_t st)
    {
        LH_BESIDE_CHK(hipEventRecord(ev, st));
        pending = true;
        return LH_OK;
    }
    void covered() { pending = false; }
};

// ---- the readers' front end --------------------------------------------------------------------------
// What a reader's call works on: the opened snapshot, the unit's context on its device, and the cells as they are.
template <class Ctx> struct Source : Opened {
    Ctx *cx = nullptr;
    const void *cells = nullptr;
    uint32_t nrows = 0, cell_bytes = 0;
};
// Which rows a call reads: [first, first + n), or -- the *_ids forms -- rows ids[0 .. n) in that order, from a host array
// (checked and copied by the call) or a device array (read by the kernel, which guards every id itself: lh::row_of).
struct RowSel {
    uint32_t first = 0;
    const uint32_t *ids = nullptr;
    bool by_id = false, on_device = false;
};
inline RowSel rows_from(uint32_t first) { return RowSel{first, nullptr, false, false}; }
inline RowSel rows_by_id(const uint32_t *ids, bool on_device) { return RowSel{0, ids, true, on_device}; }
// the *_ids forms' own causes of LH_EINVAL, decided before anything else (so that they win over the early LH_ERANGE)
inline bool bad_ids(const RowSel &sel, size_t n) { return sel.by_id && ((!sel.ids && n > 0) || misaligned(sel.ids, 4)); }
// a row of lh_count_le*'s bounds that no call takes: a NaN, or a decreasing pair (-0.0 == 0.0; equal neighbours are allowed)
inline bool bad_bounds(const double *b, size_t nb)
{
    for (size_t j = 0; j < nb; j++)
        if (b[j] != b[j] || (j && b[j] < b[j - 1])) return true;
    return false;
}
// LH_ERANGE for rows a snapshot of `nrows` rows does not have: the end of the block, or the first id of a host list at or
// beyond nrows.  (A device list is not looked at.)  n <= 2^32 - 1: the units' argument checks came first.
inline int rows_in(const RowSel &sel, size_t n, uint32_t nrows)
{
    if (!sel.by_id) return n > nrows || sel.first > nrows - n ? LH_ERANGE : LH_OK;
    if (!sel.on_device)
        for (size_t m = 0; m < n; m++)
            if (sel.ids[m] >= nrows) return LH_ERANGE;
    return LH_OK;
}
// Step one, before any device call: the cells, and LH_ERANGE for rows the snapshot does not have.
template <class Ctx> int source_cells(lh_snapshot *s, const RowSel &sel, size_t nmetrics, Source<Ctx> &q)
{
    void *cells = nullptr;
    const int rc = lh_snapshot_cells(s, &cells, &q.nrows, &q.cell_bytes);
    if (rc) return rc;
    q.cells = cells;
    return rows_in(sel, nmetrics, q.nrows);
}
template <class Ctx> int source_cells(lh_snapshot *s, uint32_t first, size_t nmetrics, Source<Ctx> &q)
{
    return source_cells(s, rows_from(first), nmetrics, q);
}
// whole 4-bin groups are readable up to bin 65 535, and the cells have one of the two widths the kernels are built for
template <class Ctx> bool usable(const Source<Ctx> &q)
{
    return q.stride >= (size_t)LH_NKEYS + 4 && q.cells && (q.cell_bytes == 4 || q.cell_bytes == 8);
}
// Step two: spans, device, context, stream and stride; LH_ESTATE for a snapshot the kernels cannot walk.
template <class Ctx> int source_open(lh_snapshot *s, Source<Ctx> &q)
{
    const int rc = open_snapshot(s, q, q.cx);
    if (rc) return rc;
    return usable(q) ? LH_OK : LH_ESTATE;
}
// The two steps for a reader of a list of snapshots, q[i] the source of snaps[i]; the work goes on the LAST one's stream and
// the unit's context is q[n - 1].cx (lh_compare.hip, lh_movers.hip: {base, cur}).  Between the steps a reader whose empty
// call writes nothing returns (lh_compare.hip, lh_across.hip); one whose empty call writes n_out takes both first
// (lh_movers.hip).  Step one: LH_ERANGE for rows any of the snapshots does not have, the first in list order.
template <class Ctx> int list_cells(lh_snapshot *const *snaps, size_t n, const RowSel &sel, size_t nmetrics, Source<Ctx> *q)
{
    for (size_t i = 0; i < n; i++) {
        const int rc = source_cells(snaps[i], sel, nmetrics, q[i]);
        if (rc) return rc;
    }
    return LH_OK;
}
template <class Ctx> int list_cells(lh_snapshot *const *snaps, size_t n, uint32_t first, size_t nmetrics, Source<Ctx> *q)
{
    return list_cells(snaps, n, rows_from(first), nmetrics, q);
}
// Step two: all opened in list order (the last one's device stays current), then LH_EINVAL for more than one device (the
// check that needs them all), then LH_ESTATE.
template <class Ctx> int list_open(lh_snapshot *const *snaps, size_t n, Source<Ctx> *q)
{
    for (size_t i = 0; i < n; i++) {
        const int rc = open_snapshot(snaps[i], q[i], q[i].cx);
        if (rc) return rc;
    }
    for (size_t i = 0; i + 1 < n; i++)
        if (q[i].device != q[n - 1].device) return LH_EINVAL;
    for (size_t i = 0; i < n; i++)
        if (!usable(q[i])) return LH_ESTATE;
    return LH_OK;
}
// (the context's mutex held)  What is enqueued on `to` from here on runs behind what every stream of from[0 .. n) holds now:
// an event per distinct stream other than `to` is recorded there and waited for by `to`.  ev[0 .. n): the unit's events for
// this, each created on first use.
static inline int order_behind(hipEvent_t *ev, const hipStream_t *from, size_t n, hipStream_t to)
{
    for (size_t i = 0; i < n; i++) {
        bool done = from[i] == to;
        for (size_t j = 0; j < i && !done; j++) done = from[j] == from[i];
        if (done) continue;
        if (!ev[i]) LH_BESIDE_CHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        LH_BESIDE_CHK(hipEventRecord(ev[i], from[i]));
        LH_BESIDE_CHK(hipStreamWaitEvent(to, ev[i], 0));
    }
    return LH_OK;
}
static inline int order_behind(hipEvent_t &ev, hipStream_t from, hipStream_t to) { return order_behind(&ev, &from, 1, to); }
inline const uint32_t *ranges_from(const Opened &o, uint32_t first) { return o.ranges + 2 * (size_t)first; }

// A host id list on its way to the kernel: the unit's two grown blocks (part of its context).
struct IdBlocks {
    uint32_t *h_ids = nullptr, *d_ids = nullptr; // the caller's list, copied (pinned); in HBM for the kernel
    size_t h_cap = 0, d_cap = 0;
};
// (the context's mutex held)  The id array the kernel of an id-list call reads, n > 0 entries: the caller's own device array,
// or the host list -- which rows_in has checked -- copied into the pinned block before this returns and from there into HBM
// by a copy on `st`, ahead of the kernel.  Only a host form stages, and it waits for `st` before it returns (after a failure
// too: settle_ids), so the two blocks are free again when the mutex is.  The kernel guards every id it reads whatever the
// host saw (lh::row_of): a list the caller changes under the call reads other rows, or none, never beyond the snapshot.
inline int stage_ids(IdBlocks &b, const RowSel &sel, size_t n, hipStream_t st, const uint32_t *&ids)
{
    ids = sel.ids;
    if (!sel.by_id || sel.on_device) return LH_OK;
    int rc = grow_pinned(b.h_ids, b.h_cap, n, 1024);
    if (!rc) rc = grow_device(b.d_ids, b.d_cap, n, 1024);
    if (rc) return rc;
    std::memcpy(b.h_ids, sel.ids, n * sizeof(uint32_t));
    LH_BESIDE_CHK(hipMemcpyAsync(b.d_ids, b.h_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ids = b.d_ids;
    return LH_OK;
}
// a host form's way out: after a failure behind stage_ids the copy may still be under way
inline int settle_ids(int rc, const RowSel &sel, hipStream_t st)
{
    if (rc && sel.by_id && !sel.on_device && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
    return rc;
}

// Host arrays of doubles, one element or one row per entry, on their way to the kernel as stage_ids' list is: the unit's two grown
// blocks (part of its context).
struct DoubleBlocks {
    double *h = nullptr, *d = nullptr; // the caller's arrays, copied (pinned); in HBM for the kernel
    size_t h_cap = 0, d_cap = 0;
};
// (the context's mutex held)  What the kernel of a HOST form reads for the caller's arrays a[0 .. na) and b[0 .. nb) (b may be null
// with nb == 0), which the call has checked: both copied into the pinned block before this returns, one behind the other, and from
// there into HBM by ONE copy on `st`, ahead of the kernel.  The host form waits for `st` before it returns, after a failure too, so
// the two blocks are free again when the mutex is.  A device form stages nothing: its kernel reads the caller's own device arrays.
inline int stage_doubles(DoubleBlocks &blk, const double *a, size_t na, const double *b, size_t nb, hipStream_t st, const double *&d_a,
                         const double *&d_b)
{
    int rc = grow_pinned(blk.h, blk.h_cap, na + nb, 1024);
    if (!rc) rc = grow_device(blk.d, blk.d_cap, na + nb, 1024);
    if (rc) return rc;
    std::memcpy(blk.h, a, na * sizeof(double));
    if (nb) std::memcpy(blk.h + na, b, nb * sizeof(double));
    LH_BESIDE_CHK(hipMemcpyAsync(blk.d, blk.h, (na + nb) * sizeof(double), hipMemcpyHostToDevice, st));
    d_a = blk.d;
    d_b = blk.d + na;
    return LH_OK;
}

// f(c): c the cells of row `first`, typed by their width (const uint32_t * or const unsigned long long *).  A generic
// lambda names the type as cell_of<decltype(c)>.
template <class P> using cell_of = std::remove_cv_t<std::remove_pointer_t<P>>;
template <class Ctx, class F> void with_cells(const Source<Ctx> &q, uint32_t first, F f)
{
    if (q.cell_bytes == 4) f(static_cast<const uint32_t *>(q.cells) + (size_t)first * q.stride);
    else f(static_cast<const lh::u64 *>(q.cells) + (size_t)first * q.stride);
}

// The launch shape of a call of M rows: a wave per row from `wave_from` rows on (the unit's switch), a workgroup per row
// below.
struct RowShape {
    bool wave;
    dim3 grid, block;
};
inline RowShape row_shape(uint32_t M, uint32_t wave_from)
{
    const bool wave = M >= wave_from;
    return {wave, dim3(wave ? (M + lh::ROW_WAVES - 1) / lh::ROW_WAVES : M), dim3(wave ? lh::ROW_BLOCK : lh::WG)};
}

// (the context's mutex held)  The unit's value table on this device (`slot`, null until the first call that needs it),
// generated by `kernel` (lh::k_value_table of the unit) on `st`.  The table is complete before the call that generates it
// goes on (one stream wait, once per device): later calls on other streams need no ordering against it.
static inline int ensure_table(double *&slot, hipStream_t st, void (*kernel)(double *))
{
    if (slot) return LH_OK;
    double *t = nullptr;
    LH_BESIDE_CHK(hipMalloc((void **)&t, (size_t)LH_NKEYS * sizeof(double)));
    hipLaunchKernelGGL(kernel, dim3(LH_NKEYS / 256), dim3(256), 0, st, t);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(t);
        return LH_EDEVICE;
    }
    slot = t;
    return LH_OK;
}

// lh_tool_*_switch: the rows from which a call takes its wave form; 0 restores the default
inline void switch_exchange(std::atomic<uint32_t> &v, uint32_t value, uint32_t dflt, uint32_t *previous)
{
    const uint32_t old = v.exchange(value ? value : dflt, std::memory_order_relaxed);
    if (previous) *previous = old;
}

} // namespace beside
} // namespace lh
