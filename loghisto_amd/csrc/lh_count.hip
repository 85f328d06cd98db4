// lh_count.hip -- lh_count_le* (include/loghisto_gpu.h): how many of a snapshot's samples lie at or below given values,
// per name.  The running count of percentile()'s bucket walk (/root/reference/metrics.go:389-418) read at a VALUE
// instead of searched for a fraction: cum[m][j] = sum of the cells of metric m (metrics.go:54-60, 278) whose key is
// <= compress(bounds[j]) (metrics.go:316-322), total[m] = all of them.  Counts, unlike percentiles, add up across
// intervals, ranks and processes.
//
// Built BESIDE the engine, on its public C ABI only: lh_beside.h says what that gives a reader.  Read-only.
//
// A bound becomes E = the number of leading bins it takes in (0 .. 65 536): bin(compress(b)) + 1, by the same
// arithmetic the threshold table of the ingest is generated with (lh::d_kext_golog of 1 + |b|); 0 for -Inf and for
// negative bounds beyond the int16 key range, 65 536 for +Inf and positive ones beyond it.  cum = the prefix sum of the
// row at E.
//
// Two shapes, chosen by the number of rows of the call (lh_tool_count_le_switch moves the switch for measurements):
//   k_count_le_wave   one WAVE per row, 256 bins per step (4 consecutive bins per lane: one 16-byte load of 32-bit
//                     cells, two of 64-bit ones, only by lanes whose group starts at or below hi), 64-bit lane sums, a
//                     DPP inclusive scan, and -- only in a step that some bound's bin falls into (one ballot) -- the
//                     prefix at that bin fetched from the lane that owns it.  The next step's loads are issued before
//                     the current step is scanned.  For thousands of rows with narrow spans.
//   k_count_le_block  one WORKGROUP of 16 waves per row: the waves sum the row's 256-bin chunks independently (four
//                     chunks in flight per wave), wave 0 scans the chunk totals in LDS, and each bound then costs one
//                     more read of the one chunk its bin lies in.  A single wave walks a full-span row (65 536 bins,
//                     512 KiB) as 256 dependent steps; this form takes two barriers.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <type_traits>

namespace {

using namespace lh; // (lh_wave.h)
using namespace lh::beside;

// Rows of a call from which a row gets a wave, not a workgroup.  profiles/count_le.txt has both shapes either side: over
// windows of a few hundred bins the wave form is ahead from 1 024 rows on and the two are level at 256; over one
// full-span row the workgroup is several times faster -- so few rows, which may be wide, get workgroups.
constexpr uint32_t CL_WAVE_FROM_DEFAULT = 1024;

// shared bounds travel in the kernel arguments (512 bytes); per-metric ones are read from `pb`
struct LeBounds { double b[LH_MAX_BOUNDS]; };

// (Both kernels, IDS: entry m reads row ids[m] of the snapshot -- lh::row_of, whose guard against `nrows` leaves an empty span;
// m still indexes the outputs and the per-metric bounds.  Otherwise row m of the block; ids and nrows are not looked at.)
template <typename CELL, bool IDS>
__global__ __launch_bounds__(ROW_BLOCK) void k_count_le_wave(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                            uint32_t nmetrics, size_t stride, const LeBounds sb,
                                                            const double *__restrict__ pb, uint32_t nb, u64 *__restrict__ cum,
                                                            u64 *__restrict__ total, const uint32_t *__restrict__ ids,
                                                            uint32_t nrows)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const uint32_t r = row_of<IDS>(ids, nrows, m);
    const Span sp = row_span<IDS>(ranges, r);
    const uint32_t hi = sp.hi;
    u64 res = 0, carry = 0;
    if (sp.any()) { // wave-uniform; an empty row costs two loads and two stores
        const CELL *__restrict__ row = cells + (size_t)r * stride;
        const uint32_t base0 = sp.base0();
        u64 c[4], nx[4];
        load4_cells(row, base0 + 4 * lane, hi, c);
        uint32_t E = 0;
        if (lane < nb) E = le_take(pb ? pb[(size_t)m * nb + lane] : sb.b[lane]);
        bool pend = lane < nb && E > base0; // a bound at or below the span's first bin: 0
        for (uint32_t base = base0; base <= hi; base += STEP) {
            load4_cells(row, base + STEP + 4 * lane, hi, nx); // the next step's cells: in flight under this step's scan
            const u64 t = (c[0] + c[1]) + (c[2] + c[3]);
            const u64 inc = wave_scan_incl_u64(t);
            // (every pending E is > base: an earlier step would have taken it otherwise)
            const bool in = pend && E <= base + STEP;
            if (__builtin_amdgcn_ballot_w64(in)) { // wave-uniform
                const uint32_t idx = in ? E - 1 - base : 0, f = idx >> 2, k = idx & 3;
                const u64 p0 = carry + (inc - t) + c[0], p1 = p0 + c[1], p2 = p1 + c[2], p3 = p2 + c[3];
                const u64 v0 = shfl_u64(p0, f), v1 = shfl_u64(p1, f), v2 = shfl_u64(p2, f), v3 = shfl_u64(p3, f);
                if (in) {
                    res = k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3;
                    pend = false;
                }
            }
            carry += readlane_u64(inc, 63);
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = nx[k];
        }
        if (pend) res = carry; // beyond the last step: everything
    }
    if (cum && lane < nb) cum[(size_t)m * nb + lane] = res;
    if (total && lane == 0) total[m] = carry;
}

template <typename CELL, bool IDS>
__global__ __launch_bounds__(WG) void k_count_le_block(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                          uint32_t nmetrics, size_t stride, const LeBounds sb,
                                                          const double *__restrict__ pb, uint32_t nb, u64 *__restrict__ cum,
                                                          u64 *__restrict__ total, const uint32_t *__restrict__ ids,
                                                          uint32_t nrows)
{
    __shared__ u64 s_chunk[CHUNKS]; // the chunks' totals, then their exclusive prefix
    __shared__ u64 s_total;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    if (m >= nmetrics) return;
    const uint32_t r = row_of<IDS>(ids, nrows, m);
    const Span sp = row_span<IDS>(ranges, r);
    const uint32_t hi = sp.hi;
    if (!sp.any()) { // workgroup-uniform
        if (cum && threadIdx.x < nb) cum[(size_t)m * nb + threadIdx.x] = 0;
        if (total && threadIdx.x == 0) total[m] = 0;
        return;
    }
    const CELL *__restrict__ row = cells + (size_t)r * stride;
    const uint32_t base0 = sp.base0(), nchunks = (hi - base0) / STEP + 1; // <= CHUNKS
    constexpr uint32_t U = 4;
    for (uint32_t c0 = wave; c0 < nchunks; c0 += WG_WAVES * U) { // wave-uniform
        u64 t[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) { // (a chunk beyond the span starts beyond hi: nothing is read)
            u64 c[4];
            load4_cells(row, base0 + (c0 + u * WG_WAVES) * STEP + 4 * lane, hi, c);
            t[u] = (c[0] + c[1]) + (c[2] + c[3]);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const u64 inc = wave_scan_incl_u64(t[u]);
            const uint32_t ch = c0 + u * WG_WAVES;
            if (lane == 63 && ch < nchunks) s_chunk[ch] = inc;
        }
    }
    __syncthreads();
    if (wave == 0) {
        u64 v[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) v[k] = 4 * lane + k < nchunks ? s_chunk[4 * lane + k] : 0;
        const u64 t = (v[0] + v[1]) + (v[2] + v[3]);
        const u64 inc = wave_scan_incl_u64(t);
        u64 ex = inc - t;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            s_chunk[4 * lane + k] = ex;
            ex += v[k];
        }
        if (lane == 63) s_total = inc;
    }
    __syncthreads();
    const u64 tot = s_total;
    for (uint32_t j = wave; j < nb; j += WG_WAVES) { // a wave per bound (wave-uniform throughout)
        const uint32_t E = (uint32_t)__builtin_amdgcn_readfirstlane((int)le_take(pb ? pb[(size_t)m * nb + j] : sb.b[j]));
        u64 val = 0;
        if (E > base0) {
            const uint32_t idx = E - 1 - base0, ch = idx / STEP;
            if (ch >= nchunks) {
                val = tot;
            } else {
                u64 c[4];
                load4_cells(row, base0 + ch * STEP + 4 * lane, hi, c);
                const u64 t = (c[0] + c[1]) + (c[2] + c[3]);
                const u64 inc = wave_scan_incl_u64(t);
                const uint32_t k = idx & 3, f = (idx % STEP) >> 2;
                const u64 pre = (inc - t) + c[0] + (k >= 1 ? c[1] : 0) + (k >= 2 ? c[2] : 0) + (k >= 3 ? c[3] : 0);
                val = s_chunk[ch] + readlane_u64(pre, f);
            }
        }
        if (cum && lane == 0) cum[(size_t)m * nb + j] = val;
    }
    if (total && threadIdx.x == 0) total[m] = tot;
}

// ---- host side --------------------------------------------------------------------------------------
// Per-device state of this unit (device_ctx<CountCtx>).  `mu` is held for the length of a call -- the host form's wait for
// its results included, so host-form calls on one device take turns even when their snapshots belong to different engines.
// Snapshots of different engines run on different streams: everything below that outlives a call (the bounds blocks) is
// guarded by an event, not by stream order.
struct CountCtx {
    std::mutex mu;
    ResultBlocks res;                       // host form
    double *h_bounds = nullptr, *d_bounds = nullptr; // per-metric bounds: the caller's, copied (pinned); in HBM for the kernel
    size_t hb_cap = 0, db_cap = 0;          // (in doubles)
    EventGuard guard;                       // behind the last kernel that reads d_bounds
    IdBlocks ids;                           // host form of lh_count_le_ids
};
std::atomic<uint32_t> g_wave_from{CL_WAVE_FROM_DEFAULT};

// every check that needs neither the snapshot nor a device
int check_args(lh_snapshot *s, const RowSel &sel, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, const void *cum,
               const void *total)
{
    if (bad_ids(sel, nmetrics)) return LH_EINVAL;
    if (!s || nb == 0 || nb > LH_MAX_BOUNDS || !bounds || (!cum && !total) || (flags & ~(uint32_t)LH_LE_PER_METRIC)) return LH_EINVAL;
    if (misaligned(bounds, 8) || misaligned(cum, 8) || misaligned(total, 8)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32): not a row of bounds is read
    const size_t rows = (flags & LH_LE_PER_METRIC) ? nmetrics : 1;
    for (size_t r = 0; r < rows; r++)
        if (bad_bounds(bounds + r * nb, nb)) return LH_EINVAL; // NaN / a decreasing row (-0.0 == 0.0)
    return LH_OK;
}

typedef lh::beside::Source<CountCtx> Source;

// (cx->mu held) enqueue the count of rows [first, first + nmetrics), or of rows ids[0 .. nmetrics), on the snapshot's stream
int enqueue(const Source &q, const RowSel &sel, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, u64 *d_cum,
            u64 *d_total)
{
    CountCtx *cx = q.cx;
    const uint32_t *ids = nullptr;
    const int ri = stage_ids(cx->ids, sel, nmetrics, q.stream, ids);
    if (ri) return ri;
    LeBounds sb;
    const double *pb = nullptr;
    if (flags & LH_LE_PER_METRIC) {
        const size_t n = nmetrics * nb;
        int rc = cx->guard.host_wait(); // an earlier call's copy / kernel may still read the two blocks
        if (!rc) rc = grow_pinned(cx->h_bounds, cx->hb_cap, n, 4096);
        if (!rc) rc = grow_device(cx->d_bounds, cx->db_cap, n, 4096);
        if (!rc) rc = cx->guard.create();
        if (rc) return rc;
        std::memcpy(cx->h_bounds, bounds, n * sizeof(double));
        // (into HBM by the copy engine, not fetched over PCIe by every wave)
        LH_BESIDE_CHK(hipMemcpyAsync(cx->d_bounds, cx->h_bounds, n * sizeof(double), hipMemcpyHostToDevice, q.stream));
        std::memset(sb.b, 0, sizeof sb.b);
        pb = cx->d_bounds;
    } else {
        for (size_t j = 0; j < LH_MAX_BOUNDS; j++) sb.b[j] = j < nb ? bounds[j] : 0.0;
    }
    const uint32_t M = (uint32_t)nmetrics, NB = (uint32_t)nb;
    const uint32_t *ranges = ranges_from(q, sel.first);
    const RowShape sh = row_shape(M, g_wave_from.load(std::memory_order_relaxed));
    const auto launch = [&](auto by_id) {
        constexpr bool IDS = decltype(by_id)::value;
        with_cells(q, sel.first, [&](auto *c) {
            typedef cell_of<decltype(c)> CELL;
            if (sh.wave)
                hipLaunchKernelGGL((k_count_le_wave<CELL, IDS>), sh.grid, sh.block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum,
                                   d_total, ids, q.nrows);
            else
                hipLaunchKernelGGL((k_count_le_block<CELL, IDS>), sh.grid, sh.block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum,
                                   d_total, ids, q.nrows);
        });
    };
    if (sel.by_id) launch(std::true_type());
    else launch(std::false_type());
    LH_BESIDE_CHK(hipGetLastError());
    return pb ? cx->guard.record(q.stream) : LH_OK;
}

int count_le(lh_snapshot *s, const RowSel &sel, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, uint64_t *cum,
             uint64_t *total, bool device_form)
{
    int rc = check_args(s, sel, nmetrics, bounds, nb, flags, cum, total);
    if (rc) return rc;
    Source q;
    rc = source_cells(s, sel, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) return LH_OK; // before any device call
    rc = source_open(s, q);
    if (rc) return rc;
    CountCtx *cx = q.cx;
    std::lock_guard<std::mutex> g(cx->mu);
    if (device_form)
        return enqueue(q, sel, nmetrics, bounds, nb, flags, reinterpret_cast<u64 *>(cum), reinterpret_cast<u64 *>(total));

    // host form: results to HBM, then back to the caller's arrays
    const HostOut out[2] = {{cum, nmetrics * nb * sizeof(u64)}, {total, nmetrics * sizeof(u64)}};
    rc = host_results(cx->res, q.stream, out, [&](unsigned char *const(&dev)[2]) {
        return enqueue(q, sel, nmetrics, bounds, nb, flags, reinterpret_cast<u64 *>(dev[0]), reinterpret_cast<u64 *>(dev[1]));
    });
    if (rc) return settle_ids(rc, sel, q.stream);
    if (flags & LH_LE_PER_METRIC) cx->guard.covered(); // this call recorded the event on the stream it has just waited for
    return LH_OK;
}

} // namespace

extern "C" {

int lh_count_le(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, uint64_t *cum,
                uint64_t *total)
{
    return count_le(s, rows_from(first), nmetrics, bounds, nb, flags, cum, total, false);
}

int lh_count_le_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags,
                       uint64_t *d_cum, uint64_t *d_total)
{
    return count_le(s, rows_from(first), nmetrics, bounds, nb, flags, d_cum, d_total, true);
}

int lh_count_le_ids(lh_snapshot *s, const uint32_t *ids, size_t n, const double *bounds, size_t nb, uint32_t flags, uint64_t *cum,
                    uint64_t *total)
{
    return count_le(s, rows_by_id(ids, false), n, bounds, nb, flags, cum, total, false);
}

int lh_count_le_ids_device(lh_snapshot *s, const uint32_t *d_ids, size_t n, const double *bounds, size_t nb, uint32_t flags,
                           uint64_t *d_cum, uint64_t *d_total)
{
    return count_le(s, rows_by_id(d_ids, true), n, bounds, nb, flags, d_cum, d_total, true);
}

int lh_tool_count_le_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, CL_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

} // extern "C"
