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

namespace {

using namespace lh::beside;
using lh::le_take;
using lh::load4_cells;
using lh::readlane_u64;
using lh::shfl_u64;
using lh::wave_scan_incl_u64;

typedef unsigned long long u64;

constexpr int CL_BLOCK = 256, CL_WAVES = CL_BLOCK / 64; // k_count_le_wave: four rows per workgroup
constexpr int CL_WG = 1024, CL_WG_WAVES = CL_WG / 64;   // k_count_le_block
constexpr uint32_t CL_STEP = 256;                       // bins a wave takes per step
constexpr uint32_t CL_CHUNKS = LH_NKEYS / CL_STEP;      // chunks of the widest span (a span starts at a multiple of 4)
// Rows of a call from which a row gets a wave, not a workgroup.  profiles/count_le.txt has both shapes either side: over
// windows of a few hundred bins the wave form is ahead from 1 024 rows on and the two are level at 256; over one
// full-span row the workgroup is several times faster -- so few rows, which may be wide, get workgroups.
constexpr uint32_t CL_WAVE_FROM_DEFAULT = 1024;
static_assert(CL_CHUNKS == 4 * 64, "wave 0 scans the chunk totals four per lane");

// shared bounds travel in the kernel arguments (512 bytes); per-metric ones are read from `pb`
struct LeBounds { double b[LH_MAX_BOUNDS]; };

// (how many leading bins a bound takes in: le_take, lh_wave.h)

template <typename CELL>
__global__ __launch_bounds__(CL_BLOCK) void k_count_le_wave(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                            uint32_t nmetrics, size_t stride, const LeBounds sb,
                                                            const double *__restrict__ pb, uint32_t nb, u64 *__restrict__ cum,
                                                            u64 *__restrict__ total)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * CL_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const uint32_t lo = ranges[2 * (size_t)m], hi = min(ranges[2 * (size_t)m + 1], (uint32_t)LH_NKEYS - 1);
    u64 res = 0, carry = 0;
    if (lo <= hi) { // wave-uniform; an empty row costs two loads and two stores
        const CELL *__restrict__ row = cells + (size_t)m * stride;
        const uint32_t base0 = lo & ~3u; // (cells below lo are zero) whole groups: every load is 16-byte aligned
        u64 c[4], nx[4];
        load4_cells(row, base0 + 4 * lane, hi, c);
        uint32_t E = 0;
        if (lane < nb) E = le_take(pb ? pb[(size_t)m * nb + lane] : sb.b[lane]);
        bool pend = lane < nb && E > base0; // a bound at or below the span's first bin: 0
        for (uint32_t base = base0; base <= hi; base += CL_STEP) {
            load4_cells(row, base + CL_STEP + 4 * lane, hi, nx); // the next step's cells: in flight under this step's scan
            const u64 t = (c[0] + c[1]) + (c[2] + c[3]);
            const u64 inc = wave_scan_incl_u64(t);
            // (every pending E is > base: an earlier step would have taken it otherwise)
            const bool in = pend && E <= base + CL_STEP;
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

template <typename CELL>
__global__ __launch_bounds__(CL_WG) void k_count_le_block(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                          uint32_t nmetrics, size_t stride, const LeBounds sb,
                                                          const double *__restrict__ pb, uint32_t nb, u64 *__restrict__ cum,
                                                          u64 *__restrict__ total)
{
    __shared__ u64 s_chunk[CL_CHUNKS]; // the chunks' totals, then their exclusive prefix
    __shared__ u64 s_total;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    if (m >= nmetrics) return;
    const uint32_t lo = ranges[2 * (size_t)m], hi = min(ranges[2 * (size_t)m + 1], (uint32_t)LH_NKEYS - 1);
    if (lo > hi) { // workgroup-uniform
        if (cum && threadIdx.x < nb) cum[(size_t)m * nb + threadIdx.x] = 0;
        if (total && threadIdx.x == 0) total[m] = 0;
        return;
    }
    const CELL *__restrict__ row = cells + (size_t)m * stride;
    const uint32_t base0 = lo & ~3u, nchunks = (hi - base0) / CL_STEP + 1; // <= CL_CHUNKS
    constexpr uint32_t U = 4;
    for (uint32_t c0 = wave; c0 < nchunks; c0 += CL_WG_WAVES * U) { // wave-uniform
        u64 t[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) { // (a chunk beyond the span starts beyond hi: nothing is read)
            u64 c[4];
            load4_cells(row, base0 + (c0 + u * CL_WG_WAVES) * CL_STEP + 4 * lane, hi, c);
            t[u] = (c[0] + c[1]) + (c[2] + c[3]);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const u64 inc = wave_scan_incl_u64(t[u]);
            const uint32_t ch = c0 + u * CL_WG_WAVES;
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
    for (uint32_t j = wave; j < nb; j += CL_WG_WAVES) { // a wave per bound (wave-uniform throughout)
        const uint32_t E = (uint32_t)__builtin_amdgcn_readfirstlane((int)le_take(pb ? pb[(size_t)m * nb + j] : sb.b[j]));
        u64 val = 0;
        if (E > base0) {
            const uint32_t idx = E - 1 - base0, ch = idx / CL_STEP;
            if (ch >= nchunks) {
                val = tot;
            } else {
                u64 c[4];
                load4_cells(row, base0 + ch * CL_STEP + 4 * lane, hi, c);
                const u64 t = (c[0] + c[1]) + (c[2] + c[3]);
                const u64 inc = wave_scan_incl_u64(t);
                const uint32_t k = idx & 3, f = (idx % CL_STEP) >> 2;
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
    hipEvent_t ev = nullptr;                // behind the last kernel that reads d_bounds, on whichever stream that was
    bool ev_pending = false;                // cleared only by a wait on `ev` itself: another stream's sync says nothing
};
std::atomic<uint32_t> g_wave_from{CL_WAVE_FROM_DEFAULT};

// every check that needs neither the snapshot nor a device
int check_args(lh_snapshot *s, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, const void *cum, const void *total)
{
    if (!s || nb == 0 || nb > LH_MAX_BOUNDS || !bounds || (!cum && !total) || (flags & ~(uint32_t)LH_LE_PER_METRIC)) return LH_EINVAL;
    if (misaligned(bounds, 8) || misaligned(cum, 8) || misaligned(total, 8)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32): not a row of bounds is read
    const size_t rows = (flags & LH_LE_PER_METRIC) ? nmetrics : 1;
    for (size_t r = 0; r < rows; r++) {
        const double *b = bounds + r * nb;
        for (size_t j = 0; j < nb; j++)
            if (b[j] != b[j] || (j && b[j] < b[j - 1])) return LH_EINVAL; // NaN / a decreasing row (-0.0 == 0.0)
    }
    return LH_OK;
}

struct Source : Opened {
    CountCtx *cx = nullptr;
    const void *cells = nullptr;
    uint32_t nrows = 0, cell_bytes = 0;
};

// (cx->mu held) enqueue the count of rows [first, first + nmetrics) on the snapshot's stream
int enqueue(const Source &q, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, u64 *d_cum,
            u64 *d_total)
{
    CountCtx *cx = q.cx;
    LeBounds sb;
    const double *pb = nullptr;
    if (flags & LH_LE_PER_METRIC) {
        const size_t n = nmetrics * nb;
        if (cx->ev_pending) { // an earlier call's copy / kernel may still read the two blocks
            LH_BESIDE_CHK(hipEventSynchronize(cx->ev));
            cx->ev_pending = false;
        }
        int rc = grow_pinned(cx->h_bounds, cx->hb_cap, n, 4096);
        if (!rc) rc = grow_device(cx->d_bounds, cx->db_cap, n, 4096);
        if (rc) return rc;
        if (!cx->ev) LH_BESIDE_CHK(hipEventCreateWithFlags(&cx->ev, hipEventDisableTiming));
        std::memcpy(cx->h_bounds, bounds, n * sizeof(double));
        // (into HBM by the copy engine, not fetched over PCIe by every wave)
        LH_BESIDE_CHK(hipMemcpyAsync(cx->d_bounds, cx->h_bounds, n * sizeof(double), hipMemcpyHostToDevice, q.stream));
        std::memset(sb.b, 0, sizeof sb.b);
        pb = cx->d_bounds;
    } else {
        for (size_t j = 0; j < LH_MAX_BOUNDS; j++) sb.b[j] = j < nb ? bounds[j] : 0.0;
    }
    const uint32_t M = (uint32_t)nmetrics, NB = (uint32_t)nb;
    const uint32_t *ranges = q.ranges + 2 * (size_t)first;
    const bool wave = M >= g_wave_from.load(std::memory_order_relaxed);
    const dim3 grid(wave ? (M + CL_WAVES - 1) / CL_WAVES : M), block(wave ? CL_BLOCK : CL_WG);
    if (q.cell_bytes == 4) {
        const uint32_t *c = static_cast<const uint32_t *>(q.cells) + (size_t)first * q.stride;
        if (wave) hipLaunchKernelGGL(k_count_le_wave<uint32_t>, grid, block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum, d_total);
        else hipLaunchKernelGGL(k_count_le_block<uint32_t>, grid, block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum, d_total);
    } else {
        const u64 *c = static_cast<const u64 *>(q.cells) + (size_t)first * q.stride;
        if (wave) hipLaunchKernelGGL(k_count_le_wave<u64>, grid, block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum, d_total);
        else hipLaunchKernelGGL(k_count_le_block<u64>, grid, block, 0, q.stream, c, ranges, M, q.stride, sb, pb, NB, d_cum, d_total);
    }
    LH_BESIDE_CHK(hipGetLastError());
    if (pb) {
        LH_BESIDE_CHK(hipEventRecord(cx->ev, q.stream));
        cx->ev_pending = true;
    }
    return LH_OK;
}

int count_le(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, uint64_t *cum,
             uint64_t *total, bool device_form)
{
    int rc = check_args(s, nmetrics, bounds, nb, flags, cum, total);
    if (rc) return rc;
    Source q;
    void *cells = nullptr;
    rc = lh_snapshot_cells(s, &cells, &q.nrows, &q.cell_bytes);
    if (rc) return rc;
    q.cells = cells;
    if (nmetrics > q.nrows || first > q.nrows - nmetrics) return LH_ERANGE;
    if (nmetrics == 0) return LH_OK;
    rc = open_snapshot(s, q, q.cx);
    if (rc) return rc;
    if (q.stride < (size_t)LH_NKEYS + 4 || !q.cells || (q.cell_bytes != 4 && q.cell_bytes != 8)) return LH_ESTATE;
    CountCtx *cx = q.cx;
    std::lock_guard<std::mutex> g(cx->mu);
    if (device_form)
        return enqueue(q, first, nmetrics, bounds, nb, flags, reinterpret_cast<u64 *>(cum), reinterpret_cast<u64 *>(total));

    // host form: results to HBM, then back to the caller's arrays
    const HostOut out[2] = {{cum, nmetrics * nb * sizeof(u64)}, {total, nmetrics * sizeof(u64)}};
    rc = host_results(cx->res, q.stream, out, [&](unsigned char *const(&dev)[2]) {
        return enqueue(q, first, nmetrics, bounds, nb, flags, reinterpret_cast<u64 *>(dev[0]), reinterpret_cast<u64 *>(dev[1]));
    });
    if (rc) return rc;
    if (flags & LH_LE_PER_METRIC) cx->ev_pending = false; // this call recorded `ev` on the stream it has just waited for
    return LH_OK;
}

} // namespace

extern "C" {

int lh_count_le(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags, uint64_t *cum,
                uint64_t *total)
{
    return count_le(s, first, nmetrics, bounds, nb, flags, cum, total, false);
}

int lh_count_le_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags,
                       uint64_t *d_cum, uint64_t *d_total)
{
    return count_le(s, first, nmetrics, bounds, nb, flags, d_cum, d_total, true);
}

int lh_tool_count_le_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, CL_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

} // extern "C"
