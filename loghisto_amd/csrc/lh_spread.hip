// lh_spread.hip -- lh_spread* (include/loghisto_gpu.h): how spread out a name's samples are, and what they add up to once
// the slowest few per cent are cut off.  One more weighted walk of the kind processHistograms does
// (/root/reference/metrics.go:342-346: `sum += value * float64(count)` over the buckets), cut at the bucket percentile()
// selects (metrics.go:406-418: the first bucket at which float64(sofar) / float64(total) >= p).  Per name:
//   count = sum of c[b]                     sum = sum of D[b] * float64(c[b])            (metrics.go:344)
//   m2    = sum of float64(c[b]) * (D[b] - sum / float64(count))^2     -- the CENTRED second moment, in a second walk
// and per percentile the selected key, the inclusive prefix count at its bin and the prefix of `sum` there.  From these a
// caller has statsd's std / mean_90 / sum_90 / count_90 / upper_90, a registry's stddev and the mean of the tail.
// RESOLUTION IS THE BUCKET, as for lh_count_le: every sample of the selected bucket is taken in.
//
// Built BESIDE the engine, on its public C ABI only: lh_beside.h says what that gives a reader.  Read-only.
//
// D[b] = decompress(bin_to_key(b)) comes from a table this unit generates once per device with lh::d_decompress_bin (this
// file is built with -ffp-contract=off like the engine's own generator: the same instructions, the same bits as the D[] of
// lh_codec_tables).  512 KiB, resident in L2 beside the windows; evaluating exp() per cell would cost an IEEE divide each.
//
// Two shapes, chosen by the number of rows of the call (lh_tool_spread_switch moves the switch for measurements):
//   k_spread_wave   one WAVE per row, 256 bins per step (4 consecutive bins per lane: one 16-byte load of 32-bit cells,
//                   two of 64-bit ones, and two 16-byte loads of the table, only by lanes whose group starts at or below
//                   hi), 64-bit lane counts, double lane sums, DPP inclusive scans; the next step's loads are issued before
//                   the current step is worked on.  For thousands of rows with narrow spans.
//   k_spread_block  one WORKGROUP of 16 waves per row: the waves reduce the row's 256-bin chunks independently, wave 0
//                   scans the chunk totals in LDS, and each percentile then costs one more read of the one chunk its
//                   threshold falls into.  For calls of few rows, which may span all 65 536 bins.
// Each row takes two walks.  Walk 1 gives count and sum, hence the mean and the thresholds T = the smallest prefix count
// that reaches p (pct_threshold, lh_wave.h: tests/test_pct_threshold_model.py has the arithmetic).  Walk 2 re-reads the window
// (L2-resident at typical spans) for m2 and, in the steps a threshold falls into, the key, count_le and sum_le.  The walk's
// state, the chunk scan and lookup and the key's store are lh_pct.h's.
// Every floating-point sum is taken in a fixed order (per lane over the steps in ascending order, then one DPP tree over
// the lanes; chunk totals in ascending order), so a result does not depend on timing -- but the two shapes associate
// differently and agree to rounding only.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_pct.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <type_traits>

namespace {

using namespace lh; // (lh_wave.h, lh_pct.h)
using namespace lh::beside;

// Rows of a call from which a row gets a wave, not a workgroup.  profiles/spread.txt has both shapes either side: over
// windows of a few hundred bins the workgroup is ahead at 256 rows (13.4 against 16.6 us at nine percentiles) and the wave
// from 1 024 on (16.4 against 23.5); over one full-span row the workgroup is four to five times faster -- so few rows,
// which may be wide, get workgroups.
constexpr uint32_t SP_WAVE_FROM_DEFAULT = 1024;

// (SpreadOut, central4 and sums_in_step are lh_pct.h's: lh_kept.hip's k_kept_spread takes the same walk 2.)

// (Both kernels, IDS: entry m reads row ids[m] of the snapshot -- lh::row_of, whose guard against `nrows` leaves an empty span;
// m still indexes the outputs.  Otherwise row m of the block; ids and nrows are not looked at.)
template <typename CELL, bool IDS>
__global__ __launch_bounds__(ROW_BLOCK) void k_spread_wave(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                          uint32_t nmetrics, size_t stride, const double *__restrict__ D,
                                                          const PctArgs pa, uint32_t np, const SpreadOut o,
                                                          const uint32_t *__restrict__ ids, uint32_t nrows)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const uint32_t r = row_of<IDS>(ids, nrows, m);
    const Span sp = row_span<IDS>(ranges, r);
    const uint32_t hi = sp.hi;
    u64 total = 0, r_cle = 0;
    double sum = 0.0, m2 = 0.0, r_sle = 0.0;
    Open pct; // lane i < np: percentile i
    if (sp.any()) {               // wave-uniform; an empty row costs two loads and its stores
        const CELL *__restrict__ row = cells + (size_t)r * stride;
        const uint32_t base0 = sp.base0();
        u64 c[4], nc[4];
        double d[4], nd[4], t[4];
        // ---- walk 1: count and sum
        {
            u64 cnt = 0;
            double ps = 0.0;
            load4(row, D, base0 + 4 * lane, hi, c, d);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4(row, D, base + STEP + 4 * lane, hi, nc, nd); // the next step's: in flight under this step's work
                cnt += (c[0] + c[1]) + (c[2] + c[3]);
                ps += terms4(c, d, t);
#pragma unroll
                for (int k = 0; k < 4; k++) { c[k] = nc[k]; d[k] = nd[k]; }
            }
            total = readlane_u64(wave_scan_incl_u64(cnt), 63);
            sum = readlane_f64(wave_scan_incl_f64(ps), 63);
        }
        if (total) { // wave-uniform
            // ---- walk 2: the centred moment; the steps the thresholds fall into
            const double mean = sum / (double)total;
            pct.open(lane < np ? pct_threshold(pa.p[lane], total) : PCT_NONE);
            double run = 0.0, q = 0.0; // the lane's terms of the steps so far; its share of m2
            load4(row, D, base0 + 4 * lane, hi, c, d);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4(row, D, base + STEP + 4 * lane, hi, nc, nd);
                q += central4(c, d, mean);
                const double ts = terms4(c, d, t);
                if (pct.todo) { // wave-uniform
                    const u64 tc = (c[0] + c[1]) + (c[2] + c[3]);
                    uint32_t here = pct.ending(tc);
                    if (here) {
                        u64 pre[4];
                        pct.prefixes(c, tc, pre);
                        const double sbefore = readlane_f64(wave_scan_incl_f64(run), 63);
                        const double incs = wave_scan_incl_f64(ts);
                        for (; here; here &= here - 1) {
                            const uint32_t i = (uint32_t)__builtin_ctz(here);
                            u64 cle;
                            double sle;
                            const uint32_t idx = sums_in_step(pre, t, incs, sbefore, pct.threshold(i), cle, sle);
                            if (lane == i) {
                                pct.found = base + idx;
                                r_cle = cle;
                                r_sle = sle;
                            }
                        }
                    }
                }
                run += ts;
#pragma unroll
                for (int k = 0; k < 4; k++) { c[k] = nc[k]; d[k] = nd[k]; }
            }
            m2 = readlane_f64(wave_scan_incl_f64(q), 63);
        } else {
            sum = 0.0;
        }
    }
    if (lane == 0) {
        if (o.count) o.count[m] = total;
        if (o.sum) o.sum[m] = sum;
        if (o.m2) o.m2[m] = m2;
    }
    if (lane < np) {
        const size_t at = (size_t)m * np + lane;
        store_pct(o.pkeys, o.pvalid, at, pct.found);
        if (o.count_le) o.count_le[at] = r_cle;
        if (o.sum_le) o.sum_le[at] = r_sle;
    }
}

template <typename CELL, bool IDS>
__global__ __launch_bounds__(WG) void k_spread_block(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                        uint32_t nmetrics, size_t stride, const double *__restrict__ D,
                                                        const PctArgs pa, uint32_t np, const SpreadOut o,
                                                        const uint32_t *__restrict__ ids, uint32_t nrows)
{
    __shared__ u64 s_cnt[CHUNKS];    // the chunks' counts, then their exclusive prefix
    __shared__ double s_sum[CHUNKS]; // the chunks' sums, then their exclusive prefix (ascending order)
    __shared__ double s_m2[WG_WAVES];
    __shared__ u64 s_total;
    __shared__ double s_tsum;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    if (m >= nmetrics) return;
    const uint32_t r = row_of<IDS>(ids, nrows, m);
    const Span sp = row_span<IDS>(ranges, r);
    const uint32_t hi = sp.hi;
    const CELL *__restrict__ row = cells + (size_t)(IDS && r == NO_ROW ? 0 : r) * stride; // (no row: never read, nchunks is 0)
    const uint32_t base0 = sp.base0(), nchunks = sp.any() ? (hi - base0) / STEP + 1 : 0; // <= CHUNKS
    constexpr uint32_t U = 2;
    // ---- walk 1: every chunk's count and sum
    for (uint32_t c0 = wave; c0 < nchunks; c0 += WG_WAVES * U) { // wave-uniform
        u64 c[U][4];
        double d[U][4], t[4];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) // (a chunk beyond the span starts beyond hi: nothing is read)
            load4(row, D, base0 + (c0 + u * WG_WAVES) * STEP + 4 * lane, hi, c[u], d[u]);
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const u64 inc = wave_scan_incl_u64((c[u][0] + c[u][1]) + (c[u][2] + c[u][3]));
            const double incs = wave_scan_incl_f64(terms4(c[u], d[u], t));
            const uint32_t ch = c0 + u * WG_WAVES;
            if (lane == 63 && ch < nchunks) {
                s_cnt[ch] = inc;
                s_sum[ch] = incs;
            }
        }
    }
    __syncthreads();
    if (wave == 0) scan_chunks((lds_u64)s_cnt, (lds_f64)s_sum, nchunks, lane, (lds_u64)&s_total, (lds_f64)&s_tsum);
    __syncthreads();
    const u64 total = s_total;
    if (total == 0) { // workgroup-uniform: an empty row, or a span over nothing but zeros
        if (threadIdx.x == 0) {
            if (o.count) o.count[m] = 0;
            if (o.sum) o.sum[m] = 0.0;
            if (o.m2) o.m2[m] = 0.0;
        }
        if (threadIdx.x < np) {
            const size_t at = (size_t)m * np + threadIdx.x;
            if (o.pkeys) o.pkeys[at] = 0;
            if (o.pvalid) o.pvalid[at] = 0;
            if (o.count_le) o.count_le[at] = 0;
            if (o.sum_le) o.sum_le[at] = 0.0;
        }
        return;
    }
    const double sum = s_tsum, mean = sum / (double)total;
    // ---- walk 2: the centred moment, by the same chunks
    {
        double q = 0.0;
        for (uint32_t c0 = wave; c0 < nchunks; c0 += WG_WAVES * U) {
            u64 c[U][4];
            double d[U][4];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) load4(row, D, base0 + (c0 + u * WG_WAVES) * STEP + 4 * lane, hi, c[u], d[u]);
#pragma unroll
            for (uint32_t u = 0; u < U; u++) q += central4(c[u], d[u], mean);
        }
        const double qs = wave_scan_incl_f64(q);
        if (lane == 63) s_m2[wave] = qs;
    }
    // ---- a wave per percentile (wave-uniform throughout): the chunk its threshold falls into, read once more
    for (uint32_t i = wave; i < np; i += WG_WAVES) {
        const u64 T = pct_threshold(pa.p[i], total);
        uint32_t bin = 0xffffffffu;
        u64 cle = 0;
        double sle = 0.0;
        if (T != PCT_NONE) {
            const uint32_t ch = chunk_of((lds_u64)s_cnt, nchunks, lane, T);
            u64 c[4], pre[4];
            double d[4], t[4];
            load4(row, D, base0 + ch * STEP + 4 * lane, hi, c, d);
            const double ts = terms4(c, d, t);
            const u64 tc = (c[0] + c[1]) + (c[2] + c[3]);
            // (prefix4, lh_pct.h, written out: through the helper this kernel measures 1 % slower, profiles/pct_walk_isa.txt)
            u64 sofar = s_cnt[ch] + (wave_scan_incl_u64(tc) - tc);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sofar += c[k];
                pre[k] = sofar;
            }
            bin = base0 + ch * STEP + sums_in_step(pre, t, wave_scan_incl_f64(ts), s_sum[ch], T, cle, sle);
        }
        if (lane == 0) {
            const size_t at = (size_t)m * np + i;
            store_pct(o.pkeys, o.pvalid, at, bin);
            if (o.count_le) o.count_le[at] = cle;
            if (o.sum_le) o.sum_le[at] = sle;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double m2 = 0.0;
        for (int w = 0; w < WG_WAVES; w++) m2 += s_m2[w]; // (a wave without a chunk left +0)
        if (o.count) o.count[m] = total;
        if (o.sum) o.sum[m] = sum;
        if (o.m2) o.m2[m] = m2;
    }
}

// ---- host side --------------------------------------------------------------------------------------
// Per-device state of this unit (device_ctx<SpreadCtx>).  `mu` is held for the length of a call -- the host form's wait
// for its results included, so host-form calls on one device take turns even when their snapshots belong to different
// engines.
struct SpreadCtx {
    std::mutex mu;
    double *d_table = nullptr; // D[LH_NKEYS]
    ResultBlocks res;          // host form
    IdBlocks ids;              // host form of lh_spread_ids
};
std::atomic<uint32_t> g_wave_from{SP_WAVE_FROM_DEFAULT};

// every check that needs neither the snapshot nor a device (the percentiles' and the outputs': lh_pct.h's check_spread_args)
int check_args(lh_snapshot *s, const RowSel &sel, size_t nmetrics, const double *p, size_t np, SpreadOut &o)
{
    if (bad_ids(sel, nmetrics) || !s) return LH_EINVAL;
    const int rc = check_spread_args(p, np, o);
    if (rc) return rc;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    return LH_OK;
}

typedef lh::beside::Source<SpreadCtx> Source;

// (cx->mu held) enqueue the walks of rows [first, first + nmetrics), or of rows ids[0 .. nmetrics), on the snapshot's stream
int enqueue(const Source &q, const RowSel &sel, size_t nmetrics, const double *p, size_t np, const SpreadOut &o)
{
    SpreadCtx *cx = q.cx;
    const uint32_t *ids = nullptr;
    int rc = ensure_table(cx->d_table, q.stream, lh::k_value_table<SpreadCtx>);
    if (!rc) rc = stage_ids(cx->ids, sel, nmetrics, q.stream, ids);
    if (rc) return rc;
    const PctArgs pa = pct_args(p, np);
    const uint32_t M = (uint32_t)nmetrics, NP = (uint32_t)np;
    const uint32_t *ranges = ranges_from(q, sel.first);
    const double *D = cx->d_table;
    const RowShape sh = row_shape(M, g_wave_from.load(std::memory_order_relaxed));
    const auto launch = [&](auto by_id) {
        constexpr bool IDS = decltype(by_id)::value;
        with_cells(q, sel.first, [&](auto *c) {
            typedef cell_of<decltype(c)> CELL;
            if (sh.wave)
                hipLaunchKernelGGL((k_spread_wave<CELL, IDS>), sh.grid, sh.block, 0, q.stream, c, ranges, M, q.stride, D, pa, NP, o, ids,
                                   q.nrows);
            else
                hipLaunchKernelGGL((k_spread_block<CELL, IDS>), sh.grid, sh.block, 0, q.stream, c, ranges, M, q.stride, D, pa, NP, o, ids,
                                   q.nrows);
        });
    };
    if (sel.by_id) launch(std::true_type());
    else launch(std::false_type());
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

int spread(lh_snapshot *s, const RowSel &sel, size_t nmetrics, const double *p, size_t np, SpreadOut o, bool device_form)
{
    int rc = check_args(s, sel, nmetrics, p, np, o);
    if (rc) return rc;
    Source q;
    rc = source_cells(s, sel, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) return LH_OK; // before any device call
    rc = source_open(s, q);
    if (rc) return rc;
    SpreadCtx *cx = q.cx;
    std::lock_guard<std::mutex> g(cx->mu);
    if (device_form) return enqueue(q, sel, nmetrics, p, np, o);

    // host form: results to HBM, then back to the caller's arrays
    rc = spread_host_results(cx->res, q.stream, o, nmetrics, np, [&](const SpreadOut &d) { return enqueue(q, sel, nmetrics, p, np, d); });
    return settle_ids(rc, sel, q.stream);
}

} // namespace

extern "C" {

int lh_spread(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np, uint64_t *count, double *sum,
              double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le)
{
    const SpreadOut o = {reinterpret_cast<u64 *>(count), sum, m2, pkeys, pvalid, reinterpret_cast<u64 *>(count_le), sum_le};
    return spread(s, rows_from(first), nmetrics, p, np, o, false);
}

int lh_spread_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np, uint64_t *d_count,
                     double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le)
{
    const SpreadOut o = {reinterpret_cast<u64 *>(d_count), d_sum, d_m2, d_pkeys, d_pvalid, reinterpret_cast<u64 *>(d_count_le),
                         d_sum_le};
    return spread(s, rows_from(first), nmetrics, p, np, o, true);
}

int lh_spread_ids(lh_snapshot *s, const uint32_t *ids, size_t n, const double *p, size_t np, uint64_t *count, double *sum,
                  double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le)
{
    const SpreadOut o = {reinterpret_cast<u64 *>(count), sum, m2, pkeys, pvalid, reinterpret_cast<u64 *>(count_le), sum_le};
    return spread(s, rows_by_id(ids, false), n, p, np, o, false);
}

int lh_spread_ids_device(lh_snapshot *s, const uint32_t *d_ids, size_t n, const double *p, size_t np, uint64_t *d_count,
                         double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le)
{
    const SpreadOut o = {reinterpret_cast<u64 *>(d_count), d_sum, d_m2, d_pkeys, d_pvalid, reinterpret_cast<u64 *>(d_count_le),
                         d_sum_le};
    return spread(s, rows_by_id(d_ids, true), n, p, np, o, true);
}

int lh_tool_spread_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, SP_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

} // extern "C"
