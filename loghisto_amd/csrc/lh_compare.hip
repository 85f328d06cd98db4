// lh_compare.hip -- lh_compare* (include/loghisto_gpu.h): how a name's distribution in one snapshot (`cur`) differs from
// its distribution in another (`base`): the previous interval, a stored baseline, the canary against the fleet.  One more
// bucket walk of the kind percentile() does (/root/reference/metrics.go:389-418: `sofar += *count` over the cells in
// ascending key order), taken over TWO rows at once.  With a[j] / b[j] the cells of base / cur, A_j / B_j their inclusive
// prefix counts and na / nb the totals, per name:
//   X_j = |A_j nb - B_j na|        an exact 128-bit integer: na nb times the distance of the two normalised prefixes
//   j*  = the lowest bin at which X_j is largest  -> ks_key, ks_below_a = A_j*, ks_below_b = B_j*,
//         ks = |float64(A_j*) / float64(na) - float64(B_j*) / float64(nb)|   (Kolmogorov-Smirnov; the argmax is integer)
//   w1    = sum over j of X_j / (na nb)            (earth mover's distance, in buckets)
//   shift = the same sum with the sign of A_j nb - B_j na: positive when cur sits higher
// A term of the two sums is float64(X_j >> s) / float64(na nb >> s), s = what na nb has beyond 64 bits: the shift drops
// less than 2^-63 of a term that is at most 1, and the conversions and the divide round three times -- no cancellation of
// two rounded quotients, whatever the counts.
//
// Built BESIDE the engine, on its public C ABI only (lh_beside.h), like lh_spread.hip, whose two shapes these are:
//   k_compare_wave   one WAVE per row, 256 bins per step (4 consecutive bins per lane and row), the next step's loads issued
//                    before the current step is worked on.  For calls of many rows.
//   k_compare_block  one WORKGROUP of 16 waves per row: the waves total the 256-bin chunks, wave 0 scans the chunk totals in
//                    LDS so that each wave knows the prefixes its chunks start from, then the waves walk their chunks again.
//                    For calls of few rows, which may span all 65 536 bins.
// Each row takes two walks over the union of the two dirty spans (from its start aligned down to a multiple of 4): walk 1
// gives na and nb; walk 2 carries both prefixes, each lane's largest X with its bin and prefixes (strictly larger only: a
// lane meets its bins in ascending order, so it keeps the lowest), and the lane's share of the two sums.  A row is only
// read inside its OWN span (its cells outside are zero by the engine's contract, and a row that was never marked has
// lo > hi: nothing of it is read).  Bins behind the union span need no mask: there A = na and B = nb, X = 0.
// The wave's best (X, bin) is found without LDS: four DPP max-reductions over the 32-bit words of X from the top, the lanes
// that fall short dropping out, then a DPP min of the bin among those left.  The sums are taken in a fixed order (per
// lane over its bins in ascending order, one DPP tree over the lanes, the waves of a workgroup in ascending order), so a
// result does not depend on timing -- the two shapes associate differently and agree to rounding only.
// Read-only: no store goes to a cell, a span or either engine.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_pair.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <mutex>

namespace {

using namespace lh; // (lh_wave.h)
using namespace lh::beside;

// Rows of a call from which a row gets a wave, not a workgroup: lh_spread's default, whose walks these are, until
// tools/compare_bench.py has been run (profiles/compare.txt).
constexpr uint32_t CP_WAVE_FROM_DEFAULT = 1024;

// (CompareOut, a name's eight results, and store_row, the lane that writes them: lh_pair.h)

template <typename CA, typename CB>
__global__ __launch_bounds__(ROW_BLOCK) void k_compare_wave(const CA *__restrict__ cells_a, const uint32_t *__restrict__ ranges_a,
                                                           size_t stride_a, const CB *__restrict__ cells_b,
                                                           const uint32_t *__restrict__ ranges_b, size_t stride_b,
                                                           uint32_t nmetrics, const CompareOut o)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const Span sa = or_empty(own_span(ranges_a, m)), sb = or_empty(own_span(ranges_b, m));
    const uint32_t base0 = min(sa.lo, sb.lo), hi = max(sa.hi, sb.hi); // the union; base0 == NO_BIN: neither row was marked
    u64 na = 0, nb = 0, ba = 0, bb = 0;
    uint32_t bin = NO_BIN;
    double w1 = 0.0, shift = 0.0;
    if (base0 != NO_BIN) { // wave-uniform
        const CA *__restrict__ ra = cells_a + (size_t)m * stride_a;
        const CB *__restrict__ rb = cells_b + (size_t)m * stride_b;
        u64 a[4], b[4], xa[4], xb[4];
        // ---- walk 1: the totals
        {
            u64 ta = 0, tb = 0;
            load4_in(ra, base0 + 4 * lane, sa, a);
            load4_in(rb, base0 + 4 * lane, sb, b);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4_in(ra, base + STEP + 4 * lane, sa, xa); // the next step's: in flight under this step's work
                load4_in(rb, base + STEP + 4 * lane, sb, xb);
                ta += sum4(a);
                tb += sum4(b);
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = xa[k]; b[k] = xb[k]; }
            }
            na = readlane_u64(wave_scan_incl_u64(ta), 63);
            nb = readlane_u64(wave_scan_incl_u64(tb), 63);
        }
        if (na && nb) { // wave-uniform
            // ---- walk 2: the prefixes, the largest X and the sums
            const Scale sc = make_scale(na, nb);
            Best r;
            best_init(r);
            u64 ca = 0, cb = 0; // what lies below the step
            load4_in(ra, base0 + 4 * lane, sa, a);
            load4_in(rb, base0 + 4 * lane, sb, b);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4_in(ra, base + STEP + 4 * lane, sa, xa);
                load4_in(rb, base + STEP + 4 * lane, sb, xb);
                const u64 ta = sum4(a), tb = sum4(b);
                const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
                take4(r, sc, base + 4 * lane, ca + (ia - ta), cb + (ib - tb), a, b);
                ca += readlane_u64(ia, 63);
                cb += readlane_u64(ib, 63);
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = xa[k]; b[k] = xb[k]; }
            }
            u128 x;
            wave_best(r, x, bin, ba, bb);
            w1 = readlane_f64(wave_scan_incl_f64(r.w), 63);
            shift = readlane_f64(wave_scan_incl_f64(r.s), 63);
        }
    }
    if (lane == 0) store_row(o, m, na, nb, bin, ba, bb, w1, shift);
}

template <typename CA, typename CB>
__global__ __launch_bounds__(WG) void k_compare_block(const CA *__restrict__ cells_a, const uint32_t *__restrict__ ranges_a,
                                                         size_t stride_a, const CB *__restrict__ cells_b,
                                                         const uint32_t *__restrict__ ranges_b, size_t stride_b,
                                                         uint32_t nmetrics, const CompareOut o)
{
    __shared__ u64 s_a[CHUNKS], s_b[CHUNKS]; // the chunks' totals, then their exclusive prefixes
    __shared__ u64 s_na, s_nb;
    __shared__ u64 s_xh[WG_WAVES], s_xl[WG_WAVES], s_ba[WG_WAVES], s_bb[WG_WAVES]; // the waves' bests
    __shared__ uint32_t s_bin[WG_WAVES];
    __shared__ double s_w[WG_WAVES], s_s[WG_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    if (m >= nmetrics) return;
    const Span sa = or_empty(own_span(ranges_a, m)), sb = or_empty(own_span(ranges_b, m));
    const uint32_t base0 = min(sa.lo, sb.lo), hi = max(sa.hi, sb.hi);
    const uint32_t nchunks = base0 != NO_BIN ? (hi - base0) / STEP + 1 : 0; // <= CHUNKS
    const CA *__restrict__ ra = cells_a + (size_t)m * stride_a;
    const CB *__restrict__ rb = cells_b + (size_t)m * stride_b;
    constexpr uint32_t U = 2;
    // ---- walk 1: every chunk's totals
    for (uint32_t c0 = wave; c0 < nchunks; c0 += WG_WAVES * U) { // wave-uniform
        u64 a[U][4], b[U][4];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) { // (a chunk beyond the span starts beyond hi: nothing is read)
            const uint32_t b0 = base0 + (c0 + u * WG_WAVES) * STEP + 4 * lane;
            load4_in(ra, b0, sa, a[u]);
            load4_in(rb, b0, sb, b[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const u64 ia = wave_scan_incl_u64(sum4(a[u])), ib = wave_scan_incl_u64(sum4(b[u]));
            const uint32_t ch = c0 + u * WG_WAVES;
            if (lane == 63 && ch < nchunks) {
                s_a[ch] = ia;
                s_b[ch] = ib;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        u64 va[4], vb[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const bool in = 4 * lane + k < nchunks;
            va[k] = in ? s_a[4 * lane + k] : 0;
            vb[k] = in ? s_b[4 * lane + k] : 0;
        }
        const u64 ta = sum4(va), tb = sum4(vb);
        const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
        u64 ea = ia - ta, eb = ib - tb;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            s_a[4 * lane + k] = ea;
            s_b[4 * lane + k] = eb;
            ea += va[k];
            eb += vb[k];
        }
        if (lane == 63) {
            s_na = ia;
            s_nb = ib;
        }
    }
    __syncthreads();
    const u64 na = s_na, nb = s_nb;
    if (na == 0 || nb == 0) { // workgroup-uniform
        if (threadIdx.x == 0) store_row(o, m, na, nb, NO_BIN, 0, 0, 0.0, 0.0);
        return;
    }
    // ---- walk 2, by the same chunks
    {
        const Scale sc = make_scale(na, nb);
        Best r;
        best_init(r);
        for (uint32_t c0 = wave; c0 < nchunks; c0 += WG_WAVES * U) {
            u64 a[U][4], b[U][4];
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t b0 = base0 + (c0 + u * WG_WAVES) * STEP + 4 * lane;
                load4_in(ra, b0, sa, a[u]);
                load4_in(rb, b0, sb, b[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t ch = c0 + u * WG_WAVES;
                if (ch < nchunks) { // wave-uniform
                    const u64 ta = sum4(a[u]), tb = sum4(b[u]);
                    const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
                    take4(r, sc, base0 + ch * STEP + 4 * lane, s_a[ch] + (ia - ta), s_b[ch] + (ib - tb), a[u], b[u]);
                }
            }
        }
        u128 x;
        uint32_t bin;
        u64 ba, bb;
        wave_best(r, x, bin, ba, bb);
        const double w = wave_scan_incl_f64(r.w), s = wave_scan_incl_f64(r.s);
        if (lane == 63) {
            s_xh[wave] = (u64)(x >> 64);
            s_xl[wave] = (u64)x;
            s_bin[wave] = bin;
            s_ba[wave] = ba;
            s_bb[wave] = bb;
            s_w[wave] = w;
            s_s[wave] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u128 x = 0;
        uint32_t bin = NO_BIN;
        u64 ba = 0, bb = 0;
        double w1 = 0.0, shift = 0.0;
        for (int w = 0; w < WG_WAVES; w++) { // (a wave without a chunk left X = 0, NO_BIN and +0)
            const u128 xw = ((u128)s_xh[w] << 64) | s_xl[w];
            if (xw > x || (xw == x && s_bin[w] < bin)) {
                x = xw;
                bin = s_bin[w];
                ba = s_ba[w];
                bb = s_bb[w];
            }
            w1 += s_w[w];
            shift += s_s[w];
        }
        store_row(o, m, na, nb, bin, ba, bb, w1, shift);
    }
}

// ---- host side --------------------------------------------------------------------------------------
// Per-device state of this unit (device_ctx<CompareCtx>).  `mu` is held for the length of a call, the host form's wait for
// its results included.  `order`: the event that puts cur's stream behind base's when the two differ.
struct CompareCtx {
    std::mutex mu;
    hipEvent_t order = nullptr;
    ResultBlocks res; // host form
};
std::atomic<uint32_t> g_wave_from{CP_WAVE_FROM_DEFAULT};

// every check that needs neither a snapshot nor a device
int check_args(lh_snapshot *base, lh_snapshot *cur, size_t nmetrics, uint32_t flags, const CompareOut &o)
{
    if (!base || !cur || flags != 0) return LH_EINVAL;
    if (!o.count_a && !o.count_b && !o.ks && !o.ks_key && !o.below_a && !o.below_b && !o.w1 && !o.shift) return LH_EINVAL;
    if (misaligned(o.count_a, 8) || misaligned(o.count_b, 8) || misaligned(o.ks, 8) || misaligned(o.ks_key, 2) ||
        misaligned(o.below_a, 8) || misaligned(o.below_b, 8) || misaligned(o.w1, 8) || misaligned(o.shift, 8))
        return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    return LH_OK;
}

typedef lh::beside::Source<CompareCtx> Source;

// (cx->mu held) enqueue the walks of rows [first, first + nmetrics) on cur's stream, behind what base's stream holds
int enqueue(const Source &a, const Source &b, uint32_t first, size_t nmetrics, const CompareOut &o)
{
    const int rc = order_behind(b.cx->order, a.stream, b.stream);
    if (rc) return rc;
    const uint32_t M = (uint32_t)nmetrics;
    const uint32_t *ra = ranges_from(a, first), *rb = ranges_from(b, first);
    const RowShape sh = row_shape(M, g_wave_from.load(std::memory_order_relaxed));
    with_cells(a, first, [&](auto *ca) {
        with_cells(b, first, [&](auto *cb) {
            typedef cell_of<decltype(ca)> CA;
            typedef cell_of<decltype(cb)> CB;
            if (sh.wave)
                hipLaunchKernelGGL((k_compare_wave<CA, CB>), sh.grid, sh.block, 0, b.stream, ca, ra, a.stride, cb, rb, b.stride, M, o);
            else
                hipLaunchKernelGGL((k_compare_block<CA, CB>), sh.grid, sh.block, 0, b.stream, ca, ra, a.stride, cb, rb, b.stride, M, o);
        });
    });
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

int compare(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t flags, const CompareOut &o,
            bool device_form)
{
    int rc = check_args(base, cur, nmetrics, flags, o);
    if (rc) return rc;
    lh_snapshot *const snaps[2] = {base, cur};
    Source q[2];
    const Source &a = q[0], &b = q[1];
    rc = list_cells(snaps, 2, first, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) return LH_OK; // before any device call
    rc = list_open(snaps, 2, q);
    if (rc) return rc;
    CompareCtx *cx = b.cx;
    std::lock_guard<std::mutex> g(cx->mu);
    if (device_form) return enqueue(a, b, first, nmetrics, o);

    // host form: results to HBM, then back to the caller's arrays
    return compare_host_results(cx->res, b.stream, o, nmetrics, [&](const CompareOut &d) { return enqueue(a, b, first, nmetrics, d); });
}

} // namespace

extern "C" {

int lh_compare(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t flags, uint64_t *count_a,
               uint64_t *count_b, double *ks, int16_t *ks_key, uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1,
               double *shift)
{
    const CompareOut o = {reinterpret_cast<u64 *>(count_a), reinterpret_cast<u64 *>(count_b), ks, ks_key,
                          reinterpret_cast<u64 *>(ks_below_a), reinterpret_cast<u64 *>(ks_below_b), w1, shift};
    return compare(base, cur, first, nmetrics, flags, o, false);
}

int lh_compare_device(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t flags, uint64_t *d_count_a,
                      uint64_t *d_count_b, double *d_ks, int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b,
                      double *d_w1, double *d_shift)
{
    const CompareOut o = {reinterpret_cast<u64 *>(d_count_a), reinterpret_cast<u64 *>(d_count_b), d_ks, d_ks_key,
                          reinterpret_cast<u64 *>(d_ks_below_a), reinterpret_cast<u64 *>(d_ks_below_b), d_w1, d_shift};
    return compare(base, cur, first, nmetrics, flags, o, true);
}

int lh_tool_compare_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, CP_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

} // extern "C"
