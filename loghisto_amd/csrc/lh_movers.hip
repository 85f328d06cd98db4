// lh_movers.hip -- lh_movers* (include/loghisto_gpu.h): the k names of a range whose distribution moved most between two
// snapshots, by one of lh_compare's three distances or by how far the bucket of a percentile moved.  lh_compare.hip's two-row
// walk (the bucket walk of percentile(), /root/reference/metrics.go:389-418, over two rows at once) joined with lh_top.hip's
// select: a score per row goes to HBM and k entries travel.  The first reader that SELECTS ACROSS names over TWO snapshots;
// the reference has no counterpart for the selection.  What is ranked is what the library already returns:
//   ks, w1, shift   of lh_compare(base, cur, ...): ks bit-equal to it in either of its shapes, w1 and shift bit-equal to
//                   k_compare_wave's (the same steps, the same take4, the same per-lane order, the same DPP tree)
//   percentile      bin_cur - bin_base of the buckets lh_extract_rows selects for p in the two snapshots (the first bin whose
//                   inclusive prefix count reaches pct_threshold(p, total)), an exact integer in buckets
// Nothing is summed across names, no cell is written and no new statistic is defined.
//
// Built BESIDE the engine, on its public C ABI only: lh_beside.h says what that gives a reader.  Read-only.
//
// Two passes on cur's stream (behind an event on base's when the two differ, as lh_compare does):
//   k_movers_score  one WAVE per row, four rows per workgroup, 256 bins per step over the union of the two rows' spans (each
//                   row read inside its own span only: load4_in), the next step's loads issued before the current step is
//                   worked on.  Walk 1 gives both totals.  Walk 2 is k_compare_wave's for the three distances (lh_pair.h);
//                   for LH_MOVERS_BY_PERCENTILE it is ONE joint walk that carries both prefixes, finds in each row the first
//                   bin whose prefix reaches that row's threshold by k_top_score's ballot scheme, and leaves as soon as both
//                   are found.  Each row leaves a record in a scratch block in HBM: the ORDER-PRESERVING key of the score
//                   (order_key_f64, complemented for LH_MOVERS_ASCENDING so that the select pass always takes the LARGEST
//                   keys), a candidate word (0 when either total is 0: such a row is never ranked; else bit 32 and, below
//                   it, the two int16 keys), both totals and the score's bits.
//   k_select        lh_select.h's, shared with lh_top.hip: one workgroup, an exact radix select, a prefix count in index order
//                   and a bitonic sort by (key descending, id ascending); this unit's MoversEmit writes a winner's entry.
// One wave shape and a one-workgroup select are lh_top's UNMEASURED DEFAULTS here too; tools/movers_bench.py measures both
// passes at 65 536 names (profiles/movers.txt).  Every floating-point sum is taken in a fixed order.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_pair.h"
#include "lh_select.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <mutex>

namespace {

using namespace lh; // (lh_wave.h)
using namespace lh::beside;

// (the rows' records, MoversRecords, their candidate word and the winner's entry, MoversEmit: lh_select.h, shared with
// lh_kept.hip's lh_kept_movers*)

// The first bin of a step whose inclusive prefix reaches T, given that the step's last one does (k_top_score's scheme):
// c the lane's four cells, tc their sum, inc its inclusive scan over the lanes, carry what lies below the step.
__device__ __forceinline__ uint32_t first_reaching(uint32_t base, u64 T, u64 carry, u64 inc, u64 tc, const u64 (&c)[4])
{
    const u64 p0 = carry + (inc - tc) + c[0], p1 = p0 + c[1], p2 = p1 + c[2], p3 = p2 + c[3];
    // the first lane whose last bin reaches T (lane 63's does), and how many of its bins stay below
    const uint32_t f = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(p3 >= T));
    const uint32_t below = (p0 < T ? 1u : 0u) + (p1 < T ? 1u : 0u) + (p2 < T ? 1u : 0u);
    return base + 4 * f + (uint32_t)__builtin_amdgcn_readlane((int)below, (int)f);
}

template <typename CA, typename CB>
__global__ __launch_bounds__(ROW_BLOCK) void k_movers_score(const CA *__restrict__ cells_a, const uint32_t *__restrict__ ranges_a,
                                                           size_t stride_a, const CB *__restrict__ cells_b,
                                                           const uint32_t *__restrict__ ranges_b, size_t stride_b,
                                                           uint32_t nmetrics, uint32_t by, double arg, u64 flip,
                                                           const MoversRecords r)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const Span sa = or_empty(own_span(ranges_a, m)), sb = or_empty(own_span(ranges_b, m));
    const uint32_t base0 = min(sa.lo, sb.lo), hi = max(sa.hi, sb.hi); // the union; base0 == NO_BIN: neither row was marked
    u64 na = 0, nb = 0;
    double score = 0.0;
    uint32_t keys = 0; // key << 16 | key_base
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
        if (na && nb && by != LH_MOVERS_BY_PERCENTILE) { // wave-uniform
            // ---- walk 2: the prefixes, the largest X and the sums (k_compare_wave's)
            const Scale sc = make_scale(na, nb);
            Best t;
            best_init(t);
            u64 ca = 0, cb = 0; // what lies below the step
            load4_in(ra, base0 + 4 * lane, sa, a);
            load4_in(rb, base0 + 4 * lane, sb, b);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4_in(ra, base + STEP + 4 * lane, sa, xa);
                load4_in(rb, base + STEP + 4 * lane, sb, xb);
                const u64 ta = sum4(a), tb = sum4(b);
                const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
                take4(t, sc, base + 4 * lane, ca + (ia - ta), cb + (ib - tb), a, b);
                ca += readlane_u64(ia, 63);
                cb += readlane_u64(ib, 63);
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = xa[k]; b[k] = xb[k]; }
            }
            u128 x;
            uint32_t bin;
            u64 ba, bb;
            wave_best(t, x, bin, ba, bb);
            const double w1 = readlane_f64(wave_scan_incl_f64(t.w), 63);
            const double shift = readlane_f64(wave_scan_incl_f64(t.s), 63);
            if (by == LH_MOVERS_BY_KS) { // (lh_compare's store_row: an X of 0 everywhere is a distance of 0 at key 0)
                if (bin != NO_BIN) {
                    score = fabs((double)ba / (double)na - (double)bb / (double)nb);
                    keys = (uint32_t)(uint16_t)(int16_t)lh::bin_to_key(bin) << 16;
                }
            } else {
                score = by == LH_MOVERS_BY_W1 ? w1 : shift;
            }
        } else if (na && nb) {
            // ---- walk 2: in each row the first bin whose inclusive prefix reaches its T (the host keeps arg in [0, 1]:
            // 1 <= T <= total, and the bin is an occupied one of the row's own span)
            const u64 Ta = readlane_u64(pct_threshold(arg, na), 0), Tb = readlane_u64(pct_threshold(arg, nb), 0);
            u64 ca = 0, cb = 0;
            uint32_t fa = NO_BIN, fb = NO_BIN;
            load4_in(ra, base0 + 4 * lane, sa, a);
            load4_in(rb, base0 + 4 * lane, sb, b);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4_in(ra, base + STEP + 4 * lane, sa, xa);
                load4_in(rb, base + STEP + 4 * lane, sb, xb);
                const u64 ta = sum4(a), tb = sum4(b);
                const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
                const u64 ea = ca + readlane_u64(ia, 63), eb = cb + readlane_u64(ib, 63);
                if (fa == NO_BIN && Ta <= ea) fa = first_reaching(base, Ta, ca, ia, ta, a); // wave-uniform: it is in this step
                if (fb == NO_BIN && Tb <= eb) fb = first_reaching(base, Tb, cb, ib, tb, b);
                if (fa != NO_BIN && fb != NO_BIN) break;
                ca = ea;
                cb = eb;
#pragma unroll
                for (int k = 0; k < 4; k++) { a[k] = xa[k]; b[k] = xb[k]; }
            }
            if (fa == NO_BIN) fa = hi; // (totals that wrapped: some bin of the span)
            if (fb == NO_BIN) fb = hi;
            score = (double)((long long)fb - (long long)fa);
            keys = (uint32_t)(uint16_t)(int16_t)lh::bin_to_key(fb) << 16 | (uint32_t)(uint16_t)(int16_t)lh::bin_to_key(fa);
        }
    }
    if (lane == 0) {
        const bool is_cand = na != 0 && nb != 0;
        r.key[m] = order_key_f64(score) ^ flip;
        r.cand[m] = is_cand ? MOVER_CANDIDATE | keys : 0;
        r.count_a[m] = na;
        r.count_b[m] = nb;
        r.score[m] = (u64)__double_as_longlong(score);
    }
}

// ---- host side: lh_select.h's, around this unit's enqueue --------------------------------------------------------
// Per-device state of this unit (device_ctx<MoversCtx>).  `mu` is held for the length of a call, the host form's wait for
// its results included.  `order`: the event that puts cur's stream behind base's when the two differ.
struct MoversCtx {
    std::mutex mu;
    hipEvent_t order = nullptr;
    SelectState sel; // the records: five arrays (MoversRecords)
};

// every check that needs neither a snapshot nor a device
int check_args(lh_snapshot *base, lh_snapshot *cur, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, const void *out,
               const void *n_out, uintptr_t n_out_align)
{
    if (!base || !cur || by > LH_MOVERS_BY_PERCENTILE || (flags & ~(uint32_t)LH_MOVERS_ASCENDING)) return LH_EINVAL;
    if (by == LH_MOVERS_BY_PERCENTILE && !(arg >= 0.0 && arg <= 1.0)) return LH_EINVAL; // NaN too: no bucket to rank by
    return select_check_args(nmetrics, k, out, n_out, n_out_align);
}

typedef Source<MoversCtx> MoversSource;

// both snapshots' cells, spans, device and stream: LH_ERANGE for rows either does not have, LH_EINVAL for two devices,
// LH_ESTATE for cells the kernels cannot walk.  (The empty call comes behind it: it writes n_out.)
int open_sources(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, MoversSource (&q)[2])
{
    lh_snapshot *const snaps[2] = {base, cur};
    const int rc = list_cells(snaps, 2, first, nmetrics, q);
    return rc ? rc : list_open(snaps, 2, q);
}

// (cx->mu held) enqueue both passes over rows [first, first + nmetrics) on cur's stream, behind what base's stream holds.
// ev[0 .. 2] (may be null): events to record before the score pass, between the passes and behind the select pass
// (lh_tool_movers_passes_ms).
int enqueue(const MoversSource &a, const MoversSource &b, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
            lh_mover_entry *d_out, uint32_t *d_n_out, hipEvent_t *ev = nullptr)
{
    MoversCtx *cx = b.cx;
    u64 *base = nullptr;
    size_t npad = 0;
    int rc = order_behind(cx->order, a.stream, b.stream);
    if (!rc) rc = select_records(cx->sel, b.stream, nmetrics, MOVERS_FIELDS, base, npad);
    if (rc) return rc;
    const MoversRecords r = movers_records(base, npad);
    const uint32_t M = (uint32_t)nmetrics;
    const uint32_t *ra = ranges_from(a, first), *rb = ranges_from(b, first);
    const u64 flip = (flags & LH_MOVERS_ASCENDING) ? ~0ull : 0ull;
    const RowShape sh = row_shape(M, 0); // (one shape: a wave per row whatever M)
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[0], b.stream));
    with_cells(a, first, [&](auto *ca) {
        with_cells(b, first, [&](auto *cb) {
            typedef cell_of<decltype(ca)> CA;
            typedef cell_of<decltype(cb)> CB;
            hipLaunchKernelGGL((k_movers_score<CA, CB>), sh.grid, sh.block, 0, b.stream, ca, ra, a.stride, cb, rb, b.stride, M, by, arg,
                               flip, r);
        });
    });
    LH_BESIDE_CHK(hipGetLastError());
    return select_pass(cx->sel, b.stream, r.key, r.cand, M, k, MoversEmit{r, first, d_out}, d_n_out, ev);
}

} // namespace

extern "C" {

int lh_movers(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
              lh_mover_entry *out, size_t *n_out)
{
    int rc = check_args(base, cur, nmetrics, by, arg, k, flags, out, n_out, alignof(size_t));
    if (rc) return rc;
    MoversSource q[2];
    const MoversSource &a = q[0], &b = q[1];
    rc = open_sources(base, cur, first, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) {
        *n_out = 0;
        return LH_OK;
    }
    std::lock_guard<std::mutex> g(b.cx->mu);
    const auto both = [&](lh_mover_entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
        return enqueue(a, b, first, nmetrics, by, arg, k, flags, d_out, d_n_out, ev);
    };
    return select_host_form(b.cx->sel, b.stream, k, out, n_out, both);
}

int lh_movers_device(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                     uint32_t flags, lh_mover_entry *d_out, uint32_t *d_n_out)
{
    int rc = check_args(base, cur, nmetrics, by, arg, k, flags, d_out, d_n_out, alignof(uint32_t));
    if (rc) return rc;
    MoversSource q[2];
    const MoversSource &a = q[0], &b = q[1];
    rc = open_sources(base, cur, first, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) {
        LH_BESIDE_CHK(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t), b.stream));
        return LH_OK;
    }
    std::lock_guard<std::mutex> g(b.cx->mu);
    return enqueue(a, b, first, nmetrics, by, arg, k, flags, d_out, d_n_out);
}

int lh_tool_movers_passes_ms(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                             uint32_t flags, float *score_ms, float *select_ms)
{
    alignas(8) unsigned char own[8] = {0}; // (the results stay in the unit's own block)
    int rc = check_args(base, cur, nmetrics, by, arg, k, flags, own, own, 1);
    if (rc) return rc;
    if (!score_ms || !select_ms || nmetrics == 0) return LH_EINVAL;
    MoversSource q[2];
    const MoversSource &a = q[0], &b = q[1];
    rc = open_sources(base, cur, first, nmetrics, q);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(b.cx->mu);
    const auto both = [&](lh_mover_entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
        return enqueue(a, b, first, nmetrics, by, arg, k, flags, d_out, d_n_out, ev);
    };
    return select_passes_ms<lh_mover_entry>(b.cx->sel, b.stream, k, score_ms, select_ms, both);
}

} // extern "C"
