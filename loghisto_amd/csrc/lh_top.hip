// lh_top.hip -- lh_top* (include/loghisto_gpu.h): the k names of a range that lead by count, by sum, by the bucket a
// percentile falls into, or by the samples above a value.  The first reader that SELECTS ACROSS names instead of answering
// per name; the reference has no counterpart for the selection.  What is ranked is what the library already returns:
//   count, sum   processHistograms (/root/reference/metrics.go:336-376; sum = sum of D[b] * float64(c[b]), metrics.go:344)
//   percentile   the bucket percentile() selects (metrics.go:389-418): the first bin whose inclusive prefix count reaches
//                pct_threshold(p, count) -- lh_extract_rows' pkey
//   count above  count minus the running count lh_count_le reads at the value (le_take, lh_wave.h: the same bound-to-key
//                rule, +-Inf and the saturation beyond extended key 32 767 included; bucket resolution)
// Nothing is summed across names, no cell is written and no new statistic is defined.
//
// Built BESIDE the engine, on its public C ABI only: lh_beside.h says what that gives a reader.  Read-only.
//
// Two passes on the snapshot's stream:
//   k_top_score   one WAVE per row, four rows per workgroup, 256 bins per step over the row's span (4 consecutive bins per
//                 lane through load4_cells, the next step's loads issued before the current step is worked on, as
//                 k_spread_wave does).  Walk 1 gives count and sum (D[] is this unit's own table, generated once per
//                 device with lh::d_decompress_bin as lh_spread.hip's is) and, for BY_COUNT_ABOVE, the cells of the bins at
//                 or beyond the bound's take; BY_PERCENTILE takes a second walk to the first bin whose prefix reaches the
//                 threshold.  Each row leaves a record in a scratch block in HBM: a 64-bit ORDER-PRESERVING key (an integer
//                 as it is; a float64 by the sign-flip of its bits after -0.0 has become +0.0; complemented for
//                 LH_TOP_ASCENDING, so that the select pass always takes the LARGEST keys), its count, its sum and its pkey
//                 or count above.  Whether a row is a candidate is NOT in the key (a complemented key takes any value):
//                 it is count != 0.
//   k_select      (lh_select.h, shared with lh_movers.hip) ONE workgroup of 1 024 threads looping over the records: an exact
//                 k-th-key search by radix, the winners by a prefix count in index order, a bitonic sort by (key descending, id
//                 ascending); this unit's TopEmit writes a winner's entry.  One total order: the result depends on neither
//                 timing nor launch shape.
// One wave shape and a one-workgroup select are UNMEASURED DEFAULTS: a full-span row costs its wave 256 steps per walk, and
// the select pass reads the keys nine times with one workgroup.  tools/top_bench.py measures both passes at 65 536 names and
// a full-span row; that measurement decides whether the workgroup-per-row shape lh_count.hip and lh_spread.hip carry, or a
// histogram pass over several workgroups, is added.  Every floating-point sum is taken in a fixed order (per lane over the steps in ascending order,
// then one DPP tree over the lanes).
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_select.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <mutex>

namespace {

using namespace lh; // (lh_wave.h)
using namespace lh::beside;

// (the rows' records, TopRecords, and the winner's entry, TopEmit: lh_select.h, shared with lh_kept.hip's lh_kept_top*)

template <typename CELL>
__global__ __launch_bounds__(ROW_BLOCK) void k_top_score(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                        uint32_t nmetrics, size_t stride, const double *__restrict__ D,
                                                        uint32_t by, double arg, u64 flip, const TopRecords r)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const Span sp = own_span(ranges, m);
    const uint32_t hi = sp.hi;
    u64 total = 0, above = 0;
    double sum = 0.0;
    uint32_t found = 0; // BY_PERCENTILE: the selected bin
    if (sp.any()) {     // wave-uniform; an empty row costs two loads and its stores
        const CELL *__restrict__ row = cells + (size_t)m * stride;
        const uint32_t base0 = sp.base0();
        u64 c[4], nc[4];
        double d[4], nd[4];
        // ---- walk 1: count and sum; the cells at or beyond the bound's take
        {
            const bool want_above = by == LH_TOP_BY_COUNT_ABOVE; // wave-uniform
            const uint32_t take = want_above ? le_take(arg) : 0u;
            u64 cnt = 0, ab = 0;
            double ps = 0.0;
            load4(row, D, base0 + 4 * lane, hi, c, d);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4(row, D, base + STEP + 4 * lane, hi, nc, nd); // the next step's: in flight under this step's work
                cnt += (c[0] + c[1]) + (c[2] + c[3]);
                double t[4]; // (terms4, lh_wave.h, written out: through the helper this kernel's code comes out reordered)
#pragma unroll
                for (int k = 0; k < 4; k++) t[k] = d[k] * (double)c[k];
                ps += (t[0] + t[1]) + (t[2] + t[3]);
                if (want_above) {
                    const uint32_t b0 = base + 4 * lane;
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) ab += b0 + k >= take ? c[k] : 0;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) { c[k] = nc[k]; d[k] = nd[k]; }
            }
            total = readlane_u64(wave_scan_incl_u64(cnt), 63);
            sum = readlane_f64(wave_scan_incl_f64(ps), 63);
            above = readlane_u64(wave_scan_incl_u64(ab), 63);
        }
        if (total == 0) sum = 0.0;
        if (total && by == LH_TOP_BY_PERCENTILE) { // wave-uniform
            // ---- walk 2: the first bin whose inclusive prefix reaches T (the host keeps arg in [0, 1]: 1 <= T <= total)
            const u64 T = readlane_u64(pct_threshold(arg, total), 0);
            u64 carry = 0;
            found = hi;
            load4_cells(row, base0 + 4 * lane, hi, c);
            for (uint32_t base = base0; base <= hi; base += STEP) {
                load4_cells(row, base + STEP + 4 * lane, hi, nc);
                const u64 tc = (c[0] + c[1]) + (c[2] + c[3]);
                const u64 inc = wave_scan_incl_u64(tc);
                const u64 end = carry + readlane_u64(inc, 63);
                if (T <= end) { // wave-uniform: it is in this step
                    // (find_in_step, lh_pct.h, written out: through the helper this kernel's code comes out reordered and two
                    // instructions longer, profiles/pct_walk_isa.txt)
                    const u64 p0 = carry + (inc - tc) + c[0], p1 = p0 + c[1], p2 = p1 + c[2], p3 = p2 + c[3];
                    // the first lane whose last bin reaches T (lane 63's does), and how many of its bins stay below
                    const uint32_t f = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(p3 >= T));
                    const uint32_t below = (p0 < T ? 1u : 0u) + (p1 < T ? 1u : 0u) + (p2 < T ? 1u : 0u);
                    found = base + 4 * f + (uint32_t)__builtin_amdgcn_readlane((int)below, (int)f);
                    break;
                }
                carry = end;
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = nc[k];
            }
        }
    }
    if (lane == 0) {
        u64 key, aux = 0;
        if (by == LH_TOP_BY_COUNT) {
            key = total;
        } else if (by == LH_TOP_BY_SUM) {
            key = order_key_f64(sum);
        } else if (by == LH_TOP_BY_PERCENTILE) {
            key = found;
            aux = total ? (u64)(uint16_t)(int16_t)lh::bin_to_key(found) : 0;
        } else {
            key = above;
            aux = above;
        }
        r.key[m] = key ^ flip;
        r.count[m] = total;
        r.sum[m] = sum;
        r.aux[m] = aux;
    }
}

// ---- host side: lh_select.h's, around this unit's enqueue --------------------------------------------------------
// Per-device state of this unit (device_ctx<TopCtx>).  `mu` is held for the length of a call -- the host form's wait for
// its results included, so host-form calls on one device take turns even when their snapshots belong to different
// engines.
struct TopCtx {
    std::mutex mu;
    double *d_table = nullptr; // D[LH_NKEYS]
    SelectState sel;           // the records: four arrays (TopRecords)
};

// every check that needs neither the snapshot nor a device
int check_args(lh_snapshot *s, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, const void *out, const void *n_out,
               uintptr_t n_out_align)
{
    if (!s || by > LH_TOP_BY_COUNT_ABOVE || (flags & ~(uint32_t)LH_TOP_ASCENDING)) return LH_EINVAL;
    if (by == LH_TOP_BY_PERCENTILE && !(arg >= 0.0 && arg <= 1.0)) return LH_EINVAL; // NaN too: no bucket to rank by
    if (by == LH_TOP_BY_COUNT_ABOVE && arg != arg) return LH_EINVAL;
    return select_check_args(nmetrics, k, out, n_out, n_out_align);
}

typedef Source<TopCtx> TopSource;

// (cx->mu held) enqueue both passes over rows [first, first + nmetrics) on the snapshot's stream.  ev[0 .. 2] (may be
// null): events to record before the score pass, between the passes and behind the select pass (lh_tool_top_passes_ms).
int enqueue(const TopSource &q, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, lh_top_entry *d_out,
            uint32_t *d_n_out, hipEvent_t *ev = nullptr)
{
    TopCtx *cx = q.cx;
    u64 *base = nullptr;
    size_t npad = 0;
    int rc = ensure_table(cx->d_table, q.stream, lh::k_value_table<TopCtx>);
    if (!rc) rc = select_records(cx->sel, q.stream, nmetrics, TOP_FIELDS, base, npad);
    if (rc) return rc;
    const TopRecords r = top_records(base, npad);
    const uint32_t M = (uint32_t)nmetrics;
    const uint32_t *ranges = ranges_from(q, first);
    const u64 flip = (flags & LH_TOP_ASCENDING) ? ~0ull : 0ull;
    const RowShape sh = row_shape(M, 0); // (one shape: a wave per row whatever M)
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[0], q.stream));
    with_cells(q, first, [&](auto *c) {
        hipLaunchKernelGGL(k_top_score<cell_of<decltype(c)>>, sh.grid, sh.block, 0, q.stream, c, ranges, M, q.stride, cx->d_table, by, arg,
                           flip, r);
    });
    LH_BESIDE_CHK(hipGetLastError());
    return select_pass(cx->sel, q.stream, r.key, r.count, M, k, TopEmit{r, first, by, d_out}, d_n_out, ev);
}

// the snapshot's cells, spans, device and stream; LH_ERANGE for rows it does not have.  (The empty call comes behind it:
// it writes n_out.)
int open_source(lh_snapshot *s, uint32_t first, size_t nmetrics, TopSource &q)
{
    const int rc = source_cells(s, first, nmetrics, q);
    return rc ? rc : source_open(s, q);
}

} // namespace

extern "C" {

int lh_top(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, lh_top_entry *out,
           size_t *n_out)
{
    int rc = check_args(s, nmetrics, by, arg, k, flags, out, n_out, alignof(size_t));
    if (rc) return rc;
    TopSource q;
    rc = open_source(s, first, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) {
        *n_out = 0;
        return LH_OK;
    }
    std::lock_guard<std::mutex> g(q.cx->mu);
    const auto both = [&](lh_top_entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
        return enqueue(q, first, nmetrics, by, arg, k, flags, d_out, d_n_out, ev);
    };
    return select_host_form(q.cx->sel, q.stream, k, out, n_out, both);
}

int lh_top_device(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
                  lh_top_entry *d_out, uint32_t *d_n_out)
{
    int rc = check_args(s, nmetrics, by, arg, k, flags, d_out, d_n_out, alignof(uint32_t));
    if (rc) return rc;
    TopSource q;
    rc = open_source(s, first, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) {
        LH_BESIDE_CHK(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t), q.stream));
        return LH_OK;
    }
    std::lock_guard<std::mutex> g(q.cx->mu);
    return enqueue(q, first, nmetrics, by, arg, k, flags, d_out, d_n_out);
}

int lh_tool_top_passes_ms(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
                          float *score_ms, float *select_ms)
{
    alignas(8) unsigned char own[8] = {0}; // (the results stay in the unit's own block)
    int rc = check_args(s, nmetrics, by, arg, k, flags, own, own, 1);
    if (rc) return rc;
    if (!score_ms || !select_ms || nmetrics == 0) return LH_EINVAL;
    TopSource q;
    rc = open_source(s, first, nmetrics, q);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(q.cx->mu);
    const auto both = [&](lh_top_entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
        return enqueue(q, first, nmetrics, by, arg, k, flags, d_out, d_n_out, ev);
    };
    return select_passes_ms<lh_top_entry>(q.cx->sel, q.stream, k, score_ms, select_ms, both);
}

} // extern "C"
