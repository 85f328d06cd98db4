// lh_across.hip -- lh_across* (include/loghisto_gpu.h): count, sum, nbuckets and the percentile buckets of a name over SEVERAL
// snapshots at once -- p99 over the last 10 seconds while emitting every second, or over the ranks and engines of one device.
// Counts add across intervals and percentiles do not (that is why lh_count_le exists): a percentile over K intervals needs
// the K rows of cells added together and walked once.  With c_i[b] the cells of the name in snaps[i]:
//   C[b] = sum over i of c_i[b], in 64 bits -- the cell atomic.AddUint64 would have left had the samples arrived in one
//          interval (metrics.go:278, 292); two narrow cells of 0xffffffff give 0x1fffffffe
//   count = sum of C[b]        sum = sum of D[b] * float64(C[b])  (metrics.go:344)        nbuckets = bins with C[b] != 0
//   present_bits: bit i set iff snaps[i] holds a sample of the name
//   per percentile the bucket percentile() selects on C (metrics.go:389-418): the first bin whose inclusive prefix reaches
//   pct_threshold(p, count) -- bit for bit what lh_extract_rows returns for a snapshot that holds C.
// Nothing is summed across names, no cell is written and no new statistic is defined.
//
// Built BESIDE the engine, on its public C ABI only (lh_beside.h), like lh_spread.hip, whose two shapes these are:
//   k_across_wave   one WAVE per row, 256 bins per step (4 consecutive bins per lane).  For calls of many rows.
//   k_across_block  one WORKGROUP of 16 waves per row: the waves reduce the 256-bin chunks independently, wave 0 scans the
//                   chunk totals in LDS, and each percentile then costs one more read of the one chunk its threshold falls
//                   into.  For calls of few rows, which may span all 65 536 bins.
// The snapshots travel as ONE by-value record (AcrossSnaps: 16 row-0 addresses, 16 span addresses, their number and a mask
// of the narrow ones).  A wave opens a name by having lane i read snapshot i's own span and work out the address of its
// row (Rows); the walk then runs over the UNION of the spans, from the least lo aligned down to a multiple of 4 to the
// largest hi, and takes snapshot i's span and address out of lane i (v_readlane: scalar registers, no array of 16 in
// anybody's registers).  A row is only read inside its OWN span (or_empty's, by load4_in's rule; the loads are this unit's
// own because of what fetch4 says): a name never marked in some snapshot has lo > hi there, and nothing of it is read.
// Per step and lane the 16-byte loads of IN_FLIGHT snapshots are issued back to back and only then added up, so they are
// under way together; lanes n .. of a last, partial set hold empty spans and ask for nothing.
// Three builds of each shape: every snapshot narrow (uint32 cells), every snapshot wide, or a mixture -- there the width is
// a wave-uniform branch per snapshot, and both arms leave the loaded 16 / 32 bytes as they came (unpacked when they are
// added), so that no arm has to wait for its load.
// Each row takes two walks.  Walk 1 gives count, sum, nbuckets and present_bits, hence the thresholds; walk 2 re-reads the
// windows (L2-resident at typical spans) up to the step the last threshold falls into.  The sum is taken in a fixed order
// (per lane over the steps in ascending order, then one DPP tree over the lanes; chunk totals in ascending order): a
// result does not depend on timing -- the two shapes associate differently and agree to rounding only.
// Read-only: no store goes to a cell, a span or any engine.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_pct.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <type_traits>

namespace {

using namespace lh; // (lh_wave.h, lh_pct.h)
using namespace lh::beside;

// Rows of a call from which a row gets a wave, not a workgroup: lh_spread's default, whose walks these are
// (profiles/across.txt).
constexpr uint32_t AC_WAVE_FROM_DEFAULT = 1024;
static_assert(LH_MAX_ACROSS <= 32, "a snapshot per lane, their set in one 32-bit mask");

constexpr uint32_t IN_FLIGHT = 8; // snapshots whose loads a lane has under way together
static_assert(LH_MAX_ACROSS % IN_FLIGHT == 0 && LH_MAX_ACROSS <= 64, "the lanes of a last, partial set exist");

enum { ALL_NARROW = 0, ALL_WIDE = 1, MIXED = 2 };

struct AcrossSnaps { // by value in the kernel arguments (264 bytes)
    const void *cells[LH_MAX_ACROSS];      // row `first` of snapshot i, at the snapshot's own width
    const uint32_t *ranges[LH_MAX_ACROSS]; // the span of row `first`
    uint32_t n, narrow;                    // bit i of narrow: snapshot i has 4-byte cells
};

typedef ListOut<uint32_t> AcrossOut; // present_bits: a bit per snapshot

// 16 bytes of a row as they lie in memory (4-byte aligned at least), through a pointer that says GLOBAL: an address taken out
// of a lane is an integer, and a load through a generic pointer made of it would be a flat one, which every LDS wait then
// waits for too
typedef uint32_t u32x4_a4v __attribute__((ext_vector_type(4), aligned(4)));
typedef const __attribute__((address_space(1))) u32x4_a4v *gcells;

// One name in the n snapshots, as a wave holds it: lane i has snapshot i's own span (or_empty; lanes from n on: empty) and
// the address of its row; every lane has the union.
struct Rows {
    uint32_t lo, hi;
    u64 row;
    uint32_t base0, uhi; // base0 == NO_BIN: the name was never marked in any of them
};
// `at`: the row, from lh::row_of -- row m of the block, or (IDS) row ids[m] of the snapshots, NO_ROW for an id at or beyond
// the rows of the shortest of them: every lane's span is then empty (row_span) and no address is made
template <int MODE, bool IDS> __device__ __forceinline__ Rows open_rows(const AcrossSnaps &s, uint32_t at, size_t stride, uint32_t lane)
{
    Rows r;
    r.lo = NO_BIN;
    r.hi = 0;
    r.row = 0;
    if (lane < s.n) {
        const Span sp = or_empty(row_span<IDS>(s.ranges[lane], at));
        const bool narrow = MODE == ALL_NARROW || (MODE == MIXED && ((s.narrow >> lane) & 1u));
        r.lo = sp.lo;
        r.hi = sp.hi;
        if (!IDS || at != NO_ROW) r.row = (u64)(uintptr_t)s.cells[lane] + (u64)at * stride * (narrow ? 4u : 8u);
    }
    r.base0 = ~wave_max_u32(~r.lo); // the least lo (NO_BIN's complement is 0)
    r.uhi = wave_max_u32(r.hi);
    return r;
}

// What a lane has under way of one snapshot: the 16 bytes of four narrow cells, or the 32 of four wide ones, AS THEY CAME,
// each load's four words one value -- widening them (or moving single words) inside the guarded load would make every
// load wait for itself.
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
template <int MODE> struct Raw { u32x4v a, b; }; // (b: bins 2 and 3 of wide cells; unused, and gone, in the narrow build)
// bins b0 .. b0 + 3 of the name in snapshot i (wave-uniform i), zeros outside its own span (load4_in's rule: b0 a multiple
// of 4 at or above the span's lo aligned down, and at or below its hi <= 65 535, so the group ends inside the row)
template <int MODE> __device__ __forceinline__ void fetch4(const Rows &r, uint32_t narrow, uint32_t i, uint32_t b0, Raw<MODE> &x)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)r.lo, (int)i);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)r.hi, (int)i);
    const u64 row = readlane_u64(r.row, i);
    x.a = 0;
    x.b = 0;
    if (b0 >= lo && b0 <= hi) {
        if (MODE == ALL_NARROW || (MODE == MIXED && ((narrow >> i) & 1u))) { // wave-uniform
            x.a = *(gcells)(row + 4ull * b0);
        } else {
            const gcells rp = (gcells)(row + 8ull * b0);
            x.a = rp[0];
            x.b = rp[1];
        }
    }
}
// (the empty asm keeps the compiler from moving the widening up into fetch4's guarded region)
template <int MODE> __device__ __forceinline__ void unpack4(Raw<MODE> &x, uint32_t narrow, uint32_t i, u64 (&c)[4])
{
    asm volatile("" : "+v"(x.a));
    if (MODE != ALL_NARROW) asm volatile("" : "+v"(x.b));
    if (MODE == ALL_NARROW || (MODE == MIXED && ((narrow >> i) & 1u))) {
        c[0] = x.a.x; c[1] = x.a.y; c[2] = x.a.z; c[3] = x.a.w;
    } else {
        c[0] = (u64)x.a.x | (u64)x.a.y << 32; c[1] = (u64)x.a.z | (u64)x.a.w << 32;
        c[2] = (u64)x.b.x | (u64)x.b.y << 32; c[3] = (u64)x.b.z | (u64)x.b.w << 32;
    }
}
// C[b0 .. b0 + 3]: the lane's four bins summed over the snapshots in list order, in 64 bits.  SEEN: bit i of `seen` is set
// when snapshot i has a sample in them.
template <int MODE, bool SEEN>
__device__ __forceinline__ void sum_rows(const Rows &r, uint32_t n, uint32_t narrow, uint32_t b0, u64 (&C)[4], uint32_t &seen)
{
    C[0] = C[1] = C[2] = C[3] = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += IN_FLIGHT) { // wave-uniform
        Raw<MODE> x[IN_FLIGHT];
#pragma unroll
        for (uint32_t j = 0; j < IN_FLIGHT; j++) fetch4<MODE>(r, narrow, i0 + j, b0, x[j]);
#pragma unroll
        for (uint32_t j = 0; j < IN_FLIGHT; j++) {
            u64 c[4];
            unpack4<MODE>(x[j], narrow, i0 + j, c);
            if (SEEN) seen |= (((c[0] | c[1]) | (c[2] | c[3])) != 0 ? 1u : 0u) << (i0 + j);
#pragma unroll
            for (int k = 0; k < 4; k++) C[k] += c[k];
        }
    }
}

// (Both kernels, IDS: entry m reads row ids[m] of every snapshot, `nrows` the rows of the shortest of them; m still indexes
// the outputs.  Otherwise row m of the blocks; ids and nrows are not looked at.)
template <int MODE, bool IDS>
__global__ __launch_bounds__(ROW_BLOCK) void k_across_wave(const AcrossSnaps s, uint32_t nmetrics, size_t stride,
                                                          const double *__restrict__ D, const PctArgs pa, uint32_t np,
                                                          const AcrossOut o, const uint32_t *__restrict__ ids, uint32_t nrows)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nmetrics) return; // wave-uniform
    const Rows r = open_rows<MODE, IDS>(s, row_of<IDS>(ids, nrows, m), stride, lane);
    const uint32_t hi = r.uhi;
    u64 total = 0;
    double sum = 0.0;
    uint32_t nb = 0, present = 0, none = 0;
    Open pct; // lane i < np: percentile i
    if (r.base0 != NO_BIN) { // wave-uniform
        u64 C[4];
        // ---- walk 1: count, sum, the occupied bins and who has a sample
        {
            u64 cnt = 0;
            double ps = 0.0, d[4], t[4];
            uint32_t occ = 0, seen = 0;
            for (uint32_t base = r.base0; base <= hi; base += STEP) {
                load4_values(D, base + 4 * lane, hi, d);
                sum_rows<MODE, true>(r, s.n, s.narrow, base + 4 * lane, C, seen);
                cnt += sum4(C);
                ps += terms4(C, d, t);
                occ += occupied4(C);
            }
            total = readlane_u64(wave_scan_incl_u64(cnt), 63);
            sum = readlane_f64(wave_scan_incl_f64(ps), 63);
            nb = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl_u32(occ), 63);
            present = wave_or_u32(seen);
        }
        if (total) { // wave-uniform
            // ---- walk 2: up to the step the last threshold falls into
            pct.open(lane < np ? pct_threshold(pa.p[lane], total) : PCT_NONE);
            for (uint32_t base = r.base0; base <= hi && pct.todo; base += STEP) {
                sum_rows<MODE, false>(r, s.n, s.narrow, base + 4 * lane, C, none);
                pct.step(C, sum4(C), base, lane);
            }
        } else {
            sum = 0.0;
            nb = 0;
            present = 0;
        }
    }
    if (lane == 0) {
        if (o.count) o.count[m] = total;
        if (o.sum) o.sum[m] = sum;
        if (o.nbuckets) o.nbuckets[m] = nb;
        if (o.present) o.present[m] = present;
    }
    if (lane < np) store_pct(o.pkeys, o.pvalid, (size_t)m * np + lane, pct.found);
}

template <int MODE, bool IDS>
__global__ __launch_bounds__(WG) void k_across_block(const AcrossSnaps s, uint32_t nmetrics, size_t stride,
                                                        const double *__restrict__ D, const PctArgs pa, uint32_t np,
                                                        const AcrossOut o, const uint32_t *__restrict__ ids, uint32_t nrows)
{
    __shared__ u64 s_cnt[CHUNKS];    // the chunks' counts, then their exclusive prefix
    __shared__ double s_sum[CHUNKS]; // the chunks' sums, then their exclusive prefix (ascending order)
    __shared__ uint32_t s_occ[WG_WAVES], s_seen[WG_WAVES];
    __shared__ u64 s_total;
    __shared__ double s_tsum;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    if (m >= nmetrics) return;
    const Rows r = open_rows<MODE, IDS>(s, row_of<IDS>(ids, nrows, m), stride, lane); // (every wave for itself)
    const uint32_t hi = r.uhi, base0 = r.base0;
    const uint32_t nchunks = base0 != NO_BIN ? (hi - base0) / STEP + 1 : 0; // <= CHUNKS
    uint32_t none = 0;
    // ---- walk 1: every chunk's count and sum
    {
        uint32_t occ = 0, seen = 0;
        for (uint32_t ch = wave; ch < nchunks; ch += WG_WAVES) { // wave-uniform
            u64 C[4];
            double d[4], t[4];
            load4_values(D, base0 + ch * STEP + 4 * lane, hi, d);
            sum_rows<MODE, true>(r, s.n, s.narrow, base0 + ch * STEP + 4 * lane, C, seen);
            const u64 inc = wave_scan_incl_u64(sum4(C));
            const double incs = wave_scan_incl_f64(terms4(C, d, t));
            occ += occupied4(C);
            if (lane == 63) {
                s_cnt[ch] = inc;
                s_sum[ch] = incs;
            }
        }
        occ = wave_scan_incl_u32(occ);
        seen = wave_or_u32(seen);
        if (lane == 63) {
            s_occ[wave] = occ;
            s_seen[wave] = seen;
        }
    }
    __syncthreads();
    if (wave == 0) scan_chunks((lds_u64)s_cnt, (lds_f64)s_sum, nchunks, lane, (lds_u64)&s_total, (lds_f64)&s_tsum);
    __syncthreads();
    const u64 total = s_total;
    if (threadIdx.x == 0) {
        uint32_t nb = 0, present = 0;
        for (int w = 0; w < WG_WAVES; w++) { // (a wave without a chunk left 0)
            nb += s_occ[w];
            present |= s_seen[w];
        }
        if (o.count) o.count[m] = total;
        if (o.sum) o.sum[m] = total ? s_tsum : 0.0;
        if (o.nbuckets) o.nbuckets[m] = total ? nb : 0;
        if (o.present) o.present[m] = total ? present : 0;
    }
    // ---- a wave per percentile (wave-uniform throughout): the chunk its threshold falls into, read once more
    for (uint32_t i = wave; i < np; i += WG_WAVES) {
        uint32_t bin = NO_BIN;
        const u64 T = total ? pct_threshold(pa.p[i], total) : PCT_NONE;
        if (T != PCT_NONE) {
            const uint32_t ch = chunk_of((lds_u64)s_cnt, nchunks, lane, T);
            u64 C[4], pre[4];
            sum_rows<MODE, false>(r, s.n, s.narrow, base0 + ch * STEP + 4 * lane, C, none);
            const u64 tc = sum4(C);
            prefix4(C, s_cnt[ch], tc, wave_scan_incl_u64(tc), pre);
            bin = base0 + ch * STEP + find_in_step(pre, T);
        }
        if (lane == 0) store_pct(o.pkeys, o.pvalid, (size_t)m * np + i, bin);
    }
}

// ---- host side --------------------------------------------------------------------------------------
// Per-device state of this unit (device_ctx<AcrossCtx>).  `mu` is held for the length of a call, the host form's wait for
// its results included.  `order`: the events that put the last snapshot's stream behind the others'.
struct AcrossCtx {
    std::mutex mu;
    double *d_table = nullptr; // D[LH_NKEYS]
    hipEvent_t order[LH_MAX_ACROSS] = {};
    ResultBlocks res;          // host form
    IdBlocks ids;              // host form of lh_across_ids
};
std::atomic<uint32_t> g_wave_from{AC_WAVE_FROM_DEFAULT};

typedef lh::beside::Source<AcrossCtx> Source;

// (cx->mu held) enqueue the walks of rows [first, first + nmetrics), or of rows ids[0 .. nmetrics), on the last snapshot's
// stream, behind what the others' streams hold
int enqueue(const Source *q, size_t nsnaps, const RowSel &sel, size_t nmetrics, const double *p, size_t np, const AcrossOut &o)
{
    const Source &last = q[nsnaps - 1];
    AcrossCtx *cx = last.cx;
    hipStream_t from[LH_MAX_ACROSS];
    for (size_t i = 0; i < nsnaps; i++) from[i] = q[i].stream;
    int rc = order_behind(cx->order, from, nsnaps, last.stream);
    if (!rc) rc = ensure_table(cx->d_table, last.stream, lh::k_value_table<AcrossCtx>);
    const uint32_t *ids = nullptr;
    if (!rc) rc = stage_ids(cx->ids, sel, nmetrics, last.stream, ids);
    if (rc) return rc;
    const uint32_t first = sel.first;
    uint32_t nrows = last.nrows; // what an id is guarded against: the rows of the shortest snapshot
    for (size_t i = 0; i < nsnaps; i++) nrows = q[i].nrows < nrows ? q[i].nrows : nrows;
    const PctArgs pa = pct_args(p, np);
    AcrossSnaps s;
    s.n = (uint32_t)nsnaps;
    s.narrow = 0;
    for (size_t i = 0; i < LH_MAX_ACROSS; i++) {
        const bool in = i < nsnaps;
        s.cells[i] = in ? static_cast<const unsigned char *>(q[i].cells) + (size_t)first * q[i].stride * q[i].cell_bytes : nullptr;
        s.ranges[i] = in ? ranges_from(q[i], first) : nullptr;
        if (in && q[i].cell_bytes == 4) s.narrow |= 1u << i;
    }
    const uint32_t M = (uint32_t)nmetrics, NP = (uint32_t)np;
    const double *D = cx->d_table;
    const size_t stride = last.stride; // (lh_row_stride(): one for all)
    const RowShape sh = row_shape(M, g_wave_from.load(std::memory_order_relaxed));
    const auto launch_as = [&](auto mode, auto by_id) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool IDS = decltype(by_id)::value;
        if (sh.wave) hipLaunchKernelGGL((k_across_wave<MODE, IDS>), sh.grid, sh.block, 0, last.stream, s, M, stride, D, pa, NP, o, ids, nrows);
        else hipLaunchKernelGGL((k_across_block<MODE, IDS>), sh.grid, sh.block, 0, last.stream, s, M, stride, D, pa, NP, o, ids, nrows);
    };
    const auto launch = [&](auto mode) {
        if (sel.by_id) launch_as(mode, std::true_type());
        else launch_as(mode, std::false_type());
    };
    if (s.narrow == (1u << nsnaps) - 1u) launch(std::integral_constant<int, ALL_NARROW>());
    else if (s.narrow == 0) launch(std::integral_constant<int, ALL_WIDE>());
    else launch(std::integral_constant<int, MIXED>());
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

int across(lh_snapshot *const *snaps, size_t nsnaps, const RowSel &sel, size_t nmetrics, const double *p, size_t np, uint32_t flags,
           AcrossOut o, bool device_form)
{
    int rc = check_list_args(snaps, nsnaps, LH_MAX_ACROSS, sel, nmetrics, p, np, flags, o);
    if (rc) return rc;
    Source q[LH_MAX_ACROSS];
    rc = list_cells(snaps, nsnaps, sel, nmetrics, q);
    if (rc) return rc;
    if (nmetrics == 0) return LH_OK; // before any device call
    rc = list_open(snaps, nsnaps, q);
    if (rc) return rc;
    AcrossCtx *cx = q[nsnaps - 1].cx;
    std::lock_guard<std::mutex> g(cx->mu);
    if (device_form) return enqueue(q, nsnaps, sel, nmetrics, p, np, o);

    // host form: results to HBM, then back to the caller's arrays
    rc = list_host_results(cx->res, q[nsnaps - 1].stream, o, nmetrics, np,
                             [&](const AcrossOut &d) { return enqueue(q, nsnaps, sel, nmetrics, p, np, d); });
    return settle_ids(rc, sel, q[nsnaps - 1].stream);
}

} // namespace

extern "C" {

int lh_across(lh_snapshot *const *snaps, size_t nsnaps, uint32_t first, size_t nmetrics, const double *p, size_t np, uint32_t flags,
              uint64_t *count, double *sum, uint32_t *nbuckets, uint32_t *present_bits, int16_t *pkeys, uint8_t *pvalid)
{
    const AcrossOut o = {reinterpret_cast<u64 *>(count), sum, nbuckets, present_bits, pkeys, pvalid};
    return across(snaps, nsnaps, rows_from(first), nmetrics, p, np, flags, o, false);
}

int lh_across_device(lh_snapshot *const *snaps, size_t nsnaps, uint32_t first, size_t nmetrics, const double *p, size_t np,
                     uint32_t flags, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets, uint32_t *d_present_bits,
                     int16_t *d_pkeys, uint8_t *d_pvalid)
{
    const AcrossOut o = {reinterpret_cast<u64 *>(d_count), d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid};
    return across(snaps, nsnaps, rows_from(first), nmetrics, p, np, flags, o, true);
}

int lh_across_ids(lh_snapshot *const *snaps, size_t nsnaps, const uint32_t *ids, size_t n, const double *p, size_t np, uint32_t flags,
                  uint64_t *count, double *sum, uint32_t *nbuckets, uint32_t *present_bits, int16_t *pkeys, uint8_t *pvalid)
{
    const AcrossOut o = {reinterpret_cast<u64 *>(count), sum, nbuckets, present_bits, pkeys, pvalid};
    return across(snaps, nsnaps, rows_by_id(ids, false), n, p, np, flags, o, false);
}

int lh_across_ids_device(lh_snapshot *const *snaps, size_t nsnaps, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                         uint32_t flags, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets, uint32_t *d_present_bits,
                         int16_t *d_pkeys, uint8_t *d_pvalid)
{
    const AcrossOut o = {reinterpret_cast<u64 *>(d_count), d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid};
    return across(snaps, nsnaps, rows_by_id(d_ids, true), n, p, np, flags, o, true);
}

int lh_tool_across_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, AC_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

} // extern "C"
