// lh_pct.h -- the percentile walk of the readers beside the engine: "the first bin whose inclusive prefix reaches
// pct_threshold(p, total)" (metrics.go:406-418), once, for lh_spread.hip, lh_across.hip and lh_kept.hip.  On top of lh_wave.h,
// whose header lists the readers and what every reader starts with.
//   PctArgs, pct_args         the percentiles, by value in the kernel arguments, and the host loop that fills them
//   occupied4, load4_values   a 4-bin group's occupied bins; its entries of the value table alone
//   prefix4, locate_in_step, find_in_step   the prefixes at a lane's four bins; where, inside a step of 256, they reach T
//   central4, sums_in_step, SpreadOut       the spread readers' walk 2: a group's centred terms, the search that also returns
//                                           count_le and sum_le, and their out record
//   Open                      the open thresholds of a wave that walks a row in ascending steps (a percentile per lane)
//   scan_chunks, chunk_of     the workgroup shape: wave 0's scan of the chunk totals in LDS, the chunk a threshold falls into
//   store_pct                 a percentile's key and flag
// Three pieces keep a text of their own, each with a comment at the place (profiles/pct_walk_isa.txt has the figures):
// the spread readers' search, which also returns count_le and sum_le (sums_in_step, below), k_spread_block's pre[4] (through prefix4
// that kernel measures 1 % slower) and k_top_score's search (through find_in_step its code comes out reordered).  And K2's
// copy of the step (lh_kernels.hip's k_extract_wave, pass 2): that file and every header it includes are what the committed
// profiles are stamped with, so it cannot include this one.  A change to the step goes to those four too, by hand.
// The host side is in this header as well, behind the device part: the out record (ListOut), its way through host_results
// and the argument check of the two readers of a LIST of sources, lh_across.hip (snapshots) and lh_kept.hip (kept intervals);
// the same two for the spread readers (check_spread_args, spread_host_results).
#pragma once

#include "lh_beside.h"
#include "lh_wave.h"

namespace lh {

static_assert(LH_MAX_PERCENTILES <= 32, "a percentile per lane, their set in one 32-bit mask");

struct PctArgs { double p[LH_MAX_PERCENTILES]; }; // by value in the kernel arguments (256 bytes)
inline PctArgs pct_args(const double *p, size_t np)
{
    PctArgs pa;
    for (size_t i = 0; i < LH_MAX_PERCENTILES; i++) pa.p[i] = i < np ? p[i] : 0.0;
    return pa;
}

__device__ __forceinline__ uint32_t occupied4(const u64 (&C)[4])
{
    return (C[0] ? 1u : 0u) + (C[1] ? 1u : 0u) + (C[2] ? 1u : 0u) + (C[3] ? 1u : 0u);
}
// the value table's entries of bins b0 .. b0 + 3; a lane whose group starts beyond hi asks for nothing
__device__ __forceinline__ void load4_values(const double *__restrict__ D, uint32_t b0, uint32_t hi, double (&d)[4])
{
    d[0] = d[1] = d[2] = d[3] = 0.0;
    if (b0 <= hi) {
        const f64x2_a8 *dp = reinterpret_cast<const f64x2_a8 *>(D + b0);
        const f64x2_a8 d01 = dp[0], d23 = dp[1];
        d[0] = d01.a; d[1] = d01.b; d[2] = d23.a; d[3] = d23.b;
    }
}

// pre[k]: the inclusive prefix at the lane's bin k.  `before` counts everything below the step, tc is sum4(C) and inc its
// inclusive scan over the lanes.
__device__ __forceinline__ void prefix4(const u64 (&C)[4], u64 before, u64 tc, u64 inc, u64 (&pre)[4])
{
    u64 sofar = before + (inc - tc);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        sofar += C[k];
        pre[k] = sofar;
    }
}
// Where, inside a step of 256, the first inclusive prefix reaches T (wave-uniform T): the first lane whose last bin does
// (wave-uniform) and, per lane, how many of its bins stay below.  The caller knows that the step's last prefix reaches T;
// with a total that wrapped none may, and the answer is then unspecified (lane 63's group).
struct InStep { uint32_t lane, below; };
__device__ __forceinline__ InStep locate_in_step(const u64 (&pre)[4], u64 T)
{
    const unsigned long long reach = __builtin_amdgcn_ballot_w64(pre[3] >= T);
    InStep h;
    h.lane = reach ? (uint32_t)__builtin_ctzll(reach) : 63u;
    h.below = (pre[0] < T ? 1u : 0u) + (pre[1] < T ? 1u : 0u) + (pre[2] < T ? 1u : 0u);
    return h;
}
// ... as the index of that bin in the step
__device__ __forceinline__ uint32_t find_in_step(const u64 (&pre)[4], u64 T)
{
    const InStep h = locate_in_step(pre, T);
    return 4 * h.lane + (uint32_t)__builtin_amdgcn_readlane((int)h.below, (int)h.lane);
}

// float64(count) * (value - mean)^2 of a lane's four bins (an empty cell adds +0)
__device__ __forceinline__ double central4(const u64 (&c)[4], const double (&d)[4], double mean)
{
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double dev = d[k] - mean;
        q[k] = (double)c[k] * (dev * dev);
    }
    return (q[0] + q[1]) + (q[2] + q[3]);
}

// find_in_step with what the spread readers add (lh_spread.hip's two kernels, lh_kept.hip's k_kept_spread), in one piece as it
// was in lh_spread.hip (on top of locate_in_step that unit's kernels come out reordered, and without that function's guard for
// an empty ballot, which this text never had).
// One step of 256 bins in which threshold T is reached (wave-uniform T; `before` counts / `sbefore` sums everything below
// the step).  pre[k]: inclusive prefix count at the lane's bin k; t[k]: the bins' terms; incs: inclusive scan over the lanes
// of the terms' sums.  Returns the index of the bin inside the step, the prefix count and the prefix sum there.
__device__ __forceinline__ uint32_t sums_in_step(const u64 (&pre)[4], const double (&t)[4], double incs, double sbefore, u64 T,
                                                 u64 &cle, double &sle)
{
    // the first lane whose last bin reaches T (lane 63's does), and how many of its bins stay below
    const unsigned long long reach = __builtin_amdgcn_ballot_w64(pre[3] >= T);
    const uint32_t f = (uint32_t)__builtin_ctzll(reach);
    const uint32_t below = (pre[0] < T ? 1u : 0u) + (pre[1] < T ? 1u : 0u) + (pre[2] < T ? 1u : 0u);
    const u64 csel = below == 0 ? pre[0] : below == 1 ? pre[1] : below == 2 ? pre[2] : pre[3];
    double psel = t[0];
    if (below >= 1) psel += t[1];
    if (below >= 2) psel += t[2];
    if (below >= 3) psel += t[3];
    const double lanes_below = readlane_f64(incs, f ? f - 1 : 0);
    cle = readlane_u64(csel, f);
    sle = (sbefore + (f ? lanes_below : 0.0)) + readlane_f64(psel, f);
    return 4 * f + (uint32_t)__builtin_amdgcn_readlane((int)below, (int)f);
}

// The thresholds of a row that a wave walks in ascending steps of 256 bins: lane i < np owns percentile i, the smallest
// prefix count T that reaches it and, once the walk has passed it, its bin.
struct Open {
    uint32_t found = NO_BIN; // NO_BIN: none (yet)
    u64 T, carry;            // (from open() on)  carry: the samples below the next step
    uint32_t todo;           // percentiles without a bin yet
    u64 before, inc;         // of the step ending() saw last: the samples below it, the scan of its lanes' sums
    // `mine`: the lane's pct_threshold(pa.p[lane], total), PCT_NONE from lane np on.  (The caller reads pa: through a
    // reference the load of a kernel argument would be a flat one.)
    __device__ __forceinline__ void open(u64 mine)
    {
        T = mine;
        todo = (uint32_t)__builtin_amdgcn_ballot_w64(T != PCT_NONE);
        carry = 0;
    }
    // One step, tc the sum of the lane's four bins: the percentiles whose threshold falls into it.  For those the caller
    // takes the step's prefixes and finds each one's bin (step(); k_spread_wave, with its sums_in_step).
    __device__ __forceinline__ uint32_t ending(u64 tc)
    {
        inc = wave_scan_incl_u64(tc);
        before = carry;
        carry += readlane_u64(inc, 63);
        // (every open threshold is > before: it would have ended in an earlier step otherwise)
        const uint32_t here = (uint32_t)__builtin_amdgcn_ballot_w64(T <= carry) & todo;
        todo &= ~here;
        return here;
    }
    __device__ __forceinline__ void prefixes(const u64 (&C)[4], u64 tc, u64 (&pre)[4]) const { prefix4(C, before, tc, inc, pre); }
    __device__ __forceinline__ u64 threshold(uint32_t i) const { return readlane_u64(T, i); } // wave-uniform i
    // the step of a reader that wants the bins alone; `base`: the step's first bin
    __device__ __forceinline__ void step(const u64 (&C)[4], u64 tc, uint32_t base, uint32_t lane)
    {
        uint32_t here = ending(tc);
        if (here) {
            u64 pre[4];
            prefixes(C, tc, pre);
            for (; here; here &= here - 1) {
                const uint32_t i = (uint32_t)__builtin_ctz(here);
                const uint32_t idx = find_in_step(pre, threshold(i));
                if (lane == i) found = base + idx;
            }
        }
    }
};

// ---- the workgroup shape: WG_WAVES waves reduce a row's chunks of STEP bins, one lane-63 total each into cnt[] / sum[]
// in LDS (pointers that say so: through a reference the accesses would start out as flat ones).
typedef __attribute__((address_space(3))) u64 *lds_u64;
typedef __attribute__((address_space(3))) double *lds_f64;
// (wave 0, between two __syncthreads)  The chunks' counts and sums become their exclusive prefixes, in ascending order,
// and the row's totals go to *total / *tsum.
__device__ __forceinline__ void scan_chunks(lds_u64 cnt, lds_f64 sum, uint32_t nchunks, uint32_t lane, lds_u64 total, lds_f64 tsum)
{
    u64 v[4];
    double w[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        v[k] = 0;
        w[k] = 0.0;
        if (4 * lane + k < nchunks) { // (one guarded region for both loads)
            v[k] = cnt[4 * lane + k];
            w[k] = sum[4 * lane + k];
        }
    }
    const u64 tv = (v[0] + v[1]) + (v[2] + v[3]);
    const u64 inc = wave_scan_incl_u64(tv);
    const double incs = wave_scan_incl_f64(((w[0] + w[1]) + w[2]) + w[3]);
    const double up = __shfl_up(incs, 1, 64); // what the lanes below add up to
    u64 ex = inc - tv;
    double exs = lane ? up : 0.0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        cnt[4 * lane + k] = ex;
        sum[4 * lane + k] = exs;
        ex += v[k];
        exs += w[k];
    }
    if (lane == 63) {
        *total = inc;
        *tsum = incs;
    }
}
// (a whole wave, T wave-uniform, 1 <= T <= total)  The last chunk with fewer than T samples below it: the one T falls into.
// Chunk 0 has none below, so there is one.
__device__ __forceinline__ uint32_t chunk_of(lds_u64 cnt, uint32_t nchunks, uint32_t lane, u64 T)
{
    uint32_t nlow = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        nlow += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(4 * lane + k < nchunks && cnt[4 * lane + k] < T));
    return nlow - 1;
}

// percentile `at` of the call: its int16 key and whether there is one (found == NO_BIN: none)
__device__ __forceinline__ void store_pct(int16_t *pkeys, uint8_t *pvalid, size_t at, uint32_t found)
{
    const bool ok = found != NO_BIN;
    if (pkeys) pkeys[at] = ok ? (int16_t)bin_to_key(found) : (int16_t)0;
    if (pvalid) pvalid[at] = ok ? 1 : 0;
}

// the seven outputs of the spread readers (lh_spread*, lh_kept_spread*), each null when not asked for
struct SpreadOut {
    u64 *count;
    double *sum, *m2;
    int16_t *pkeys;
    uint8_t *pvalid;
    u64 *count_le;
    double *sum_le;
};

// ---- host side: the readers of a list of sources ------------------------------------------------------------------------
namespace beside {

// The six outputs, each null when not asked for.  PRESENT: a bit per source -- uint32_t for up to 32 of them, u64 for 64.
template <class PRESENT> struct ListOut {
    u64 *count;
    double *sum;
    uint32_t *nbuckets;
    PRESENT *present;
    int16_t *pkeys;
    uint8_t *pvalid;
    // The host form's blocks (host_results): the 8-byte arrays, the 4-byte ones, the keys, the flags -- so `present` is
    // behind nbuckets when it is 4 bytes wide and ahead of it when it is 8.
    static constexpr size_t NB = sizeof(PRESENT) == 8 ? 3 : 2, PR = 5 - NB;
    void blocks(size_t nmetrics, size_t np, HostOut (&out)[6]) const
    {
        const size_t per_m = nmetrics, per_p = nmetrics * np;
        out[0] = {count, per_m * 8};
        out[1] = {sum, per_m * 8};
        out[NB] = {nbuckets, per_m * 4};
        out[PR] = {present, per_m * sizeof(PRESENT)};
        out[4] = {pkeys, per_p * 2};
        out[5] = {pvalid, per_p};
    }
    static ListOut on_device(unsigned char *const (&dev)[6])
    {
        return {reinterpret_cast<u64 *>(dev[0]),     reinterpret_cast<double *>(dev[1]),  reinterpret_cast<uint32_t *>(dev[NB]),
                reinterpret_cast<PRESENT *>(dev[PR]), reinterpret_cast<int16_t *>(dev[4]), reinterpret_cast<uint8_t *>(dev[5])};
    }
};
// (the context's mutex held)  The host form: `enqueue(d)` puts the work that fills d -- o's arrays, in HBM -- on `st`.
template <class PRESENT, class Enqueue>
int list_host_results(ResultBlocks &rb, hipStream_t st, const ListOut<PRESENT> &o, size_t nmetrics, size_t np, Enqueue enqueue)
{
    HostOut out[6];
    o.blocks(nmetrics, np, out);
    return host_results(rb, st, out, [&](unsigned char *const(&dev)[6]) { return enqueue(ListOut<PRESENT>::on_device(dev)); });
}

// unless `list` is a list of 1 .. `most` handles, none of them NULL
template <class H> bool bad_list(H *const *list, size_t n, size_t most)
{
    if (!list || misaligned(list, alignof(H *)) || n == 0 || n > most) return true;
    for (size_t i = 0; i < n; i++)
        if (!list[i]) return true;
    return false;
}

// Every check that needs neither a source nor a device: a list of 1 .. `most` handles, a row selection, percentiles, the
// six outputs.  With np == 0 the per-percentile outputs are ignored: they are nulled here, and count for nothing.
template <class H, class PRESENT>
int check_list_args(H *const *list, size_t n, size_t most, const RowSel &sel, size_t nmetrics, const double *p, size_t np,
                    uint32_t flags, ListOut<PRESENT> &o)
{
    if (bad_ids(sel, nmetrics) || bad_list(list, n, most)) return LH_EINVAL;
    if (np > LH_MAX_PERCENTILES || (np && !p) || flags != 0) return LH_EINVAL;
    if (np == 0) {
        o.pkeys = nullptr;
        o.pvalid = nullptr;
    }
    if (!o.count && !o.sum && !o.nbuckets && !o.present && !o.pkeys && !o.pvalid) return LH_EINVAL;
    if ((np && misaligned(p, 8)) || misaligned(o.count, 8) || misaligned(o.sum, 8) || misaligned(o.nbuckets, 4) ||
        misaligned(o.present, sizeof(PRESENT)) || misaligned(o.pkeys, 2))
        return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    return LH_OK;
}

// ---- the spread readers (lh_spread.hip over a snapshot, lh_kept.hip over kept intervals) ---------------------------------------
// Their checks of the percentiles and the seven outputs, which need neither a source nor a device (LH_EINVAL, or LH_OK).  With
// np == 0 the per-percentile outputs are ignored: they are nulled here, and count for nothing.
inline int check_spread_args(const double *p, size_t np, SpreadOut &o)
{
    if (np > LH_MAX_PERCENTILES || (np && !p)) return LH_EINVAL;
    if (np == 0) {
        o.pkeys = nullptr;
        o.pvalid = nullptr;
        o.count_le = nullptr;
        o.sum_le = nullptr;
    }
    if (!o.count && !o.sum && !o.m2 && !o.pkeys && !o.pvalid && !o.count_le && !o.sum_le) return LH_EINVAL;
    if ((np && misaligned(p, 8)) || misaligned(o.count, 8) || misaligned(o.sum, 8) || misaligned(o.m2, 8) ||
        misaligned(o.pkeys, 2) || misaligned(o.count_le, 8) || misaligned(o.sum_le, 8))
        return LH_EINVAL;
    return LH_OK;
}
// (the context's mutex held)  Their host form: `enqueue(d)` puts the work that fills d -- o's arrays, in HBM -- on `st`.  The
// 8-byte arrays, then the keys, then the flags.
template <class Enqueue>
int spread_host_results(ResultBlocks &rb, hipStream_t st, const SpreadOut &o, size_t nmetrics, size_t np, Enqueue enqueue)
{
    const size_t per_m = nmetrics, per_p = nmetrics * np;
    const HostOut out[7] = {{o.count, per_m * 8},    {o.sum, per_m * 8},    {o.m2, per_m * 8},   {o.count_le, per_p * 8},
                            {o.sum_le, per_p * 8}, {o.pkeys, per_p * 2}, {o.pvalid, per_p}};
    return host_results(rb, st, out, [&](unsigned char *const(&dev)[7]) {
        SpreadOut d;
        d.count = reinterpret_cast<u64 *>(dev[0]);
        d.sum = reinterpret_cast<double *>(dev[1]);
        d.m2 = reinterpret_cast<double *>(dev[2]);
        d.count_le = reinterpret_cast<u64 *>(dev[3]);
        d.sum_le = reinterpret_cast<double *>(dev[4]);
        d.pkeys = reinterpret_cast<int16_t *>(dev[5]);
        d.pvalid = reinterpret_cast<uint8_t *>(dev[6]);
        return enqueue(d);
    });
}

} // namespace beside
} // namespace lh
