// lh_wave.h -- the device side of the units that read a snapshot (lh_count.hip, lh_spread.hip, lh_top.hip, lh_compare.hip,
// lh_movers.hip, lh_across.hip -- with lh_pair.h for a walk over two rows and lh_select.h for a selection across names; a
// new reader starts here and in lh_beside.h):
//   wave primitives   DPP scans, cross-lane reads, the packed 16-byte load types
//   the arithmetic    the percentile threshold (pct_threshold) and the bound-to-key rule (le_take)
//   the row walk      the geometry of the two launch shapes, a row's own span (Span, own_span), which row an entry of a call
//                     reads (row_of, row_span: the block's m-th, or -- the *_ids forms -- the one an id array names), a row's 4-bin group as one
//                     load (load4_cells; load4_in inside a span; load4 with the bins' values), a group's count and weighted
//                     sum (sum4, terms4) and the generator of the value table (k_value_table)
// The wave primitives, the threshold and the packed types are also K2's (lh_kernels.hip's k_extract_wave): the only copy
// (tests/test_pct_threshold_model.py has the threshold's arithmetic, tests/test_gpu_extract_thresholds.py and
// tests/test_gpu_spread.py hold it to the oracle).  Every unit that includes it is built with -ffp-contract=off (build.py's _COMMON).
#pragma once

#include "lh_codec.h"

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lh {

typedef unsigned long long u64; // (uint64_t is unsigned long: a distinct type)

// The two launch shapes of a reader.  Wave form: a wave per row, ROW_WAVES rows per workgroup.  Workgroup form: WG_WAVES
// waves per row.  Either way a wave takes STEP bins per step, four consecutive ones per lane.
constexpr int ROW_BLOCK = 256, ROW_WAVES = ROW_BLOCK / 64;
constexpr int WG = 1024, WG_WAVES = WG / 64;
constexpr uint32_t STEP = 256;
constexpr uint32_t CHUNKS = LH_NKEYS / STEP; // chunks of the widest span (a span starts at a multiple of 4)
static_assert(CHUNKS == 4 * 64, "wave 0 scans the chunk totals four per lane");
constexpr uint32_t NO_BIN = 0xffffffffu;

// ---------------------------------------------------------------------------
// Wave-level arithmetic that stays in the VALU (DPP): k_extract_wave's scans and reductions.  __shfl_up / __shfl_down
// compile to ds_bpermute_b32 -- a round trip through the LDS crossbar each, two per 64-bit value -- and round 4's
// wave kernel issued 216 of them per name.
// ---------------------------------------------------------------------------
#define LH_DPP32(x, ctrl, rows) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(x), (ctrl), (rows), 0xf, false))
template <int CTRL, int ROWS> __device__ __forceinline__ uint64_t dpp_u64(uint64_t x)
{
    const uint32_t lo = LH_DPP32((uint32_t)x, CTRL, ROWS), hi = LH_DPP32((uint32_t)(x >> 32), CTRL, ROWS);
    return ((uint64_t)hi << 32) | lo; // lanes without a source (or outside ROWS) get 0
}
template <int CTRL, int ROWS> __device__ __forceinline__ double dpp_f64(double x) // ... +0.0
{
    return __longlong_as_double((long long)dpp_u64<CTRL, ROWS>((uint64_t)__double_as_longlong(x)));
}
// inclusive prefix sum over the 64 lanes: four steps inside the rows of 16 lanes (row_shr:1/2/4/8), then lane 15 of
// rows 0 and 2 into rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31)
__device__ __forceinline__ uint64_t wave_scan_incl_u64(uint64_t x)
{
    x += dpp_u64<0x111, 0xf>(x);
    x += dpp_u64<0x112, 0xf>(x);
    x += dpp_u64<0x114, 0xf>(x);
    x += dpp_u64<0x118, 0xf>(x);
    x += dpp_u64<0x142, 0xa>(x);
    x += dpp_u64<0x143, 0xc>(x);
    return x;
}
__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t x)
{
    x += LH_DPP32(x, 0x111, 0xf);
    x += LH_DPP32(x, 0x112, 0xf);
    x += LH_DPP32(x, 0x114, 0xf);
    x += LH_DPP32(x, 0x118, 0xf);
    x += LH_DPP32(x, 0x142, 0xa);
    x += LH_DPP32(x, 0x143, 0xc);
    return x;
}
// the same tree in float64: one fixed association, whatever the timing
__device__ __forceinline__ double wave_scan_incl_f64(double x)
{
    x += dpp_f64<0x111, 0xf>(x);
    x += dpp_f64<0x112, 0xf>(x);
    x += dpp_f64<0x114, 0xf>(x);
    x += dpp_f64<0x118, 0xf>(x);
    x += dpp_f64<0x142, 0xa>(x);
    x += dpp_f64<0x143, 0xc>(x);
    return x;
}
// the maximum / the bitwise OR over the 64 lanes, wave-uniform (the same tree; lanes without a source add 0)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
    x = max(x, LH_DPP32(x, 0x111, 0xf));
    x = max(x, LH_DPP32(x, 0x112, 0xf));
    x = max(x, LH_DPP32(x, 0x114, 0xf));
    x = max(x, LH_DPP32(x, 0x118, 0xf));
    x = max(x, LH_DPP32(x, 0x142, 0xa));
    x = max(x, LH_DPP32(x, 0x143, 0xc));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x)
{
    x |= LH_DPP32(x, 0x111, 0xf);
    x |= LH_DPP32(x, 0x112, 0xf);
    x |= LH_DPP32(x, 0x114, 0xf);
    x |= LH_DPP32(x, 0x118, 0xf);
    x |= LH_DPP32(x, 0x142, 0xa);
    x |= LH_DPP32(x, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t x, uint32_t src) // src wave-uniform
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double readlane_f64(double x, uint32_t src)
{
    return __longlong_as_double((long long)readlane_u64((uint64_t)__double_as_longlong(x), src));
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, uint32_t src) // src per lane
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, (int)src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), (int)src, 64);
    return ((uint64_t)hi << 32) | lo;
}
// x of lane + D for the lanes whose lane + D is in the same row of 16 (what the others get does not matter to the caller)
template <int D> __device__ __forceinline__ double row_down_f64(double x)
{
    return __longlong_as_double((long long)dpp_u64<0x100 + D, 0xf>((uint64_t)__double_as_longlong(x))); // row_shl:D
}

// metrics.go:413 as an INTEGER threshold: float64(sofar) / float64(total) >= p is monotone in sofar, so there is a
// smallest prefix count T in [1, total] that reaches percentile p, and "the first bucket that reaches p" is the first
// bin whose inclusive prefix is >= T (that bin is occupied: the prefix moves there).  One to three IEEE divides per
// (name, percentile) -- by the lane that owns the percentile -- instead of one per cell.  PCT_NONE: no prefix reaches p
// (p > 1 or NaN: the key is omitted, metrics.go:417).
constexpr uint64_t PCT_NONE = ~0ull;
__device__ __forceinline__ bool pct_reached(uint64_t s, double ft, double p) { return (double)s / ft >= p; }
__device__ inline uint64_t pct_threshold(double p, uint64_t total)
{
    if (!(1.0 >= p)) return PCT_NONE; // the largest quotient is float64(total) / float64(total) == 1
    if (p <= 0.0) return 1;           // the first occupied bucket
    const double ft = (double)total, est = p * ft;
    uint64_t s = est >= 18446744073709549568.0 ? total : (uint64_t)est;
    if ((double)s < est) s++; // ceil(p * total): the threshold itself unless a rounding went the other way
    s = s < 1 ? 1 : (s > total ? total : s);
    if (pct_reached(s, ft, p) && (s == 1 || !pct_reached(s - 1, ft, p))) return s; // two divides: the usual case
#pragma unroll 1
    for (int it = 0; it < 4 && s > 1 && pct_reached(s - 1, ft, p); it++) s--;
#pragma unroll 1
    for (int it = 0; it < 4 && s < total && !pct_reached(s, ft, p); it++) s++;
    if (pct_reached(s, ft, p) && (s == 1 || !pct_reached(s - 1, ft, p))) return s;
    // not settled in four steps either way (totals beyond 2^53, where float64(s) moves in steps): bisection;
    // reached(total) holds
    uint64_t lo = 0, hi = total;
#pragma unroll 1
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (pct_reached(mid, ft, p)) hi = mid; else lo = mid;
    }
    return hi;
}

// How many leading bins bound b takes in (0 .. 65 536): bin(compress(b)) + 1 (metrics.go:316-322 with the extended key
// before its int16 truncation, by the arithmetic the ingest's threshold table is generated with; -0.0 and 0.0 both give
// key 0).  0 for -Inf and for negative bounds beyond the int16 key range, 65 536 for +Inf and positive ones beyond it.
// The host refused NaN.  lh_count_le*'s bound-to-key rule, and lh_top's for LH_TOP_BY_COUNT_ABOVE.
constexpr uint32_t LE_TAKE_ALL = LH_NKEYS;
__device__ __forceinline__ uint32_t le_take(double b)
{
    const double a = fabs(b);
    if (!(a <= 1.7976931348623157e308)) return b > 0 ? LE_TAKE_ALL : 0u; // +-Inf
    const int kext = d_kext_golog(1.0 + a);
    if (kext > 32767) return b > 0 ? LE_TAKE_ALL : 0u;                     // where the reference's int16 keys wrap
    return key_to_bin(b < 0 ? -kext : kext) + 1u;
}

// 16 bytes at an 8-byte-aligned address as ONE load (global_load_dwordx4; unaligned vector access is on for HSA)
struct __attribute__((packed, aligned(8))) u64x2_a8 { uint64_t a, b; };
struct __attribute__((packed, aligned(8))) f64x2_a8 { double a, b; };
struct __attribute__((packed, aligned(4))) u32x4_a4 { uint32_t a, b, c, d; };

// bins b0 .. b0 + 3 of a row; a lane whose group starts beyond hi asks for nothing.  The caller keeps hi <= 65 535 and
// the rows at least LH_NKEYS + 4 cells apart, so the group ends inside the row's own stride.  (ACC: the caller's 64-bit
// unsigned type -- uint64_t and unsigned long long are distinct.)
template <typename CELL, typename ACC>
__device__ __forceinline__ void load4_cells(const CELL *__restrict__ row, uint32_t b0, uint32_t hi, ACC (&c)[4])
{
    static_assert(sizeof(ACC) == 8 && (sizeof(CELL) == 4 || sizeof(CELL) == 8), "32- or 64-bit cells into 64-bit counts");
    c[0] = c[1] = c[2] = c[3] = 0;
    if (b0 <= hi) {
        if constexpr (sizeof(CELL) == 4) {
            const u32x4_a4 q = *reinterpret_cast<const u32x4_a4 *>(row + b0);
            c[0] = q.a; c[1] = q.b; c[2] = q.c; c[3] = q.d;
        } else {
            const u64x2_a8 *rp = reinterpret_cast<const u64x2_a8 *>(row + b0);
            const u64x2_a8 c01 = rp[0], c23 = rp[1];
            c[0] = c01.a; c[1] = c01.b; c[2] = c23.a; c[3] = c23.b;
        }
    }
}

// One row's own span [lo, hi]: its cells outside are zero, and a row that was never marked has lo > hi -- nothing of it may
// be read.  A walk enters at base0(), lo aligned down to a multiple of 4: whole groups, every load 16-byte aligned.
struct Span {
    uint32_t lo, hi;
    __device__ __forceinline__ bool any() const { return lo <= hi; }
    __device__ __forceinline__ uint32_t base0() const { return lo & ~3u; }
};
__device__ __forceinline__ Span own_span(const uint32_t *__restrict__ ranges, uint32_t m)
{
    Span s;
    s.lo = ranges[2 * (size_t)m];
    s.hi = min(ranges[2 * (size_t)m + 1], (uint32_t)LH_NKEYS - 1);
    return s;
}
// Which row entry m of a call reads.  A contiguous call (IDS false) reads row m of the block it was handed; an id-list call
// (the *_ids forms) reads row ids[m] of the snapshot -- m is wave-uniform, so that is one uniform load per row and the row's
// address is scalar from there on.  An id at or beyond `nrows` gives NO_ROW: row_span then returns an empty span, the one a
// row that was never marked has, and by the rule above nothing of such a row is read -- not its span either.  m stays the
// index of every output (and of a per-entry input such as lh_count_le's bounds row).
constexpr uint32_t NO_ROW = 0xffffffffu;
template <bool IDS> __device__ __forceinline__ uint32_t row_of(const uint32_t *__restrict__ ids, uint32_t nrows, uint32_t m)
{
    if constexpr (!IDS) {
        return m;
    } else {
        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)m); // (unsigned: a list may pass 2^31 entries)
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)ids[at]);
        return r < nrows ? r : NO_ROW;
    }
}
template <bool IDS> __device__ __forceinline__ Span row_span(const uint32_t *__restrict__ ranges, uint32_t r)
{
    if constexpr (IDS) {
        if (r == NO_ROW) {
            Span s;
            s.lo = NO_BIN;
            s.hi = 0;
            return s;
        }
    }
    return own_span(ranges, r);
}
// the same, entered at a multiple of 4, with lo = NO_BIN > hi = 0 for a row that was never marked: what a union of spans
// (the least lo, the largest hi) and load4_in take
__device__ __forceinline__ Span or_empty(Span s)
{
    Span r;
    r.lo = s.any() ? s.base0() : NO_BIN;
    r.hi = s.any() ? s.hi : 0u;
    return r;
}
// bins b0 .. b0 + 3 of a row, zeros outside its own span `s` (from or_empty; b0 a multiple of 4; hi <= 65 535: the group ends inside the row).
// For a walk that may leave the span at its lower end (lh_compare.hip's, over the union of two); one that starts at
// base0() calls load4_cells.
// (lh_across.hip's fetch4 restates this rule for a row whose address comes out of a lane: a change here goes there too.)
template <typename CELL>
__device__ __forceinline__ void load4_in(const CELL *__restrict__ row, uint32_t b0, Span s, u64 (&c)[4])
{
    load4_cells(row, b0 >= s.lo ? b0 : NO_BIN, s.hi, c); // (NO_BIN > hi: nothing is asked for)
}
// bins b0 .. b0 + 3 of a row and their entries of the value table; a lane whose group starts beyond hi asks for nothing.
// b0 is a multiple of 4 and hi <= 65 535, so the group ends inside the row (and inside the table's LH_NKEYS entries).
// (d is zeroed BEFORE load4_cells: behind it the compiler keeps two guarded regions apart, profiles/shared_headers_isa.txt)
template <typename CELL>
__device__ __forceinline__ void load4(const CELL *__restrict__ row, const double *__restrict__ D, uint32_t b0, uint32_t hi,
                                      u64 (&c)[4], double (&d)[4])
{
    d[0] = d[1] = d[2] = d[3] = 0.0;
    load4_cells(row, b0, hi, c);
    if (b0 <= hi) {
        const f64x2_a8 *dp = reinterpret_cast<const f64x2_a8 *>(D + b0);
        const f64x2_a8 d01 = dp[0], d23 = dp[1];
        d[0] = d01.a; d[1] = d01.b; d[2] = d23.a; d[3] = d23.b;
    }
}
// The value table: D[b] = decompress(bin_to_key(b)), the bits of lh_codec_tables' D[] (-ffp-contract=off).  512 KiB,
// resident in L2 beside the windows; evaluating exp() per cell would cost an IEEE divide each.  A unit that weighs cells
// generates its own, once per device (beside::ensure_table), with k_value_table<its context type>: an instantiation per
// unit, none in a unit that has no use for it.
template <class Unit> __global__ __launch_bounds__(256) void k_value_table(double *__restrict__ D)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < LH_NKEYS) D[b] = d_decompress_bin(b);
}

__device__ __forceinline__ u64 sum4(const u64 (&c)[4]) { return (c[0] + c[1]) + (c[2] + c[3]); }
// value * float64(count) of a lane's four bins (metrics.go:344) and their sum, always associated the same way
__device__ __forceinline__ double terms4(const u64 (&c)[4], const double (&d)[4], double (&t)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = d[k] * (double)c[k];
    return (t[0] + t[1]) + (t[2] + t[3]);
}

} // namespace lh
