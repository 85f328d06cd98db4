// lh_pair.h -- the device side of the units that walk TWO rows at once, a name in one snapshot against the same name in
// another (lh_compare.hip, lh_movers.hip), or in one list of kept intervals against another (lh_kept.hip's k_kept_compare):
// what the walk is scaled by (Scale), a lane's state of it (Best), a name's results and the lane that stores them (CompareOut,
// store_row), a lane's four
// bins (take4) and the wave's largest X at its lowest bin (wave_best, without LDS: DPP max-reductions, lh_wave.h's wave_max_u32, over the
// 32-bit words of X from the top).  lh_compare.hip's header says what X, ks, w1 and shift are; a unit that wants the bits of
// k_compare_wave's sums calls these in its order: the steps in ascending order per lane, then one DPP tree over the lanes.
// Behind the device part, CompareOut's way through host_results (compare_host_results), for lh_compare.hip and lh_kept.hip.
#pragma once

#include "lh_beside.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

namespace lh {

typedef unsigned __int128 u128;

// What a name's walk is scaled by: the totals, and na nb as the divisor of the sums' terms.
struct Scale {
    u64 na, nb;
    uint32_t sh; // the bits na nb has beyond 64
    double den;  // float64(na nb >> sh)
};
__device__ __forceinline__ Scale make_scale(u64 na, u64 nb)
{
    Scale s;
    s.na = na;
    s.nb = nb;
    const u128 p = (u128)na * nb;
    const u64 ph = (u64)(p >> 64);
    s.sh = ph ? 64u - (uint32_t)__builtin_clzll(ph) : 0u; // <= 64
    s.den = (double)(u64)(p >> s.sh);
    return s;
}

// A lane's state of walk 2
struct Best {
    u128 x;      // the largest X so far
    uint32_t bin;
    u64 a, b;    // the prefixes there
    double w, s; // the lane's share of w1 and of shift
};
__device__ __forceinline__ void best_init(Best &r)
{
    r.x = 0;
    r.bin = NO_BIN;
    r.a = r.b = 0;
    r.w = r.s = 0.0;
}
// A name's eight results, each null when not asked for (lh_compare*'s and lh_kept_compare*'s outputs)
struct CompareOut {
    u64 *count_a, *count_b;
    double *ks;
    int16_t *ks_key;
    u64 *below_a, *below_b;
    double *w1, *shift;
};
// one lane writes a name's results; bin == NO_BIN: the two normalised distributions are identical
__device__ __forceinline__ void store_row(const CompareOut &o, uint32_t m, u64 na, u64 nb, uint32_t bin, u64 a, u64 b, double w1,
                                          double shift)
{
    double ks = 0.0;
    if (na == 0 || nb == 0) {
        ks = w1 = shift = __builtin_nan("");
        bin = NO_BIN;
    }
    if (bin == NO_BIN) a = b = 0;
    else ks = fabs((double)a / (double)na - (double)b / (double)nb);
    if (o.count_a) o.count_a[m] = na;
    if (o.count_b) o.count_b[m] = nb;
    if (o.ks) o.ks[m] = ks;
    if (o.ks_key) o.ks_key[m] = bin == NO_BIN ? (int16_t)0 : (int16_t)bin_to_key(bin);
    if (o.below_a) o.below_a[m] = a;
    if (o.below_b) o.below_b[m] = b;
    if (o.w1) o.w1[m] = w1;
    if (o.shift) o.shift[m] = shift;
}
// the lane's four bins bin0 .. bin0 + 3; pa / pb: the prefixes below them
__device__ __forceinline__ void take4(Best &r, const Scale &sc, uint32_t bin0, u64 pa, u64 pb, const u64 (&a)[4], const u64 (&b)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        pa += a[k];
        pb += b[k];
        const u128 xa = (u128)pa * sc.nb, xb = (u128)pb * sc.na;
        const bool up = xa >= xb;
        const u128 x = up ? xa - xb : xb - xa;
        if (x > r.x) {
            r.x = x;
            r.bin = bin0 + k;
            r.a = pa;
            r.b = pb;
        }
        const double t = (double)(u64)(x >> sc.sh) / sc.den;
        r.w += t;
        r.s += up ? t : -t;
    }
}
// The wave's best: the largest X, at the lowest bin among equals (wave-uniform results).  X == 0 everywhere: NO_BIN.
__device__ __forceinline__ void wave_best(const Best &r, u128 &x, uint32_t &bin, u64 &a, u64 &b)
{
    bool in = true;
#pragma unroll
    for (int w = 3; w >= 0; w--) {
        const uint32_t word = (uint32_t)(r.x >> (32 * w));
        const uint32_t top = wave_max_u32(in ? word : 0u);
        in = in && word == top;
    }
    const uint32_t inv = wave_max_u32(in ? ~r.bin : 0u); // the lowest bin: the largest complement (NO_BIN's is 0)
    const uint32_t src = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(in && ~r.bin == inv)); // (lane 0 at least, with NO_BIN)
    bin = ~inv;
    a = readlane_u64(r.a, src);
    b = readlane_u64(r.b, src);
    x = ((u128)readlane_u64((u64)(r.x >> 64), src) << 64) | readlane_u64((u64)r.x, src);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
namespace beside {

// (the context's mutex held)  The host form of lh_compare* and lh_kept_compare*: `enqueue(d)` puts the work that fills d -- o's
// arrays, in HBM -- on `st`.  The 8-byte arrays, then the keys.
template <class Enqueue>
int compare_host_results(ResultBlocks &rb, hipStream_t st, const CompareOut &o, size_t nmetrics, Enqueue enqueue)
{
    const size_t n8 = nmetrics * 8;
    const HostOut out[8] = {{o.count_a, n8}, {o.count_b, n8}, {o.ks, n8},    {o.below_a, n8},
                            {o.below_b, n8}, {o.w1, n8},      {o.shift, n8}, {o.ks_key, nmetrics * 2}};
    return host_results(rb, st, out, [&](unsigned char *const(&dev)[8]) {
        CompareOut d;
        d.count_a = reinterpret_cast<u64 *>(dev[0]);
        d.count_b = reinterpret_cast<u64 *>(dev[1]);
        d.ks = reinterpret_cast<double *>(dev[2]);
        d.below_a = reinterpret_cast<u64 *>(dev[3]);
        d.below_b = reinterpret_cast<u64 *>(dev[4]);
        d.w1 = reinterpret_cast<double *>(dev[5]);
        d.shift = reinterpret_cast<double *>(dev[6]);
        d.ks_key = reinterpret_cast<int16_t *>(dev[7]);
        return enqueue(d);
    });
}

} // namespace beside
} // namespace lh
