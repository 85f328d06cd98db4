// lh_fmt.h -- Go's %f for a float64 on the device (strconv.FormatFloat(v, 'f', 6, 64): the exact decimal expansion, 6
// fractional digits, round-half-even on the exact value, "NaN" / "+Inf" / "-Inf"), and the workgroup scan the line kernels
// lay their output out with.  The only copy: K6 (lh_kernels_fmt.hip) and lh_lines.hip both format with it, and
// tests/test_gpu_serialize.py (test_format_f_matches_go_percent_f) and tests/test_gpu_lines.py hold it to the oracle
// through either.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lh {
namespace fmt {

constexpr int BLOCK = 256;        // one thread per line
constexpr int WAVES = BLOCK / 64;
constexpr uint32_t MAX_F = 317;   // the longest %f: '-' + 309 integer digits + '.' + 6

struct Dec {
    uint64_t ip;    // integer part (kind 0)
    uint32_t frac;  // 6 fractional digits as an integer 0..999999 (kind 0)
    uint32_t kind;  // 0: |v| < 2^64, 1: |v| >= 2^64 (an integer), 2: NaN, 3: Inf
    uint32_t neg;
};

__device__ __forceinline__ Dec decompose(double v)
{
    Dec d;
    const uint64_t bits = (uint64_t)__double_as_longlong(v);
    d.neg = (uint32_t)(bits >> 63);
    d.ip = 0;
    d.frac = 0;
    const uint32_t eb = (uint32_t)(bits >> 52) & 0x7ffu;
    if (eb == 0x7ffu) {
        d.kind = (bits & 0xfffffffffffffull) ? 2u : 3u;
        return d;
    }
    const double a = __longlong_as_double((long long)(bits & 0x7fffffffffffffffull));
    if (a >= 18446744073709551616.0) {
        d.kind = 1;
        return d;
    }
    d.kind = 0;
    d.ip = (uint64_t)a; // exact: a < 2^64
    if (a < 9007199254740992.0) {
        const double fp = a - (double)d.ip; // exact: the fractional part of a float64 is a float64
        if (fp != 0.0) {
            const uint64_t fb = (uint64_t)__double_as_longlong(fp);
            uint32_t fe = (uint32_t)(fb >> 52) & 0x7ffu;
            uint64_t fm = fb & 0xfffffffffffffull;
            if (fe) fm |= 1ull << 52; else fe = 1;
            const uint32_t s = 1075u - fe; // fp = fm * 2^-s, s >= 1
            if (s <= 74u) {                // else fp * 1e6 < 2^53 * 2^20 / 2^75 = 0.25: rounds to 0, no tie
                const unsigned __int128 P = (unsigned __int128)fm * 1000000u; // < 2^73
                uint64_t q = (uint64_t)(P >> s);
                const unsigned __int128 rem = P & ((((unsigned __int128)1) << s) - 1);
                const unsigned __int128 half = ((unsigned __int128)1) << (s - 1);
                if (rem > half || (rem == half && (q & 1))) q++;
                if (q == 1000000u) { q = 0; d.ip++; }
                d.frac = (uint32_t)q;
            }
        }
    }
    return d;
}

__device__ __forceinline__ uint32_t ndigits_u64(uint64_t x)
{
    if (x >= 10000000000000000000ull) return 20;
    uint32_t n = 1;
    uint64_t p = 10;
    while (x >= p) { n++; p *= 10; }
    return n;
}

__device__ __forceinline__ void put_digits(char *dst, uint64_t x, uint32_t nd)
{
    for (int i = (int)nd - 1; i >= 0; i--) {
        const uint64_t q = x / 10;
        dst[i] = (char)('0' + (uint32_t)(x - q * 10));
        x = q;
    }
}

// |v| >= 2^64: the value is the integer mant * 2^sh.  Decimal digits by repeated division by 1e9 (the rare path).
// Returns the digit count; writes them when dst != nullptr.  (static: every unit that includes this has its own, out of line.)
static __device__ __noinline__ uint32_t big_digits(uint64_t bits, char *dst)
{
    const uint32_t eb = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t mant = (bits & 0xfffffffffffffull) | (1ull << 52);
    const uint32_t sh = eb - 1075u; // 11 .. 971
    uint32_t w[33];
    for (int i = 0; i < 33; i++) w[i] = 0;
    const uint32_t wi = sh >> 5, bi = sh & 31u;
    const unsigned __int128 m = (unsigned __int128)mant << bi; // < 2^84
    w[wi] = (uint32_t)m;
    w[wi + 1] = (uint32_t)(m >> 32);
    w[wi + 2] = (uint32_t)(m >> 64);
    int nw = (int)wi + 3;
    while (nw > 0 && w[nw - 1] == 0) nw--;
    uint32_t chunk[36];
    int nc = 0;
    while (nw > 0) {
        uint64_t rem = 0;
        for (int i = nw - 1; i >= 0; i--) {
            const uint64_t cur = (rem << 32) | w[i];
            const uint64_t q = cur / 1000000000ull;
            w[i] = (uint32_t)q;
            rem = cur - q * 1000000000ull;
        }
        chunk[nc++] = (uint32_t)rem;
        while (nw > 0 && w[nw - 1] == 0) nw--;
    }
    const uint32_t top = ndigits_u64(chunk[nc - 1]);
    const uint32_t nd = top + 9u * (uint32_t)(nc - 1);
    if (dst) {
        put_digits(dst, chunk[nc - 1], top);
        char *p = dst + top;
        for (int c = nc - 2; c >= 0; c--, p += 9) put_digits(p, chunk[c], 9);
    }
    return nd;
}

// Length of "%f" of v; writes the text when WRITE.
template <bool WRITE> __device__ __forceinline__ uint32_t fmt_f(double v, char *dst)
{
    const Dec d = decompose(v);
    if (d.kind == 2u) {
        if (WRITE) { dst[0] = 'N'; dst[1] = 'a'; dst[2] = 'N'; }
        return 3;
    }
    if (d.kind == 3u) {
        if (WRITE) { dst[0] = d.neg ? '-' : '+'; dst[1] = 'I'; dst[2] = 'n'; dst[3] = 'f'; }
        return 4;
    }
    uint32_t pos = 0;
    if (d.neg) {
        if (WRITE) dst[0] = '-';
        pos = 1;
    }
    uint32_t nd;
    if (d.kind == 1u) {
        nd = big_digits((uint64_t)__double_as_longlong(v), WRITE ? dst + pos : nullptr);
    } else {
        nd = ndigits_u64(d.ip);
        if (WRITE) put_digits(dst + pos, d.ip, nd);
    }
    pos += nd;
    if (WRITE) {
        dst[pos] = '.';
        put_digits(dst + pos + 1, d.frac, 6);
    }
    return pos + 7;
}

// exclusive prefix of v over the BLOCK threads of a workgroup, and their total (s_w: WAVES words of LDS).  Every thread of
// the workgroup calls it; what was written to LDS before it is visible behind it.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if ((int)lane >= d) inc += y;
    }
    __syncthreads();
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        if (w < (int)wave) base += s_w[w];
        tot += s_w[w];
    }
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ char *put_bytes(char *dst, const char *src, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) dst[i] = src[i];
    return dst + n;
}

} // namespace fmt
} // namespace lh
