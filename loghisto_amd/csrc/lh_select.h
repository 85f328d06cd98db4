// lh_select.h -- the select pass of the units that pick k names out of a range (lh_top.hip, lh_movers.hip, and lh_kept.hip's
// lh_kept_top* / lh_kept_movers*, which share the first two's records and Emit functors: they are here): a score pass of
// the unit leaves, per row, a 64-bit ORDER-PRESERVING key (larger is ahead; order_key_f64 makes one of a float64) and a
// candidate word (0: the row is never ranked) in HBM, and k_select takes the k largest keys among the candidates, equal keys
// lowest index first, and sorts them.  What a winner's entry looks like is the unit's own: its Emit functor writes it.
//   k_select  ONE workgroup of 1 024 threads looping over the records.  An exact k-th-key search, MSB first, eight passes of
//             8 bits with a 256-entry histogram in LDS (a wave whose records all fall into one bin adds them with one
//             atomic: the high bytes of counts are mostly zero); then one pass in index order that takes every record ahead of
//             the k-th key and, of those equal to it, the lowest indices -- a prefix count over the records, never an atomic
//             whose order depends on timing; then a bitonic sort of the at most 1 024 winners by (key descending, index
//             ascending) in LDS; then emit(i, t) for the winner i of every slot t, and n_out.  One total order: the result
//             depends on neither timing nor launch shape.
//   k_select_windows  the same body (select_block) with one workgroup per WINDOW of a call that selects in many at once: window w's
//             records lie w * npad records into every field, its entries w * k entries into out, its count in n_out[w].
// Both arrays are padded to whole groups of SEL_PER records (16-byte loads stay inside the block).
//
// Behind the kernels, the host side of "score pass, then k_select" (a new selecting reader starts there): SelectState,
// select_check_args, select_records, select_pass, select_host_form and select_passes_ms; for a call of many windows,
// select_windows_pass and select_windows_host_form.  The unit keeps its context type with its own mutex, its record struct,
// its score kernel, its Emit and its enqueue.
#pragma once

#include "../../include/loghisto_gpu.h"
#include "lh_beside.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <cstring>

namespace lh {

constexpr int SEL_WG = 1024, SEL_WAVES = SEL_WG / 64;   // k_select
constexpr uint32_t SEL_PER = 4;                         // consecutive records per thread and tile
constexpr uint32_t SEL_TILE = SEL_WG * SEL_PER;
constexpr uint32_t NO_SLOT = 0xffffffffu;               // the index of a padding slot of the sort: behind every record
static_assert(LH_MAX_TOP == SEL_WG, "a thread per winner in the sort");
static_assert(SEL_TILE <= 0x10000, "a tile's two prefix counts share one 32-bit scan");

// a float64 as an unsigned integer of the same order (-0.0 == +0.0; the host sees to it that no NaN is ranked)
__device__ __forceinline__ u64 order_key_f64(double x)
{
    if (x == 0.0) x = 0.0; // -0.0 -> +0.0
    const u64 b = (u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// One more record in bin d of the histogram for the lanes with `in` set.  A wave whose records share the bin (every pass
// over bytes the keys have in common) adds them with ONE atomic instead of up to 64 on one address.  Called under
// workgroup-uniform control.  (Integer adds: the histogram does not depend on their order.)
__device__ __forceinline__ void hist_add(uint32_t *hist, bool in, uint32_t d, uint32_t lane)
{
    const unsigned long long act = __builtin_amdgcn_ballot_w64(in);
    if (!act) return; // wave-uniform
    const uint32_t lead = (uint32_t)__builtin_ctzll(act);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)lead);
    if (__builtin_amdgcn_ballot_w64(in && d == d0) == act) {
        if (lane == lead) atomicAdd(&hist[d0 & 255u], (uint32_t)__builtin_popcountll(act));
    } else if (in) {
        atomicAdd(&hist[d & 255u], 1u);
    }
}

// records i0 .. i0 + 3 (i0 a multiple of 4; the arrays are padded to whole groups): their keys, and -- only where some
// record of the group passes `keep` -- their counts.  ok[j]: record i0 + j exists, passes `keep` and is a candidate.
template <class Keep>
__device__ __forceinline__ void load_records(const u64 *__restrict__ key, const u64 *__restrict__ count, size_t i0, uint32_t n,
                                             u64 (&kk)[SEL_PER], bool (&ok)[SEL_PER], Keep keep)
{
#pragma unroll
    for (uint32_t j = 0; j < SEL_PER; j++) { kk[j] = 0; ok[j] = false; }
    if (i0 >= n) return;
    const u64x2_a8 *kp = reinterpret_cast<const u64x2_a8 *>(key + i0);
    const u64x2_a8 k01 = kp[0], k23 = kp[1];
    kk[0] = k01.a; kk[1] = k01.b; kk[2] = k23.a; kk[3] = k23.b;
    bool any = false;
#pragma unroll
    for (uint32_t j = 0; j < SEL_PER; j++) {
        ok[j] = j < n - i0 && keep(kk[j]);
        any = any || ok[j];
    }
    if (!any) return;
    const u64x2_a8 *cp = reinterpret_cast<const u64x2_a8 *>(count + i0);
    const u64x2_a8 c01 = cp[0], c23 = cp[1];
    ok[0] = ok[0] && c01.a != 0; ok[1] = ok[1] && c01.b != 0; ok[2] = ok[2] && c23.a != 0; ok[3] = ok[3] && c23.b != 0;
}

// (a key, an index) ahead of another in the result: the larger key, then the lower index.  Padding slots (key 0, index
// NO_SLOT) stay behind every record.
__device__ __forceinline__ bool ahead(u64 ka, uint32_t ia, u64 kb, uint32_t ib) { return ka > kb || (ka == kb && ia < ib); }

// (the whole workgroup of SEL_WG threads)  key / cand: the n records (cand[i] == 0: record i is no candidate).  emit(i, t): winner
// i lands in slot t (t < *n_out = min(k, candidates); slot 0 is the leader).  1 <= k <= LH_MAX_TOP.  The body of k_select and of
// k_select_windows: the LDS below is the kernel's that calls it.
template <class Emit>
__device__ __forceinline__ void select_block(const u64 *__restrict__ key, const u64 *__restrict__ cand, uint32_t n, uint32_t k,
                                             const Emit emit, uint32_t *__restrict__ n_out)
{
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_part[SEL_WAVES];
    __shared__ uint32_t s_digit, s_rem, s_take;
    __shared__ u64 s_wkey[LH_MAX_TOP];
    __shared__ uint32_t s_widx[LH_MAX_TOP];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ntiles = n / SEL_TILE + (n % SEL_TILE != 0); // (n + SEL_TILE - 1 would wrap near 2^32)

    // ---- the k-th largest key among the candidates: `prefix` holds its bytes above `shift`; of the candidates that share
    // them, the rem-th largest is looked for
    u64 prefix = 0;
    uint32_t rem = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (uint32_t t = 0; t < ntiles; t++) { // workgroup-uniform
            u64 kk[SEL_PER];
            bool ok[SEL_PER];
            load_records(key, cand, (size_t)t * SEL_TILE + SEL_PER * tid, n, kk, ok,
                         [&](u64 x) { return shift == 56 || (x >> (shift + 8)) == prefix; });
#pragma unroll
            for (uint32_t j = 0; j < SEL_PER; j++) hist_add(s_hist, ok[j], (uint32_t)(kk[j] >> shift) & 255u, lane);
        }
        __syncthreads();
        if (wave == 0) {
            // bins in DESCENDING order, four per lane: position q = 4 * lane + j is bin 255 - q
            uint32_t v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) v[j] = s_hist[255u - (4 * lane + j)];
            const uint32_t tv = (v[0] + v[1]) + (v[2] + v[3]);
            const uint32_t inc = wave_scan_incl_u32(tv);
            const uint32_t all = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            // (the top byte's pass counts the candidates: fewer than k, and all of them are taken; none, and rem is 0)
            const uint32_t want = shift == 56 ? min(rem, all) : rem;
            if (shift == 56 && lane == 0) s_take = want;
            if (want == 0) {
                if (lane == 0) s_rem = 0;
            } else {
                // the first position whose inclusive count reaches `want` (all >= want: one does)
                const uint32_t f = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(inc >= want));
                if (lane == f) {
                    uint32_t run = inc - tv, j = 0;
                    while (j < 3 && run + v[j] < want) run += v[j++];
                    s_digit = 255u - (4 * lane + j);
                    s_rem = want - run; // among the records of that bin
                }
            }
        }
        __syncthreads();
        rem = s_rem;
        if (rem == 0) { // workgroup-uniform: no candidate at all
            if (tid == 0) *n_out = 0;
            return;
        }
        prefix = (prefix << 8) | s_digit;
        // (s_hist, s_digit and s_rem are written again only behind the next pass's first barrier)
    }
    // `prefix` is the k-th key (the last candidate's when there are fewer than k), nwin records are taken: the nahead that
    // are strictly ahead of it and the first rem, in index order, of those equal to it.
    const u64 kth = prefix;
    const uint32_t nwin = min(s_take, (uint32_t)LH_MAX_TOP), nahead = nwin - min(rem, nwin);

    // ---- the winners into LDS, by a prefix count over the records in index order
    uint32_t gt_base = 0, eq_base = 0; // records of either kind in the tiles so far
    for (uint32_t t = 0; t < ntiles && (gt_base < nahead || eq_base < rem); t++) { // workgroup-uniform
        u64 kk[SEL_PER];
        bool ok[SEL_PER];
        const size_t i0 = (size_t)t * SEL_TILE + SEL_PER * tid; // (the last tile's tail may lie beyond 2^32)
        load_records(key, cand, i0, n, kk, ok, [&](u64 x) { return x >= kth; });
        uint32_t mine = 0; // records ahead in the high half, equal ones in the low half (a tile has at most 4 096 of each)
#pragma unroll
        for (uint32_t j = 0; j < SEL_PER; j++) mine += ok[j] ? (kk[j] > kth ? 0x10000u : 1u) : 0u;
        const uint32_t inc = wave_scan_incl_u32(mine);
        if (lane == 63) s_part[wave] = inc;
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < SEL_WAVES; w++) {
            const uint32_t p = s_part[w];
            before += w < wave ? p : 0u;
            tile += p;
        }
        before += inc - mine;
        uint32_t gpos = gt_base + (before >> 16), epos = eq_base + (before & 0xffffu);
#pragma unroll
        for (uint32_t j = 0; j < SEL_PER; j++) {
            if (!ok[j]) continue;
            uint32_t slot = NO_SLOT;
            if (kk[j] > kth) slot = gpos++;
            else if (epos++ < rem) slot = nahead + (epos - 1);
            if (slot < nwin) { // (every slot handed out is: the guard keeps a wrong count from writing outside the block)
                s_wkey[slot] = kk[j];
                s_widx[slot] = (uint32_t)(i0 + j); // (an existing record: below n)
            }
        }
        gt_base += tile >> 16;
        eq_base += tile & 0xffffu;
        __syncthreads(); // s_part is rewritten by the next tile
    }

    // ---- bitonic sort of the winners by (key descending, index ascending), padded to a power of two
    uint32_t width = 1;
    while (width < nwin) width <<= 1;
    if (tid >= nwin && tid < width) {
        s_wkey[tid] = 0;
        s_widx[tid] = NO_SLOT;
    }
    for (uint32_t size = 2; size <= width; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const uint32_t other = tid ^ stride;
            if (other > tid && other < width) {
                const u64 ka = s_wkey[tid], kb = s_wkey[other];
                const uint32_t ia = s_widx[tid], ib = s_widx[other];
                const bool up = (tid & size) == 0; // this run ends up with its leader first
                if (ahead(kb, ib, ka, ia) == up) {
                    s_wkey[tid] = kb; s_widx[tid] = ib;
                    s_wkey[other] = ka; s_widx[other] = ia;
                }
            }
        }
    }
    __syncthreads();
    // (every winner's index is below n: the guard keeps a wrong slot from reading outside the block)
    if (tid < nwin && s_widx[tid] < n) emit(s_widx[tid], tid);
    if (tid == 0) *n_out = nwin;
}

// ONE selection: one workgroup over the n records
template <class Emit>
__global__ __launch_bounds__(SEL_WG) void k_select(const u64 *__restrict__ key, const u64 *__restrict__ cand, uint32_t n, uint32_t k,
                                                   const Emit emit, uint32_t *__restrict__ n_out)
{
    select_block(key, cand, n, k, emit, n_out);
}

// ONE SELECTION PER WINDOW (lh_kept_top_series* / lh_kept_movers_series*): workgroup w = blockIdx.x runs the same body over window
// w's records, key + w * npad and cand + w * npad (npad: n padded to whole groups of SEL_PER, so every window's block starts on
// 32 bytes), with the Emit advanced to that window -- its record fields by w * npad, its out by w * k -- and the count to
// n_out[w].  The windows share nothing: no atomic and no order between them, and each keeps k_select's one total order.
template <class Emit>
__global__ __launch_bounds__(SEL_WG) void k_select_windows(const u64 *__restrict__ key, const u64 *__restrict__ cand, uint32_t n,
                                                           uint32_t npad, uint32_t k, const Emit emit, uint32_t *__restrict__ n_out)
{
    const size_t at = (size_t)blockIdx.x * npad;
    select_block(key + at, cand + at, n, k, emit.window(at, (size_t)blockIdx.x * k), n_out + blockIdx.x);
}

// ---- the records and the Emit of the two kinds of selection, each shared by the unit that scores snapshots and the one that
// scores kept intervals (lh_top.hip / lh_movers.hip, lh_kept.hip): one array per field, each padded to whole groups of SEL_PER
// (16-byte loads stay inside the block).
struct TopRecords {
    u64 *key;    // order-preserving, larger is ahead
    u64 *count;  // 0: not a candidate
    double *sum;
    u64 *aux;    // BY_PERCENTILE: the int16 key's 16 bits; BY_COUNT_ABOVE: the count above; else 0
};
// winner i lands in slot t
struct TopEmit {
    TopRecords r;
    uint32_t first, by;
    lh_top_entry *out;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t t) const
    {
        const u64 aux = r.aux[i];
        lh_top_entry e;
        e.id = first + i;
        e.pkey = by == LH_TOP_BY_PERCENTILE ? (int16_t)(uint16_t)aux : (int16_t)0;
        e.reserved = 0;
        e.count = r.count[i];
        e.sum = r.sum[i];
        e.above = by == LH_TOP_BY_COUNT_ABOVE ? aux : 0;
        out[t] = e;
    }
    // the Emit of the window whose records begin `at` records into every field and whose entries begin `to` entries into out
    __device__ __forceinline__ TopEmit window(size_t at, size_t to) const
    {
        return TopEmit{TopRecords{r.key + at, r.count + at, r.sum + at, r.aux + at}, first, by, out + to};
    }
};

constexpr u64 MOVER_CANDIDATE = 1ull << 32; // the candidate word of a row that is ranked; its low 32 bits: key << 16 | key_base
struct MoversRecords {
    u64 *key;     // order-preserving, larger is ahead
    u64 *cand;    // 0: not a candidate
    u64 *count_a, *count_b;
    u64 *score;   // the float64's bits
};
// winner i lands in slot t
struct MoversEmit {
    MoversRecords r;
    uint32_t first;
    lh_mover_entry *out;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t t) const
    {
        const uint32_t keys = (uint32_t)r.cand[i];
        lh_mover_entry e;
        e.id = first + i;
        e.key = (int16_t)(uint16_t)(keys >> 16);
        e.key_base = (int16_t)(uint16_t)keys;
        e.count_a = r.count_a[i];
        e.count_b = r.count_b[i];
        e.score = __longlong_as_double((long long)r.score[i]);
        out[t] = e;
    }
    // (TopEmit::window's)
    __device__ __forceinline__ MoversEmit window(size_t at, size_t to) const
    {
        return MoversEmit{MoversRecords{r.key + at, r.cand + at, r.count_a + at, r.count_b + at, r.score + at}, first, out + to};
    }
};
static_assert(sizeof(lh_top_entry) == 32 && sizeof(lh_mover_entry) == 32, "32-byte entries");

// ---- host side --------------------------------------------------------------------------------------
namespace beside {

// the fields of the two record kinds carved out of select_records' block
static inline TopRecords top_records(u64 *base, size_t npad)
{
    TopRecords r;
    r.key = base;
    r.count = r.key + npad;
    r.sum = reinterpret_cast<double *>(r.count + npad);
    r.aux = reinterpret_cast<u64 *>(r.sum + npad);
    return r;
}
static inline MoversRecords movers_records(u64 *base, size_t npad)
{
    MoversRecords r;
    r.key = base;
    r.cand = r.key + npad;
    r.count_a = r.cand + npad;
    r.count_b = r.count_a + npad;
    r.score = r.count_b + npad;
    return r;
}
constexpr size_t TOP_FIELDS = 4, MOVERS_FIELDS = 5;

// What a selecting unit keeps per device beside its own mutex and extras (a member of its context: device_ctx hands out
// one slot array per context type, so units never wait for each other).  Snapshots of different engines run on
// different streams, and the records block outlives a device-form call: it is guarded by an event, not by stream order.
struct __attribute__((visibility("hidden"))) SelectState { // (hidden: the library exports nothing of this header)
    u64 *d_records = nullptr; // the unit's arrays of padded nmetrics 8-byte fields, one behind the other
    size_t rec_cap = 0;       // (in records)
    ResultBlocks res;         // host form: k entries and n_out
    EventGuard guard;         // behind the last select pass
};

// The checks of a selecting call that need neither a snapshot nor what is ranked.  A unit returns this AFTER its own
// LH_EINVAL causes (handles, `by`, `arg`, flags): every LH_EINVAL wins over the early LH_ERANGE.
static inline int select_check_args(size_t nmetrics, size_t k, const void *out, const void *n_out, uintptr_t n_out_align)
{
    if (k == 0 || k > LH_MAX_TOP) return LH_EINVAL;
    if (!out || !n_out || misaligned(out, 8) || misaligned(n_out, n_out_align)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    return LH_OK;
}

// (the context's mutex held)  The records of a call of nmetrics rows whose passes go on `st`: `fields` arrays of npad
// 8-byte fields from `base` on, npad = nmetrics padded to whole groups of SEL_PER.  The unit carves its fields out of that.
static inline int select_records(SelectState &ss, hipStream_t st, size_t nmetrics, size_t fields, u64 *&base, size_t &npad)
{
    int rc = ss.guard.create();
    if (rc) return rc;
    npad = (nmetrics + SEL_PER - 1) & ~(size_t)(SEL_PER - 1);
    if (ss.rec_cap < npad) rc = ss.guard.host_wait(); // the block is about to be freed: an earlier call's passes may still use it
    if (!rc) rc = grow_device(ss.d_records, ss.rec_cap, npad, 4096, fields * sizeof(u64));
    // (another stream's call may still read the records: this one's passes wait for it on the device, not on the host)
    if (!rc) rc = ss.guard.stream_wait(st);
    base = ss.d_records;
    return rc;
}

// (the context's mutex held; behind the unit's score launch)  The second pass over the n records on `st`, and the guard's
// event behind it.  ev (may be null): ev[1] is recorded between the passes and ev[2] behind the select pass; ev[0], before
// the score pass, is the unit's.
template <class Emit>
int select_pass(SelectState &ss, hipStream_t st, const u64 *key, const u64 *cand, uint32_t n, size_t k, const Emit &emit,
                uint32_t *d_n_out, hipEvent_t *ev)
{
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_select<Emit>, dim3(1), dim3(SEL_WG), 0, st, key, cand, n, (uint32_t)k, emit, d_n_out);
    LH_BESIDE_CHK(hipGetLastError());
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[2], st));
    return ss.guard.record(st);
}

// (the context's mutex held; behind the unit's score launch over nwin windows' records)  select_pass' launch for a call of nwin
// windows, window w's n records at w * npad, its entries at d_out + w * k (inside `emit`), its count at d_n_out[w].  The guard's
// event is NOT recorded here: such a call runs chunk after chunk over one reused block, which stream order protects, and records
// the guard behind the last one.
template <class Emit>
int select_windows_pass(hipStream_t st, const u64 *key, const u64 *cand, uint32_t n, uint32_t npad, uint32_t nwin, size_t k,
                        const Emit &emit, uint32_t *d_n_out, hipEvent_t *ev)
{
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_select_windows<Emit>, dim3(nwin), dim3(SEL_WG), 0, st, key, cand, n, npad, (uint32_t)k, emit, d_n_out);
    LH_BESIDE_CHK(hipGetLastError());
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[2], st));
    return LH_OK;
}

// where the nwin counts lie behind nwin * k entries of a landing block, and what the two take together
static inline size_t select_counts_at(size_t nwin, size_t k, size_t entry_bytes) { return nwin * k * entry_bytes; }
static inline size_t select_landing_bytes(size_t nwin, size_t k, size_t entry_bytes)
{
    return select_counts_at(nwin, k, entry_bytes) + ((nwin * sizeof(uint32_t) + 7) & ~(size_t)7);
}

// (the context's mutex held) the host form's landing blocks: k entries, then n_out
static inline int select_result_blocks(ResultBlocks &res, size_t need)
{
    int rc = grow_device(res.d_res, res.d_cap, need, RESULT_FLOOR);
    if (!rc) rc = grow_pinned(res.h_res, res.h_cap, need, RESULT_FLOOR);
    return rc;
}

// (the context's mutex held, the wait included)  The host form around the unit's enqueue(d_out, d_n_out, ev) -> status,
// which puts both passes on `st`.  Entries at and beyond n_out are not written, and n_out is known only once the select
// pass has run: the k entries and n_out come back in one copy into the unit's pinned block, whatever memory `out` is, and
// the first n_out entries go on from there (at most 32 KiB; straight into a pinned `out` would be a second round trip).
template <class Entry, class Enqueue>
int select_host_form(SelectState &ss, hipStream_t st, size_t k, Entry *out, size_t *n_out, Enqueue enqueue)
{
    const size_t bytes = k * sizeof(Entry);
    int rc = select_result_blocks(ss.res, bytes + 8);
    if (rc) return rc;
    rc = enqueue(reinterpret_cast<Entry *>(ss.res.d_res), reinterpret_cast<uint32_t *>(ss.res.d_res + bytes), (hipEvent_t *)nullptr);
    if (rc) return rc;
    LH_BESIDE_CHK(hipMemcpyAsync(ss.res.h_res, ss.res.d_res, bytes + 8, hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    const uint32_t *h_n = reinterpret_cast<const uint32_t *>(ss.res.h_res + bytes);
    if (*h_n > k) return LH_ESTATE;
    std::memcpy(out, ss.res.h_res, (size_t)*h_n * sizeof(Entry));
    ss.guard.covered(); // this call recorded the event on the stream it has just waited for
    *n_out = *h_n;
    return LH_OK;
}

// (the context's mutex held, the wait included)  The host form of a call of nwin windows around the unit's enqueue(d_out, d_n_out)
// -> status, which puts every pass on `st` and records the guard: nwin * k entries and nwin counts come back in ONE copy into the
// unit's pinned block (at most LH_MAX_WINDOWS * LH_MAX_TOP entries of 32 bytes and 512 bytes of counts), and the first n_out[w]
// entries of each window go on from there to out + w * k.  Nothing is written to the caller's arrays unless every count is sane.
template <class Entry, class Enqueue>
int select_windows_host_form(SelectState &ss, hipStream_t st, size_t nwin, size_t k, Entry *out, size_t *n_out, Enqueue enqueue)
{
    const size_t counts_at = select_counts_at(nwin, k, sizeof(Entry)), bytes = select_landing_bytes(nwin, k, sizeof(Entry));
    int rc = select_result_blocks(ss.res, bytes);
    if (rc) return rc;
    rc = enqueue(reinterpret_cast<Entry *>(ss.res.d_res), reinterpret_cast<uint32_t *>(ss.res.d_res + counts_at));
    if (rc) return rc;
    LH_BESIDE_CHK(hipMemcpyAsync(ss.res.h_res, ss.res.d_res, bytes, hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    ss.guard.covered(); // this call recorded the event on the stream it has just waited for
    const uint32_t *h_n = reinterpret_cast<const uint32_t *>(ss.res.h_res + counts_at);
    const Entry *h_out = reinterpret_cast<const Entry *>(ss.res.h_res);
    for (size_t w = 0; w < nwin; w++)
        if (h_n[w] > k) return LH_ESTATE;
    for (size_t w = 0; w < nwin; w++) {
        std::memcpy(out + w * k, h_out + w * k, (size_t)h_n[w] * sizeof(Entry));
        n_out[w] = h_n[w];
    }
    return LH_OK;
}

// (the context's mutex held)  lh_tool_*_passes_ms: both passes once, the results left in the unit's own block, with the
// device time of each.  A failure before the times are read leaves score_ms / select_ms untouched.  nwin: the windows of a
// per-window call's chunk (k entries and a count each); 1 for the others.
template <class Entry, class Enqueue>
int select_passes_ms(SelectState &ss, hipStream_t st, size_t k, float *score_ms, float *select_ms, Enqueue enqueue, size_t nwin = 1)
{
    const size_t bytes = select_counts_at(nwin, k, sizeof(Entry));
    int rc = select_result_blocks(ss.res, select_landing_bytes(nwin, k, sizeof(Entry)));
    if (rc) return rc;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3 && rc == LH_OK; i++)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = LH_EDEVICE;
    if (rc == LH_OK) rc = enqueue(reinterpret_cast<Entry *>(ss.res.d_res), reinterpret_cast<uint32_t *>(ss.res.d_res + bytes), ev);
    if (rc == LH_OK && (hipStreamSynchronize(st) != hipSuccess || hipEventElapsedTime(score_ms, ev[0], ev[1]) != hipSuccess ||
                        hipEventElapsedTime(select_ms, ev[1], ev[2]) != hipSuccess))
        rc = LH_EDEVICE;
    if (rc == LH_OK) ss.guard.covered();
    for (int i = 0; i < 3; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (rc == LH_EDEVICE) (void)hipGetLastError();
    return rc;
}

} // namespace beside
} // namespace lh
