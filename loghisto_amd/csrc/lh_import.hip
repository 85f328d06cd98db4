// lh_import.hip -- cells back IN: lh_snapshot_add_buckets* (include/loghisto_gpu.h), the inverse of lh_buckets_all.
//
// The reference's interval is RawMetricSet.Histograms, name -> {int16 key -> count} (/root/reference/metrics.go:54-60),
// and its cells are a commutative integer sum (atomic.AddUint64, metrics.go:278, 292): adding another process's interval,
// an older interval of one's own, or a checkpoint is  snapshot[id][key] += count  per CELL, not per sample.
//
// Built BESIDE the engine, on its public C ABI only (lh_beside.h), and the one such unit that WRITES:
//   lh_snapshot_cells       number of rows, without moving anything
//   lh_snapshot_rows        the uint64 view (a snapshot of 32-bit cells moves to its wide store first)
//   lh_snapshot_stream      the stream the snapshot's extract / clear work is ordered on: the adds go there
//   lh_snapshot_mark_dirty  declares the buffer's cell sizes unknown to a later lh_snapshot_merge.  Called on ONE touched
//                           row with one of that row's own added bins, so that it widens no span: the kernels keep the
//                           spans tight themselves (atomicMin / atomicMax per run of equal ids)
//
// Shape of the add kernels: lane l of a wave takes cell 64 u + l of its group, so
// that one atomic wave-instruction covers 64 CONSECUTIVE entries -- raw sets arrive grouped by name with ascending keys,
// which makes that 512 contiguous bytes of one row -- instead of 64 entries 8 cells apart (a lane that owned 8
// consecutive cells would read them with 16-byte loads, and spread every atomic instruction over 64 separate 64-byte
// segments).  The loads are therefore 8 / 4 / 2 bytes per lane, each instruction contiguous over the wave, several groups
// in flight.  The 64-bit adds return nothing (global_atomic_add_x2 without glc).
#include "../../include/loghisto_gpu.h"
#include "lh_beside.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

namespace {

using namespace lh::beside;

typedef unsigned long long u64;

constexpr int IM_BLOCK = 256;          // 4 waves
constexpr int IM_UNROLL = 8;           // groups of 64 entries a wave keeps in flight
constexpr uint32_t IM_NOID = 0xffffffffu;
constexpr uint32_t IM_EMPTY_LO = LH_NKEYS, IM_EMPTY_HI = 0;
constexpr size_t IM_STAGE_CELLS = size_t(1) << 21; // host forms: entries per pinned staging chunk (28 MiB)

// what the validation pre-pass of the device forms brings back (one small copy, one stream wait per call)
struct ImportResult {
    uint32_t bad;        // an id >= nrows / offsets that decrease
    uint32_t touch_row;  // one entry with count != 0: its row ...
    uint32_t touch_bin;  // ... and bin (for the lh_snapshot_mark_dirty call)
    uint32_t reserved;
    u64 nnz;             // entries with count != 0
    u64 touch_idx;       // the lowest such entry's index (~0: none)
};

__device__ __forceinline__ uint32_t bin_of(int16_t key) { return (uint32_t)(uint16_t)key ^ 0x8000u; }

// Every lane brings (id, lo, hi): the span of the bins it added to row id (lo > hi: none; id == IM_NOID: nothing to
// report).  One atomicMin + one atomicMax per RUN of equal ids in the wave (segmented inclusive scan over the lanes,
// the run's last lane holds its union), not per cell.  All 64 lanes call it.
__device__ __forceinline__ void wave_range_update(uint32_t *__restrict__ ranges, uint32_t id, uint32_t lo, uint32_t hi)
{
    const int lane = threadIdx.x & 63;
    const uint32_t prev = __shfl_up(id, 1, 64), next = __shfl_down(id, 1, 64);
    int head = lane == 0 || prev != id;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t plo = __shfl_up(lo, d, 64), phi = __shfl_up(hi, d, 64);
        const int ph = __shfl_up(head, d, 64);
        if (lane >= d && !head) {
            lo = min(lo, plo);
            hi = max(hi, phi);
            head = ph;
        }
    }
    const bool tail = lane == 63 || next != id;
    if (tail && id != IM_NOID && lo <= hi) {
        atomicMin(ranges + 2 * (size_t)id, lo);
        atomicMax(ranges + 2 * (size_t)id + 1, hi);
    }
}

// rows[ids[i]][bin(keys[i])] += counts[i], i < n.  Persistent workgroups, grid-stride over tiles of 4 waves x IM_UNROLL
// groups; ids were validated before the launch and are checked again here (a store never leaves the rows).
__global__ __launch_bounds__(IM_BLOCK) void k_add_coo(const uint32_t *__restrict__ ids, const int16_t *__restrict__ keys,
                                                      const u64 *__restrict__ counts, size_t n, u64 *__restrict__ rows,
                                                      uint32_t *__restrict__ ranges, uint32_t nrows, size_t stride)
{
    constexpr size_t WAVE_TILE = 64 * IM_UNROLL, TILE = (IM_BLOCK / 64) * WAVE_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ntiles = (n + TILE - 1) / TILE;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t base = t * TILE + (size_t)wave * WAVE_TILE + lane;
        u64 c[IM_UNROLL];
        uint32_t id[IM_UNROLL], bin[IM_UNROLL];
        if (base - lane + WAVE_TILE <= n) { // the whole wave tile is there: every load issued before the first use
#pragma unroll
            for (int u = 0; u < IM_UNROLL; u++) c[u] = __builtin_nontemporal_load(counts + base + u * 64);
#pragma unroll
            for (int u = 0; u < IM_UNROLL; u++) id[u] = __builtin_nontemporal_load(ids + base + u * 64);
#pragma unroll
            for (int u = 0; u < IM_UNROLL; u++) bin[u] = bin_of(__builtin_nontemporal_load(keys + base + u * 64));
        } else {
#pragma unroll
            for (int u = 0; u < IM_UNROLL; u++) {
                const size_t i = base + u * 64;
                const bool in = i < n;
                c[u] = in ? counts[i] : 0;
                id[u] = in ? ids[i] : IM_NOID;
                bin[u] = in ? bin_of(keys[i]) : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < IM_UNROLL; u++) {
            const bool add = c[u] != 0 && id[u] < nrows;
            if (add) atomicAdd(rows + (size_t)id[u] * stride + bin[u], c[u]);
            wave_range_update(ranges, id[u] < nrows ? id[u] : IM_NOID, add ? bin[u] : IM_EMPTY_LO, add ? bin[u] : IM_EMPTY_HI);
        }
    }
}

// Metric first + m gets keys / counts[offsets[m] .. offsets[m + 1]): one wave per row walks its segment coalesced, keeps
// min / max bin in registers and issues one span update per row.  No id array is read: 10 bytes per cell, not 14.
__global__ __launch_bounds__(IM_BLOCK) void k_add_csr(const u64 *__restrict__ offsets, const int16_t *__restrict__ keys,
                                                      const u64 *__restrict__ counts, uint32_t first, uint32_t nmetrics,
                                                      u64 *__restrict__ rows, uint32_t *__restrict__ ranges, size_t stride)
{
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * (IM_BLOCK / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (IM_BLOCK / 64);
    for (uint32_t m = wave; m < nmetrics; m += nwaves) {
        const u64 a = offsets[m], b = offsets[m + 1];
        if (a >= b) continue; // (wave-uniform)
        u64 *__restrict__ row = rows + (size_t)(first + m) * stride;
        uint32_t lo = IM_EMPTY_LO, hi = IM_EMPTY_HI;
        for (u64 i0 = a; i0 < b; i0 += 64 * U) {
            u64 c[U];
            uint32_t bin[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const u64 i = i0 + u * 64 + lane;
                c[u] = i < b ? __builtin_nontemporal_load(counts + i) : 0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const u64 i = i0 + u * 64 + lane;
                bin[u] = i < b ? bin_of(__builtin_nontemporal_load(keys + i)) : 0;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (c[u] != 0) {
                    atomicAdd(row + bin[u], c[u]);
                    lo = min(lo, bin[u]);
                    hi = max(hi, bin[u]);
                }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor(lo, d, 64));
            hi = max(hi, (uint32_t)__shfl_xor(hi, d, 64));
        }
        if (lane == 0 && lo <= hi) {
            atomicMin(ranges + 2 * (size_t)(first + m), lo);
            atomicMax(ranges + 2 * (size_t)(first + m) + 1, hi);
        }
    }
}

// ---- validation pre-pass of the device forms ------------------------------------------------------
__global__ void k_result_init(ImportResult *res)
{
    res->bad = 0;
    res->touch_row = res->touch_bin = res->reserved = 0;
    res->nnz = 0;
    res->touch_idx = ~u64(0);
}

// one set of atomics per wave, at the end of its grid-stride loop
__device__ __forceinline__ void result_fold(ImportResult *res, uint32_t bad, u64 nnz, u64 idx)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bad |= (uint32_t)__shfl_xor(bad, d, 64);
        nnz += (u64)__shfl_xor(nnz, d, 64);
        const u64 o = (u64)__shfl_xor(idx, d, 64);
        idx = o < idx ? o : idx;
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&res->bad, 1u);
        if (nnz) atomicAdd(&res->nnz, nnz);
        if (idx != ~u64(0)) atomicMin(&res->touch_idx, idx);
    }
}

__global__ __launch_bounds__(IM_BLOCK) void k_check_coo(const uint32_t *__restrict__ ids, const u64 *__restrict__ counts,
                                                        size_t n, uint32_t nrows, ImportResult *res)
{
    uint32_t bad = 0;
    u64 nnz = 0, idx = ~u64(0);
    for (size_t i = (size_t)blockIdx.x * IM_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IM_BLOCK) {
        bad |= ids[i] >= nrows;
        if (counts[i] != 0) {
            nnz++;
            idx = i < idx ? i : idx;
        }
    }
    result_fold(res, bad, nnz, idx);
}

__global__ __launch_bounds__(IM_BLOCK) void k_check_offsets(const u64 *__restrict__ offsets, uint32_t nmetrics, ImportResult *res)
{
    uint32_t bad = 0;
    for (size_t i = (size_t)blockIdx.x * IM_BLOCK + threadIdx.x; i < nmetrics; i += (size_t)gridDim.x * IM_BLOCK)
        bad |= offsets[i] > offsets[i + 1];
    result_fold(res, bad, 0, ~u64(0));
}

// runs behind k_check_offsets on the same stream: decreasing offsets bound nothing, and then no count is read
__global__ __launch_bounds__(IM_BLOCK) void k_check_csr_counts(const u64 *__restrict__ offsets, uint32_t nmetrics,
                                                               const u64 *__restrict__ counts, ImportResult *res)
{
    if (res->bad) return;
    const u64 a = offsets[0], b = offsets[nmetrics];
    if (!counts) { // the caller passed no cell arrays: only an all-empty CSR may do that
        if (b > a && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&res->bad, 1u);
        return;
    }
    u64 nnz = 0, idx = ~u64(0);
    for (u64 i = a + (u64)blockIdx.x * IM_BLOCK + threadIdx.x; i < b; i += (u64)gridDim.x * IM_BLOCK) {
        if (counts[i] != 0) {
            nnz++;
            idx = i < idx ? i : idx;
        }
    }
    result_fold(res, 0, nnz, idx);
}

// the (row, bin) of entry touch_idx; one thread.  offsets == nullptr: COO.
__global__ void k_locate(const uint32_t *__restrict__ ids, const u64 *__restrict__ offsets, uint32_t first, uint32_t nmetrics,
                         const int16_t *__restrict__ keys, ImportResult *res)
{
    if (res->bad || res->touch_idx == ~u64(0)) return;
    const u64 i = res->touch_idx;
    uint32_t row;
    if (!offsets) {
        row = ids[i];
    } else { // the last m with offsets[m] <= i (offsets are non-decreasing: checked)
        uint32_t lo = 0, hi = nmetrics - 1;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (offsets[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        row = first + lo;
    }
    res->touch_row = row;
    res->touch_bin = bin_of(keys[i]);
}

// ---- host side --------------------------------------------------------------------------------------
// Per-device state of this unit (device_ctx<ImportCtx>).  `mu` is held for the length of a call: the staging and the
// result word are one per device.
struct ImportCtx {
    std::mutex mu;
    int cus = 0;
    ImportResult *d_res = nullptr, *h_res = nullptr;
    char *h_stage = nullptr; // pinned; the kernels read it in place over PCIe, as the ingest lanes' buffers are read
    size_t stage_cells = 0;
};

struct Target : Opened {
    lh_snapshot *s = nullptr;
    ImportCtx *cx = nullptr;
    u64 *rows = nullptr;
    uint32_t nrows = 0;
};

// device, stream, spans.  Moves nothing yet.
int target_open(lh_snapshot *s, Target &t)
{
    t.s = s;
    return open_snapshot(s, t, t.cx);
}

// (cx->mu held)
int ctx_ready(ImportCtx *cx)
{
    if (!cx->cus) {
        int dev = 0, cus = 0;
        LH_BESIDE_CHK(hipGetDevice(&dev));
        LH_BESIDE_CHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        cx->cus = cus > 0 ? cus : 256;
    }
    if (!cx->d_res) LH_BESIDE_CHK(hipMalloc((void **)&cx->d_res, sizeof(ImportResult)));
    if (!cx->h_res) LH_BESIDE_CHK(hipHostMalloc((void **)&cx->h_res, sizeof(ImportResult), hipHostMallocDefault));
    return LH_OK;
}

// The uint64 view: a snapshot of 32-bit cells moves to its wide store here (LH_ENOMEM if that cannot be had).
int target_rows(Target &t)
{
    void *p = nullptr;
    uint32_t nrows = 0;
    const int rc = lh_snapshot_rows(t.s, &p, &nrows);
    if (rc) return rc;
    if (!p || ((uintptr_t)p & 7) || nrows != t.nrows) return LH_ESTATE;
    t.rows = static_cast<u64 *>(p);
    return LH_OK;
}

unsigned grid_for(const ImportCtx *cx, size_t items, size_t per_block)
{
    const size_t want = (items + per_block - 1) / per_block, cap = (size_t)cx->cus * 8;
    return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

int launch_add_coo(const Target &t, const uint32_t *ids, const int16_t *keys, const u64 *counts, size_t n)
{
    hipLaunchKernelGGL(k_add_coo, dim3(grid_for(t.cx, n, (IM_BLOCK / 64) * 64 * IM_UNROLL)), dim3(IM_BLOCK), 0, t.stream, ids,
                       keys, counts, n, t.rows, t.ranges, t.nrows, t.stride);
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

// Host entries -> the device, a staging chunk at a time.  `next` fills ids / keys / counts[0 .. cap) with the next
// entries whose count is not 0 and returns how many there were (0: done).
template <typename Next> int add_staged(Target &t, size_t nnz, Next next)
{
    ImportCtx *cx = t.cx;
    const size_t want = std::min(nnz, IM_STAGE_CELLS);
    const int grc = grow_pinned(cx->h_stage, cx->stage_cells, want, 4096, 14); // 14 bytes per entry
    if (grc) return grc;
    const size_t cap = cx->stage_cells;
    u64 *h_counts = reinterpret_cast<u64 *>(cx->h_stage);
    uint32_t *h_ids = reinterpret_cast<uint32_t *>(cx->h_stage + cap * 8);
    int16_t *h_keys = reinterpret_cast<int16_t *>(cx->h_stage + cap * 12);
    for (;;) {
        const size_t k = next(h_ids, h_keys, h_counts, cap);
        if (!k) break;
        int rc = launch_add_coo(t, h_ids, h_keys, h_counts, k);
        if (rc) return rc;
        LH_BESIDE_CHK(hipStreamSynchronize(t.stream)); // the staging is rewritten / the caller's arrays are the caller's again
    }
    return LH_OK;
}

// device forms: run the pre-pass that was enqueued, bring the result back
int result_fetch(const Target &t, ImportResult &out)
{
    ImportCtx *cx = t.cx;
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_res, cx->d_res, sizeof(ImportResult), hipMemcpyDeviceToHost, t.stream));
    LH_BESIDE_CHK(hipStreamSynchronize(t.stream));
    out = *cx->h_res;
    return LH_OK;
}

} // namespace

extern "C" {

int lh_snapshot_add_buckets(lh_snapshot *s, const uint32_t *ids, const int16_t *keys, const uint64_t *counts, size_t n)
{
    if (!s || (n && (!ids || !keys || !counts)) || misaligned(ids, 4) || misaligned(keys, 2) || misaligned(counts, 8))
        return LH_EINVAL;
    if (n == 0) return LH_OK;
    Target t;
    void *cells = nullptr;
    uint32_t cell_bytes = 0;
    int rc = lh_snapshot_cells(s, &cells, &t.nrows, &cell_bytes);
    if (rc) return rc;
    // all or nothing: the whole batch is checked before a cell moves
    size_t nnz = 0, touch = n;
    for (size_t i = 0; i < n; i++) {
        if (ids[i] >= t.nrows) return LH_ERANGE;
        if (counts[i] != 0) {
            if (!nnz) touch = i;
            nnz++;
        }
    }
    if (!nnz) return LH_OK;
    rc = target_open(s, t);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(t.cx->mu);
    rc = ctx_ready(t.cx);
    if (rc) return rc;
    rc = target_rows(t);
    if (rc) return rc;
    size_t at = 0;
    rc = add_staged(t, nnz, [&](uint32_t *h_ids, int16_t *h_keys, u64 *h_counts, size_t cap) {
        size_t k = 0;
        for (; at < n && k < cap; at++) {
            if (counts[at] == 0) continue;
            h_ids[k] = ids[at];
            h_keys[k] = keys[at];
            h_counts[k] = counts[at];
            k++;
        }
        return k;
    });
    if (rc) return rc;
    const uint32_t bin = (uint32_t)(uint16_t)keys[touch] ^ 0x8000u;
    return lh_snapshot_mark_dirty(s, ids[touch], 1, bin, bin);
}

int lh_snapshot_add_buckets_csr(lh_snapshot *s, uint32_t first, size_t nmetrics, const uint64_t *offsets,
                                const int16_t *keys, const uint64_t *counts)
{
    if (!s || (nmetrics && !offsets) || misaligned(offsets, 8) || misaligned(keys, 2) || misaligned(counts, 8)) return LH_EINVAL;
    Target t;
    void *cells = nullptr;
    uint32_t cell_bytes = 0;
    int rc = lh_snapshot_cells(s, &cells, &t.nrows, &cell_bytes);
    if (rc) return rc;
    if ((uint64_t)first + nmetrics > t.nrows) return LH_ERANGE;
    if (nmetrics == 0) return LH_OK;
    for (size_t m = 0; m < nmetrics; m++)
        if (offsets[m] > offsets[m + 1]) return LH_EINVAL;
    if (offsets[0] == offsets[nmetrics]) return LH_OK;
    if (!keys || !counts) return LH_EINVAL;
    size_t nnz = 0;
    uint64_t touch = 0;
    for (uint64_t i = offsets[0]; i < offsets[nmetrics]; i++) {
        if (counts[i] != 0) {
            if (!nnz) touch = i;
            nnz++;
        }
    }
    if (!nnz) return LH_OK;
    rc = target_open(s, t);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(t.cx->mu);
    rc = ctx_ready(t.cx);
    if (rc) return rc;
    rc = target_rows(t);
    if (rc) return rc;
    // the staged chunks carry their ids (a chunk may start in the middle of a row): the COO kernel adds them
    size_t m = 0;
    uint64_t at = offsets[0];
    uint32_t touch_row = first;
    bool have_row = false;
    rc = add_staged(t, nnz, [&](uint32_t *h_ids, int16_t *h_keys, u64 *h_counts, size_t cap) {
        size_t k = 0;
        while (m < nmetrics && k < cap) {
            if (at >= offsets[m + 1]) {
                m++;
                continue;
            }
            if (counts[at] != 0) {
                if (!have_row && at == touch) {
                    touch_row = first + (uint32_t)m;
                    have_row = true;
                }
                h_ids[k] = first + (uint32_t)m;
                h_keys[k] = keys[at];
                h_counts[k] = counts[at];
                k++;
            }
            at++;
        }
        return k;
    });
    if (rc) return rc;
    const uint32_t bin = (uint32_t)(uint16_t)keys[touch] ^ 0x8000u;
    return lh_snapshot_mark_dirty(s, touch_row, 1, bin, bin);
}

int lh_snapshot_add_buckets_device(lh_snapshot *s, const uint32_t *d_ids, const int16_t *d_keys, const uint64_t *d_counts,
                                   size_t n)
{
    if (!s || (n && (!d_ids || !d_keys || !d_counts)) || misaligned(d_ids, 4) || misaligned(d_keys, 2) ||
        misaligned(d_counts, 8))
        return LH_EINVAL;
    if (n == 0) return LH_OK;
    Target t;
    void *cells = nullptr;
    uint32_t cell_bytes = 0;
    int rc = lh_snapshot_cells(s, &cells, &t.nrows, &cell_bytes);
    if (rc) return rc;
    rc = target_open(s, t);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(t.cx->mu);
    rc = ctx_ready(t.cx);
    if (rc) return rc;
    ImportResult *res = t.cx->d_res;
    hipLaunchKernelGGL(k_result_init, dim3(1), dim3(1), 0, t.stream, res);
    hipLaunchKernelGGL(k_check_coo, dim3(grid_for(t.cx, n, IM_BLOCK * 8)), dim3(IM_BLOCK), 0, t.stream, d_ids,
                       reinterpret_cast<const u64 *>(d_counts), n, t.nrows, res);
    hipLaunchKernelGGL(k_locate, dim3(1), dim3(1), 0, t.stream, d_ids, static_cast<const u64 *>(nullptr), 0u, 0u, d_keys, res);
    LH_BESIDE_CHK(hipGetLastError());
    ImportResult r;
    rc = result_fetch(t, r);
    if (rc) return rc;
    if (r.bad) return LH_ERANGE;
    if (!r.nnz) return LH_OK;
    rc = target_rows(t);
    if (rc) return rc;
    rc = launch_add_coo(t, d_ids, d_keys, reinterpret_cast<const u64 *>(d_counts), n);
    if (rc) return rc;
    return lh_snapshot_mark_dirty(s, r.touch_row, 1, r.touch_bin, r.touch_bin);
}

int lh_snapshot_add_buckets_csr_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const uint64_t *d_offsets,
                                       const int16_t *d_keys, const uint64_t *d_counts)
{
    if (!s || (nmetrics && !d_offsets) || misaligned(d_offsets, 8) || misaligned(d_keys, 2) || misaligned(d_counts, 8))
        return LH_EINVAL;
    Target t;
    void *cells = nullptr;
    uint32_t cell_bytes = 0;
    int rc = lh_snapshot_cells(s, &cells, &t.nrows, &cell_bytes);
    if (rc) return rc;
    if ((uint64_t)first + nmetrics > t.nrows) return LH_ERANGE;
    if (nmetrics == 0) return LH_OK;
    rc = target_open(s, t);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(t.cx->mu);
    rc = ctx_ready(t.cx);
    if (rc) return rc;
    ImportResult *res = t.cx->d_res;
    // (an all-empty CSR may come without cell arrays, as the host form's may: the pre-pass reports anything else as bad)
    const u64 *offs = reinterpret_cast<const u64 *>(d_offsets);
    const u64 *cnt = d_keys && d_counts ? reinterpret_cast<const u64 *>(d_counts) : nullptr;
    const uint32_t M = (uint32_t)nmetrics;
    hipLaunchKernelGGL(k_result_init, dim3(1), dim3(1), 0, t.stream, res);
    hipLaunchKernelGGL(k_check_offsets, dim3(grid_for(t.cx, nmetrics, IM_BLOCK)), dim3(IM_BLOCK), 0, t.stream, offs, M, res);
    hipLaunchKernelGGL(k_check_csr_counts, dim3((unsigned)t.cx->cus * 8), dim3(IM_BLOCK), 0, t.stream, offs, M, cnt, res);
    hipLaunchKernelGGL(k_locate, dim3(1), dim3(1), 0, t.stream, static_cast<const uint32_t *>(nullptr), offs, first, M, d_keys, res);
    LH_BESIDE_CHK(hipGetLastError());
    ImportResult r;
    rc = result_fetch(t, r);
    if (rc) return rc;
    if (r.bad) return LH_EINVAL;
    if (!r.nnz) return LH_OK;
    rc = target_rows(t);
    if (rc) return rc;
    hipLaunchKernelGGL(k_add_csr, dim3(grid_for(t.cx, nmetrics, IM_BLOCK / 64)), dim3(IM_BLOCK), 0, t.stream, offs, d_keys, cnt,
                       first, M, t.rows, t.ranges, t.stride);
    LH_BESIDE_CHK(hipGetLastError());
    return lh_snapshot_mark_dirty(s, r.touch_row, 1, r.touch_bin, r.touch_bin);
}

} // extern "C"
