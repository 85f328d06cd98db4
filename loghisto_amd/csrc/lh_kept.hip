// lh_kept.hip -- lh_keep / lh_kept_* (include/loghisto_gpu.h): an interval's occupied cells kept in COMPACT form in device
// memory after its snapshot is gone, and the snapshot readers' outputs over a list of up to 64 such copies -- lh_across' first,
// then lh_compare's, lh_count_le's, lh_spread's, lh_top's and lh_movers' further down: p99 over the last minute of 1 s
// intervals while no dense epoch buffer of them is alive.  A dense buffer is 4 GiB at 8 192 names; the occupied cells
// of an interval are a few hundred (int16 key, uint64 count) pairs per name (RawMetricSet.Histograms, metrics.go:54-60).
// With c_i[b] the cells of a name in kept[i]:
//   C[b] = sum over i of c_i[b], in 64 bits -- the cell atomic.AddUint64 would have left had the samples arrived in one
//          interval (metrics.go:278)
//   count, sum, nbuckets, the percentile buckets: lh_across' definitions word for word (metrics.go:336-418), i.e. what
//   lh_extract_rows returns for a snapshot that holds C.  present_bits: bit i set iff kept[i] holds a cell of the name.
// Nothing is summed across names, no cell of a snapshot is written and no new statistic is defined.
//
// Built BESIDE the engine, on its public C ABI only (lh_beside.h, lh_wave.h), like lh_across.hip, whose out record, argument
// check and find_in_step it shares (lh_pct.h).
//
// THE HANDLE is one allocation of exactly  offsets[nrows + 1] | row_count[nrows] | counts[cells] | keys[cells]  (uint64,
// uint64, uint64, int16): lh_buckets_all's CSR arrays of the same rows -- keys ascending by bin -- which
// lh_snapshot_add_buckets_csr_device takes as they are, plus each row's sum of cells.  lh_keep makes it on the snapshot's
// stream in three kernels: k_keep_count (a wave per row: the row's occupied cells and their sum), k_keep_scan (one
// workgroup: the exclusive prefix of the former, the two grand totals), then -- the totals brought back, the allocation
// made -- k_keep_fill (a wave per row again: the cells to their places).  It returns when the copy is complete; the handle
// then depends on neither the snapshot nor the engine, and never changes.
//
// THE READER, k_kept_across, in two shapes switched by the rows of a call like the other readers:
//   NW = 1    one WAVE per row, four rows per workgroup, a tile of its own each
//   NW = 16   one WORKGROUP of 16 waves per row: the waves share the scatter (wave w takes handles w, w + 16, ...), wave 0
//             walks the tile.  Same walk, same order: the two shapes agree bit for bit, sum included.
// Lane i opens handle i: its row's segment [begin, end) of the CSR arrays, its row_count -- whose sum over the lanes is the
// row's total, so every threshold (lh_wave.h's pct_threshold) is known BEFORE any cell is read -- and its first and last
// bin.  The union span of the segments is then covered by TILES of KEPT_TILE bins of uint64 in LDS (8 KiB a tile; 32 KiB
// static per workgroup in the wave shape).  Per tile: the start t0 is the least bin not yet taken, aligned down to 4 (empty
// stretches between tiles cost nothing); every segment's entries inside [t0, t0 + KEPT_TILE) are one contiguous run --
// found by a binary search per lane from the second tile on -- and are added into the tile with 64-bit LDS adds; then the
// tile is walked in ascending bins, 256 per step, with lh_across' step: running prefix, nbuckets, the percentile bins and
// the sum of D[b] * float64(C[b]) (per lane over the steps in ascending order, one DPP tree over the lanes at the end).
// The walk puts zeros back where it read, so the next tile starts clean.  Integer cell sums do not depend on the order of
// the adds and the float walk is fixed: no result depends on timing.
//
// THE MERGE, lh_kept_merge: up to 64 handles rolled up into ONE new handle of rows [first, first + nmetrics) -- 60 x 1 s into a
// minute, 60 minutes into an hour -- that holds exactly what lh_keep would return for a snapshot whose cells are C: per row
// the union of the handles' bins ascending by bin, each with its 64-bit wrapping sum, a sum that wrapped to 0 not listed (not
// an occupied cell); row_count[m] the wrapping sum of the row's cells, which is the wrapping sum of the handles' own
// row_count entries, so no cell is read for it.  lh_keep's three steps with the reader's row walk in the outer two:
// k_merge_count, k_keep_scan as it is, the totals brought back and the allocation made, k_merge_fill (each step's non-zero
// cells to off[m] plus a running position, from a wave scan of occupied4 as in k_keep_fill; not launched without a cell).
// The open and the turns over the tiles are ONE device function (Row, turns) that takes the walk's step: the reader's is
// lh_across', the count pass's counts the non-zero cells, the fill pass's places them.  Both passes have the reader's two
// shapes, switched by the rows of the call through the same switch, and give identical bytes.  Synchronous like lh_keep, on
// the caller's stream, under the unit's mutex from the first look at a handle to the end (no lh_kept_release frees an input
// under it); it only reads its inputs, so it records no event on them, and the new handle depends on none of them.
//
// THE GATHER, lh_kept_gather*: the merge with the row of handle i chosen PER HANDLE by a map (src[i * n + m], LH_KEPT_NO_ROW: none) --
// handles of other processes, of the time before a restart, of ranks that own other name blocks, whose row numbers mean other names.
// The merge's two passes take the row of lane i through a row-source type (BlockRows / MappedRows: one device body each for both
// entry points); a row outside handle i's block empties lane i's segment alone (Row::open_own), where the readers' settle empties
// the entry.  One handle is a permutation of rows and goes without the tile: lengths, then keys and counts verbatim (k_gather1_*).
// The host form stages the map as an id list is staged; synchronous, under the mutex, no hold: lh_kept_merge's host side (born_of).
//
// THE GROUP, lh_kept_group*: the merge with MANY rows of every handle feeding one output row -- a CSR of groups over absolute rows
// (goff, members), the roll-up of a service over its endpoints.  A third row source of the same two bodies (GroupRows): a row's
// sources are the pairs (handle, member); at most 64 sit one a lane and take the gather's open and turns, more go through the same
// tile in chunks of 64 (chunk_turns).  The device form clamps goff to the members in both passes; the host form holds goff to a CSR
// and the members to every handle's block, and stages both through the id list's blocks.  Host side: lh_kept_merge's (born_of).
//
// THE SLIDE, lh_kept_slide: new window = old window + newest interval - oldest interval as a NEW handle, so that a rolling minute
// emitted every second reads one merged handle and two small ones a tick where lh_kept_merge reads all sixty.  A[b] / S[b] = the
// wrapping sums over the `add` / `sub` lists (the merge's C[b], once per side), the handle holds A[b] - S[b]: cells are unsigned
// integer counts, so the result is bit for bit lh_kept_merge's of the window's handles and nothing drifts however long it runs.  The
// merge's three steps with the compare's TWO tiles a row (turns_of<NW, 2, KEPT_COMPARE_TILE>, the lists as one, add first):
// k_slide_count / k_slide_fill take the difference in the step, never in LDS.  A cell with S[b] > A[b] refuses the call: the count
// pass folds row << 16 | bin into one word behind the two totals with a 64-bit atomic min (k_kept_check's pattern), make() brings
// it back with them and returns before anything is allocated; the fill pass is not launched.
//
// THE COMPARE, lh_kept_compare*: lh_compare's outputs (lh_compare.hip's header has X, ks, w1 and shift) for a[j] = the sum over
// the `base` list of the name's cell j and b[j] = the same over the `cur` list -- a kept baseline against a kept interval
// with no dense buffer alive.  Up to 64 handles in the two lists together, which travel as ONE list (base first) with the
// number of base handles beside it: lane i opens handle i as in the reader, na / nb are the wrapping sums of row_count over
// the lanes of each side, so the scale (lh_pair.h's make_scale) is known before a cell is read and the row is walked ONCE,
// where lh_compare walks it twice.  k_kept_compare has the reader's two shapes behind the same switch and takes the same
// turns with TWO tiles a row, one per side (KEPT_COMPARE_TILE bins each): handle i scatters into its side's tile, the walk
// hands the step both sides' four cells and k_compare_wave's walk 2 follows (two wave scans, take4).  The tiles cover occupied
// stretches only, and X is constant where no cell is: for the g bins between the end of the last step walked and the start
// of the next tile's first, lane 0 adds g x the term once, just before that step (one product, one add).  Every bin from
// the lowest to the highest occupied one thereby counts exactly once; bins beyond the last occupied one have A = na and
// B = nb and add an exact 0.  Wave 0 alone walks in both shapes, so they agree bit for bit, sums included.  Device forms put
// ALL handles of both lists under one hold.
//
// THE TWO OTHER PER-NAME READERS, lh_kept_count_le* and lh_kept_spread*: lh_count_le's and lh_spread's outputs, word for word, for
// a snapshot whose cells are C -- the last hour's SLO ratio and `le` buckets, the last minute's std and trimmed sums, with no
// dense buffer alive.  Both take the reader's Row and turns as they are, in its two shapes behind the same switch.
//   k_kept_count_le  ONE turn with k_count_le_wave's step: lane j owns bound j (E = le_take, lh_wave.h), and the prefix is
//                    fetched from the lane that owns the bound's bin only in a step some pending bound falls into.  `base` jumps
//                    between tiles: a pending bound whose E is at or below the step's base lies before the first tile or in a
//                    stretch no tile covers and takes the running carry; one beyond the last step takes everything.  total is
//                    the wrapping sum of the row_count entries.  The bounds are one row shared by all names and travel by value
//                    beside the list (512 + 1 544 bytes); a row per name (LH_LE_PER_METRIC) would need a guarded device block
//                    -- see the next paragraph -- and is refused.  Integer sums only: the shapes agree exactly.
//   k_kept_spread    TWO turns over the same row (the opened Row is kept and taken again; the tile is zero on return).  The
//                    count comes from row_count, so the thresholds are known before a cell is read.  Walk 1: sum.  Walk 2:
//                    k_spread_wave's -- m2 about sum / float64(count) and, in the steps a threshold falls into, key, count_le
//                    and sum_le (central4 and sums_in_step, which lh_pct.h now holds for both units), with the unit's d_table.
//                    Wave 0 alone walks in both shapes, per lane over the steps in ascending order, then one DPP tree over the
//                    lanes: the two shapes agree BIT FOR BIT, floating-point outputs included (lh_spread's own two shapes
//                    associate differently and agree to rounding only).
//
// PER WINDOW OF THE LIST, lh_kept_series* and lh_kept_heat*: lh_kept_across*' and lh_kept_count_le*'s outputs for up to LH_MAX_WINDOWS
// contiguous slices [lo, hi) of the list in ONE launch -- each second's p99 of the last minute, a heat map of `le` bands per second --
// where a call per window pays the mutex, a launch, an id copy and a hold each time.  The bodies of k_kept_across and k_kept_count_le
// are device functions that take the slice (across_entry, count_le_entry: lane i opens handle lo + i, the turns run over hi - lo
// handles); those kernels hand them the whole list, k_kept_series / k_kept_heat one window per blockIdx.y.  Window-major outputs,
// entry (w, m) at w * n + m: window w's block is byte for byte the reader's output for (kept + lo, hi - lo), sum included, in both
// shapes -- but for present_bits, the ballot shifted left by lo (bit i: kept[i] of the WHOLE list).  The windows travel by value
// (KeptWindows, 256 bytes).  The shape switch takes the ENTRIES of a call, windows x rows.
// lh_kept_spread_series* and lh_kept_drift* do the same for lh_kept_spread* and lh_kept_compare*: the bodies of k_kept_spread and
// k_kept_compare are spread_entry (a slice, both turns over its handles) and compare_entry (a PAIR of slices (base, cur) of the one
// list: lane i < base.len opens handle base.lo + i, lane base.len + j handle cur.lo + j -- the parent's lanes for "base's handles,
// then cur's", so the slices may overlap, coincide and stand in either order); the parents hand them the whole list, k_kept_spread_series
// / k_kept_drift one window per blockIdx.y (KeptDriftWindows: four bytes a window, 512 bytes by value; at most LH_MAX_KEPT handles in
// a window's two slices, which the host checks).  Window w's block is byte for byte the parent's output for the slice(s), floats
// included, in both shapes: the same LDS, no scratch, wave 0 alone walking.  Top and movers per window stay out (a select per window).
// A ROW OF BOUNDS PER ENTRY, lh_kept_slo* and lh_kept_burn*: the per-name thresholds k_kept_count_le refuses, as NEW entry points whose
// rows are handled the way the id lists are -- a host form stages its host array on the call's stream (lh_beside.h's stage_doubles
// beside stage_ids: a pinned block and a device block of KeptCtx) and waits before it returns, a device form reads the caller's own
// device array -- so no block of the unit's outlives a call and nothing needs a guard.  count_le_entry takes its bounds through a
// source type (SharedBounds: the by-value row of the two kernels above; RowBounds: lane j loads bounds[m * nb + j], one coalesced
// load a wave), and its walk is count_le_walk, which hands lane j its count and every lane the total.  k_kept_slo is k_kept_heat
// with RowBounds: entry (w, m) is byte for byte what lh_kept_heat_ids* writes for window w and the one row of entry m.  A device
// array is any bytes: the lanes never look at each other's bound (a decreasing row is answered bound by bound), le_take gives a
// NaN no bin.  lh_kept_burn*: one bound and one budget an entry, one rate a window (by value, KeptRates); k_kept_burn_score decides
// fires = total != 0 && (double)(total - cum) > (rate[w] * budget[m]) * (double)total in lane 0 of the wave that owns entry (w, m)
// and adds 1 to miss[m] when it does NOT (n words from SelectState's guarded block, zeroed on the call's stream: an integer sum,
// whatever the order); k_kept_burn_emit, ONE workgroup in k_keep_scan's pattern, walks m ascending, writes the first k records
// {entry, row} of the entries with miss == 0 and the count of all of them.  No result depends on timing or on the kernel shape.
// A FAMILY'S TWO FORMS ARE ONE PATH.  On the device each of the eight kernels is its `__shared__` tile, the start every kernel of
// a call's entries has (Seat::take: the bound check, the tile clear; Seat::row: ids[m] or first + m) and the family's entry function,
// handed the whole list or the window of blockIdx.y (KeptWindows::slice, KeptDriftWindows::slices, window_entry); the two score
// kernels start the same way.  On the host a family has ONE front end and ONE enqueue (kept_across, kept_count_le, kept_spread,
// kept_compare and their enqueue_*), which take the windows as something optional (Windows; WHOLE_LIST for the parents, and
// lh_kept_compare* joins its two lists into lh_kept_drift*'s one): the forms differ in the windows' term of the first LH_EINVAL test,
// in the launch, in the entries a host form brings back and in the order of the two handle checks, which run() makes from an
// explicit argument.  The extern "C" wrappers build the output structs with kept_out / compare_out / spread_out.
//
// THE TWO SELECTING READERS, lh_kept_top* and lh_kept_movers*: lh_top's and lh_movers' selections -- the k names of a range that lead,
// or that moved most between two lists -- for a snapshot whose cells are C, so that k entries travel and no dense buffer is filled.
// Two score kernels in front of lh_select.h's k_select, whose records (TopRecords, MoversRecords) and Emit functors that header
// now holds for lh_top.hip / lh_movers.hip and this unit alike.  Every ranked value is one the per-name readers above return:
//   k_kept_top_score     the reader's Row and ONE turn: count from row_count (a candidate iff != 0), so the percentile's threshold and
//                        the bound's take are known before a cell is read; sum by k_kept_across' step in its order (BIT-EQUAL to
//                        its sum); BY_PERCENTILE: lane 0 owns the one threshold of Open, k_kept_across' search and bin;
//                        BY_COUNT_ABOVE: the cells at or beyond le_take(arg), bins being absolute (count minus k_kept_count_le's cum).
//   k_kept_movers_score  k_kept_compare's open, totals, turns, take4, gap product and wave_best through ONE device function
//                        (compare_turns): ks, w1 and shift are BIT-EQUAL to lh_kept_compare's.  BY_PERCENTILE: one joint turn that
//                        carries both prefixes and finds each side's first bin reaching its own threshold; the turns are not left
//                        early (the tiles come back zeroed), the step does nothing once both are found.
// Both in the reader's two shapes behind the same switch, wave 0 alone walking: identical bytes.  KeptCtx has ONE SelectState (calls
// take turns under its mutex), its records block always sized for the movers' five fields; device forms put ALL listed handles
// under one hold, and the records block is guarded by SelectState's event.  Out of scope: a BY_COUNT pass that skips the cell walk,
// a multi-workgroup select, _ids forms, more than 64 handles a call (lh_kept_merge first).
// PER WINDOW, lh_kept_top_series* and lh_kept_movers_series*, which lift top and movers per window from the lists above: the select
// per window they waited for is ONE SELECT WORKGROUP PER WINDOW.  The bodies of the two score kernels are top_score_entry (a slice, as
// across_entry) and movers_score_entry (a pair of slices, compare_entry's lanes) and write record e; the parents hand them the whole
// list and e = m, k_kept_top_score_series / k_kept_movers_score_series one window per blockIdx.y (KeptWindows / KeptDriftWindows) and
// e = w * npad + m, npad the rows padded to SEL_PER as select_records pads them.  lh_select.h's k_select_windows then runs k_select's
// body with workgroup w over key + w * npad, cand + w * npad, its Emit advanced by w * npad records and w * k entries, the count to
// n_out[w]: no atomic and no order between windows, k_select's LDS a workgroup.  Window w's block is byte for byte the parent's output
// for the slice(s), sum and score included, in both shapes.  nwin * npad records of 40 bytes would be 320 MiB at 128 windows x 65 536
// names, so the host runs the two passes over CHUNKS of consecutive windows on the one stream -- the largest window count whose
// records fit KEPT_SELECT_BYTES (64 MiB; lh_tool_kept_select_bytes), never less than one: up to 8 192 names one chunk at any nwin,
// 25 windows a chunk at 65 536 -- each chunk's kernels given the windows from its first on and out / n_out advanced; stream order
// protects the reused block between chunks and the guard's event is recorded behind the last select.  Host forms bring nwin * k
// entries and nwin counts back in ONE copy (4 MiB + 512 B at most) and hand n_out[w] entries a window on.  Still out of scope:
// sharing cell reads between overlapping windows, a select that spreads ONE window over several workgroups, _ids forms, more than
// 64 handles a call.
//
// SAVE AND LOAD, lh_kept_save* / lh_kept_load*: a handle's single allocation verbatim behind a 64-byte header (loghisto_gpu.h has the
// format), to host or device memory and back into a NEW handle on any device, with no engine anywhere.  A save is two copies and a
// wait.  A load copies the block into its exact allocation and then PROVES there, on the call's stream, what lh_keep guarantees and
// every kernel of this unit trusts -- offsets monotone from 0 to `cells`, at most LH_NKEYS cells a row, bins strictly ascending within
// a row, no zero cell, row_count the wrapping sum of the row, samples the wrapping sum of row_count -- before the handle exists:
// k_kept_check (a wave per row, safe on arbitrary bytes) and k_kept_check_samples (one workgroup) fold the first violation, by row,
// index and cause, into one uint64 with an atomic min, which comes back in one 8-byte copy.  The header's own causes are decided
// on the host.  lh_kept_values hands out the unit's value table, for a process that has no engine to ask.
//
// THE COMPACT BLOB, lh_kept_encode* / lh_kept_decode*: the same handle at a few bytes a cell instead of ten, for files, wires and PCIe
// -- per row the counts at the narrowest width that holds the largest and the bins as byte deltas (loghisto_gpu.h has the format;
// one handle has ONE encoding).  Encode: k_enc_size (a wave per row: desc[m] and the record's length), k_keep_scan as it is,
// the total brought back, k_enc_fill (a wave per row writes every byte of its record).  Decode proves untrusted bytes into an
// ordinary handle in two stages: k_dec_dir reads the directory ALONE, two k_keep_scan give the cells' and the records' offsets and
// the totals the header must state -- a refusal here is final --; then k_dec_fill, a wave per row inside ranges that are proven by
// then, writes the handle's arrays and folds the first violation as k_kept_check does, and k_kept_check_samples closes.
//
// THE LIST OF HANDLES TRAVELS BY VALUE (KeptList: 64 records of 24 bytes -- address of the allocation, cells, first, nrows;
// 1.5 KiB of the 4 KiB a kernel's arguments may take).  A block in device memory would have to be guarded across streams:
// a device-form call returns while its kernel is still to read the block, so the next call, on whatever stream, would wait
// on the HOST for the previous one before rewriting it, or the unit would keep a pool of blocks.  By value there is nothing
// to guard and two device-form calls on two streams never meet in a block of the unit's.
//
// WHAT IS GUARDED IS EACH HANDLE'S ALLOCATION, against lh_kept_release while enqueued work still reads it.  A device-form
// call records ONE event behind its kernel (CallEvent, from a pool of the device's context), and every handle of its list
// then points to that event and counts as a user of it.  A handle may be read on any number of streams, and an event holds
// one record only; so before the record the call's stream is made to wait (on the device: hipStreamWaitEvent) for the event
// each of its handles pointed to until now -- once per distinct event, which in the steady state of one list read again and
// again is one wait.  The new event is thereby behind EVERY reader of the handle so far, on whichever stream, and
// lh_kept_release has one event to wait for: the one the handle points to.  An event that no handle points to any more goes
// back to the pool (the waits on it that are already enqueued keep the record they saw).  lh_kept_hold puts work of the
// caller's own that reads lh_kept_arrays' pointers under the same guard.  Host forms return with their work complete.
// Read-only: no store goes to a handle's arrays after lh_keep, to a cell, a span or any engine.
#include "../../include/loghisto_gpu.h"
#include "../../include/loghisto_gpu_tuning.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_pair.h"
#include "lh_pct.h"
#include "lh_select.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <type_traits>

namespace {

using namespace lh; // (lh_wave.h, lh_pct.h)
using namespace lh::beside;

constexpr uint32_t KEPT_WAVE_FROM_DEFAULT = 1024; // lh_spread's default; profiles/kept.txt has both shapes
constexpr uint32_t KEPT_TILE = 1024;              // bins of a tile: a lognormal name's union span fits one
static_assert(KEPT_TILE % STEP == 0 && ROW_WAVES * KEPT_TILE * sizeof(u64) <= 65536, "whole steps; 64 KiB static LDS at most");
static_assert(LH_MAX_KEPT == 64, "a handle per lane, their set in one 64-bit mask");
// bins of each of the compare's two tiles (one per side): half the reader's width, 32 KiB static in the wave shape.  At the
// reader's width that shape holds the 64 KiB a kernel may have static and measures a quarter slower at 65 536 names, while the
// workgroup shape (calls of fewer than 1 024 rows) measures up to a third faster: profiles/kept_compare.txt has both widths.
#ifndef LH_KEPT_COMPARE_TILE
#define LH_KEPT_COMPARE_TILE 512
#endif
constexpr uint32_t KEPT_COMPARE_TILE = LH_KEPT_COMPARE_TILE;
static_assert(KEPT_COMPARE_TILE % STEP == 0 && KEPT_COMPARE_TILE >= STEP && ROW_WAVES * 2 * KEPT_COMPARE_TILE * sizeof(u64) <= 65536,
              "whole steps; 64 KiB static LDS at most");

// one handle as the kernel sees it.  offsets at `block`, row_count = offsets + nrows + 1, counts = row_count + nrows, keys
// behind counts.
struct KeptRec {
    u64 block; // its address: an integer, see gu64
    u64 cells;
    uint32_t first, nrows;
};
struct KeptList { // by value in the kernel arguments (1 544 bytes)
    KeptRec h[LH_MAX_KEPT];
    uint32_t n;
};

typedef ListOut<u64> KeptOut; // present_bits: a bit per handle

// A handle's arrays through pointers that say GLOBAL: their addresses travel as integers -- in the list, then from lane to
// lane -- and a load through a generic pointer made of one would be a flat one, which every LDS wait then waits for too
// (lh_across.hip's gcells), here in the loop of the tile's LDS adds.
typedef const __attribute__((address_space(1))) u64 *gu64;
typedef const __attribute__((address_space(1))) int16_t *gkeys;
__device__ __forceinline__ uint32_t bin_of(int16_t key) { return key_to_bin((int)key); }

// ---- lh_keep ----------------------------------------------------------------------------------------------------------
// a wave per row of the block: nnz[m + 1] = the row's occupied cells, row_count[m] = their sum (wrapping)
template <typename CELL>
__global__ __launch_bounds__(ROW_BLOCK) void k_keep_count(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                         size_t stride, uint32_t nrows, u64 *__restrict__ nnz,
                                                         u64 *__restrict__ row_count)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    const Span sp = own_span(ranges, m);
    u64 cnt = 0;
    uint32_t occ = 0;
    if (sp.any()) {
        const CELL *row = cells + (size_t)m * stride;
        for (uint32_t base = sp.base0(); base <= sp.hi; base += STEP) {
            u64 c[4];
            load4_cells(row, base + 4 * lane, sp.hi, c);
            cnt += sum4(c);
            occ += occupied4(c);
        }
    }
    cnt = wave_scan_incl_u64(cnt);
    occ = wave_scan_incl_u32(occ);
    if (lane == 63) {
        nnz[(size_t)m + 1] = occ;
        row_count[m] = cnt;
    }
}

// one workgroup: off[1 .. nrows] becomes its own inclusive prefix (off[0] = 0: the CSR offsets), totals = {cells, samples}
__global__ __launch_bounds__(WG) void k_keep_scan(u64 *__restrict__ off, const u64 *__restrict__ row_count, uint32_t nrows,
                                                  u64 *__restrict__ totals)
{
    __shared__ u64 s_w[WG_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0, samples = 0;
    for (u64 base = 0; base < nrows; base += WG) { // uniform
        const u64 i = base + threadIdx.x;
        const bool in = i < nrows;
        const u64 v = in ? off[i + 1] : 0;
        samples += in ? row_count[i] : 0;
        const u64 inc = wave_scan_incl_u64(v);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        u64 below = 0, all = 0;
        for (uint32_t k = 0; k < (uint32_t)WG_WAVES; k++) {
            const u64 t = s_w[k];
            below += k < wave ? t : 0;
            all += t;
        }
        if (in) off[i + 1] = carry + below + inc;
        carry += all;
        __syncthreads();
    }
    samples = wave_scan_incl_u64(samples);
    if (lane == 63) s_w[wave] = samples;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 all = 0;
        for (uint32_t k = 0; k < (uint32_t)WG_WAVES; k++) all += s_w[k];
        off[0] = 0;
        totals[0] = carry;
        totals[1] = all;
    }
}

// a wave per row: the row's occupied cells to keys / counts[off[m] .. off[m + 1]), ascending by bin.  (Nothing is stored at
// or beyond off[m + 1], whatever the cells hold now.)
template <typename CELL>
__global__ __launch_bounds__(ROW_BLOCK) void k_keep_fill(const CELL *__restrict__ cells, const uint32_t *__restrict__ ranges,
                                                        size_t stride, uint32_t nrows, const u64 *__restrict__ off,
                                                        int16_t *__restrict__ keys, u64 *__restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    const Span sp = own_span(ranges, m);
    if (!sp.any()) return;
    u64 at = off[m];
    const u64 lim = off[(size_t)m + 1];
    const CELL *row = cells + (size_t)m * stride;
    for (uint32_t base = sp.base0(); base <= sp.hi && at < lim; base += STEP) {
        u64 c[4];
        const uint32_t b0 = base + 4 * lane;
        load4_cells(row, b0, sp.hi, c);
        const uint32_t n = occupied4(c), inc = wave_scan_incl_u32(n);
        u64 pos = at + (inc - n);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (c[k] && pos < lim) {
                keys[pos] = (int16_t)bin_to_key(b0 + k);
                counts[pos] = c[k];
                pos++;
            }
        at += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
}

// ---- the reader ---------------------------------------------------------------------------------------------------------
// the tile's adds are complete and visible before anything behind this reads it (and the other way round)
template <int NW> __device__ __forceinline__ void tile_sync()
{
    if constexpr (NW == 1) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // (a wave's LDS operations execute in order)
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// ---- a row of a list of handles: the open and the turns, once for the reader and for lh_kept_merge's two passes ----------
// Lane i's view of handle i's segment of the row: the cursor and the end in its CSR arrays, the addresses of those (as
// integers: they travel from lane to lane), its row_count entry, the bin at the cursor.  hi: the last bin of the union.
struct Row {
    u64 cur = 0, end = 0, rc = 0, keys = 0, counts = 0;
    uint32_t next = NO_BIN, hi = 0;
    bool outside = false;
    // (lane < the list's n)  row r of handle h; a row outside its block marks the whole entry empty (settle)
    __device__ __forceinline__ void open(const KeptRec h, uint32_t r)
    {
        const uint32_t lr = r - h.first;
        if (r < h.first || lr >= h.nrows) {
            outside = true;
        } else {
            const gu64 offsets = (gu64)h.block, row_count = offsets + (size_t)h.nrows + 1;
            cur = offsets[lr];
            end = offsets[(size_t)lr + 1];
            rc = row_count[lr];
            counts = h.block + 8 * (2 * (u64)h.nrows + 1);
            keys = counts + 8 * h.cells;
            if (end > h.cells || cur > end) cur = end = 0; // (never: lh_keep made them)
        }
    }
    // (lane < the list's n)  lh_kept_gather's: row r of handle h for THIS handle alone.  LH_KEPT_NO_ROW, or a row outside h's block,
    // leaves the lane's segment empty (rc 0) and nothing is read for it; the other lanes' segments stay what they are.
    __device__ __forceinline__ void open_own(const KeptRec h, uint32_t r)
    {
        if (r != LH_KEPT_NO_ROW && r >= h.first && r - h.first < h.nrows) open(h, r);
    }
    // (the whole wave)  A row outside the block of ANY handle is empty in all; the first and the last bin of each segment
    __device__ __forceinline__ void settle()
    {
        if (__builtin_amdgcn_ballot_w64(outside)) { // wave-uniform
            cur = end = 0;
            rc = 0;
        }
        uint32_t last = 0;
        if (end > cur) {
            next = bin_of(((gkeys)keys)[cur]);
            last = bin_of(((gkeys)keys)[end - 1]);
        }
        hi = wave_max_u32(last);
    }
};

// The turns over a row's tiles (the tile is zero on entry, and again on return): the start of each, the scatter of every
// handle's run inside it, then -- wave 0 of the NW that share the tile -- the ascending walk, 256 bins a step, which hands
// step(C, base) the lane's four summed cells of bins base + 4 * lane .. + 3 and puts zeros back.  Every wave of a workgroup
// takes the same turns: the state below is the same in all.  w: which of the NW scatterers this wave is; n: the handles.
// With SIDES == 2 (the compare) the row has two tiles of TILE bins, the second right behind the first: handles 0 .. n0 - 1
// add into the first and the others into the second, the walk hands step(A, B, base) the lane's four cells of each and
// puts zeros back in both.  Between two tiles no step is taken: `base` jumps.
template <int NW, int SIDES, uint32_t TILE, class Step>
__device__ __forceinline__ void turns_of(Row &row, uint32_t n, uint32_t n0, u64 *tile, uint32_t lane, uint32_t w, Step step)
{
    tile_sync<NW>(); // the tile is zero
    for (uint32_t from = 0;;) {
        if (from) { // the first entry at or above `from`
            u64 a = row.cur, b = row.end;
            while (a < b) {
                const u64 mid = a + (b - a) / 2;
                if (bin_of(((gkeys)row.keys)[mid]) < from) a = mid + 1;
                else b = mid;
            }
            row.cur = a;
            row.next = row.cur < row.end ? bin_of(((gkeys)row.keys)[row.cur]) : NO_BIN;
        }
        const uint32_t least = ~wave_max_u32(~row.next);
        if (least == NO_BIN) break;
        const uint32_t t0 = least & ~3u, tend = t0 + TILE;
        // ---- scatter: handle i's run inside the tile, 64 entries a turn
        for (uint32_t i = w; i < n; i += NW) { // wave-uniform
            u64 c = readlane_u64(row.cur, i);
            const u64 e = readlane_u64(row.end, i);
            const gkeys kp = (gkeys)readlane_u64(row.keys, i);
            const gu64 cp = (gu64)readlane_u64(row.counts, i);
            u64 *to = tile;
            if constexpr (SIDES == 2) to = i < n0 ? tile : tile + TILE;
            while (c < e) {
                const u64 idx = c + lane;
                bool in = false;
                if (idx < e) {
                    const uint32_t at = bin_of(kp[idx]) - t0;
                    if (at < TILE) {
                        in = true;
                        atomicAdd(&to[at], cp[idx]);
                    }
                }
                const uint32_t took = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
                c += took;
                if (took < 64) break;
            }
        }
        tile_sync<NW>();
        // ---- walk, and zeros back
        if (w == 0) {
            const uint32_t wend = min(tend - 1, row.hi);
            for (uint32_t base = t0; base <= wend; base += STEP) {
                const uint32_t at = base + 4 * lane - t0;
                u64 C[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    C[k] = tile[at + k];
                    tile[at + k] = 0;
                }
                if constexpr (SIDES == 2) {
                    u64 B[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        B[k] = tile[TILE + at + k];
                        tile[TILE + at + k] = 0;
                    }
                    step(C, B, base);
                } else {
                    step(C, base);
                }
            }
        }
        tile_sync<NW>();
        if (tend > row.hi) break; // nothing lies beyond
        from = tend;
    }
}
// the one-sided turns of the reader and of lh_kept_merge's two passes
template <int NW, class Step>
__device__ __forceinline__ void turns(Row &row, uint32_t n, u64 *tile, uint32_t lane, uint32_t w, Step step)
{
    turns_of<NW, 1, KEPT_TILE>(row, n, n, tile, lane, w, step);
}

// the tile (of the kernel's s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE]), the scatterer and the entry of a call that this wave
// works on, for the two shapes.  WORDS: what a row has in LDS (the compare's two tiles are one such block).
template <int NW, uint32_t WORDS = KEPT_TILE> struct Seat {
    uint32_t lane, w, m;
    u64 *tile;
    __device__ __forceinline__ Seat(u64 (*s_tile)[WORDS])
    {
        const uint32_t wave = threadIdx.x >> 6;
        lane = threadIdx.x & 63;
        w = NW == 1 ? 0u : wave;
        m = NW == 1 ? blockIdx.x * ROW_WAVES + wave : blockIdx.x;
        tile = s_tile[NW == 1 ? wave : 0];
    }
    __device__ __forceinline__ void clear() const
    {
        for (uint32_t i = NW == 1 ? lane : threadIdx.x; i < WORDS; i += NW * 64) tile[i] = 0;
    }
    // How a kernel over M entries starts: false for a seat beyond them (uniform for all that share a tile), else the tile is cleared
    __device__ __forceinline__ bool take(uint32_t M) const
    {
        if (m >= M) return false;
        clear();
        return true;
    }
    // The row of entry m.  IDS: ids[m] (an absolute row number, as `first` is); otherwise first + m.  A row outside the block of
    // ANY handle read gives the empty entry, and nothing is read for it (Row::settle).
    template <bool IDS> __device__ __forceinline__ uint32_t row(uint32_t first, const uint32_t *__restrict__ ids) const
    {
        if constexpr (IDS) return (uint32_t)__builtin_amdgcn_readfirstlane((int)ids[__builtin_amdgcn_readfirstlane((int)m)]);
        else return first + m;
    }
};

// A window of the list: its handles [lo, lo + len), which one entry of a call reads.  The whole list is {0, s.n}.
struct Slice {
    uint32_t lo, len;
};
// The windows of lh_kept_series* / lh_kept_heat* / lh_kept_spread_series*, by value in the kernel arguments beside the list (256
// bytes): w[k] = {lo, hi}.  A window kernel has one window per blockIdx.y: slice() is its own (lo < hi <= s.n: the host checked).
struct KeptWindows {
    uint8_t w[LH_MAX_WINDOWS][2];
    __device__ __forceinline__ Slice slice() const
    {
        const uint32_t lo = w[blockIdx.y][0], hi = w[blockIdx.y][1];
        return Slice{lo, hi - lo};
    }
};
static_assert(LH_MAX_KEPT <= 255, "a window's ends in a byte each");
// Window-major outputs: entry (w, m) of a window kernel at w * nmetrics + m, so that window w's block of every output is what the
// parent kernel writes for the window's slice(s) of the list -- the same entry function, hence the same bytes.
__device__ __forceinline__ size_t window_entry(uint32_t m, uint32_t nmetrics) { return (size_t)blockIdx.y * nmetrics + m; }

// (every wave that shares the tile, which is zero)  Entry e of the outputs: row r over the handles of `win`.  Lane i opens handle
// win.lo + i and the turns run over win.len handles; present_bits speaks of the WHOLE list (bit i: s.h[i]).  A row outside the
// block of ANY handle of the window gives the empty entry, and nothing is read for it.
template <int NW>
__device__ __forceinline__ void across_entry(const Seat<NW> &at, const KeptList &s, const Slice win, uint32_t r, size_t e,
                                             const double *__restrict__ D, const PctArgs &pa, uint32_t np, const KeptOut &o)
{
    const uint32_t lane = at.lane;
    Row row;
    if (lane < win.len) row.open(s.h[win.lo + lane], r);
    row.settle();
    const u64 total = readlane_u64(wave_scan_incl_u64(row.rc), 63);
    const u64 present = __builtin_amdgcn_ballot_w64(row.end > row.cur) << win.lo;
    const uint32_t hi = row.hi;

    double ps = 0.0;
    uint32_t occ = 0;
    Open pct; // lane i < np: percentile i
    if (total) {                       // uniform
        pct.open(lane < np ? pct_threshold(pa.p[lane], total) : PCT_NONE);
        turns<NW>(row, win.len, at.tile, lane, at.w, [&](const u64 (&C)[4], uint32_t base) {
            double d[4], t[4];
            load4_values(D, base + 4 * lane, hi, d);
            const u64 tc = sum4(C);
            ps += terms4(C, d, t);
            occ += occupied4(C);
            pct.step(C, tc, base, lane);
        });
    }
    if (at.w != 0) return;
    const double sum = readlane_f64(wave_scan_incl_f64(ps), 63);
    const uint32_t nb = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl_u32(occ), 63);
    if (lane == 0) {
        if (o.count) o.count[e] = total;
        if (o.sum) o.sum[e] = total ? sum : 0.0;
        if (o.nbuckets) o.nbuckets[e] = total ? nb : 0;
        if (o.present) o.present[e] = total ? present : 0;
    }
    if (lane < np) {
        store_pct(o.pkeys, o.pvalid, e * np + lane, pct.found);
    }
}

// lh_kept_across*: the entry over the whole list (lane i opens handle i)
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_across(const KeptList s, uint32_t nmetrics, uint32_t first,
                                                                          const double *__restrict__ D, const PctArgs pa,
                                                                          uint32_t np, const KeptOut o,
                                                                          const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    across_entry<NW>(at, s, Slice{0, s.n}, at.template row<IDS>(first, ids), at.m, D, pa, np, o);
}

// lh_kept_series*: the same entry per WINDOW of the list -- but for present_bits, which across_entry shifts left by the window's lo
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_series(const KeptList s, const KeptWindows sw, uint32_t nmetrics,
                                                                          uint32_t first, const double *__restrict__ D,
                                                                          const PctArgs pa, uint32_t np, const KeptOut o,
                                                                          const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    across_entry<NW>(at, s, sw.slice(), r, window_entry(at.m, nmetrics), D, pa, np, o);
}
static_assert(sizeof(KeptList) + sizeof(KeptWindows) + sizeof(PctArgs) + sizeof(KeptOut) + 5 * 8 < 4096,
              "k_kept_series' arguments inside the 4 KiB argument segment");

// ---- lh_kept_merge, lh_kept_gather, lh_kept_group -------------------------------------------------------------------------------------
// The two passes around k_keep_scan in the reader's two shapes, ONE device body each (merge_count, merge_fill) that takes the row of
// lane i through a row-source type, as count_le_entry takes its bounds:
//   BlockRows{first}    lh_kept_merge: row first + m of EVERY handle (the host checked that each holds the block; Row::open)
//   MappedRows{src, n}  lh_kept_gather: row src[i * n + m] of handle i, for that handle alone (Row::open_own: LH_KEPT_NO_ROW or a row
//                       outside handle i's block leaves lane i's segment empty and nothing else).  One 4-byte load a lane, from 64
//                       lines that neighbouring rows share.  TRANSPOSED: the map as k_gather_transpose leaves it, src[m * nk + i],
//                       one line a row (lh_tool_kept_gather_route; profiles/kept_gather.txt has both).
//   GroupRows{goff, members, ...}  lh_kept_group: the rows members[goff[m] .. goff[m + 1]) of EVERY handle, each for that handle alone
//                       (Row::open_own again).  Its sources are the pairs (handle, member), as many as the call likes: at most 64 of
//                       them are seated one a lane and take the same open and turns as the two above; more go in chunks of 64
//                       (chunk_turns).
// count: nnz[m + 1] = the non-zero cells of the union -- a sum that wrapped to 0 is none --, row_count[m] = the wrapping sum of the
// handles' own row_count entries (which is the wrapping sum of the cells).
struct BlockRows {
    uint32_t first;
    __device__ __forceinline__ void open(Row &row, const KeptRec h, uint32_t, uint32_t m) const { row.open(h, first + m); }
};
template <bool TRANSPOSED> struct MappedRows {
    const uint32_t *__restrict__ src;
    uint32_t n, nk; // output rows, handles
    __device__ __forceinline__ void open(Row &row, const KeptRec h, uint32_t i, uint32_t m) const
    {
        row.open_own(h, TRANSPOSED ? src[(size_t)m * nk + i] : src[(size_t)i * n + m]);
    }
};

// The summed row of output row at.m, handed to `step` 256 bins a step (turns); returns the wrapping sum of its sources' row_count
// entries.  One source a lane: lane i is handle i, its row the row source's.
template <int NW, class Rows, class Step>
__device__ __forceinline__ u64 summed_row(const Seat<NW> &at, const KeptList &s, const Rows &rows, Step step)
{
    Row row;
    if (at.lane < s.n) rows.open(row, s.h[at.lane], at.lane, at.m);
    row.settle();
    const u64 total = readlane_u64(wave_scan_incl_u64(row.rc), 63);
    turns<NW>(row, s.n, at.tile, at.lane, at.w, step);
    return total;
}

// ---- lh_kept_group's row source ---------------------------------------------------------------------------------------------------
// What the NW waves of a workgroup-per-row kernel tell each other in a chunked row: each wave's least bin of a turn, and at the first
// open its last bin and its sum of row_count entries.  (A wave per row shares nothing.)
template <int NW> struct ChunkShare {
    u64 rc[NW];
    uint32_t least[NW], hi[NW];
};
__device__ __forceinline__ u64 uniform_u64(u64 v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (u64)hi << 32 | lo;
}
// Output row m sums the rows members[a .. a + len) of each of the nk handles, with a = min(goff[m], nmembers) and the end clamped
// the same way (an end at or before a: none) -- the device form's arrays are any bytes, and both passes clamp alike.  SOURCE x of
// the row, x < len * nk, is member x % len of handle x / len: handle-major, so that the 64 sources of a chunk read one or two lines
// of `members`.
template <int NW> struct GroupRows {
    const u64 *__restrict__ goff;          // ngroups + 1 entries
    const uint32_t *__restrict__ members;  // nmembers entries
    u64 nmembers;                          // <= 0xffffffff
    uint32_t nk;                           // handles
    ChunkShare<NW> *share;
    // (uniform for all that share a tile)  the first member and the number of members of row m: two 8-byte loads
    __device__ __forceinline__ void span(uint32_t m, u64 &a, u64 &len) const
    {
        const u64 g0 = uniform_u64(goff[m]), g1 = uniform_u64(goff[(size_t)m + 1]);
        a = g0 < nmembers ? g0 : nmembers;
        const u64 b = g1 < nmembers ? g1 : nmembers;
        len = b > a ? b - a : 0;
    }
    // (x < len * nk)  source x: a LH_KEPT_NO_ROW member, or one outside this handle's block, leaves the segment empty (Row::open_own)
    __device__ __forceinline__ void open(Row &row, const KeptList &s, u64 a, u64 len, u64 x) const
    {
        const u64 i = x / len, j = x - i * len;
        row.open_own(s.h[i], members[a + j]);
    }
};

// The turns of a row of S > 64 sources, in chunks of 64: lane l of chunk c is source 64 * c + l, and wave w of the NW that share the
// tile takes the chunks w, w + NW, ...  Per turn a FIRST SWEEP opens every chunk again -- the offsets, then (behind the first tile)
// the binary search to `from`, one key -- for the least bin of all, which decides t0 as in turns_of; a SECOND SWEEP scatters the runs
// of every chunk into the one tile (a wave whose only chunk is still open keeps it); then turns_of's ascending walk hands `step` its
// cells and puts zeros back.  hi (the last bin of the union) and the sum of the row_count entries are taken at the first open.  The
// chunk count, `from`, t0 and hi are the same in every wave: all control flow around the readlanes, ballots and barriers is
// uniform.  The adds are integer adds: no byte depends on the chunk order, the shape or the timing.  (The tile is zero on entry and
// again on return.)  Returns the wrapping sum of the sources' row_count entries.
template <int NW, class Step>
__device__ __forceinline__ u64 chunk_turns(const Seat<NW> &at, const KeptList &s, const GroupRows<NW> &g, u64 a, u64 len, u64 S, Step step)
{
    const uint32_t lane = at.lane, w = at.w;
    u64 *tile = at.tile;
    const u64 chunks = (S + 63) / 64;
    u64 total = 0;
    uint32_t hi = 0;
    // source x of the row as the turn from bin `from` finds it: the cursor at the first entry at or above `from`, the bin there
    const auto reopen = [&](Row &row, u64 x, uint32_t from) {
        row = Row();
        if (x < S) g.open(row, s, a, len, x);
        if (from) {
            u64 lo = row.cur, up = row.end;
            while (lo < up) {
                const u64 mid = lo + (up - lo) / 2;
                if (bin_of(((gkeys)row.keys)[mid]) < from) lo = mid + 1;
                else up = mid;
            }
            row.cur = lo;
        }
        if (row.cur < row.end) row.next = bin_of(((gkeys)row.keys)[row.cur]);
    };
    tile_sync<NW>(); // the tile is zero
    Row row;
    for (uint32_t from = 0;;) {
        // ---- first sweep: the least bin at or above `from`
        uint32_t next = NO_BIN, last = 0;
        u64 rc = 0;
        for (u64 c = w; c < chunks; c += NW) { // wave-uniform
            reopen(row, 64 * c + lane, from);
            next = min(next, row.next);
            if (!from) { // uniform
                rc += row.rc;
                if (row.end > row.cur) last = max(last, bin_of(((gkeys)row.keys)[row.end - 1]));
            }
        }
        uint32_t least = ~wave_max_u32(~next);
        if (!from) {
            hi = wave_max_u32(last);
            total = readlane_u64(wave_scan_incl_u64(rc), 63);
        }
        if constexpr (NW > 1) {
            ChunkShare<NW> &sh = *g.share;
            if (lane == 0) {
                sh.least[w] = least;
                if (!from) {
                    sh.hi[w] = hi;
                    sh.rc[w] = total;
                }
            }
            __syncthreads(); // (the next turn's stores come behind the two barriers of this one)
            least = NO_BIN;
            for (int k = 0; k < NW; k++) least = min(least, sh.least[k]);
            if (!from) {
                hi = 0;
                total = 0;
                for (int k = 0; k < NW; k++) {
                    hi = max(hi, sh.hi[k]);
                    total += sh.rc[k];
                }
            }
        }
        if (least == NO_BIN) break;
        const uint32_t t0 = least & ~3u, tend = t0 + KEPT_TILE;
        // ---- second sweep: every source's run inside the tile, 64 entries a turn; only the sources that have one
        for (u64 c = w; c < chunks; c += NW) { // wave-uniform
            if (chunks > NW) reopen(row, 64 * c + lane, from); // (else this wave's one chunk is open)
            for (u64 live = __builtin_amdgcn_ballot_w64(row.next < tend); live; live &= live - 1) {
                const uint32_t i = (uint32_t)__builtin_ctzll(live);
                u64 cur = readlane_u64(row.cur, i);
                const u64 e = readlane_u64(row.end, i);
                const gkeys kp = (gkeys)readlane_u64(row.keys, i);
                const gu64 cp = (gu64)readlane_u64(row.counts, i);
                while (cur < e) {
                    const u64 idx = cur + lane;
                    bool in = false;
                    if (idx < e) {
                        const uint32_t bin = bin_of(kp[idx]) - t0;
                        if (bin < KEPT_TILE) {
                            in = true;
                            atomicAdd(&tile[bin], cp[idx]);
                        }
                    }
                    const uint32_t took = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(in));
                    cur += took;
                    if (took < 64) break;
                }
            }
        }
        tile_sync<NW>();
        // ---- walk, and zeros back
        if (w == 0) {
            const uint32_t wend = min(tend - 1, hi);
            for (uint32_t base = t0; base <= wend; base += STEP) {
                const uint32_t at4 = base + 4 * lane - t0;
                u64 C[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    C[k] = tile[at4 + k];
                    tile[at4 + k] = 0;
                }
                step(C, base);
            }
        }
        tile_sync<NW>();
        if (tend > hi) break; // nothing lies beyond
        from = tend;
    }
    return total;
}

// lh_kept_group's summed row: S = nk * len sources.  S <= 64 is exactly the gather's open and turns, one source a lane.
template <int NW, class Step>
__device__ __forceinline__ u64 summed_row(const Seat<NW> &at, const KeptList &s, const GroupRows<NW> &g, Step step)
{
    u64 a, len;
    g.span(at.m, a, len);
    const u64 S = len * g.nk;
    if (S > 64) return chunk_turns<NW>(at, s, g, a, len, S, step); // uniform for all that share a tile
    Row row;
    if (at.lane < S) g.open(row, s, a, len, at.lane);
    row.settle();
    const u64 total = readlane_u64(wave_scan_incl_u64(row.rc), 63);
    turns<NW>(row, (uint32_t)S, at.tile, at.lane, at.w, step);
    return total;
}

template <int NW, class Rows>
__device__ __forceinline__ void merge_count(const KeptList &s, uint32_t nrows, const Rows rows, u64 *__restrict__ nnz,
                                            u64 *__restrict__ row_count, u64 (*s_tile)[KEPT_TILE])
{
    const Seat<NW> at(s_tile);
    const uint32_t lane = at.lane, m = at.m;
    if (m >= nrows) return; // uniform for all that share a tile
    at.clear();
    uint32_t occ = 0;
    const u64 total = summed_row<NW>(at, s, rows, [&](const u64 (&C)[4], uint32_t) { occ += occupied4(C); });
    if (at.w != 0) return;
    occ = wave_scan_incl_u32(occ);
    if (lane == 63) {
        nnz[(size_t)m + 1] = occ;
        row_count[m] = total;
    }
}

// fill: the same turns; each step's non-zero cells to keys / counts[off[m] .. off[m + 1]), ascending by bin, as k_keep_fill
// places them.  (Nothing is stored at or beyond off[m + 1].)
template <int NW, class Rows>
__device__ __forceinline__ void merge_fill(const KeptList &s, uint32_t nrows, const Rows rows, const u64 *__restrict__ off,
                                           int16_t *__restrict__ keys, u64 *__restrict__ counts, u64 (*s_tile)[KEPT_TILE])
{
    const Seat<NW> at(s_tile);
    const uint32_t lane = at.lane, m = at.m;
    if (m >= nrows) return; // uniform for all that share a tile
    u64 to = off[m];
    const u64 lim = off[(size_t)m + 1];
    if (to >= lim) return; // (the same)
    at.clear();
    summed_row<NW>(at, s, rows, [&](const u64 (&C)[4], uint32_t base) {
        const uint32_t b0 = base + 4 * lane, n = occupied4(C), inc = wave_scan_incl_u32(n);
        u64 pos = to + (inc - n);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (C[k] && pos < lim) {
                keys[pos] = (int16_t)bin_to_key(b0 + k);
                counts[pos] = C[k];
                pos++;
            }
        to += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    });
}

// lh_kept_merge: rows [first, first + nrows) of every handle of the list
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_merge_count(const KeptList s, uint32_t nrows, uint32_t first,
                                                                          u64 *__restrict__ nnz, u64 *__restrict__ row_count)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    merge_count<NW>(s, nrows, BlockRows{first}, nnz, row_count, s_tile);
}
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_merge_fill(const KeptList s, uint32_t nrows, uint32_t first,
                                                                         const u64 *__restrict__ off, int16_t *__restrict__ keys,
                                                                         u64 *__restrict__ counts)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    merge_fill<NW>(s, nrows, BlockRows{first}, off, keys, counts, s_tile);
}

// lh_kept_gather*: output row m takes row src[i * n + m] of handle i (the map holds s.n * n entries: the host sized it)
template <int NW, bool TRANSPOSED>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_gather_count(const KeptList s, uint32_t n,
                                                                           const uint32_t *__restrict__ src, u64 *__restrict__ nnz,
                                                                           u64 *__restrict__ row_count)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    merge_count<NW>(s, n, MappedRows<TRANSPOSED>{src, n, s.n}, nnz, row_count, s_tile);
}
template <int NW, bool TRANSPOSED>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_gather_fill(const KeptList s, uint32_t n, const uint32_t *__restrict__ src,
                                                                          const u64 *__restrict__ off, int16_t *__restrict__ keys,
                                                                          u64 *__restrict__ counts)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    merge_fill<NW>(s, n, MappedRows<TRANSPOSED>{src, n, s.n}, off, keys, counts, s_tile);
}
// lh_kept_group*: output row m sums the rows members[goff[m] .. goff[m + 1]) of every handle (goff: ngroups + 1 entries, members:
// nmembers; both clamped as GroupRows::span says, so any bytes will do)
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_group_count(const KeptList s, uint32_t ngroups, const u64 *__restrict__ goff,
                                                                          const uint32_t *__restrict__ members, u64 nmembers,
                                                                          u64 *__restrict__ nnz, u64 *__restrict__ row_count)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    __shared__ ChunkShare<NW> s_share;
    merge_count<NW>(s, ngroups, GroupRows<NW>{goff, members, nmembers, s.n, &s_share}, nnz, row_count, s_tile);
}
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_group_fill(const KeptList s, uint32_t ngroups, const u64 *__restrict__ goff,
                                                                         const uint32_t *__restrict__ members, u64 nmembers,
                                                                         const u64 *__restrict__ off, int16_t *__restrict__ keys,
                                                                         u64 *__restrict__ counts)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    __shared__ ChunkShare<NW> s_share;
    merge_fill<NW>(s, ngroups, GroupRows<NW>{goff, members, nmembers, s.n, &s_share}, off, keys, counts, s_tile);
}
// the map of nk handles x n rows, handle-major, to row-major: to[m * nk + i] = src[i * n + m] (one thread an entry of `to`)
__global__ __launch_bounds__(ROW_BLOCK) void k_gather_transpose(const uint32_t *__restrict__ src, uint32_t n, uint32_t nk,
                                                                uint32_t *__restrict__ to)
{
    const u64 e = (u64)blockIdx.x * ROW_BLOCK + threadIdx.x;
    if (e >= (u64)n * nk) return;
    const u64 m = e / nk, i = e % nk;
    to[e] = src[i * n + m];
}

// THE DIRECT ROUTE of a gather of ONE handle: a permutation, selection or duplication of rows, no cell changes and no tile is
// needed.  A handle's cells are non-zero and ascending by invariant (lh_keep made them, lh_kept_load* proved them), so the bytes are
// the tile route's.  count: a thread per output row, nnz[m + 1] = the source row's length, row_count[m] its row_count entry.
__global__ __launch_bounds__(ROW_BLOCK) void k_gather1_count(const KeptRec h, uint32_t n, const uint32_t *__restrict__ src,
                                                            u64 *__restrict__ nnz, u64 *__restrict__ row_count)
{
    const u64 m = (u64)blockIdx.x * ROW_BLOCK + threadIdx.x;
    if (m >= n) return;
    Row row;
    row.open_own(h, src[m]);
    nnz[m + 1] = row.end - row.cur;
    row_count[m] = row.rc;
}
// n elements from the global address `from` to `to`, by the nt threads of which this is thread t: 16 bytes an access over the
// stretch where source and destination are 16-byte aligned TOGETHER (their addresses agree modulo 16), element by element before
// and behind it, and everywhere when they never are.
typedef uint32_t v4u __attribute__((ext_vector_type(4))); // 16 bytes, a native vector: one global_load_dwordx4
typedef const __attribute__((address_space(1))) v4u *gvec;
template <class T> __device__ __forceinline__ void copy_run(T *__restrict__ to, u64 from, u64 n, uint32_t t, uint32_t nt)
{
    typedef const __attribute__((address_space(1))) T *gsrc;
    constexpr u64 PER = 16 / sizeof(T);
    const gsrc src = (gsrc)from;
    u64 head = 0, body = 0;
    if ((((u64)(uintptr_t)to ^ from) & 15) == 0) {
        head = ((16 - (from & 15)) & 15) / sizeof(T);
        head = head < n ? head : n;
        body = (n - head) / PER;
    }
    for (u64 i = t; i < head; i += nt) to[i] = src[i];
    const gvec s4 = (gvec)(from + head * sizeof(T));
    v4u *d4 = reinterpret_cast<v4u *>(to + head);
    for (u64 i = t; i < body; i += nt) d4[i] = s4[i];
    for (u64 i = head + body * PER + t; i < n; i += nt) to[i] = src[i];
}
// fill: the source row's keys and counts verbatim to keys / counts[off[m] .. off[m + 1]); a wave per row, or a workgroup per row.
// (Nothing is stored at or beyond off[m + 1], whatever the map holds now.)
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_gather1_fill(const KeptRec h, uint32_t n, const uint32_t *__restrict__ src,
                                                                           const u64 *__restrict__ off, int16_t *__restrict__ keys,
                                                                           u64 *__restrict__ counts)
{
    const uint32_t wave = threadIdx.x >> 6, m = NW == 1 ? blockIdx.x * ROW_WAVES + wave : blockIdx.x;
    if (m >= n) return; // uniform for the wave / the workgroup
    const u64 to = off[m], lim = off[(size_t)m + 1];
    if (to >= lim) return;
    Row row;
    row.open_own(h, (uint32_t)__builtin_amdgcn_readfirstlane((int)src[m]));
    const u64 len = min(row.end - row.cur, lim - to);
    const uint32_t t = NW == 1 ? threadIdx.x & 63 : threadIdx.x, nt = NW == 1 ? 64 : WG;
    copy_run<u64>(counts + to, row.counts + 8 * row.cur, len, t, nt);
    copy_run<int16_t>(keys + to, row.keys + 2 * row.cur, len, t, nt);
}

// ---- lh_kept_slide ------------------------------------------------------------------------------------------------------------
// The merge's two passes with the compare's two tiles: handles 0 .. nadd - 1 of the list are `add`, the others `sub`; each side
// is an UNSIGNED sum in its own tile (no subtraction happens in LDS) and the step takes A[k] - B[k].  count: nnz[m + 1] = the
// non-zero differences, row_count[m] = the wrapping sum of the add handles' row_count entries minus the same over sub; a cell
// with B[k] > A[k] -- decided on the wrapped sums -- is folded into *verdict as row << 16 | bin (the ABSOLUTE row) with a 64-bit
// atomic min, k_kept_check's pattern: the lowest row, in it the lowest bin, whatever the timing and the shape (SLIDE_CLEAN: none).
// Wave 0 alone walks in both shapes.  With no sub handle every B is 0 and the bytes are k_merge_count's / k_merge_fill's.
constexpr u64 SLIDE_CLEAN = ~0ull;
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_slide_count(const KeptList s, uint32_t nadd, uint32_t nrows,
                                                                          uint32_t first, u64 *__restrict__ nnz,
                                                                          u64 *__restrict__ row_count, u64 *__restrict__ verdict)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    const uint32_t lane = at.lane, m = at.m;
    if (m >= nrows) return; // uniform for all that share the tiles
    at.clear();
    Row row; // lane i opens handle i
    if (lane < s.n) row.open(s.h[lane], first + m);
    row.settle();
    const u64 ra = readlane_u64(wave_scan_incl_u64(lane < nadd ? row.rc : 0), 63);
    const u64 rb = readlane_u64(wave_scan_incl_u64(lane < nadd ? 0 : row.rc), 63);
    uint32_t occ = 0, under = NO_BIN; // the lane's lowest bin that would go below zero
    turns_of<NW, 2, KEPT_COMPARE_TILE>(row, s.n, nadd, at.tile, lane, at.w, [&](const u64 (&A)[4], const u64 (&B)[4], uint32_t base) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            occ += A[k] != B[k] ? 1u : 0u;
            if (B[k] > A[k]) under = min(under, base + 4 * lane + k); // (ascending steps: the first one stays)
        }
    });
    if (at.w != 0) return;
    occ = wave_scan_incl_u32(occ);
    under = ~wave_max_u32(~under);
    if (lane == 63) {
        nnz[(size_t)m + 1] = occ;
        row_count[m] = ra - rb;
    }
    if (under != NO_BIN && lane == 0) atomicMin(verdict, (u64)(first + m) << 16 | under);
}

// fill (launched for a clean verdict only: A[k] >= B[k] everywhere): k_merge_fill's placing, of the non-zero differences
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_slide_fill(const KeptList s, uint32_t nadd, uint32_t nrows,
                                                                         uint32_t first, const u64 *__restrict__ off,
                                                                         int16_t *__restrict__ keys, u64 *__restrict__ counts)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    const uint32_t lane = at.lane, m = at.m;
    if (m >= nrows) return; // uniform for all that share the tiles
    u64 to = off[m];
    const u64 lim = off[(size_t)m + 1];
    if (to >= lim) return; // (the same)
    at.clear();
    Row row;
    if (lane < s.n) row.open(s.h[lane], first + m);
    row.settle();
    turns_of<NW, 2, KEPT_COMPARE_TILE>(row, s.n, nadd, at.tile, lane, at.w, [&](const u64 (&A)[4], const u64 (&B)[4], uint32_t base) {
        const u64 C[4] = {A[0] - B[0], A[1] - B[1], A[2] - B[2], A[3] - B[3]};
        const uint32_t b0 = base + 4 * lane, n = occupied4(C), inc = wave_scan_incl_u32(n);
        u64 pos = to + (inc - n);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (C[k] && pos < lim) {
                keys[pos] = (int16_t)bin_to_key(b0 + k);
                counts[pos] = C[k];
                pos++;
            }
        to += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    });
}

// ---- lh_kept_compare ----------------------------------------------------------------------------------------------------------
// Handles 0 .. nbase - 1 of the list are `base`, the others `cur`; rows as in k_kept_across.  One walk: k_compare_wave's walk 2
// over the steps the tiles cover, and for the bins between two tiles -- X is constant there -- their number times the term,
// added by lane 0 just before the step behind them.
// (na and nb both non-zero)  The walk itself, for k_kept_compare and for k_kept_movers_score, whose three distances are thereby
// the same bits: the turns over the opened row's two tiles with the step above, into the lane's b (best_init'ed by the caller).
template <int NW>
__device__ __forceinline__ void compare_turns(Row &row, uint32_t n, uint32_t nbase, u64 *tile, uint32_t lane, uint32_t w, u64 na,
                                              u64 nb, Best &b)
{
    const Scale sc = make_scale(na, nb);
    u64 ca = 0, cb = 0;        // what lies below the step
    uint32_t behind = NO_BIN;  // the bin behind the last step taken (NO_BIN: none yet)
    turns_of<NW, 2, KEPT_COMPARE_TILE>(row, n, nbase, tile, lane, w, [&](const u64 (&A)[4], const u64 (&B)[4], uint32_t base) {
        if (behind != NO_BIN && base > behind && lane == 0) { // bins [behind, base) lie in no tile: the prefixes stay ca, cb
            const u128 xa = (u128)ca * sc.nb, xb = (u128)cb * sc.na;
            const bool up = xa >= xb;
            const u128 x = up ? xa - xb : xb - xa;
            const double t = (double)(base - behind) * ((double)(u64)(x >> sc.sh) / sc.den);
            b.w += t;
            b.s += up ? t : -t;
        }
        const u64 ta = sum4(A), tb = sum4(B);
        const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
        take4(b, sc, base + 4 * lane, ca + (ia - ta), cb + (ib - tb), A, B);
        ca += readlane_u64(ia, 63);
        cb += readlane_u64(ib, 63);
        behind = base + STEP;
    });
}

// The windows of lh_kept_drift*, by value in the kernel arguments beside the list (512 bytes): w[k] = {base_lo, base_hi, cur_lo,
// cur_hi}.  One window per blockIdx.y: slices() gives its own pair (lo < hi <= s.n on both sides, at most LH_MAX_KEPT handles
// together: the host checked).
struct KeptDriftWindows {
    uint8_t w[LH_MAX_WINDOWS][4];
    __device__ __forceinline__ void slices(Slice &base, Slice &cur) const
    {
        const uint32_t blo = w[blockIdx.y][0], bhi = w[blockIdx.y][1], clo = w[blockIdx.y][2], chi = w[blockIdx.y][3];
        base = Slice{blo, bhi - blo};
        cur = Slice{clo, chi - clo};
    }
};

// (every wave that shares the tiles, which are zero)  Entry e of the outputs: row r, the handles of `base` against those of `cur`,
// two slices of the ONE list that may overlap, coincide and stand in either order.  Lane i < base.len opens handle base.lo + i,
// lane base.len + j handle cur.lo + j: the lanes are what k_kept_compare's are for the list (base's handles, then cur's), so na
// comes from the first group, nb from the second, and the turns run over base.len + cur.len lanes with base.len in the first tile.
// A row outside the block of ANY handle of the two slices gives the entry of two empty sides.
template <int NW>
__device__ __forceinline__ void compare_entry(const Seat<NW, 2 * KEPT_COMPARE_TILE> &at, const KeptList &s, const Slice base,
                                              const Slice cur, uint32_t r, size_t e, const CompareOut &o)
{
    const uint32_t lane = at.lane, n = base.len + cur.len;
    Row row;
    if (lane < n) row.open(s.h[lane < base.len ? base.lo + lane : cur.lo + (lane - base.len)], r);
    row.settle();
    const u64 na = readlane_u64(wave_scan_incl_u64(lane < base.len ? row.rc : 0), 63);
    const u64 nb = readlane_u64(wave_scan_incl_u64(lane < base.len ? 0 : row.rc), 63);

    Best b;
    best_init(b);
    if (na && nb) compare_turns<NW>(row, n, base.len, at.tile, lane, at.w, na, nb, b); // uniform
    if (at.w != 0) return;
    u128 x;
    uint32_t bin;
    u64 ba, bb;
    wave_best(b, x, bin, ba, bb);
    const double w1 = readlane_f64(wave_scan_incl_f64(b.w), 63), shift = readlane_f64(wave_scan_incl_f64(b.s), 63);
    if (lane == 0) store_row(o, e, na, nb, bin, ba, bb, w1, shift);
}

// lh_kept_compare*: the entry over the whole list, handles 0 .. nbase - 1 against the others (lane i opens handle i)
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_compare(const KeptList s, uint32_t nbase, uint32_t nmetrics,
                                                                           uint32_t first, const CompareOut o,
                                                                           const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    if (!at.take(nmetrics)) return;
    compare_entry<NW>(at, s, Slice{0, nbase}, Slice{nbase, s.n - nbase}, at.template row<IDS>(first, ids), at.m, o);
}

// lh_kept_drift*: the same entry per WINDOW, a pair of slices of the one list
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_drift(const KeptList s, const KeptDriftWindows sw, uint32_t nmetrics,
                                                                         uint32_t first, const CompareOut o,
                                                                         const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    Slice base, cur;
    sw.slices(base, cur);
    compare_entry<NW>(at, s, base, cur, r, window_entry(at.m, nmetrics), o);
}
static_assert(sizeof(KeptList) + sizeof(KeptDriftWindows) + sizeof(CompareOut) + 4 * 8 < 4096,
              "k_kept_drift's arguments inside the 4 KiB argument segment");

// ---- lh_kept_top / lh_kept_movers: the score passes in front of lh_select.h's k_select ---------------------------------------------
// Rows first + m (the host refused a range outside any handle's block; such a row would still be the empty entry).  ONE turn over
// the row: the total comes from row_count, so the percentile's threshold and the bound's take are known before a cell is read.
// The sum by k_kept_across' step in its order (the same bits); BY_PERCENTILE: lane 0 owns the one threshold of lh_pct.h's Open,
// k_kept_across' search; BY_COUNT_ABOVE: the cells of the bins at or beyond the take -- bins are absolute, so a take before the
// first tile takes every cell, one in a stretch no tile covers the cells of the tiles behind it, one beyond the last step none:
// count minus what k_kept_count_le returns for the bound.  Wave 0 alone walks; its lane 0 writes the row's record (TopRecords,
// the key complemented for LH_TOP_ASCENDING: `flip`).
// (every wave that shares the tile, which is zero)  Record e: row r over the handles of `win` (across_entry's open)
template <int NW>
__device__ __forceinline__ void top_score_entry(const Seat<NW> &at, const KeptList &s, const Slice win, uint32_t r, size_t e,
                                                const double *__restrict__ D, uint32_t by, double arg, u64 flip, const TopRecords &rec)
{
    const uint32_t lane = at.lane;
    Row row; // lane i opens handle win.lo + i
    if (lane < win.len) row.open(s.h[win.lo + lane], r);
    row.settle();
    const u64 total = readlane_u64(wave_scan_incl_u64(row.rc), 63);
    const uint32_t hi = row.hi;

    double ps = 0.0;
    u64 ab = 0;
    Open pct; // lane 0: the percentile
    if (total) { // uniform
        const bool want_pct = by == LH_TOP_BY_PERCENTILE, want_above = by == LH_TOP_BY_COUNT_ABOVE; // uniform
        const uint32_t take = want_above ? le_take(arg) : 0u;
        pct.open(want_pct && lane == 0 ? pct_threshold(arg, total) : PCT_NONE);
        turns<NW>(row, win.len, at.tile, lane, at.w, [&](const u64 (&C)[4], uint32_t base) {
            double d[4], t[4];
            load4_values(D, base + 4 * lane, hi, d);
            const u64 tc = sum4(C);
            ps += terms4(C, d, t);
            if (want_pct) pct.step(C, tc, base, lane);
            if (want_above) {
                const uint32_t b0 = base + 4 * lane;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) ab += b0 + k >= take ? C[k] : 0;
            }
        });
    }
    if (at.w != 0) return;
    const double sum = total ? readlane_f64(wave_scan_incl_f64(ps), 63) : 0.0;
    const u64 above = readlane_u64(wave_scan_incl_u64(ab), 63);
    if (lane == 0) {
        uint32_t found = pct.found;
        if (found == NO_BIN) found = total ? hi : 0u; // (a total that wrapped: some bin of the row)
        u64 key, aux = 0;
        if (by == LH_TOP_BY_COUNT) {
            key = total;
        } else if (by == LH_TOP_BY_SUM) {
            key = order_key_f64(sum);
        } else if (by == LH_TOP_BY_PERCENTILE) {
            key = found;
            aux = total ? (u64)(uint16_t)(int16_t)bin_to_key(found) : 0;
        } else {
            key = above;
            aux = above;
        }
        rec.key[e] = key ^ flip;
        rec.count[e] = total;
        rec.sum[e] = sum;
        rec.aux[e] = aux;
    }
}

// lh_kept_top*: the record over the whole list (lane i opens handle i), record m
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_top_score(const KeptList s, uint32_t nmetrics, uint32_t first,
                                                                             const double *__restrict__ D, uint32_t by, double arg,
                                                                             u64 flip, const TopRecords r)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    top_score_entry<NW>(at, s, Slice{0, s.n}, first + at.m, at.m, D, by, arg, flip, r);
}

// lh_kept_top_series*: the same record per WINDOW of the list, window w's at w * npad + m (npad: nmetrics padded to whole groups
// of SEL_PER, as select_records pads a call's records: every window's block is one k_select_windows' workgroup reads as it is)
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_top_score_series(const KeptList s, const KeptWindows sw,
                                                                                    uint32_t nmetrics, uint32_t npad, uint32_t first,
                                                                                    const double *__restrict__ D, uint32_t by,
                                                                                    double arg, u64 flip, const TopRecords r)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    top_score_entry<NW>(at, s, sw.slice(), first + at.m, window_entry(at.m, npad), D, by, arg, flip, r);
}
static_assert(sizeof(KeptList) + sizeof(KeptWindows) + sizeof(TopRecords) + 7 * 8 < 4096,
              "k_kept_top_score_series' arguments inside the 4 KiB argument segment");

// Handles 0 .. nbase - 1 of the list are `base`, the others `cur`, as in k_kept_compare, whose open, totals and -- for the three
// distances -- walk, wave_best and sums these are (compare_turns): the scores are the bits lh_kept_compare returns.
// BY_PERCENTILE: ONE joint turn that carries both prefixes and finds, on each side, the first bin whose inclusive prefix reaches
// that side's threshold (k_kept_across' search, find_in_step); the turns are not left early -- the tiles must come back zeroed --
// so once both bins are found the step does nothing, and the turns only put zeros back.  Lane 0 of wave 0 writes the row's record
// (MoversRecords).
// (every wave that shares the tiles, which are zero)  Record e: row r, the handles of `base` against those of `cur` (compare_entry's
// pair of slices of the one list, and its lanes)
template <int NW>
__device__ __forceinline__ void movers_score_entry(const Seat<NW, 2 * KEPT_COMPARE_TILE> &at, const KeptList &s, const Slice base,
                                                   const Slice cur, uint32_t r, size_t e, uint32_t by, double arg, u64 flip,
                                                   const MoversRecords &rec)
{
    const uint32_t lane = at.lane, n = base.len + cur.len;
    Row row; // compare_entry's lanes: base's handles, then cur's
    if (lane < n) row.open(s.h[lane < base.len ? base.lo + lane : cur.lo + (lane - base.len)], r);
    row.settle();
    const u64 na = readlane_u64(wave_scan_incl_u64(lane < base.len ? row.rc : 0), 63);
    const u64 nb = readlane_u64(wave_scan_incl_u64(lane < base.len ? 0 : row.rc), 63);
    const bool is_cand = na != 0 && nb != 0; // uniform

    double score = 0.0;
    uint32_t keys = 0; // key << 16 | key_base
    if (by != LH_MOVERS_BY_PERCENTILE) { // uniform
        Best b;
        best_init(b);
        if (is_cand) compare_turns<NW>(row, n, base.len, at.tile, lane, at.w, na, nb, b);
        if (at.w != 0) return;
        u128 x;
        uint32_t bin;
        u64 ba, bb;
        wave_best(b, x, bin, ba, bb);
        const double w1 = readlane_f64(wave_scan_incl_f64(b.w), 63), shift = readlane_f64(wave_scan_incl_f64(b.s), 63);
        if (by == LH_MOVERS_BY_KS) { // (store_row's: an X of 0 everywhere is a distance of 0 at key 0)
            if (is_cand && bin != NO_BIN) {
                score = fabs((double)ba / (double)na - (double)bb / (double)nb);
                keys = (uint32_t)(uint16_t)(int16_t)bin_to_key(bin) << 16;
            }
        } else {
            score = by == LH_MOVERS_BY_W1 ? w1 : shift;
        }
    } else {
        uint32_t fa = NO_BIN, fb = NO_BIN;
        if (is_cand) {
            // (the host keeps arg in [0, 1]: 1 <= T <= total)
            const u64 Ta = readlane_u64(pct_threshold(arg, na), 0), Tb = readlane_u64(pct_threshold(arg, nb), 0);
            u64 ca = 0, cb = 0; // what lies below the step
            turns_of<NW, 2, KEPT_COMPARE_TILE>(row, n, base.len, at.tile, lane, at.w,
                                               [&](const u64 (&A)[4], const u64 (&B)[4], uint32_t b0) {
                if (fa != NO_BIN && fb != NO_BIN) return; // uniform: both found
                const u64 ta = sum4(A), tb = sum4(B);
                const u64 ia = wave_scan_incl_u64(ta), ib = wave_scan_incl_u64(tb);
                const u64 ea = ca + readlane_u64(ia, 63), eb = cb + readlane_u64(ib, 63);
                if (fa == NO_BIN && Ta <= ea) { // uniform: it is in this step
                    u64 pre[4];
                    prefix4(A, ca, ta, ia, pre);
                    fa = b0 + find_in_step(pre, Ta);
                }
                if (fb == NO_BIN && Tb <= eb) {
                    u64 pre[4];
                    prefix4(B, cb, tb, ib, pre);
                    fb = b0 + find_in_step(pre, Tb);
                }
                ca = ea;
                cb = eb;
            });
            if (fa == NO_BIN) fa = row.hi; // (totals that wrapped: some bin of the row)
            if (fb == NO_BIN) fb = row.hi;
            score = (double)((long long)fb - (long long)fa);
            keys = (uint32_t)(uint16_t)(int16_t)bin_to_key(fb) << 16 | (uint32_t)(uint16_t)(int16_t)bin_to_key(fa);
        }
        if (at.w != 0) return;
    }
    if (lane == 0) {
        if (!is_cand) score = 0.0;
        rec.key[e] = order_key_f64(score) ^ flip;
        rec.cand[e] = is_cand ? MOVER_CANDIDATE | keys : 0;
        rec.count_a[e] = na;
        rec.count_b[e] = nb;
        rec.score[e] = (u64)__double_as_longlong(score);
    }
}

// lh_kept_movers*: the record over the whole list, handles 0 .. nbase - 1 against the others (lane i opens handle i), record m
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_movers_score(const KeptList s, uint32_t nbase, uint32_t nmetrics,
                                                                                uint32_t first, uint32_t by, double arg, u64 flip,
                                                                                const MoversRecords r)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    if (!at.take(nmetrics)) return;
    movers_score_entry<NW>(at, s, Slice{0, nbase}, Slice{nbase, s.n - nbase}, first + at.m, at.m, by, arg, flip, r);
}

// lh_kept_movers_series*: the same record per WINDOW, a pair of slices of the one list, window w's at w * npad + m
template <int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_movers_score_series(const KeptList s, const KeptDriftWindows sw,
                                                                                       uint32_t nmetrics, uint32_t npad,
                                                                                       uint32_t first, uint32_t by, double arg,
                                                                                       u64 flip, const MoversRecords r)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][2 * KEPT_COMPARE_TILE];
    const Seat<NW, 2 * KEPT_COMPARE_TILE> at(s_tile);
    if (!at.take(nmetrics)) return;
    Slice base, cur;
    sw.slices(base, cur);
    movers_score_entry<NW>(at, s, base, cur, first + at.m, window_entry(at.m, npad), by, arg, flip, r);
}
static_assert(sizeof(KeptList) + sizeof(KeptDriftWindows) + sizeof(MoversRecords) + 6 * 8 < 4096,
              "k_kept_movers_score_series' arguments inside the 4 KiB argument segment");

// ---- lh_kept_count_le ---------------------------------------------------------------------------------------------------------
// the bounds, shared by all names, by value in the kernel arguments (512 bytes beside the list's 1 544)
struct KeptBounds { double b[LH_MAX_BOUNDS]; };
// Where count_le_entry's lane j < nb takes bound j of entry m from: the one shared row above (k_kept_count_le, k_kept_heat), or row m
// of a device array of nb doubles an entry, the caller's own or the staged copy of a host form (k_kept_slo, k_kept_burn_score: one
// coalesced load a wave).  Nothing is assumed of a row: every lane takes its bound on its own, and le_take gives a NaN no bin.
struct SharedBounds {
    const KeptBounds &sb;
    __device__ __forceinline__ double of(uint32_t lane, uint32_t) const { return sb.b[lane]; }
};
struct RowBounds {
    const double *__restrict__ rows;
    uint32_t m;
    __device__ __forceinline__ double of(uint32_t lane, uint32_t nb) const { return rows[(size_t)m * nb + lane]; }
};

// Rows as in k_kept_across.  One turn over the row with k_count_le_wave's step: lane j owns bound j, which takes in the first
// E = le_take(bounds[j]) bins, and the prefix at bin E - 1 is fetched from the lane that owns it only in a step some pending
// bound falls into.  `base` jumps between tiles: a pending bound whose E is at or below the step's base lies before the first
// tile or in a stretch no tile covers, and takes the running carry; one beyond the last step takes everything.  total is the
// wrapping sum of the handles' row_count entries: no cell is read for it (and the row is walked whatever it is: cells whose
// sum wraps to 0 still count towards cum).  Integer sums only: the two shapes agree exactly.
// (every wave that shares the tile, which is zero)  Row r over the handles of `win` (across_entry's open) against the bounds `from`
// hands out: in wave 0 of those that share the tile, lane j < nb returns what bound j takes in, and every lane has the row's total
// in `tot`.
template <int NW, class Bounds>
__device__ __forceinline__ u64 count_le_walk(const Seat<NW> &at, const KeptList &s, const Slice win, uint32_t r, const Bounds &from,
                                             uint32_t nb, u64 &tot)
{
    const uint32_t lane = at.lane;
    Row row;
    if (lane < win.len) row.open(s.h[win.lo + lane], r);
    row.settle();
    tot = readlane_u64(wave_scan_incl_u64(row.rc), 63);

    uint32_t E = 0;
    if (lane < nb) E = le_take(from.of(lane, nb));
    bool pend = lane < nb && E > 0; // a bound that takes in no bin: 0
    u64 res = 0, carry = 0;
    turns<NW>(row, win.len, at.tile, lane, at.w, [&](const u64 (&C)[4], uint32_t base) {
        if (pend && E <= base) { // every bin it takes in lies below this step: what the steps so far hold
            res = carry;
            pend = false;
        }
        const u64 t = sum4(C);
        const u64 inc = wave_scan_incl_u64(t);
        // (every pending E is > base now)
        const bool in = pend && E <= base + STEP;
        if (__builtin_amdgcn_ballot_w64(in)) { // wave-uniform
            const uint32_t idx = in ? E - 1 - base : 0, f = idx >> 2, k = idx & 3;
            const u64 p0 = carry + (inc - t) + C[0], p1 = p0 + C[1], p2 = p1 + C[2], p3 = p2 + C[3];
            const u64 v0 = shfl_u64(p0, f), v1 = shfl_u64(p1, f), v2 = shfl_u64(p2, f), v3 = shfl_u64(p3, f);
            if (in) {
                res = k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3;
                pend = false;
            }
        }
        carry += readlane_u64(inc, 63);
    });
    return pend ? carry : res; // beyond the last step: everything
}
// Entry e of the outputs from that walk
template <int NW, class Bounds>
__device__ __forceinline__ void count_le_entry(const Seat<NW> &at, const KeptList &s, const Slice win, uint32_t r, size_t e,
                                               const Bounds &from, uint32_t nb, u64 *__restrict__ cum, u64 *__restrict__ total)
{
    u64 tot;
    const u64 res = count_le_walk<NW>(at, s, win, r, from, nb, tot);
    if (at.w != 0) return;
    if (cum && at.lane < nb) cum[e * nb + at.lane] = res;
    if (total && at.lane == 0) total[e] = tot;
}

// lh_kept_count_le*: the entry over the whole list (lane i opens handle i)
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_count_le(const KeptList s, uint32_t nmetrics, uint32_t first,
                                                                            const KeptBounds sb, uint32_t nb, u64 *__restrict__ cum,
                                                                            u64 *__restrict__ total,
                                                                            const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    count_le_entry<NW>(at, s, Slice{0, s.n}, at.template row<IDS>(first, ids), at.m, SharedBounds{sb}, nb, cum, total);
}

// lh_kept_heat*: the same entry per WINDOW of the list
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_heat(const KeptList s, const KeptWindows sw, uint32_t nmetrics,
                                                                        uint32_t first, const KeptBounds sb, uint32_t nb,
                                                                        u64 *__restrict__ cum, u64 *__restrict__ total,
                                                                        const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    count_le_entry<NW>(at, s, sw.slice(), r, window_entry(at.m, nmetrics), SharedBounds{sb}, nb, cum, total);
}
static_assert(sizeof(KeptList) + sizeof(KeptWindows) + sizeof(KeptBounds) + 6 * 8 < 4096,
              "k_kept_heat's arguments inside the 4 KiB argument segment");

// ---- lh_kept_slo / lh_kept_burn: a row of bounds PER ENTRY ----------------------------------------------------------------------
// lh_kept_slo*: k_kept_heat's entry with row m of `bounds` ([nmetrics * nb] doubles in device memory) in the shared row's place: lane
// j < nb loads bounds[m * nb + j], one coalesced load a wave.  The array may be the caller's own, which no host has seen: a row
// that decreases is answered bound by bound (the lanes of count_le_walk never look at each other's bound) and a NaN takes in no bin.
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_slo(const KeptList s, const KeptWindows sw, uint32_t nmetrics,
                                                                       uint32_t first, const double *__restrict__ bounds, uint32_t nb,
                                                                       u64 *__restrict__ cum, u64 *__restrict__ total,
                                                                       const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    count_le_entry<NW>(at, s, sw.slice(), r, window_entry(at.m, nmetrics), RowBounds{bounds, at.m}, nb, cum, total);
}

// The rates of lh_kept_burn*, one per window, by value beside the list and the windows (1 KiB)
struct KeptRates { double r[LH_MAX_WINDOWS]; };
// lh_kept_burn*, pass 1: k_kept_slo's entry with ONE bound an entry, decided where it is known -- lane 0 of the wave that owns entry
// (w, m): bad = total - cum, t = rate[w] * budget[m], fires = total != 0 && (double)bad > t * (double)total; two rounded products
// (the unit is built with -ffp-contract=off), a strict compare that a NaN fails.  An entry that does NOT fire adds 1 to miss[m]
// (zero before the launch): an integer sum, whatever the order of the windows' workgroups.  cum / total (may be null) as k_kept_slo's.
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_burn_score(const KeptList s, const KeptWindows sw, const KeptRates rates,
                                                                              uint32_t nmetrics, uint32_t first,
                                                                              const double *__restrict__ bounds,
                                                                              const double *__restrict__ budget, u64 *__restrict__ cum,
                                                                              u64 *__restrict__ total, const uint32_t *__restrict__ ids,
                                                                              uint32_t *__restrict__ miss)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    u64 tot;
    const u64 res = count_le_walk<NW>(at, s, sw.slice(), r, RowBounds{bounds, at.m}, 1u, tot);
    if (at.w != 0 || at.lane != 0) return;
    const size_t e = window_entry(at.m, nmetrics);
    if (cum) cum[e] = res;
    if (total) total[e] = tot;
    const u64 bad = tot - res;
    const double t = rates.r[blockIdx.y] * budget[at.m];
    const bool fires = tot != 0 && (double)bad > t * (double)tot;
    if (!fires) atomicAdd(&miss[at.m], 1u);
}
static_assert(sizeof(KeptList) + sizeof(KeptWindows) + sizeof(KeptRates) + 8 * 8 < 4096,
              "k_kept_burn_score's arguments inside the 4 KiB argument segment");

// lh_kept_burn*, pass 2, ONE workgroup in k_keep_scan's pattern: the entries with miss[m] == 0 -- they fired in every window -- in
// ascending m, WG at a time; entry m's place is the number of reported entries below it, the first k of them are written as {m, its
// row} and *n_out is the number of all of them.  Nothing of out at or beyond min(*n_out, k) is written.
template <bool IDS>
__global__ __launch_bounds__(WG) void k_kept_burn_emit(const uint32_t *__restrict__ miss, uint32_t nmetrics, uint32_t first,
                                                       const uint32_t *__restrict__ ids, u64 k, lh_burn_hit *__restrict__ out,
                                                       u64 *__restrict__ n_out)
{
    __shared__ uint32_t s_w[WG_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (u64 base = 0; base < nmetrics; base += WG) { // uniform
        const u64 i = base + threadIdx.x;
        const bool hit = i < nmetrics && miss[i] == 0;
        const uint32_t inc = wave_scan_incl_u32(hit ? 1u : 0u);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t below = 0, all = 0;
        for (uint32_t j = 0; j < (uint32_t)WG_WAVES; j++) {
            const uint32_t t = s_w[j];
            below += j < wave ? t : 0;
            all += t;
        }
        const u64 pos = carry + below + inc - 1;
        if (hit && pos < k) {
            lh_burn_hit h;
            h.entry = (uint32_t)i;
            h.row = IDS ? ids[i] : first + (uint32_t)i;
            out[pos] = h;
        }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = carry;
}

// ---- lh_kept_spread -----------------------------------------------------------------------------------------------------------
// Rows as in k_kept_across.  lh_spread's two walks as TWO turns over the same row (the turns advance the cursors: the opened
// Row is kept and taken again; the tile is zero on return).  The count is the sum of the row_count entries, so the thresholds
// are known before a cell is read.  Walk 1: sum.  Walk 2: k_spread_wave's -- the centred moment about sum / float64(count) and,
// in the steps a threshold falls into, the key, count_le and sum_le (lh_pct.h's central4, sums_in_step).  Wave 0 alone walks
// in both shapes, per lane over the steps in ascending order, then one DPP tree over the lanes: the shapes agree bit for bit.
// (every wave that shares the tile, which is zero)  Entry e of the outputs: row r over the handles of `win` (across_entry's open)
template <int NW>
__device__ __forceinline__ void spread_entry(const Seat<NW> &at, const KeptList &s, const Slice win, uint32_t r, size_t e,
                                             const double *__restrict__ D, const PctArgs &pa, uint32_t np, const SpreadOut &o)
{
    const uint32_t lane = at.lane;
    Row row;
    if (lane < win.len) row.open(s.h[win.lo + lane], r);
    row.settle();
    const u64 total = readlane_u64(wave_scan_incl_u64(row.rc), 63);
    const uint32_t hi = row.hi;

    double sum = 0.0, m2 = 0.0, r_sle = 0.0;
    u64 r_cle = 0;
    Open pct; // lane i < np: percentile i
    if (total) { // uniform
        const Row opened = row;
        // ---- walk 1: the sum
        double ps = 0.0;
        turns<NW>(row, win.len, at.tile, lane, at.w, [&](const u64 (&C)[4], uint32_t base) {
            double d[4], t[4];
            load4_values(D, base + 4 * lane, hi, d);
            ps += terms4(C, d, t);
        });
        sum = readlane_f64(wave_scan_incl_f64(ps), 63); // (wave 0's: the others walk nothing, here and below)
        // ---- walk 2: the centred moment; the steps the thresholds fall into
        const double mean = sum / (double)total;
        pct.open(lane < np ? pct_threshold(pa.p[lane], total) : PCT_NONE);
        double run = 0.0, q = 0.0; // the lane's terms of the steps so far; its share of m2
        row = opened;
        turns<NW>(row, win.len, at.tile, lane, at.w, [&](const u64 (&C)[4], uint32_t base) {
            double d[4], t[4];
            load4_values(D, base + 4 * lane, hi, d);
            q += central4(C, d, mean);
            const double ts = terms4(C, d, t);
            if (pct.todo) { // wave-uniform
                const u64 tc = sum4(C);
                uint32_t here = pct.ending(tc);
                if (here) {
                    u64 pre[4];
                    pct.prefixes(C, tc, pre);
                    const double sbefore = readlane_f64(wave_scan_incl_f64(run), 63);
                    const double incs = wave_scan_incl_f64(ts);
                    for (; here; here &= here - 1) {
                        const uint32_t i = (uint32_t)__builtin_ctz(here);
                        u64 cle;
                        double sle;
                        const uint32_t idx = sums_in_step(pre, t, incs, sbefore, pct.threshold(i), cle, sle);
                        if (lane == i) {
                            pct.found = base + idx;
                            r_cle = cle;
                            r_sle = sle;
                        }
                    }
                }
            }
            run += ts;
        });
        m2 = readlane_f64(wave_scan_incl_f64(q), 63);
    }
    if (at.w != 0) return;
    if (lane == 0) {
        if (o.count) o.count[e] = total;
        if (o.sum) o.sum[e] = sum;
        if (o.m2) o.m2[e] = m2;
    }
    if (lane < np) {
        const size_t to = e * np + lane;
        store_pct(o.pkeys, o.pvalid, to, pct.found);
        if (o.count_le) o.count_le[to] = r_cle;
        if (o.sum_le) o.sum_le[to] = r_sle;
    }
}

// lh_kept_spread*: the entry over the whole list (lane i opens handle i)
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_spread(const KeptList s, uint32_t nmetrics, uint32_t first,
                                                                          const double *__restrict__ D, const PctArgs pa,
                                                                          uint32_t np, const SpreadOut o,
                                                                          const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    spread_entry<NW>(at, s, Slice{0, s.n}, at.template row<IDS>(first, ids), at.m, D, pa, np, o);
}

// lh_kept_spread_series*: the same entry per WINDOW of the list
template <bool IDS, int NW>
__global__ __launch_bounds__(NW == 1 ? ROW_BLOCK : WG) void k_kept_spread_series(const KeptList s, const KeptWindows sw,
                                                                                 uint32_t nmetrics, uint32_t first,
                                                                                 const double *__restrict__ D, const PctArgs pa,
                                                                                 uint32_t np, const SpreadOut o,
                                                                                 const uint32_t *__restrict__ ids)
{
    __shared__ u64 s_tile[NW == 1 ? ROW_WAVES : 1][KEPT_TILE];
    const Seat<NW> at(s_tile);
    if (!at.take(nmetrics)) return;
    const uint32_t r = at.template row<IDS>(first, ids);
    spread_entry<NW>(at, s, sw.slice(), r, window_entry(at.m, nmetrics), D, pa, np, o);
}
static_assert(sizeof(KeptList) + sizeof(KeptWindows) + sizeof(PctArgs) + sizeof(SpreadOut) + 5 * 8 < 4096,
              "k_kept_spread_series' arguments inside the 4 KiB argument segment");

// ---- lh_kept_load: the check ---------------------------------------------------------------------------------------------------
// The block of a blob -- offsets[nrows + 1] | row_count[nrows] | counts[cells] | keys[cells], copied verbatim into an allocation of
// exactly that size -- is UNTRUSTED: every kernel above loops and scatters by these arrays.  k_kept_check proves what lh_keep
// guarantees before a handle exists, a wave per row like k_keep_count, and is safe on arbitrary bytes: the host has checked
// that the four arrays of (nrows, cells) fill the allocation; the kernel reads offsets[m], offsets[m + 1] and row_count[m] for
// m < nrows, and a cell only at an index in [offsets[m], offsets[m + 1]) after it has seen offsets[m] <= offsets[m + 1] <= cells
// and at most LH_NKEYS of them: a row's walk is bounded by 1 024 steps whatever the bytes say.  No LDS, no scratch; a lane per
// cell, 64 cells a step: counts by 8-byte loads (512 contiguous bytes a wave), keys by 2-byte loads (128 bytes; the keys start
// at 8 * cells behind the counts and a row's first key at any even address, so wider loads would be unaligned at both ends of
// a row).  A violation is (row, index, cause) packed row << 32 | index << 8 | cause and folded into *verdict with a 64-bit
// atomic min: the lowest row, in it the lowest index, there the lowest cause, whatever the timing.  A row whose offsets are bad
// reports that (index 0, the lowest such cause) and reads no cell; a cell's causes have the cell's index in the row; a
// row_count that is not the wrapping sum of the row has index = the row's number of cells, behind every cell.
constexpr u64 CHECK_NONE = ~0ull;
constexpr uint32_t CHECK_NONE32 = 0xffffffffu;
__global__ __launch_bounds__(ROW_BLOCK) void k_kept_check(u64 block, uint32_t nrows, u64 cells, u64 *__restrict__ verdict)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    const gu64 off = (gu64)block, row_count = off + (size_t)nrows + 1, counts = row_count + nrows;
    const gkeys keys = (gkeys)(block + 8 * (2 * (u64)nrows + 1) + 8 * cells);
    const u64 a = off[m], b = off[(size_t)m + 1];
    uint32_t bad = CHECK_NONE32; // index << 8 | cause
    if (m == nrows - 1 && b != cells) bad = LH_KEPT_BAD_OFFSET_LAST;
    if (a <= b && b <= cells && b - a > LH_NKEYS) bad = LH_KEPT_BAD_ROW_LENGTH;
    if (a > b || b > cells) bad = LH_KEPT_BAD_OFFSET_ORDER;
    if (m == 0 && a != 0) bad = LH_KEPT_BAD_OFFSET_FIRST; // (the lowest cause code last)
    if (bad == CHECK_NONE32) { // wave-uniform: the row's cells are [a, b), inside the arrays, LH_NKEYS at most
        const uint32_t n = (uint32_t)(b - a);
        u64 cnt = 0;
        uint32_t carry = 0; // the bin of the last cell of the step before
        for (uint32_t base = 0; base < n; base += 64) { // wave-uniform
            const uint32_t i = base + lane;
            const bool in = i < n;
            uint32_t bin = 0;
            u64 c = 0;
            if (in) {
                bin = bin_of(keys[a + i]);
                c = counts[a + i];
            }
            // the bin of the cell before: lane - 1's (row_shr:1 inside a row of 16 lanes, the three lanes between rows by
            // readlane), lane 0 the carry
            uint32_t prev = LH_DPP32(bin, 0x111, 0xf);
            const uint32_t b15 = (uint32_t)__builtin_amdgcn_readlane((int)bin, 15), b31 = (uint32_t)__builtin_amdgcn_readlane((int)bin, 31),
                           b47 = (uint32_t)__builtin_amdgcn_readlane((int)bin, 47);
            prev = lane == 0 ? carry : lane == 16 ? b15 : lane == 32 ? b31 : lane == 48 ? b47 : prev;
            cnt += c;
            uint32_t v = CHECK_NONE32;
            if (in) {
                if (c == 0) v = i << 8 | LH_KEPT_BAD_ZERO_COUNT;
                if (i > 0 && prev >= bin) v = i << 8 | LH_KEPT_BAD_KEY_ORDER; // (the lower cause code last)
            }
            const uint32_t least = ~wave_max_u32(~v);
            if (least != CHECK_NONE32) { // wave-uniform: no later step holds a lower index
                bad = least;
                break;
            }
            carry = (uint32_t)__builtin_amdgcn_readlane((int)bin, 63);
        }
        if (bad == CHECK_NONE32 && readlane_u64(wave_scan_incl_u64(cnt), 63) != row_count[m]) bad = n << 8 | LH_KEPT_BAD_ROW_COUNT;
    }
    if (bad != CHECK_NONE32 && lane == 0) atomicMin(verdict, (u64)m << 32 | bad);
}
static_assert(LH_KEPT_BAD_OFFSET_FIRST < LH_KEPT_BAD_OFFSET_ORDER && LH_KEPT_BAD_OFFSET_ORDER < LH_KEPT_BAD_ROW_LENGTH &&
                  LH_KEPT_BAD_ROW_LENGTH < LH_KEPT_BAD_OFFSET_LAST && LH_KEPT_BAD_KEY_ORDER < LH_KEPT_BAD_ZERO_COUNT &&
                  LH_KEPT_BAD_SAMPLES < 256,
              "k_kept_check assigns a row's and a cell's causes in descending order of their codes; a cause is the low byte");

// one workgroup (k_keep_scan's pattern): the header's `samples` against the wrapping sum of row_count; row = nrows, behind every row
__global__ __launch_bounds__(WG) void k_kept_check_samples(u64 block, uint32_t nrows, u64 samples, u64 *__restrict__ verdict)
{
    __shared__ u64 s_w[WG_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const gu64 row_count = (gu64)block + (size_t)nrows + 1;
    u64 s = 0;
    for (u64 base = 0; base < nrows; base += WG) { // uniform
        const u64 i = base + threadIdx.x;
        s += i < nrows ? row_count[i] : 0;
    }
    s = wave_scan_incl_u64(s);
    if (lane == 63) s_w[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 all = 0;
        for (uint32_t k = 0; k < (uint32_t)WG_WAVES; k++) all += s_w[k];
        if (all != samples) atomicMin(verdict, (u64)nrows << 32 | LH_KEPT_BAD_SAMPLES);
    }
}

// ---- lh_kept_encode* / lh_kept_decode*: the compact blob (loghisto_gpu.h has the format) ------------------------------------------
// Behind the header a directory of uint32 desc[nrows] = n | cw << 20 | km << 24 (padded to 8 bytes), then per row of n >= 1 cells a
// record of S(m) bytes, 8-aligned: the counts at 1 << cw bytes each, then the bins as uint16 first + n - 1 byte deltas (km 0) or as
// uint16 bin[n] (km 1), each part zero-padded to 8.  Both directions are a wave per row in k_kept_check's shape -- a lane per cell,
// 64 cells a step, the bin of the cell before by the same DPP shift with the carry between steps -- and need no LDS: the encoder's
// first pass finds the row's largest count class and largest gap (desc[m] and S(m)), k_keep_scan turns S into the records'
// offsets, the second pass writes every byte of the record, pads included.  The decoder trusts nothing: k_dec_dir reads the
// directory ALONE and proves it (reserved bits, n <= LH_NKEYS, and with the scan's two totals on the host: the cells and the bytes
// the header states), so that by the time k_dec_fill runs every record lies inside the payload and every output range inside the
// handle's exact allocation, whatever the records hold; a row's walk is bounded by 1 024 steps and a delta row's bins by
// 65 535 + 65 535 * 256 < 2^32.  Violations fold into *verdict as k_kept_check's do: row << 32 | index << 8 | cause, atomic min.
constexpr uint32_t ENC_DESC_BITS = 0x1ffffu | 3u << 20 | 1u << 24;
__host__ __device__ inline u64 up8(u64 x) { return (x + 7) & ~7ull; }
__host__ __device__ inline u64 enc_directory_bytes(uint32_t nrows) { return 8 * (((u64)nrows + 1) / 2); }
// S(m) of a row of n cells (n < 2^17, whatever a descriptor says: under 2^21 bytes)
__host__ __device__ inline uint32_t enc_record_bytes(uint32_t n, uint32_t cw, uint32_t km)
{
    return n ? (uint32_t)(up8((u64)n << cw) + up8(km ? 2 * (u64)n : (u64)n + 1)) : 0u;
}
// cw of one count: the least of 0 .. 3 with c < 2^(8 << cw)
__device__ __forceinline__ uint32_t width_class(u64 c) { return c > 0xffffffffull ? 3u : c > 0xffffu ? 2u : c > 0xffu ? 1u : 0u; }
// x of lane - 1 (k_kept_check's shift: row_shr:1 inside a row of 16 lanes, the three lanes between rows by readlane), lane 0 the carry
__device__ __forceinline__ uint32_t lane_before(uint32_t x, uint32_t lane, uint32_t carry)
{
    const uint32_t prev = LH_DPP32(x, 0x111, 0xf);
    const uint32_t b15 = (uint32_t)__builtin_amdgcn_readlane((int)x, 15), b31 = (uint32_t)__builtin_amdgcn_readlane((int)x, 31),
                   b47 = (uint32_t)__builtin_amdgcn_readlane((int)x, 47);
    return lane == 0 ? carry : lane == 16 ? b15 : lane == 32 ? b31 : lane == 48 ? b47 : prev;
}

// encode, pass 1: a wave per row of a HANDLE (its arrays hold what lh_keep guarantees): desc[m], and S(m) into soff[m + 1]
__global__ __launch_bounds__(ROW_BLOCK) void k_enc_size(u64 block, uint32_t nrows, u64 cells, uint32_t *__restrict__ desc,
                                                       u64 *__restrict__ soff)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    const gu64 off = (gu64)block, counts = off + 2 * (size_t)nrows + 1;
    const gkeys keys = (gkeys)(block + 8 * (2 * (u64)nrows + 1) + 8 * cells);
    const u64 a = off[m];
    const uint32_t n = (uint32_t)(off[(size_t)m + 1] - a);
    uint32_t cw = 0, gap = 0, carry = 0;
    for (uint32_t base = 0; base < n; base += 64) { // wave-uniform
        const uint32_t i = base + lane;
        const bool in = i < n;
        uint32_t bin = 0;
        u64 c = 0;
        if (in) {
            bin = bin_of(keys[a + i]);
            c = counts[a + i];
        }
        const uint32_t prev = lane_before(bin, lane, carry);
        if (in) {
            cw = max(cw, width_class(c));
            if (i > 0) gap = max(gap, bin - prev);
        }
        carry = (uint32_t)__builtin_amdgcn_readlane((int)bin, 63);
    }
    cw = wave_max_u32(cw);
    const uint32_t km = wave_max_u32(gap) > 256 ? 1u : 0u;
    if (lane == 0) {
        desc[m] = n ? n | cw << 20 | km << 24 : 0u;
        soff[(size_t)m + 1] = enc_record_bytes(n, cw, km);
    }
}

// encode, pass 2: a wave per row writes desc[m] into the directory at `payload` (8-aligned; the last row's wave the pad word) and the
// row's record at payload + D + soff[m]: EVERY byte of it -- what the buffer held before does not show
__global__ __launch_bounds__(ROW_BLOCK) void k_enc_fill(u64 block, uint32_t nrows, u64 cells, const uint32_t *__restrict__ desc,
                                                       const u64 *__restrict__ soff, unsigned char *__restrict__ payload)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    const uint32_t d = desc[m];
    if (lane == 0) {
        uint32_t *dir = reinterpret_cast<uint32_t *>(payload);
        dir[m] = d;
        if (m == nrows - 1 && (nrows & 1)) dir[nrows] = 0;
    }
    const uint32_t n = d & 0x1ffffu, cw = d >> 20 & 3, km = d >> 24 & 1;
    if (!n) return;
    const gu64 off = (gu64)block, counts = off + 2 * (size_t)nrows + 1;
    const gkeys keys = (gkeys)(block + 8 * (2 * (u64)nrows + 1) + 8 * cells);
    const u64 a = off[m];
    unsigned char *rec = payload + enc_directory_bytes(nrows) + soff[m];
    const uint32_t cb = n << cw, kb = km ? 2 * n : n + 1;
    unsigned char *kp = rec + up8(cb);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += 64) { // wave-uniform
        const uint32_t i = base + lane;
        const bool in = i < n;
        uint32_t bin = 0;
        u64 c = 0;
        if (in) {
            bin = bin_of(keys[a + i]);
            c = counts[a + i];
        }
        const uint32_t prev = lane_before(bin, lane, carry);
        if (in) {
            if (cw == 0) rec[i] = (unsigned char)c;
            else if (cw == 1) reinterpret_cast<uint16_t *>(rec)[i] = (uint16_t)c;
            else if (cw == 2) reinterpret_cast<uint32_t *>(rec)[i] = (uint32_t)c;
            else reinterpret_cast<u64 *>(rec)[i] = c;
            if (km) reinterpret_cast<uint16_t *>(kp)[i] = (uint16_t)bin;
            else if (i == 0) *reinterpret_cast<uint16_t *>(kp) = (uint16_t)bin;
            else kp[1 + i] = (unsigned char)(bin - prev - 1);
        }
        carry = (uint32_t)__builtin_amdgcn_readlane((int)bin, 63);
    }
    if (lane < 8) { // at most 7 pad bytes behind each part
        if (cb + lane < up8(cb)) rec[cb + lane] = 0;
        if (kb + lane < up8(kb)) kp[kb + lane] = 0;
    }
}

// decode, stage 1: a thread per descriptor (and one for the pad word behind an odd number of them): n into off[m + 1], S(m) into
// soff[m + 1] -- 0 for a descriptor that is refused, whose row then decides the verdict.  Reads dir[0 .. nrows + (nrows & 1)) only:
// inside the payload, the host has checked bytes >= D.
__global__ __launch_bounds__(256) void k_dec_dir(const uint32_t *__restrict__ dir, uint32_t nrows, u64 *__restrict__ off,
                                                 u64 *__restrict__ soff, u64 *__restrict__ verdict)
{
    const u64 m = (u64)blockIdx.x * 256 + threadIdx.x;
    if (m > nrows) return;
    if (m == nrows) {
        if ((nrows & 1) && dir[m] != 0) atomicMin(verdict, (u64)nrows << 32 | LH_KEPT_BAD_ENC_PAD);
        return;
    }
    const uint32_t d = dir[m], n = d & 0x1ffffu;
    const bool bad = (d & ~ENC_DESC_BITS) != 0 || n > LH_NKEYS || (n == 0 && d != 0);
    off[m + 1] = bad ? 0 : n;
    soff[m + 1] = bad ? 0 : enc_record_bytes(n, d >> 20 & 3, d >> 24 & 1);
    if (bad) atomicMin(verdict, m << 32 | LH_KEPT_BAD_ENC_DESC);
}

// decode, stage 2: a wave per row of a SOUND directory, from the row's record into the handle's block (offsets already there:
// `block`'s first nrows + 1 words are the scan of n), row_count[m] too.  What stage 1 proved of the row is held once more against
// the descriptor as it reads NOW (the device form reads the caller's memory in place): a row that no longer agrees is refused
// and not walked, so no load or store leaves the payload's `bytes` or the block whatever happens to the source meanwhile.
__global__ __launch_bounds__(ROW_BLOCK) void k_dec_fill(const unsigned char *__restrict__ payload, uint32_t nrows, u64 cells, u64 bytes,
                                                       u64 block, const u64 *__restrict__ soff, u64 *__restrict__ verdict)
{
    const uint32_t lane = threadIdx.x & 63, m = blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
    if (m >= nrows) return; // wave-uniform
    u64 *off = reinterpret_cast<u64 *>(block), *row_count = off + (size_t)nrows + 1, *counts = row_count + nrows;
    int16_t *keys = reinterpret_cast<int16_t *>(counts + cells);
    const u64 a = off[m], b = off[(size_t)m + 1], ra = soff[m], rb = soff[(size_t)m + 1], D = enc_directory_bytes(nrows);
    const uint32_t d = reinterpret_cast<const uint32_t *>(payload)[m], n = d & 0x1ffffu, cw = d >> 20 & 3, km = d >> 24 & 1;
    uint32_t bad = CHECK_NONE32; // index << 8 | cause
    if ((d & ~ENC_DESC_BITS) != 0 || n > LH_NKEYS || a > b || b > cells || b - a != n || ra > rb || rb - ra != enc_record_bytes(n, cw, km) ||
        D + rb > bytes)
        bad = LH_KEPT_BAD_ENC_DESC;
    u64 cnt = 0;
    if (bad == CHECK_NONE32 && n) { // wave-uniform
        const unsigned char *rec = payload + D + ra;
        const uint32_t cb = n << cw, kb = km ? 2 * n : n + 1;
        const unsigned char *kp = rec + up8(cb);
        uint32_t carry = 0, wide = 0, gap = 0; // carry: the bin of the last cell of the step before
        for (uint32_t base = 0; base < n; base += 64) { // wave-uniform
            const uint32_t i = base + lane;
            const bool in = i < n;
            uint32_t bin = 0, step = 0;
            u64 c = 0;
            if (in) {
                if (cw == 0) c = rec[i];
                else if (cw == 1) c = reinterpret_cast<const uint16_t *>(rec)[i];
                else if (cw == 2) c = reinterpret_cast<const uint32_t *>(rec)[i];
                else c = reinterpret_cast<const u64 *>(rec)[i];
                if (km) bin = reinterpret_cast<const uint16_t *>(kp)[i];
                else step = i == 0 ? (uint32_t)*reinterpret_cast<const uint16_t *>(kp) : (uint32_t)kp[1 + i] + 1u;
            }
            if (!km) bin = carry + wave_scan_incl_u32(step); // (a lane behind the row: the row's last bin)
            const uint32_t prev = lane_before(bin, lane, carry);
            cnt += c;
            uint32_t v = CHECK_NONE32;
            if (in) {
                wide = max(wide, width_class(c));
                if (i > 0 && bin > prev) gap = max(gap, bin - prev);
                if (bin >= LH_NKEYS) v = i << 8 | LH_KEPT_BAD_ENC_KEY_RANGE;
                if (c == 0) v = i << 8 | LH_KEPT_BAD_ZERO_COUNT;
                if (km && i > 0 && prev >= bin) v = i << 8 | LH_KEPT_BAD_KEY_ORDER; // (the lowest cause code last)
                keys[a + i] = (int16_t)bin_to_key(bin & 0xffffu);
                counts[a + i] = c;
            }
            const uint32_t least = ~wave_max_u32(~v);
            if (least != CHECK_NONE32) { // wave-uniform: no later step holds a lower index
                bad = least;
                break;
            }
            carry = (uint32_t)__builtin_amdgcn_readlane((int)bin, 63);
        }
        if (bad == CHECK_NONE32) { // behind the row's cells: the pads, then the canonical widths
            uint32_t pad = 0;
            if (lane < 8) {
                if (cb + lane < up8(cb)) pad |= rec[cb + lane];
                if (kb + lane < up8(kb)) pad |= kp[kb + lane];
            }
            if (wave_max_u32(wide) != cw || (km && wave_max_u32(gap) <= 256)) bad = n << 8 | LH_KEPT_BAD_ENC_WIDTH;
            if (wave_max_u32(pad) != 0) bad = n << 8 | LH_KEPT_BAD_ENC_PAD; // (the lower cause code last)
        }
    }
    const u64 total = readlane_u64(wave_scan_incl_u64(cnt), 63);
    if (lane == 0) {
        row_count[m] = total;
        if (bad != CHECK_NONE32) atomicMin(verdict, (u64)m << 32 | bad);
    }
}
static_assert(LH_KEPT_BAD_KEY_ORDER < LH_KEPT_BAD_ZERO_COUNT && LH_KEPT_BAD_ZERO_COUNT < LH_KEPT_BAD_ENC_KEY_RANGE &&
                  LH_KEPT_BAD_ENC_KEY_RANGE < LH_KEPT_BAD_ENC_PAD && LH_KEPT_BAD_ENC_PAD < LH_KEPT_BAD_ENC_WIDTH &&
                  LH_KEPT_BAD_ENC_TOTALS < LH_KEPT_BAD_ENC_PAD && LH_KEPT_BAD_ENC_WIDTH < 256,
              "k_dec_fill assigns a cell's and a row's causes in descending order of their codes; a cause is the low byte");

// ---- host side------------------------------------------------------------------------------------------------------------
// behind a device-form call's kernel (or lh_kept_hold's caller's work); `users` handles point to it
struct CallEvent {
    hipEvent_t ev = nullptr;
    size_t users = 0;
    u64 waited_in = 0;         // the last hold() that made its stream wait for it
    CallEvent *next = nullptr; // in the pool
};
// Per-device state of this unit (device_ctx<KeptCtx>).  `mu` is held for the length of a call -- lh_keep's and the host
// forms' waits included -- and by lh_kept_release: it also guards the handles' events and their pool.
struct KeptCtx {
    std::mutex mu;
    double *d_table = nullptr; // D[LH_NKEYS]
    u64 *d_tmp = nullptr;      // lh_keep: offsets[nrows + 1] | row_count[nrows] | the two totals
    size_t tmp_cap = 0;
    u64 *h_totals = nullptr;   // pinned
    size_t totals_cap = 0;
    unsigned char *d_enc = nullptr; // lh_kept_encode* / lh_kept_decode*: an encoded blob where the caller's memory cannot take the kernels
    size_t enc_cap = 0;
    ResultBlocks res;          // host forms
    IdBlocks ids;              // host form of lh_kept_across_ids; lh_kept_gather's map and lh_kept_group's CSR, staged the same way
    uint32_t *d_map_t = nullptr; // lh_kept_gather*: the map transposed (the measurement switch's route only)
    size_t map_t_cap = 0;
    DoubleBlocks bounds;       // host forms of lh_kept_slo* / lh_kept_burn*: the per-entry bounds (and budgets), staged as the ids are
    CallEvent *pool = nullptr; // events no handle points to
    u64 holds = 0;
    SelectState sel;           // lh_kept_top* / lh_kept_movers*: ONE records block, sized for the kind with more fields (calls take
                               // turns under mu), its guard, and the host forms' landing block
};
std::atomic<uint32_t> g_wave_from{KEPT_WAVE_FROM_DEFAULT};
// lh_kept_gather* of ONE handle: the direct route (profiles/kept_gather.txt has it beside the tile route)
constexpr uint32_t GATHER_ROUTE_DEFAULT = LH_TOOL_GATHER_DIRECT;
std::atomic<uint32_t> g_gather_route{LH_TOOL_GATHER_DEFAULT};

} // namespace

struct lh_kept {
    int device = -1;
    uint32_t first = 0, nrows = 0;
    u64 cells = 0, samples = 0, bytes = 0;
    u64 *block = nullptr; // offsets | row_count | counts | keys
    KeptCtx *cx = nullptr; // its device's
    CallEvent *busy = nullptr; // behind every enqueued reader of the block so far, or null (under cx->mu)
    const u64 *offsets() const { return block; }
    const u64 *row_count() const { return block + (size_t)nrows + 1; }
    const u64 *counts() const { return row_count() + nrows; }
    const int16_t *keys() const { return reinterpret_cast<const int16_t *>(counts() + cells); }
};

namespace {

typedef lh::beside::Source<KeptCtx> KeptSource;

// The launch of every kernel k<[IDS,] NW> of this unit that walks M rows of a list: f(sh, nw) launches k<decltype(nw)::value>
// with sh's grid and block -- the shape the unit's switch gives a call of M rows, NW = 1 (a wave per row) or WG_WAVES (a
// workgroup per row).  With by_id, for the readers that have id forms: f(sh, ids, nw), IDS = decltype(ids)::value.
template <class F> int launch_shape(const RowShape &sh, F f)
{
    if (sh.wave) f(sh, std::integral_constant<int, 1>());
    else f(sh, std::integral_constant<int, WG_WAVES>());
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}
template <class F> int launch_rows(uint32_t M, F f) { return launch_shape(row_shape(M, g_wave_from.load(std::memory_order_relaxed)), f); }
template <class F> int launch_rows(uint32_t M, bool by_id, F f)
{
    if (by_id) return launch_rows(M, [&](const RowShape &sh, auto nw) { f(sh, std::true_type(), nw); });
    return launch_rows(M, [&](const RowShape &sh, auto nw) { f(sh, std::false_type(), nw); });
}
// The launch of k_kept_series / k_kept_heat, M rows in each of nwin windows: the rows' grid with a window per blockIdx.y.  The
// switch takes the ENTRIES, nwin * M: twenty ids in sixty windows are 1 200 rows' worth of work, not twenty.
template <class F> int launch_windows(uint32_t M, uint32_t nwin, bool by_id, F f)
{
    const bool wave = (u64)M * nwin >= g_wave_from.load(std::memory_order_relaxed);
    const RowShape sh = {wave, dim3(wave ? (M + ROW_WAVES - 1) / ROW_WAVES : M, nwin), dim3(wave ? ROW_BLOCK : WG)};
    if (by_id) return launch_shape(sh, [&](const RowShape &shape, auto nw) { f(shape, std::true_type(), nw); });
    return launch_shape(sh, [&](const RowShape &shape, auto nw) { f(shape, std::false_type(), nw); });
}

// (cx->mu held, the device current)  The making of a handle of rows [first, first + nrows) on `st`, for lh_keep and
// lh_kept_merge: count(off, row_count, slot) enqueues the pass that leaves nnz in off[1 ..] and the rows' sums; then the scan, the
// totals brought back, the allocation; fill(off, keys, counts) enqueues the pass that places the cells -- unless there are
// none; both return a code.  Returns when the handle is complete.  After a failure the caller waits for `st` and frees k->block.
// verdict (lh_kept_slide; null for the others, whose copies and launches are what they were): a slot right behind the two totals
// starts as SLIDE_CLEAN, count(off, row_count, slot) may fold a refusal into it, and it comes back WITH the totals into *verdict;
// unless it is still clean the call ends there with LH_ERANGE: nothing is allocated and fill is not enqueued.
template <class Count, class Fill>
int make(KeptCtx *cx, hipStream_t st, uint32_t first, uint32_t nrows, lh_kept *k, Count count, Fill fill, u64 *verdict = nullptr)
{
    const size_t head = 2 * (size_t)nrows + 1; // offsets and row_count, in uint64
    const size_t back = verdict ? 3 : 2;       // what comes back: the two totals, the verdict
    int rc = grow_device(cx->d_tmp, cx->tmp_cap, head + back, 4096);
    if (!rc) rc = grow_pinned(cx->h_totals, cx->totals_cap, back, back);
    if (rc) return rc;
    u64 *off = cx->d_tmp, *row_count = off + nrows + 1, *totals = off + head;
    if (verdict) LH_BESIDE_CHK(hipMemsetAsync(totals + 2, 0xff, sizeof(u64), st)); // SLIDE_CLEAN
    rc = count(off, row_count, verdict ? totals + 2 : nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(WG), 0, st, off, row_count, nrows, totals);
    LH_BESIDE_CHK(hipGetLastError());
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_totals, totals, back * sizeof(u64), hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    if (verdict && (*verdict = cx->h_totals[2]) != SLIDE_CLEAN) return LH_ERANGE;
    const u64 cells = cx->h_totals[0];
    if (cells > (u64)nrows * LH_NKEYS) return LH_EDEVICE; // (never)
    k->first = first;
    k->nrows = nrows;
    k->cells = cells;
    k->samples = cx->h_totals[1];
    k->bytes = head * sizeof(u64) + cells * (sizeof(u64) + sizeof(int16_t));
    LH_BESIDE_CHK(hipMalloc((void **)&k->block, (size_t)k->bytes));
    LH_BESIDE_CHK(hipMemcpyAsync(k->block, off, head * sizeof(u64), hipMemcpyDeviceToDevice, st));
    if (cells) {
        u64 *counts = k->block + head;
        rc = fill(off, reinterpret_cast<int16_t *>(counts + cells), counts);
        if (rc) return rc;
    }
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    return LH_OK;
}

// (cx->mu held, the device current)  lh_keep: from the snapshot's cells, on its stream, a wave per row
int keep(const KeptSource &q, uint32_t first, uint32_t nrows, lh_kept *k)
{
    const hipStream_t st = q.stream;
    const uint32_t *ranges = ranges_from(q, first);
    const dim3 grid((nrows + ROW_WAVES - 1) / ROW_WAVES), block(ROW_BLOCK);
    return make(
        q.cx, st, first, nrows, k,
        [&](u64 *off, u64 *row_count, u64 *) {
            with_cells(q, first, [&](auto c) {
                hipLaunchKernelGGL((k_keep_count<cell_of<decltype(c)>>), grid, block, 0, st, c, ranges, q.stride, nrows, off, row_count);
            });
            LH_BESIDE_CHK(hipGetLastError());
            return LH_OK;
        },
        [&](const u64 *off, int16_t *keys, u64 *counts) {
            with_cells(q, first, [&](auto c) {
                hipLaunchKernelGGL((k_keep_fill<cell_of<decltype(c)>>), grid, block, 0, st, c, ranges, q.stride, nrows, off, keys, counts);
            });
            LH_BESIDE_CHK(hipGetLastError());
            return LH_OK;
        });
}

// the list as the kernels take it
KeptList list_of(lh_kept *const *kept, size_t nkept)
{
    KeptList s;
    s.n = (uint32_t)nkept;
    for (size_t i = 0; i < LH_MAX_KEPT; i++) {
        const lh_kept *k = i < nkept ? kept[i] : nullptr;
        s.h[i] = KeptRec{k ? (u64)(uintptr_t)k->block : 0, k ? k->cells : 0, k ? k->first : 0, k ? k->nrows : 0};
    }
    return s;
}

// (cx->mu held, the device current)  lh_kept_merge: from the handles' own arrays, on the caller's stream, in the shape the
// reader would take for as many rows
int merge(KeptCtx *cx, lh_kept *const *kept, size_t nkept, uint32_t first, uint32_t nrows, hipStream_t st, lh_kept *k)
{
    const KeptList s = list_of(kept, nkept);
    return make(
        cx, st, first, nrows, k,
        [&](u64 *off, u64 *row_count, u64 *) {
            return launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_merge_count<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, nrows, first, off, row_count);
            });
        },
        [&](const u64 *off, int16_t *keys, u64 *counts) {
            return launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_merge_fill<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, nrows, first, off, keys, counts);
            });
        });
}

// (cx->mu held, the device current)  lh_kept_gather*: the same two passes with the row of handle i taken from the map d_src (device
// memory, nkept * n entries, handle-major).  One handle takes the direct route -- no tile: the lengths, then the rows verbatim --
// unless the measurement switch says otherwise; GATHER_TRANSPOSED first turns the map row-major in a block of the unit's.
int gather(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const uint32_t *d_src, uint32_t n, uint32_t first_out, hipStream_t st,
           lh_kept *k)
{
    const KeptList s = list_of(kept, nkept);
    uint32_t route = g_gather_route.load(std::memory_order_relaxed);
    if (route == LH_TOOL_GATHER_DEFAULT) route = GATHER_ROUTE_DEFAULT;
    if (route == LH_TOOL_GATHER_DIRECT && nkept == 1) {
        const KeptRec h = s.h[0];
        return make(
            cx, st, first_out, n, k,
            [&](u64 *off, u64 *row_count, u64 *) {
                hipLaunchKernelGGL(k_gather1_count, dim3((unsigned)(((u64)n + ROW_BLOCK - 1) / ROW_BLOCK)), dim3(ROW_BLOCK), 0, st, h, n, d_src, off, row_count);
                LH_BESIDE_CHK(hipGetLastError());
                return LH_OK;
            },
            [&](const u64 *off, int16_t *keys, u64 *counts) {
                return launch_rows(n, [&](const RowShape &sh, auto nw) {
                    hipLaunchKernelGGL((k_gather1_fill<decltype(nw)::value>), sh.grid, sh.block, 0, st, h, n, d_src, off, keys, counts);
                });
            });
    }
    const bool transposed = route == LH_TOOL_GATHER_TRANSPOSED;
    if (transposed) {
        const size_t entries = nkept * (size_t)n;
        const int rc = grow_device(cx->d_map_t, cx->map_t_cap, entries, 1024);
        if (rc) return rc;
        hipLaunchKernelGGL(k_gather_transpose, dim3((unsigned)((entries + ROW_BLOCK - 1) / ROW_BLOCK)), dim3(ROW_BLOCK), 0, st, d_src, n,
                           (uint32_t)nkept, cx->d_map_t);
        LH_BESIDE_CHK(hipGetLastError());
        d_src = cx->d_map_t;
    }
    return make(
        cx, st, first_out, n, k,
        [&](u64 *off, u64 *row_count, u64 *) {
            return launch_rows(n, [&](const RowShape &sh, auto nw) {
                constexpr int NW = decltype(nw)::value;
                if (transposed) hipLaunchKernelGGL((k_gather_count<NW, true>), sh.grid, sh.block, 0, st, s, n, d_src, off, row_count);
                else hipLaunchKernelGGL((k_gather_count<NW, false>), sh.grid, sh.block, 0, st, s, n, d_src, off, row_count);
            });
        },
        [&](const u64 *off, int16_t *keys, u64 *counts) {
            return launch_rows(n, [&](const RowShape &sh, auto nw) {
                constexpr int NW = decltype(nw)::value;
                if (transposed) hipLaunchKernelGGL((k_gather_fill<NW, true>), sh.grid, sh.block, 0, st, s, n, d_src, off, keys, counts);
                else hipLaunchKernelGGL((k_gather_fill<NW, false>), sh.grid, sh.block, 0, st, s, n, d_src, off, keys, counts);
            });
        });
}

// (cx->mu held, the device current)  lh_kept_group*: the same two passes with the rows of output row m taken from the CSR d_goff /
// d_members (device memory: ngroups + 1 and nmembers entries), for every handle of the list; the shape by the call's output rows.
int group(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const u64 *d_goff, const uint32_t *d_members, u64 nmembers, uint32_t ngroups,
          uint32_t first_out, hipStream_t st, lh_kept *k)
{
    const KeptList s = list_of(kept, nkept);
    return make(
        cx, st, first_out, ngroups, k,
        [&](u64 *off, u64 *row_count, u64 *) {
            return launch_rows(ngroups, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_group_count<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, ngroups, d_goff, d_members, nmembers, off,
                                   row_count);
            });
        },
        [&](const u64 *off, int16_t *keys, u64 *counts) {
            return launch_rows(ngroups, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_group_fill<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, ngroups, d_goff, d_members, nmembers, off,
                                   keys, counts);
            });
        });
}

// (cx->mu held)  The host form's CSR on its way to the kernels, through the id list's two blocks (IdBlocks, 4-byte words): goff's
// ngroups + 1 entries first (two words each; the blocks are aligned for them), the members behind them, copied into the pinned block
// before this returns and from there into HBM by ONE copy on `st`, ahead of the kernels.  The call waits for `st` before it returns.
int stage_groups(IdBlocks &b, const u64 *goff, const uint32_t *members, size_t nmembers, size_t ngroups, hipStream_t st, const u64 *&d_goff,
                 const uint32_t *&d_members)
{
    const size_t head = 2 * (ngroups + 1), words = head + nmembers;
    int rc = grow_pinned(b.h_ids, b.h_cap, words, 1024);
    if (!rc) rc = grow_device(b.d_ids, b.d_cap, words, 1024);
    if (rc) return rc;
    std::memcpy(b.h_ids, goff, head * sizeof(uint32_t));
    if (nmembers) std::memcpy(b.h_ids + head, members, nmembers * sizeof(uint32_t));
    LH_BESIDE_CHK(hipMemcpyAsync(b.d_ids, b.h_ids, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    d_goff = reinterpret_cast<const u64 *>(b.d_ids);
    d_members = b.d_ids + head;
    return LH_OK;
}

// (cx->mu held, the device current)  lh_kept_slide: the same with all[0 .. nadd) added and all[nadd .. n) taken away.  *verdict:
// SLIDE_CLEAN, or row << 16 | bin of the first cell that would go below zero (LH_ERANGE then, k->block still null).
int slide(KeptCtx *cx, lh_kept *const *all, size_t n, size_t nadd, uint32_t first, uint32_t nrows, hipStream_t st, lh_kept *k,
          u64 *verdict)
{
    const KeptList s = list_of(all, n);
    const uint32_t NA = (uint32_t)nadd;
    return make(
        cx, st, first, nrows, k,
        [&](u64 *off, u64 *row_count, u64 *slot) {
            return launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_slide_count<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NA, nrows, first, off, row_count, slot);
            });
        },
        [&](const u64 *off, int16_t *keys, u64 *counts) {
            return launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_slide_fill<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NA, nrows, first, off, keys, counts);
            });
        },
        verdict);
}

// What lh_kept_merge and lh_kept_slide do around their making of a handle, work(cx, st, k), once the handles of the list have
// been looked at: the unit's context on their device, a new handle, the mutex for the WHOLE call -- no lh_kept_release frees an
// input under it (they are only read: no hold) --, and after a failure the stream waited for, the block freed, *out untouched.
template <class Work> int born_of(int device, void *stream, lh_kept **out, Work work)
{
    KeptCtx *cx = device_ctx<KeptCtx>(device);
    if (!cx) return LH_EDEVICE;
    lh_kept *k = new (std::nothrow) lh_kept;
    if (!k) return LH_ENOMEM;
    k->device = device;
    k->cx = cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    {
        std::lock_guard<std::mutex> g(cx->mu);
        rc = hipSetDevice(device) == hipSuccess ? work(cx, st, k) : LH_EDEVICE;
        if (rc) {
            (void)hipGetLastError();
            if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
            if (k->block && hipFree(k->block) != hipSuccess) (void)hipGetLastError();
        }
    }
    if (rc) {
        delete k;
        return rc;
    }
    *out = k;
    return LH_OK;
}

// (cx->mu held) one user less of `e`
void unuse(KeptCtx *cx, CallEvent *e)
{
    if (e && --e->users == 0) {
        e->next = cx->pool;
        cx->pool = e;
    }
}

// (cx->mu held, the device current) what is enqueued on `st` by now reads the blocks of kept[0 .. nkept): one event behind
// it AND behind every earlier reader of these handles, to which they all point from here on.  After a failure the handles are
// as they were, and the caller waits for `st` on the host.
int hold(KeptCtx *cx, lh_kept *const *kept, size_t nkept, hipStream_t st)
{
    CallEvent *e = cx->pool;
    if (e) {
        cx->pool = e->next;
    } else {
        e = new (std::nothrow) CallEvent;
        if (!e) return LH_ENOMEM;
        const hipError_t err = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            delete e;
            return err == hipErrorOutOfMemory ? LH_ENOMEM : LH_EDEVICE;
        }
    }
    const u64 now = ++cx->holds;
    hipError_t err = hipSuccess;
    for (size_t i = 0; i < nkept && err == hipSuccess; i++) {
        CallEvent *was = kept[i]->busy;
        if (was && was->waited_in != now) {
            was->waited_in = now;
            err = hipStreamWaitEvent(st, was->ev, 0);
        }
    }
    if (err == hipSuccess) err = hipEventRecord(e->ev, st);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        e->next = cx->pool;
        cx->pool = e;
        return LH_EDEVICE;
    }
    for (size_t i = 0; i < nkept; i++)
        if (kept[i]->busy != e) { // (a handle listed twice: once)
            unuse(cx, kept[i]->busy);
            kept[i]->busy = e;
            e->users++;
        }
    return LH_OK;
}

// ---- what the readers of a list share behind their own argument checks --------------------------------------------------------
// The two checks that look at the handles.  LH_ERANGE unless every row asked for lies inside EVERY handle's block: the rows
// they all have are [lo, end).  (A device id list is not looked at: the kernels give a row outside a block the empty entry.)
int rows_in_all(lh_kept *const *kept, size_t nkept, const RowSel &sel, size_t nmetrics)
{
    u64 lo = 0, end = ~0ull;
    for (size_t i = 0; i < nkept; i++) {
        const u64 f = kept[i]->first, e = f + kept[i]->nrows;
        lo = f > lo ? f : lo;
        end = e < end ? e : end;
    }
    if (!sel.by_id) {
        if (sel.first < lo || (u64)sel.first + nmetrics > end) return LH_ERANGE;
    } else if (!sel.on_device) {
        for (size_t m = 0; m < nmetrics; m++)
            if (sel.ids[m] < lo || sel.ids[m] >= end) return LH_ERANGE;
    }
    return LH_OK;
}
// LH_EINVAL unless all handles are on one device, which *device then names
int one_device(lh_kept *const *kept, size_t nkept, int *device)
{
    *device = kept[nkept - 1]->device;
    for (size_t i = 0; i + 1 < nkept; i++)
        if (kept[i]->device != *device) return LH_EINVAL;
    return LH_OK;
}
// lh_kept_slide's checks, in the documented order, into `all` (add first): those that need no handle, then the two that look
// at them (one_device, rows_in_all)
int check_slide(lh_kept *const *add, size_t nadd, lh_kept *const *sub, size_t nsub, uint32_t first, size_t nmetrics, uint32_t flags,
                const lh_kept_under *why, const void *out, lh_kept *(&all)[LH_MAX_KEPT], int *device)
{
    if (bad_list(add, nadd, LH_MAX_KEPT) || (nsub != 0 && bad_list(sub, nsub, LH_MAX_KEPT)) || nadd + nsub > LH_MAX_KEPT) return LH_EINVAL;
    if (flags != 0 || !out || (why && why->struct_size != sizeof(lh_kept_under)) || nmetrics == 0) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE;
    std::copy(add, add + nadd, all);
    if (nsub) std::copy(sub, sub + nsub, all + nadd);
    const int rc = one_device(all, nadd + nsub, device);
    return rc ? rc : rows_in_all(all, nadd + nsub, rows_from(first), nmetrics);
}

// The order of those two checks is documented per entry point and differs: lh_kept_across*, lh_kept_count_le* and lh_kept_spread*
// look at the rows first; their window forms, lh_kept_compare*, lh_kept_drift* and the selecting readers at the devices first.
enum HandleChecks { ROWS_THEN_DEVICE, DEVICE_THEN_ROWS };

// The way of a call once its own arguments are checked and it is not empty: the two checks that look at the handles, in the
// caller's order -- the rows inside EVERY listed handle's block, whether or not a window names it --, then the unit's context on
// the handles' device, its mutex for the length of the call, the device made current.  A device form's work -- direct(cx, st)
// enqueues it on the caller's stream -- goes under ONE hold of all listed handles; a host form's -- through(cx, st) brings the
// results back to the caller's arrays and waits -- leaves nothing of the call under way, after a failure either.
template <class Direct, class Through>
int run(lh_kept *const *kept, size_t nkept, HandleChecks order, const RowSel &sel, size_t nmetrics, void *stream, bool device_form,
        Direct direct, Through through)
{
    int device = -1;
    int rc = order == ROWS_THEN_DEVICE ? rows_in_all(kept, nkept, sel, nmetrics) : one_device(kept, nkept, &device);
    if (!rc) rc = order == ROWS_THEN_DEVICE ? one_device(kept, nkept, &device) : rows_in_all(kept, nkept, sel, nmetrics);
    if (rc) return rc;
    KeptCtx *cx = device_ctx<KeptCtx>(device);
    if (!cx) return LH_EDEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> g(cx->mu);
    LH_BESIDE_CHK(hipSetDevice(device));
    if (device_form) {
        rc = direct(cx, st);
        if (rc) return rc;
        rc = hold(cx, kept, nkept, st);
        // what was enqueued reads handles that no event guards: wait here
        if (rc && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
        return rc;
    }
    rc = through(cx, st);
    if (rc && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError(); // nothing of this call is under way afterwards
    return rc;
}

// ---- the four per-name readers, each with its per-window form: ONE front end and ONE enqueue a family ----------------------------
// The windows a front end was given: none for the whole-list forms (lh_kept_across*, lh_kept_count_le*, lh_kept_spread*,
// lh_kept_compare*), else win[0 .. n) as the caller passed them, still to be checked.  A window form differs from its parent in
// four places only: the windows' term in the first LH_EINVAL test, the launch (launch_windows, the switch on n * M entries), the
// entries a host form brings back, and the order of the two handle checks.
struct Windows {
    bool given;
    const uint32_t *win;
    size_t n;
    size_t entries(size_t nmetrics) const { return given ? n * nmetrics : nmetrics; }
};
constexpr Windows WHOLE_LIST = {false, nullptr, 0};

// unless `win` holds nwin windows [lo, hi) of a list of nkept handles, 1 .. LH_MAX_WINDOWS of them, each with 0 <= lo < hi <= nkept
bool bad_windows(const uint32_t *win, size_t nwin, size_t nkept)
{
    if (!win || misaligned(win, 4) || nwin == 0 || nwin > LH_MAX_WINDOWS) return true;
    for (size_t w = 0; w < nwin; w++)
        if (win[2 * w] >= win[2 * w + 1] || win[2 * w + 1] > nkept) return true;
    return false;
}
// the windows as the kernels take them (bad_windows came first: every end fits a byte)
KeptWindows windows_of(const uint32_t *win, size_t nwin)
{
    KeptWindows sw;
    for (size_t w = 0; w < LH_MAX_WINDOWS; w++) {
        sw.w[w][0] = w < nwin ? (uint8_t)win[2 * w] : 0;
        sw.w[w][1] = w < nwin ? (uint8_t)win[2 * w + 1] : 0;
    }
    return sw;
}
// the bounds as the kernels take them
KeptBounds bounds_of(const double *bounds, size_t nb)
{
    KeptBounds sb;
    for (size_t j = 0; j < LH_MAX_BOUNDS; j++) sb.b[j] = j < nb ? bounds[j] : 0.0;
    return sb;
}

// ---- lh_kept_across* / lh_kept_series*
// (cx->mu held, the device current) the walks of rows [first, first + nmetrics), or of rows ids[0 .. nmetrics), on `st`: over the
// whole list, or in every window
int enqueue_across(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics,
                   const double *p, size_t np, const KeptOut &o, hipStream_t st)
{
    int rc = ensure_table(cx->d_table, st, lh::k_value_table<KeptCtx>);
    const uint32_t *ids = nullptr;
    if (!rc) rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (rc) return rc;
    const PctArgs pa = pct_args(p, np);
    const KeptList s = list_of(kept, nkept);
    const uint32_t M = (uint32_t)nmetrics, NP = (uint32_t)np;
    const double *D = cx->d_table;
    if (!w.given)
        return launch_rows(M, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
            hipLaunchKernelGGL((k_kept_across<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, M, sel.first, D,
                               pa, NP, o, ids);
        });
    const KeptWindows sw = windows_of(w.win, w.n);
    return launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
        hipLaunchKernelGGL((k_kept_series<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, sel.first, D,
                           pa, NP, o, ids);
    });
}

int kept_across(lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const double *p, size_t np,
                uint32_t flags, void *stream, KeptOut o, bool device_form)
{
    // every cause of LH_EINVAL, the windows' among them, ahead of the early LH_ERANGE (check_list_args' last)
    if (bad_ids(sel, nmetrics) || bad_list(kept, nkept, LH_MAX_KEPT) || (w.given && bad_windows(w.win, w.n, nkept))) return LH_EINVAL;
    const int rc = check_list_args(kept, nkept, LH_MAX_KEPT, sel, nmetrics, p, np, flags, o);
    if (rc) return rc;
    if (nmetrics == 0) return LH_OK; // before any handle is looked at
    const auto work = [&](KeptCtx *cx, hipStream_t st, const KeptOut &d) {
        return enqueue_across(cx, kept, nkept, w, sel, nmetrics, p, np, d, st);
    };
    return run(
        kept, nkept, w.given ? DEVICE_THEN_ROWS : ROWS_THEN_DEVICE, sel, nmetrics, stream, device_form,
        [&](KeptCtx *cx, hipStream_t st) { return work(cx, st, o); },
        [&](KeptCtx *cx, hipStream_t st) { // results to HBM, then back to the caller's arrays
            return list_host_results(cx->res, st, o, w.entries(nmetrics), np, [&](const KeptOut &d) { return work(cx, st, d); });
        });
}

// ---- lh_kept_count_le* / lh_kept_heat*
// (cx->mu held, the device current) the same walks with the bounds in the percentiles' place
int enqueue_count_le(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics,
                     const double *bounds, size_t nb, u64 *d_cum, u64 *d_total, hipStream_t st)
{
    const uint32_t *ids = nullptr;
    const int rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (rc) return rc;
    const KeptBounds sb = bounds_of(bounds, nb);
    const KeptList s = list_of(kept, nkept);
    const uint32_t M = (uint32_t)nmetrics, NB = (uint32_t)nb;
    if (!w.given)
        return launch_rows(M, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
            hipLaunchKernelGGL((k_kept_count_le<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, M, sel.first,
                               sb, NB, d_cum, d_total, ids);
        });
    const KeptWindows sw = windows_of(w.win, w.n);
    return launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
        hipLaunchKernelGGL((k_kept_heat<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, sel.first, sb,
                           NB, d_cum, d_total, ids);
    });
}

// lh_count_le's rules for the bounds, the two outputs and the flags.  The bounds are one row shared by all names
// (LH_LE_PER_METRIC is refused with every other flag), so every cause is an LH_EINVAL that needs no handle.
bool bad_count_le_args(const double *bounds, size_t nb, const uint64_t *cum, const uint64_t *total, uint32_t flags)
{
    if (nb == 0 || nb > LH_MAX_BOUNDS || !bounds || (!cum && !total) || flags != 0) return true;
    if (misaligned(bounds, 8) || misaligned(cum, 8) || misaligned(total, 8)) return true;
    return bad_bounds(bounds, nb);
}

int kept_count_le(lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const double *bounds,
                  size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total, bool device_form)
{
    // ---- every check that needs neither a handle nor a device: lh_count_le's, with the list in the snapshot's place
    if (bad_ids(sel, nmetrics) || bad_list(kept, nkept, LH_MAX_KEPT) || (w.given && bad_windows(w.win, w.n, nkept))) return LH_EINVAL;
    if (bad_count_le_args(bounds, nb, cum, total, flags)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    if (nmetrics == 0) return LH_OK;              // before any handle is looked at
    const size_t entries = w.entries(nmetrics);
    const auto work = [&](KeptCtx *cx, hipStream_t st, void *d_cum, void *d_total) {
        return enqueue_count_le(cx, kept, nkept, w, sel, nmetrics, bounds, nb, static_cast<u64 *>(d_cum), static_cast<u64 *>(d_total), st);
    };
    return run(
        kept, nkept, w.given ? DEVICE_THEN_ROWS : ROWS_THEN_DEVICE, sel, nmetrics, stream, device_form,
        [&](KeptCtx *cx, hipStream_t st) { return work(cx, st, cum, total); },
        [&](KeptCtx *cx, hipStream_t st) { // results to HBM, then back to the caller's arrays
            const HostOut out[2] = {{cum, entries * nb * sizeof(u64)}, {total, entries * sizeof(u64)}};
            return host_results(cx->res, st, out, [&](unsigned char *const(&dev)[2]) { return work(cx, st, dev[0], dev[1]); });
        });
}

// ---- lh_kept_slo* / lh_kept_burn*: lh_kept_heat* with bounds PER ENTRY, and the alert over them.  Per-window forms only (the whole
// list is the one window [0, nkept)), so `w` is always given.  The per-entry arrays are the ids' kind of argument: a host form's are
// checked here and staged on the call's stream (stage_doubles), a device form's are the caller's own device arrays, which the host
// never sees and the kernels take as any bytes.
// (cx->mu held, the device current)  what the kernels read for a[0 .. na) and b[0 .. nb)
int entry_doubles(KeptCtx *cx, bool device_form, const double *a, size_t na, const double *b, size_t nb, hipStream_t st,
                  const double *&d_a, const double *&d_b)
{
    if (!device_form) return stage_doubles(cx->bounds, a, na, b, nb, st, d_a, d_b);
    d_a = a;
    d_b = b;
    return LH_OK;
}

// (cx->mu held, the device current) enqueue_count_le's per-window walks with row m of `bounds` for entry m
int enqueue_slo(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics,
                const double *bounds, size_t nb, bool device_form, u64 *d_cum, u64 *d_total, hipStream_t st)
{
    const uint32_t *ids = nullptr;
    const double *rows = nullptr, *none = nullptr;
    int rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (!rc) rc = entry_doubles(cx, device_form, bounds, nmetrics * nb, nullptr, 0, st, rows, none);
    if (rc) return rc;
    const KeptList s = list_of(kept, nkept);
    const KeptWindows sw = windows_of(w.win, w.n);
    const uint32_t M = (uint32_t)nmetrics, NB = (uint32_t)nb;
    return launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
        hipLaunchKernelGGL((k_kept_slo<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, sel.first, rows,
                           NB, d_cum, d_total, ids);
    });
}

int kept_slo(lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const double *bounds, size_t nb,
             uint32_t flags, void *stream, uint64_t *cum, uint64_t *total, bool device_form)
{
    // ---- every check that needs neither a handle nor a device, lh_kept_heat*'s in its order
    if (bad_ids(sel, nmetrics) || bad_list(kept, nkept, LH_MAX_KEPT) || bad_windows(w.win, w.n, nkept)) return LH_EINVAL;
    if (nb == 0 || nb > LH_MAX_BOUNDS || !bounds || (!cum && !total) || flags != 0) return LH_EINVAL;
    if (misaligned(bounds, 8) || misaligned(cum, 8) || misaligned(total, 8)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32): not a row of bounds is read (as lh_count_le)
    if (nmetrics == 0) return LH_OK;              // before any handle is looked at
    if (!device_form)                             // a host array's rows, each by lh_count_le's rule, still before any handle
        for (size_t m = 0; m < nmetrics; m++)
            if (bad_bounds(bounds + m * nb, nb)) return LH_EINVAL;
    const size_t entries = w.entries(nmetrics);
    const auto work = [&](KeptCtx *cx, hipStream_t st, void *d_cum, void *d_total) {
        return enqueue_slo(cx, kept, nkept, w, sel, nmetrics, bounds, nb, device_form, static_cast<u64 *>(d_cum),
                           static_cast<u64 *>(d_total), st);
    };
    return run(
        kept, nkept, DEVICE_THEN_ROWS, sel, nmetrics, stream, device_form,
        [&](KeptCtx *cx, hipStream_t st) { return work(cx, st, cum, total); },
        [&](KeptCtx *cx, hipStream_t st) { // results to HBM, then back to the caller's arrays; the wait frees the staged bounds too
            const HostOut out[2] = {{cum, entries * nb * sizeof(u64)}, {total, entries * sizeof(u64)}};
            return host_results(cx->res, st, out, [&](unsigned char *const(&dev)[2]) { return work(cx, st, dev[0], dev[1]); });
        });
}

// What an lh_kept_burn* call is given beside its list, windows and rows; the four outputs are the caller's (a device form's: device
// pointers) or, handed to enqueue_burn by the host form, places in the unit's result block.
struct BurnCall {
    const double *rate, *bounds, *budget;
    size_t k;
    lh_burn_hit *out;
    uint64_t *n_out, *cum, *total;
};

// (cx->mu held, the device current)  Both passes on `st`: the n words "windows in which entry m did not fire" come from SelectState's
// guarded block (asked for in records of the movers' five fields, as every user of the block asks) and are zeroed on `st`; the
// score pass, one window per blockIdx.y in the reader's two shapes; one ordered workgroup that writes the records and the count;
// the guard's event behind it, after a failure too.
int enqueue_burn(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const BurnCall &c,
                 bool device_form, hipStream_t st)
{
    const uint32_t *ids = nullptr;
    const double *bounds = nullptr, *budget = nullptr;
    u64 *base = nullptr;
    size_t npad = 0;
    int rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (!rc) rc = entry_doubles(cx, device_form, c.bounds, nmetrics, c.budget, nmetrics, st, bounds, budget);
    const size_t words_per_record = MOVERS_FIELDS * sizeof(u64) / sizeof(uint32_t);
    if (!rc) rc = select_records(cx->sel, st, (nmetrics + words_per_record - 1) / words_per_record, MOVERS_FIELDS, base, npad);
    if (rc) return rc;
    uint32_t *miss = reinterpret_cast<uint32_t *>(base);
    const KeptList s = list_of(kept, nkept);
    const KeptWindows sw = windows_of(w.win, w.n);
    KeptRates rates;
    for (size_t i = 0; i < LH_MAX_WINDOWS; i++) rates.r[i] = i < w.n ? c.rate[i] : 0.0;
    const uint32_t M = (uint32_t)nmetrics;
    const u64 K = c.k;
    u64 *d_cum = reinterpret_cast<u64 *>(c.cum), *d_total = reinterpret_cast<u64 *>(c.total), *d_n_out = reinterpret_cast<u64 *>(c.n_out);
    rc = hipMemsetAsync(miss, 0, nmetrics * sizeof(uint32_t), st) == hipSuccess ? LH_OK : LH_EDEVICE;
    if (!rc)
        rc = launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
            hipLaunchKernelGGL((k_kept_burn_score<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, rates, M,
                               sel.first, bounds, budget, d_cum, d_total, ids, miss);
        });
    if (!rc) {
        if (sel.by_id) hipLaunchKernelGGL(k_kept_burn_emit<true>, dim3(1), dim3(WG), 0, st, miss, M, sel.first, ids, K, c.out, d_n_out);
        else hipLaunchKernelGGL(k_kept_burn_emit<false>, dim3(1), dim3(WG), 0, st, miss, M, sel.first, ids, K, c.out, d_n_out);
        if (hipGetLastError() != hipSuccess) rc = LH_EDEVICE;
    }
    if (rc == LH_EDEVICE) (void)hipGetLastError();
    const int rg = cx->sel.guard.record(st); // what was enqueued uses the block
    return rc ? rc : rg;
}

int kept_burn(lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const BurnCall &c, uint32_t flags,
              void *stream, bool device_form)
{
    // ---- every check that needs neither a handle nor a device: the ids', the list's and the windows' as lh_kept_heat* has them
    if (bad_ids(sel, nmetrics) || bad_list(kept, nkept, LH_MAX_KEPT) || bad_windows(w.win, w.n, nkept)) return LH_EINVAL;
    if (flags != 0 || !c.rate || !c.bounds || !c.budget || !c.n_out || (c.k > 0 && !c.out)) return LH_EINVAL;
    if (misaligned(c.rate, 8) || misaligned(c.bounds, 8) || misaligned(c.budget, 8) || misaligned(c.out, 4) || misaligned(c.n_out, 8) ||
        misaligned(c.cum, 8) || misaligned(c.total, 8))
        return LH_EINVAL;
    for (size_t i = 0; i < w.n; i++)
        if (!(c.rate[i] >= 0.0)) return LH_EINVAL; // a NaN too
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32): not a bound or a budget is read
    if (nmetrics == 0) return LH_OK;              // before any handle is looked at; nothing is written
    if (!device_form)                             // the host arrays, still before any handle
        for (size_t m = 0; m < nmetrics; m++)
            if (!(c.budget[m] >= 0.0) || c.bounds[m] != c.bounds[m]) return LH_EINVAL;
    return run(
        kept, nkept, DEVICE_THEN_ROWS, sel, nmetrics, stream, device_form,
        [&](KeptCtx *cx, hipStream_t st) { return enqueue_burn(cx, kept, nkept, w, sel, nmetrics, c, true, st); },
        [&](KeptCtx *cx, hipStream_t st) -> int {
            // the count and the records that can be written, min(k, n), lie first in the result block and come back in ONE copy with
            // whatever of cum / total was asked for; the first min(*n_out, k) records go on to the caller
            const size_t kk = std::min(c.k, nmetrics), head = sizeof(u64) + kk * sizeof(lh_burn_hit);
            const size_t block = w.entries(nmetrics) * sizeof(u64), at_total = head + (c.cum ? block : 0);
            const size_t need = at_total + (c.total ? block : 0);
            int rc = select_result_blocks(cx->res, need);
            if (rc) return rc;
            unsigned char *d = cx->res.d_res, *h = cx->res.h_res;
            BurnCall dev = c;
            dev.n_out = reinterpret_cast<uint64_t *>(d);
            dev.out = reinterpret_cast<lh_burn_hit *>(d + sizeof(u64));
            dev.cum = c.cum ? reinterpret_cast<uint64_t *>(d + head) : nullptr;
            dev.total = c.total ? reinterpret_cast<uint64_t *>(d + at_total) : nullptr;
            rc = enqueue_burn(cx, kept, nkept, w, sel, nmetrics, dev, false, st);
            if (rc) return rc;
            LH_BESIDE_CHK(hipMemcpyAsync(h, d, need, hipMemcpyDeviceToHost, st));
            LH_BESIDE_CHK(hipStreamSynchronize(st));
            cx->sel.guard.covered(); // this call recorded the event on the stream it has just waited for
            u64 n = 0;
            std::memcpy(&n, h, sizeof n);
            if (n > nmetrics) return LH_ESTATE;
            if (c.out) std::memcpy(c.out, h + sizeof(u64), (size_t)std::min<u64>(n, kk) * sizeof(lh_burn_hit));
            if (c.cum) std::memcpy(c.cum, h + head, block);
            if (c.total) std::memcpy(c.total, h + at_total, block);
            *c.n_out = n;
            return LH_OK;
        });
}

// ---- lh_kept_spread* / lh_kept_spread_series*
// (cx->mu held, the device current) enqueue_across' walks with k_kept_spread / k_kept_spread_series
int enqueue_spread(KeptCtx *cx, lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics,
                   const double *p, size_t np, const SpreadOut &o, hipStream_t st)
{
    int rc = ensure_table(cx->d_table, st, lh::k_value_table<KeptCtx>);
    const uint32_t *ids = nullptr;
    if (!rc) rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (rc) return rc;
    const PctArgs pa = pct_args(p, np);
    const KeptList s = list_of(kept, nkept);
    const uint32_t M = (uint32_t)nmetrics, NP = (uint32_t)np;
    const double *D = cx->d_table;
    if (!w.given)
        return launch_rows(M, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
            hipLaunchKernelGGL((k_kept_spread<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, M, sel.first, D,
                               pa, NP, o, ids);
        });
    const KeptWindows sw = windows_of(w.win, w.n);
    return launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
        hipLaunchKernelGGL((k_kept_spread_series<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M,
                           sel.first, D, pa, NP, o, ids);
    });
}

int kept_spread(lh_kept *const *kept, size_t nkept, const Windows &w, const RowSel &sel, size_t nmetrics, const double *p, size_t np,
                uint32_t flags, void *stream, SpreadOut o, bool device_form)
{
    // ---- every check that needs neither a handle nor a device: lh_spread's, with the list in the snapshot's place
    if (bad_ids(sel, nmetrics) || bad_list(kept, nkept, LH_MAX_KEPT) || (w.given && bad_windows(w.win, w.n, nkept)) || flags != 0)
        return LH_EINVAL;
    const int rc = check_spread_args(p, np, o);
    if (rc) return rc;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    if (nmetrics == 0) return LH_OK;              // before any handle is looked at
    const auto work = [&](KeptCtx *cx, hipStream_t st, const SpreadOut &d) {
        return enqueue_spread(cx, kept, nkept, w, sel, nmetrics, p, np, d, st);
    };
    return run(
        kept, nkept, w.given ? DEVICE_THEN_ROWS : ROWS_THEN_DEVICE, sel, nmetrics, stream, device_form,
        [&](KeptCtx *cx, hipStream_t st) { return work(cx, st, o); },
        [&](KeptCtx *cx, hipStream_t st) { // results to HBM, then back to the caller's arrays
            return spread_host_results(cx->res, st, o, w.entries(nmetrics), np, [&](const SpreadOut &d) { return work(cx, st, d); });
        });
}

// ---- lh_kept_compare* / lh_kept_drift*: ONE list either way -- the parent's two lists joined, base first (join_lists), or
// lh_kept_drift*'s own, of which each window names a pair of slices
// unless `win` holds nwin windows {base_lo, base_hi, cur_lo, cur_hi} of a list of nkept handles, 1 .. LH_MAX_WINDOWS of them, each
// slice with 0 <= lo < hi <= nkept and the two of a window with at most LH_MAX_KEPT handles together (a handle per lane)
bool bad_drift_windows(const uint32_t *win, size_t nwin, size_t nkept)
{
    if (!win || misaligned(win, 4) || nwin == 0 || nwin > LH_MAX_WINDOWS) return true;
    for (size_t w = 0; w < nwin; w++) {
        const uint32_t *q = win + 4 * w;
        if (q[0] >= q[1] || q[1] > nkept || q[2] >= q[3] || q[3] > nkept) return true;
        if ((size_t)(q[1] - q[0]) + (q[3] - q[2]) > LH_MAX_KEPT) return true;
    }
    return false;
}
// the windows as k_kept_drift takes them (bad_drift_windows came first: every end fits a byte)
KeptDriftWindows drift_windows_of(const uint32_t *win, size_t nwin)
{
    KeptDriftWindows sw;
    for (size_t w = 0; w < LH_MAX_WINDOWS; w++)
        for (size_t k = 0; k < 4; k++) sw.w[w][k] = w < nwin ? (uint8_t)win[4 * w + k] : 0;
    return sw;
}

// (cx->mu held, the device current) the walks of rows [first, first + nmetrics), or of rows ids[0 .. nmetrics), on `st`: all[0 ..
// nbase) against all[nbase .. n), or the pair of slices of every window
int enqueue_compare(KeptCtx *cx, lh_kept *const *all, size_t n, size_t nbase, const Windows &w, const RowSel &sel, size_t nmetrics,
                    const CompareOut &o, hipStream_t st)
{
    const uint32_t *ids = nullptr;
    const int rc = stage_ids(cx->ids, sel, nmetrics, st, ids);
    if (rc) return rc;
    const KeptList s = list_of(all, n);
    const uint32_t M = (uint32_t)nmetrics, NB = (uint32_t)nbase;
    if (!w.given)
        return launch_rows(M, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
            hipLaunchKernelGGL((k_kept_compare<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NB, M, sel.first,
                               o, ids);
        });
    const KeptDriftWindows sw = drift_windows_of(w.win, w.n);
    return launch_windows(M, (uint32_t)w.n, sel.by_id, [&](const RowShape &sh, auto by_id, auto nw) {
        hipLaunchKernelGGL((k_kept_drift<decltype(by_id)::value, decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, sel.first, o,
                           ids);
    });
}

// lh_compare's rules for the eight outputs: at least one, each aligned to its type
bool bad_compare_out(const CompareOut &o)
{
    if (!o.count_a && !o.count_b && !o.ks && !o.ks_key && !o.below_a && !o.below_b && !o.w1 && !o.shift) return true;
    return misaligned(o.count_a, 8) || misaligned(o.count_b, 8) || misaligned(o.ks, 8) || misaligned(o.ks_key, 2) ||
           misaligned(o.below_a, 8) || misaligned(o.below_b, 8) || misaligned(o.w1, 8) || misaligned(o.shift, 8);
}

// `all`: null for two lists that join_lists refused
int kept_compare(lh_kept *const *all, size_t n, size_t nbase, const Windows &w, const RowSel &sel, size_t nmetrics, uint32_t flags,
                 void *stream, const CompareOut &o, bool device_form)
{
    // ---- every check that needs neither a handle nor a device
    if (bad_ids(sel, nmetrics) || bad_list(all, n, LH_MAX_KEPT) || (w.given && bad_drift_windows(w.win, w.n, n)) || flags != 0)
        return LH_EINVAL;
    if (bad_compare_out(o)) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE; // beyond any max_metrics (uint32)
    if (nmetrics == 0) return LH_OK;              // before any handle is looked at
    const auto work = [&](KeptCtx *cx, hipStream_t st, const CompareOut &d) {
        return enqueue_compare(cx, all, n, nbase, w, sel, nmetrics, d, st);
    };
    return run(
        all, n, DEVICE_THEN_ROWS, sel, nmetrics, stream, device_form, // (a device form's hold: ALL listed handles, of both lists)
        [&](KeptCtx *cx, hipStream_t st) { return work(cx, st, o); },
        [&](KeptCtx *cx, hipStream_t st) { // results to HBM, then back to the caller's arrays
            return compare_host_results(cx->res, st, o, w.entries(nmetrics), [&](const CompareOut &d) { return work(cx, st, d); });
        });
}

// The two lists of lh_kept_compare* and lh_kept_movers* as ONE, base first (a handle per lane).  False unless each is a list of
// 1 .. LH_MAX_KEPT handles, none of them NULL, and they hold at most LH_MAX_KEPT together.
bool join_lists(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, lh_kept *(&all)[LH_MAX_KEPT])
{
    if (bad_list(base, nbase, LH_MAX_KEPT) || bad_list(cur, ncur, LH_MAX_KEPT) || nbase + ncur > LH_MAX_KEPT) return false;
    std::copy(base, base + nbase, all);
    std::copy(cur, cur + ncur, all + nbase);
    return true;
}
// lh_kept_compare*'s entry into that path
int kept_compare_lists(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, const RowSel &sel, size_t nmetrics,
                       uint32_t flags, void *stream, const CompareOut &o, bool device_form)
{
    lh_kept *all[LH_MAX_KEPT];
    const bool joined = join_lists(base, nbase, cur, ncur, all);
    return kept_compare(joined ? all : nullptr, nbase + ncur, nbase, WHOLE_LIST, sel, nmetrics, flags, stream, o, device_form);
}

// ---- lh_kept_top* / lh_kept_movers*: lh_select.h's host side around this unit's score passes -----------------------------------
// What a selecting call is given beside its list(s); `all` is one list (movers: base first), nbase == 0 for lh_kept_top*.
struct SelectCall {
    lh_kept *all[LH_MAX_KEPT];
    size_t n = 0, nbase = 0;
    uint32_t first = 0, by = 0, flags = 0;
    size_t nmetrics = 0, k = 0;
    double arg = 0.0;
    bool movers = false;
};

// (cx->mu held, the device current) both passes over rows [first, first + nmetrics) on `st`.  ev[0 .. 2] (may be null): events to
// record before the score pass, between the passes and behind the select pass (lh_tool_kept_*_passes_ms).  The records block
// is always asked for with the movers' five fields: a block a top call made also serves a movers call of as many rows.
template <class Entry> int enqueue_select(KeptCtx *cx, const SelectCall &c, hipStream_t st, Entry *d_out, uint32_t *d_n_out, hipEvent_t *ev)
{
    u64 *base = nullptr;
    size_t npad = 0;
    int rc = c.movers ? LH_OK : ensure_table(cx->d_table, st, lh::k_value_table<KeptCtx>);
    if (!rc) rc = select_records(cx->sel, st, c.nmetrics, MOVERS_FIELDS, base, npad);
    if (rc) return rc;
    const KeptList s = list_of(c.all, c.n);
    const uint32_t M = (uint32_t)c.nmetrics;
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[0], st));
    if constexpr (std::is_same<Entry, lh_top_entry>::value) {
        const TopRecords r = top_records(base, npad);
        const u64 flip = (c.flags & LH_TOP_ASCENDING) ? ~0ull : 0ull;
        const double *D = cx->d_table;
        rc = launch_rows(M, [&](const RowShape &sh, auto nw) {
            hipLaunchKernelGGL((k_kept_top_score<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, M, c.first, D, c.by, c.arg, flip, r);
        });
        if (rc) return rc;
        return select_pass(cx->sel, st, r.key, r.count, M, c.k, TopEmit{r, c.first, c.by, d_out}, d_n_out, ev);
    } else {
        const MoversRecords r = movers_records(base, npad);
        const u64 flip = (c.flags & LH_MOVERS_ASCENDING) ? ~0ull : 0ull;
        const uint32_t NB = (uint32_t)c.nbase;
        rc = launch_rows(M, [&](const RowShape &sh, auto nw) {
            hipLaunchKernelGGL((k_kept_movers_score<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NB, M, c.first, c.by, c.arg, flip, r);
        });
        if (rc) return rc;
        return select_pass(cx->sel, st, r.key, r.cand, M, c.k, MoversEmit{r, c.first, d_out}, d_n_out, ev);
    }
}

// The records block of the per-window forms holds at most this many bytes of records (five fields of 8 bytes each, as always): a
// call runs its two passes over CHUNKS of consecutive windows that fit, never less than one window.  128 windows of 65 536 names
// would be 320 MiB at once; up to 8 192 names a call of any nwin is one chunk, 65 536 names take 25 windows a chunk.
constexpr u64 KEPT_SELECT_BYTES = 64ull << 20;
std::atomic<u64> g_select_bytes{KEPT_SELECT_BYTES};
size_t select_chunk(size_t npad, size_t nwin)
{
    const u64 fit = g_select_bytes.load(std::memory_order_relaxed) / ((u64)npad * MOVERS_FIELDS * sizeof(u64));
    return (size_t)std::min<u64>(std::max<u64>(fit, 1), nwin);
}

// (cx->mu held, the device current)  lh_kept_top_series* / lh_kept_movers_series*: both passes for windows [w0, w0 + wn) of the
// call's nwin on `st`, chunk after chunk -- each chunk's score kernel and k_select_windows get the windows from its first window on,
// its records go to the ONE block (stream order protects it between chunks), its entries to d_out + (w - w0) * k and its counts to
// d_n_out + (w - w0), w its first window -- and the guard's event behind the last select.  ev (may be null; then [w0, w0 + wn) is
// ONE chunk): select_pass' three events.
template <class Entry>
int enqueue_select_windows(KeptCtx *cx, const SelectCall &c, const Windows &w, size_t w0, size_t wn, hipStream_t st, Entry *d_out,
                           uint32_t *d_n_out, hipEvent_t *ev)
{
    const size_t npad = (c.nmetrics + SEL_PER - 1) & ~(size_t)(SEL_PER - 1), chunk = select_chunk(npad, wn);
    u64 *base = nullptr;
    size_t cap = 0;
    int rc = c.movers ? LH_OK : ensure_table(cx->d_table, st, lh::k_value_table<KeptCtx>);
    if (!rc) rc = select_records(cx->sel, st, chunk * npad, MOVERS_FIELDS, base, cap); // (cap == chunk * npad: whole groups already)
    if (rc) return rc;
    const KeptList s = list_of(c.all, c.n);
    const uint32_t M = (uint32_t)c.nmetrics, NP = (uint32_t)npad;
    if (ev) LH_BESIDE_CHK(hipEventRecord(ev[0], st));
    for (size_t at = 0; at < wn && !rc; at += chunk) {
        const uint32_t nw_here = (uint32_t)std::min(chunk, wn - at);
        Entry *to = d_out + at * c.k;
        uint32_t *n_to = d_n_out + at;
        if constexpr (std::is_same<Entry, lh_top_entry>::value) {
            const TopRecords r = top_records(base, cap);
            const u64 flip = (c.flags & LH_TOP_ASCENDING) ? ~0ull : 0ull;
            const double *D = cx->d_table;
            const KeptWindows sw = windows_of(w.win + 2 * (w0 + at), nw_here);
            rc = launch_windows(M, nw_here, false, [&](const RowShape &sh, auto, auto nw) {
                hipLaunchKernelGGL((k_kept_top_score_series<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, NP, c.first, D, c.by,
                                   c.arg, flip, r);
            });
            if (!rc) rc = select_windows_pass(st, r.key, r.count, M, NP, nw_here, c.k, TopEmit{r, c.first, c.by, to}, n_to, ev);
        } else {
            const MoversRecords r = movers_records(base, cap);
            const u64 flip = (c.flags & LH_MOVERS_ASCENDING) ? ~0ull : 0ull;
            const KeptDriftWindows sw = drift_windows_of(w.win + 4 * (w0 + at), nw_here);
            rc = launch_windows(M, nw_here, false, [&](const RowShape &sh, auto, auto nw) {
                hipLaunchKernelGGL((k_kept_movers_score_series<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, sw, M, NP, c.first, c.by,
                                   c.arg, flip, r);
            });
            if (!rc) rc = select_windows_pass(st, r.key, r.cand, M, NP, nw_here, c.k, MoversEmit{r, c.first, to}, n_to, ev);
        }
    }
    // behind the last select -- after a failure too: what was enqueued uses the block
    const int rg = cx->sel.guard.record(st);
    return rc ? rc : rg;
}

// Every check that needs neither a handle nor a device, in the documented order: the list(s), the windows of a per-window form
// (w.given: ONE list, `cur`, of which lh_kept_movers_series*' windows name pairs of slices), `by`, the flags, lh_top's /
// lh_movers' rules for arg, then select_check_args (k, out, n_out, and the early LH_ERANGE behind every LH_EINVAL).  Fills c.
int check_select(SelectCall &c, lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                 uint32_t by, double arg, size_t k, uint32_t flags, const void *out, const void *n_out, uintptr_t n_out_align,
                 const Windows &w = WHOLE_LIST)
{
    const bool two_lists = c.movers && !w.given;
    if (two_lists ? !join_lists(base, nbase, cur, ncur, c.all) : bad_list(cur, ncur, LH_MAX_KEPT)) return LH_EINVAL;
    if (w.given && (c.movers ? bad_drift_windows(w.win, w.n, ncur) : bad_windows(w.win, w.n, ncur))) return LH_EINVAL;
    if (!two_lists) std::copy(cur, cur + ncur, c.all); // (nbase == 0)
    c.nbase = nbase;
    c.n = nbase + ncur;
    if (c.movers) {
        if (by > LH_MOVERS_BY_PERCENTILE || (flags & ~(uint32_t)LH_MOVERS_ASCENDING)) return LH_EINVAL;
        if (by == LH_MOVERS_BY_PERCENTILE && !(arg >= 0.0 && arg <= 1.0)) return LH_EINVAL; // NaN too: no bucket to rank by
    } else {
        if (by > LH_TOP_BY_COUNT_ABOVE || (flags & ~(uint32_t)LH_TOP_ASCENDING)) return LH_EINVAL;
        if (by == LH_TOP_BY_PERCENTILE && !(arg >= 0.0 && arg <= 1.0)) return LH_EINVAL;
        if (by == LH_TOP_BY_COUNT_ABOVE && arg != arg) return LH_EINVAL;
    }
    c.first = first;
    c.nmetrics = nmetrics;
    c.by = by;
    c.arg = arg;
    c.k = k;
    c.flags = flags;
    return select_check_args(nmetrics, k, out, n_out, n_out_align);
}

template <class Entry>
int kept_select(bool movers, lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                uint32_t by, double arg, size_t k, uint32_t flags, void *stream, Entry *out, size_t *n_out)
{
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, out, n_out, alignof(size_t));
    if (rc) return rc;
    if (nmetrics == 0) { // before any handle is looked at
        *n_out = 0;
        return LH_OK;
    }
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, false, never, [&](KeptCtx *cx, hipStream_t st) {
        return select_host_form(cx->sel, st, k, out, n_out, [&](Entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
            return enqueue_select(cx, c, st, d_out, d_n_out, ev);
        });
    });
}

template <class Entry>
int kept_select_device(bool movers, lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                       size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, Entry *d_out,
                       uint32_t *d_n_out)
{
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, d_out, d_n_out, alignof(uint32_t));
    if (rc) return rc;
    int device = -1;
    if (nmetrics == 0) { // the handles' devices alone are looked at: that is where d_n_out is zeroed
        rc = one_device(c.all, c.n, &device);
        if (rc) return rc;
        LH_BESIDE_CHK(hipSetDevice(device));
        LH_BESIDE_CHK(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t), static_cast<hipStream_t>(stream)));
        return LH_OK;
    }
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, true, // (one hold: the handles of BOTH lists)
               [&](KeptCtx *cx, hipStream_t st) { return enqueue_select(cx, c, st, d_out, d_n_out, (hipEvent_t *)nullptr); }, never);
}

template <class Entry>
int kept_select_passes_ms(bool movers, lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                          size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, float *score_ms,
                          float *select_ms)
{
    alignas(8) unsigned char own[8] = {0}; // (the results stay in the unit's own block)
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, own, own, 1);
    if (rc) return rc;
    if (!score_ms || !select_ms || nmetrics == 0) return LH_EINVAL;
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, false, never, [&](KeptCtx *cx, hipStream_t st) {
        return select_passes_ms<Entry>(cx->sel, st, k, score_ms, select_ms, [&](Entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) {
            return enqueue_select(cx, c, st, d_out, d_n_out, ev);
        });
    });
}

// ---- lh_kept_top_series* / lh_kept_movers_series*: the same two passes per WINDOW of ONE list, a select workgroup per window.  The
// checks are check_select's with the windows' term behind the list's; the handle checks, the mutex and the hold are run()'s.
template <class Entry>
int kept_select_series(bool movers, lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                       size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, Entry *out, size_t *n_out)
{
    const Windows w = {true, win, nwin};
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, out, n_out, alignof(size_t), w);
    if (rc) return rc;
    if (nmetrics == 0) { // before any handle is looked at
        std::fill(n_out, n_out + nwin, (size_t)0);
        return LH_OK;
    }
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, false, never, [&](KeptCtx *cx, hipStream_t st) {
        return select_windows_host_form(cx->sel, st, nwin, k, out, n_out, [&](Entry *d_out, uint32_t *d_n_out) {
            return enqueue_select_windows(cx, c, w, 0, nwin, st, d_out, d_n_out, (hipEvent_t *)nullptr);
        });
    });
}

template <class Entry>
int kept_select_series_device(bool movers, lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                              size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, Entry *d_out,
                              uint32_t *d_n_out)
{
    const Windows w = {true, win, nwin};
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, d_out, d_n_out, alignof(uint32_t), w);
    if (rc) return rc;
    int device = -1;
    if (nmetrics == 0) { // the handles' devices alone are looked at: that is where the nwin counts are zeroed
        rc = one_device(c.all, c.n, &device);
        if (rc) return rc;
        LH_BESIDE_CHK(hipSetDevice(device));
        LH_BESIDE_CHK(hipMemsetAsync(d_n_out, 0, nwin * sizeof(uint32_t), static_cast<hipStream_t>(stream)));
        return LH_OK;
    }
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, true, // (one hold: ALL listed handles)
               [&](KeptCtx *cx, hipStream_t st) { return enqueue_select_windows(cx, c, w, 0, nwin, st, d_out, d_n_out, (hipEvent_t *)nullptr); },
               never);
}

// lh_tool_kept_*_series_passes_ms: select_passes_ms once per chunk of the call, the two times summed over the chunks
template <class Entry>
int kept_select_series_passes_ms(bool movers, lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                 size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, float *score_ms,
                                 float *select_ms)
{
    alignas(8) unsigned char own[8] = {0}; // (the results stay in the unit's own block)
    const Windows w = {true, win, nwin};
    SelectCall c;
    c.movers = movers;
    int rc = check_select(c, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, own, own, 1, w);
    if (rc) return rc;
    if (!score_ms || !select_ms || nmetrics == 0) return LH_EINVAL;
    const auto never = [](KeptCtx *, hipStream_t) { return LH_ESTATE; };
    return run(c.all, c.n, DEVICE_THEN_ROWS, rows_from(first), nmetrics, stream, false, never, [&](KeptCtx *cx, hipStream_t st) {
        const size_t npad = (nmetrics + SEL_PER - 1) & ~(size_t)(SEL_PER - 1), chunk = select_chunk(npad, nwin);
        float score = 0.f, select = 0.f;
        for (size_t w0 = 0; w0 < nwin; w0 += chunk) {
            const size_t wn = std::min(chunk, nwin - w0);
            float a = 0.f, b = 0.f;
            const int rs = select_passes_ms<Entry>(
                cx->sel, st, k, &a, &b,
                [&](Entry *d_out, uint32_t *d_n_out, hipEvent_t *ev) { return enqueue_select_windows(cx, c, w, w0, wn, st, d_out, d_n_out, ev); },
                wn);
            if (rs) return rs;
            score += a;
            select += b;
        }
        *score_ms = score;
        *select_ms = select;
        return (int)LH_OK;
    });
}

// ---- lh_kept_save* / lh_kept_load*: the blob (loghisto_gpu.h has the format) ----------------------------------------------------
struct BlobHeader { // little-endian, as the hosts this builds for are
    unsigned char magic[8];
    uint32_t version, header_size, nkeys, first, nrows, reserved0;
    uint64_t cells, samples, bytes;
    unsigned char reserved1[8];
};
static_assert(sizeof(BlobHeader) == LH_KEPT_BLOB_HEADER && sizeof(LH_KEPT_BLOB_MAGIC) == 9, "64 bytes, 8 of them the magic");
static_assert(sizeof(lh_kept_check) == 16 && sizeof(lh_kept_under) == 16, "part of the ABI");

BlobHeader header_of(const lh_kept *k)
{
    BlobHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, LH_KEPT_BLOB_MAGIC, 8);
    h.version = LH_KEPT_BLOB_VERSION;
    h.header_size = LH_KEPT_BLOB_HEADER;
    h.nkeys = LH_NKEYS;
    h.first = k->first;
    h.nrows = k->nrows;
    h.cells = k->cells;
    h.samples = k->samples;
    h.bytes = k->bytes;
    return h;
}

// the header's causes of refusal in the documented order, `len` the blob's length; 0: none
uint32_t header_cause(const BlobHeader &h, size_t len)
{
    if (std::memcmp(h.magic, LH_KEPT_BLOB_MAGIC, 8) != 0) return LH_KEPT_BAD_MAGIC;
    if (h.version != LH_KEPT_BLOB_VERSION) return LH_KEPT_BAD_VERSION;
    if (h.header_size != LH_KEPT_BLOB_HEADER) return LH_KEPT_BAD_HEADER_SIZE;
    if (h.nkeys != LH_NKEYS) return LH_KEPT_BAD_NKEYS;
    if (h.nrows == 0) return LH_KEPT_BAD_NROWS;
    if ((u64)h.first + h.nrows > (1ull << 32)) return LH_KEPT_BAD_FIRST;
    if (h.cells > (u64)h.nrows * LH_NKEYS) return LH_KEPT_BAD_CELLS;
    if (h.bytes != (2 * (u64)h.nrows + 1) * 8 + h.cells * 10) return LH_KEPT_BAD_BYTES; // (cells <= 2^48: no wrap)
    if ((u64)len != LH_KEPT_BLOB_HEADER + h.bytes) return LH_KEPT_BAD_LENGTH;
    if (h.reserved0 != 0) return LH_KEPT_BAD_RESERVED;
    for (unsigned char c : h.reserved1)
        if (c) return LH_KEPT_BAD_RESERVED;
    return 0;
}

int refuse(lh_kept_check *why, uint32_t cause, uint32_t row = 0, uint32_t index = 0)
{
    if (why) {
        why->cause = cause;
        why->row = row;
        why->index = index;
    }
    return LH_EINVAL;
}

int kept_save(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written, bool to_device)
{
    if (!k || !buf) return LH_EINVAL;
    if (cap < LH_KEPT_BLOB_MIN) return LH_ERANGE; // before the handle is looked at
    KeptCtx *cx = k->cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> g(cx->mu); // no lh_kept_release frees the block under the copy
    const u64 size = LH_KEPT_BLOB_HEADER + k->bytes;
    if ((u64)cap < size) return LH_ERANGE;
    const BlobHeader h = header_of(k);
    unsigned char *to = static_cast<unsigned char *>(buf);
    LH_BESIDE_CHK(hipSetDevice(k->device));
    int rc = LH_OK;
    const auto chk = [&](hipError_t e) {
        if (e != hipSuccess && !rc) {
            (void)hipGetLastError();
            rc = e == hipErrorOutOfMemory ? LH_ENOMEM : LH_EDEVICE;
        }
    };
    if (to_device) chk(hipMemcpyAsync(to, &h, sizeof h, hipMemcpyHostToDevice, st)); // (h lives until the wait below)
    else std::memcpy(to, &h, sizeof h);
    chk(hipMemcpyAsync(to + sizeof h, k->block, (size_t)k->bytes, to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    chk(hipStreamSynchronize(st)); // complete on return, after a failure too
    if (rc) return rc;
    if (written) *written = (size_t)size;
    return LH_OK;
}

// the grid of a kernel that gives each of nrows rows a wave (64 bits: nrows may come from a blob and lie within ROW_WAVES of 2^32)
dim3 wave_per_row(uint32_t nrows) { return dim3((uint32_t)(((u64)nrows + ROW_WAVES - 1) / ROW_WAVES)); }

// (cx->mu held, the device current)  The block of a blob whose header `h` passed header_cause, from `src` (host or this device's
// memory) into k->block -- its exact allocation -- and checked there on `st`.  LH_EINVAL with *why filled for a block that is
// not what lh_keep makes.  After a failure the caller waits for `st` and frees k->block.
int load_block(KeptCtx *cx, const BlobHeader &h, const void *src, bool from_device, hipStream_t st, lh_kept_check *why, lh_kept *k)
{
    int rc = grow_device(cx->d_tmp, cx->tmp_cap, 1, 4096);
    if (!rc) rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
    if (rc) return rc;
    k->first = h.first;
    k->nrows = h.nrows;
    k->cells = h.cells;
    k->samples = h.samples;
    k->bytes = h.bytes;
    LH_BESIDE_CHK(hipMalloc((void **)&k->block, (size_t)h.bytes));
    LH_BESIDE_CHK(hipMemcpyAsync(k->block, src, (size_t)h.bytes, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    u64 *verdict = cx->d_tmp;
    LH_BESIDE_CHK(hipMemsetAsync(verdict, 0xff, sizeof(u64), st)); // CHECK_NONE
    const u64 block = (u64)(uintptr_t)k->block;
    hipLaunchKernelGGL(k_kept_check, wave_per_row(h.nrows), dim3(ROW_BLOCK), 0, st, block, h.nrows, h.cells, verdict);
    LH_BESIDE_CHK(hipGetLastError());
    hipLaunchKernelGGL(k_kept_check_samples, dim3(1), dim3(WG), 0, st, block, h.nrows, h.samples, verdict);
    LH_BESIDE_CHK(hipGetLastError());
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_totals, verdict, sizeof(u64), hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    const u64 v = cx->h_totals[0];
    if (v != CHECK_NONE) return refuse(why, (uint32_t)(v & 0xff), (uint32_t)(v >> 32), (uint32_t)(v >> 8) & 0xffffffu);
    return LH_OK;
}

// (the mutex held, the device current)  ms between HIP events on `st` around each of the n steps enqueue(i) puts there;
// returns when they are known
template <class Enqueue> int steps_ms(hipStream_t st, int n, float *const *ms, Enqueue enqueue)
{
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int rc = LH_OK;
    for (int i = 0; i <= n && rc == LH_OK; i++)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = LH_EDEVICE;
    if (rc == LH_OK && hipEventRecord(ev[0], st) != hipSuccess) rc = LH_EDEVICE;
    for (int i = 0; i < n && rc == LH_OK; i++) {
        enqueue(i);
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev[i + 1], st) != hipSuccess) rc = LH_EDEVICE;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = LH_EDEVICE; // nothing of the call is under way afterwards
    for (int i = 0; i < n && rc == LH_OK; i++)
        if (hipEventElapsedTime(ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = LH_EDEVICE;
    for (int i = 0; i <= n; i++)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (rc == LH_EDEVICE) (void)hipGetLastError();
    return rc;
}

int kept_load(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out, bool from_device)
{
    if (why && why->struct_size != sizeof(lh_kept_check)) return LH_EINVAL;
    if (!buf || !out || flags != 0 || device < 0 || device >= MAX_DEVICES) return refuse(why, LH_KEPT_BAD_ARG);
    if (len < LH_KEPT_BLOB_HEADER) return refuse(why, LH_KEPT_BAD_SHORT);
    BlobHeader h;
    if (!from_device) { // the header's causes before any device call
        std::memcpy(&h, buf, sizeof h);
        const uint32_t cause = header_cause(h, len);
        if (cause) return refuse(why, cause);
    }
    KeptCtx *cx = device_ctx<KeptCtx>(device);
    if (!cx) return LH_EDEVICE; // (never: the range was checked)
    lh_kept *k = new (std::nothrow) lh_kept;
    if (!k) return LH_ENOMEM;
    k->device = device;
    k->cx = cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char *src = static_cast<const unsigned char *>(buf);
    int rc;
    {
        std::lock_guard<std::mutex> g(cx->mu);
        rc = hipSetDevice(device) == hipSuccess ? LH_OK : LH_EDEVICE;
        if (!rc && from_device) { // its 64 header bytes alone come to the host
            rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
            if (!rc && (hipMemcpyAsync(cx->h_totals, src, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess))
                rc = LH_EDEVICE;
            if (!rc) {
                std::memcpy(&h, cx->h_totals, sizeof h);
                const uint32_t cause = header_cause(h, len);
                if (cause) rc = refuse(why, cause);
            }
        }
        if (!rc) rc = load_block(cx, h, src + sizeof h, from_device, st, why, k);
        if (rc) {
            (void)hipGetLastError();
            if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
            if (k->block && hipFree(k->block) != hipSuccess) (void)hipGetLastError();
        }
    }
    if (rc) {
        delete k;
        return rc;
    }
    *out = k;
    return LH_OK;
}

// ---- lh_kept_encode* / lh_kept_decode*: the compact blob ------------------------------------------------------------------------
static_assert(sizeof(LH_KEPT_ENC_MAGIC) == 9 && LH_KEPT_ENC_MIN == LH_KEPT_BLOB_HEADER + 8, "8 bytes of magic; one row, no cell");

// the encoded header's causes of refusal in the documented order, `len` the blob's length; 0: none
uint32_t enc_header_cause(const BlobHeader &h, size_t len)
{
    if (std::memcmp(h.magic, LH_KEPT_ENC_MAGIC, 8) != 0) return LH_KEPT_BAD_MAGIC;
    if (h.version != LH_KEPT_ENC_VERSION) return LH_KEPT_BAD_VERSION;
    if (h.header_size != LH_KEPT_BLOB_HEADER) return LH_KEPT_BAD_HEADER_SIZE;
    if (h.nkeys != LH_NKEYS) return LH_KEPT_BAD_NKEYS;
    if (h.nrows == 0) return LH_KEPT_BAD_NROWS;
    if ((u64)h.first + h.nrows > (1ull << 32)) return LH_KEPT_BAD_FIRST;
    if (h.cells > (u64)h.nrows * LH_NKEYS) return LH_KEPT_BAD_CELLS;
    const u64 D = enc_directory_bytes(h.nrows);
    if (h.bytes % 8 || h.bytes < D || h.bytes > D + 10 * h.cells + 6 * (u64)h.nrows) return LH_KEPT_BAD_BYTES; // (cells <= 2^48: no wrap)
    if ((u64)len != LH_KEPT_BLOB_HEADER + h.bytes) return LH_KEPT_BAD_LENGTH;
    if (h.reserved0 != 0) return LH_KEPT_BAD_RESERVED;
    for (unsigned char c : h.reserved1)
        if (c) return LH_KEPT_BAD_RESERVED;
    return 0;
}

// HIP events between the stages of ONE call, for the tools that time each kernel alone (off: nothing is created or recorded)
struct Stages {
    static constexpr int MAX = 6;
    hipEvent_t ev[MAX] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int n = 0;
    bool on, ok = true;
    hipStream_t st;
    Stages(bool on_, hipStream_t st_) : on(on_), st(st_) {}
    ~Stages()
    {
        for (int i = 0; i < n; i++)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    void mark()
    {
        if (!on || n >= MAX) return;
        if (hipEventCreate(&ev[n]) != hipSuccess || hipEventRecord(ev[n], st) != hipSuccess) ok = false;
        n++;
    }
    // (the stream waited for)  ms between marks i and j
    int ms(int i, int j, float *out) const
    {
        if (!ok || j >= n || !ev[i] || !ev[j] || hipEventElapsedTime(out, ev[i], ev[j]) != hipSuccess) {
            (void)hipGetLastError();
            return LH_EDEVICE;
        }
        return LH_OK;
    }
};

enum EncTo { ENC_SIZE, ENC_HOST, ENC_DEVICE, ENC_NOWHERE }; // ENC_NOWHERE: into the unit's own block only (the tools' timing)

// (cx->mu held, the device current)  lh_kept_encode*'s work on `st`; the caller waits for `st` after a failure
int encode_on(lh_kept *k, KeptCtx *cx, void *buf, size_t cap, hipStream_t st, size_t *written, EncTo to, Stages &clk)
{
    const uint32_t nrows = k->nrows;
    const size_t head = (size_t)nrows + 1 + 2, words = ((size_t)nrows + 1) / 2; // S and its offsets, the two totals | desc[nrows]
    int rc = grow_device(cx->d_tmp, cx->tmp_cap, head + words, 4096);
    if (!rc) rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
    if (rc) return rc;
    u64 *soff = cx->d_tmp, *totals = soff + nrows + 1;
    uint32_t *desc = reinterpret_cast<uint32_t *>(totals + 2);
    const u64 block = (u64)(uintptr_t)k->block;
    clk.mark();
    hipLaunchKernelGGL(k_enc_size, wave_per_row(nrows), dim3(ROW_BLOCK), 0, st, block, nrows, k->cells, desc, soff);
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(WG), 0, st, soff, k->row_count(), nrows, totals); // totals[0]: the records' bytes
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_totals, totals, sizeof(u64), hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    const u64 bytes = enc_directory_bytes(nrows) + cx->h_totals[0], size = LH_KEPT_BLOB_HEADER + bytes;
    if (to == ENC_SIZE) {
        *written = (size_t)size;
        return LH_OK;
    }
    if (to != ENC_NOWHERE && (u64)cap < size) return LH_ERANGE; // nothing written
    // the kernel writes aligned words: into the caller's device memory where that is 8-aligned, else into the unit's block
    const bool direct = to == ENC_DEVICE && !misaligned(buf, 8);
    unsigned char *dst = static_cast<unsigned char *>(buf);
    if (!direct) {
        rc = grow_device(cx->d_enc, cx->enc_cap, (size_t)size, (size_t)1 << 20);
        if (rc) return rc;
        dst = cx->d_enc;
    }
    BlobHeader h = header_of(k);
    std::memcpy(h.magic, LH_KEPT_ENC_MAGIC, 8);
    h.version = LH_KEPT_ENC_VERSION;
    h.bytes = bytes;
    LH_BESIDE_CHK(hipMemcpyAsync(dst, &h, sizeof h, hipMemcpyHostToDevice, st)); // (pageable: staged before the call returns)
    clk.mark();
    hipLaunchKernelGGL(k_enc_fill, wave_per_row(nrows), dim3(ROW_BLOCK), 0, st, block, nrows, k->cells, desc, soff, dst + sizeof h);
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    if (!direct && to != ENC_NOWHERE) // ONE copy of the exact size
        LH_BESIDE_CHK(hipMemcpyAsync(buf, dst, (size_t)size, to == ENC_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st)); // complete on return
    if (written) *written = (size_t)size;
    return LH_OK;
}

int kept_encode(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written, EncTo to, float *const *ms = nullptr)
{
    const bool writes = to == ENC_HOST || to == ENC_DEVICE;
    if (!k || (writes && !buf) || (to == ENC_SIZE && !written)) return LH_EINVAL;
    if (writes && cap < LH_KEPT_ENC_MIN) return LH_ERANGE; // before the handle is looked at
    KeptCtx *cx = k->cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> g(cx->mu); // no lh_kept_release frees the block under the kernels
    LH_BESIDE_CHK(hipSetDevice(k->device));
    Stages clk(ms != nullptr, st);
    int rc = encode_on(k, cx, buf, cap, st, written, to, clk);
    if (rc && rc != LH_ERANGE) { // nothing of the call is under way afterwards
        (void)hipGetLastError();
        if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
    }
    if (!rc && ms) // size | scan | fill
        for (int i = 0; i < 3 && !rc; i++) rc = clk.ms(i < 2 ? i : 3, i < 2 ? i + 1 : 4, ms[i]);
    return rc;
}

// (cx->mu held, the device current)  The payload of an encoded blob whose header `h` passed enc_header_cause, from `src` (host or
// this device's memory), decoded into k->block -- its exact allocation, made once the directory is proven -- and checked on the way,
// on `st`.  LH_EINVAL with *why filled for a payload that is not what lh_kept_encode makes.  After a failure the caller waits for
// `st` and frees k->block.
int decode_block(KeptCtx *cx, const BlobHeader &h, const void *src, bool from_device, hipStream_t st, lh_kept_check *why, lh_kept *k,
                 Stages &clk)
{
    const uint32_t nrows = h.nrows;
    const size_t rows1 = (size_t)nrows + 1;
    int rc = grow_device(cx->d_tmp, cx->tmp_cap, 2 * rows1 + 5, 4096);
    if (!rc) rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
    if (rc) return rc;
    u64 *off = cx->d_tmp, *soff = off + rows1, *back = soff + rows1, *verdict = back + 4; // back: {cells, bytes of records} | 2 unused
    const unsigned char *payload = static_cast<const unsigned char *>(src);
    if (!from_device || misaligned(src, 8)) { // the kernels read aligned words of this device's memory
        rc = grow_device(cx->d_enc, cx->enc_cap, (size_t)h.bytes, (size_t)1 << 20);
        if (rc) return rc;
        LH_BESIDE_CHK(hipMemcpyAsync(cx->d_enc, src, (size_t)h.bytes, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        payload = cx->d_enc;
    }
    LH_BESIDE_CHK(hipMemsetAsync(verdict, 0xff, sizeof(u64), st)); // CHECK_NONE
    // ---- stage 1: the directory alone
    clk.mark();
    hipLaunchKernelGGL(k_dec_dir, dim3((uint32_t)(((u64)nrows + 1 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const uint32_t *>(payload), nrows, off, soff, verdict);
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(WG), 0, st, off, soff + 1, nrows, back);      // the cells' offsets; {sum n, sum S}
    LH_BESIDE_CHK(hipGetLastError());
    hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(WG), 0, st, soff, off + 1, nrows, back + 2);  // the records' offsets
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_totals, back, 5 * sizeof(u64), hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    u64 v = cx->h_totals[4];
    if (cx->h_totals[0] != h.cells || enc_directory_bytes(nrows) + cx->h_totals[1] != h.bytes)
        v = std::min(v, (u64)nrows << 32 | LH_KEPT_BAD_ENC_TOTALS);
    if (v != CHECK_NONE) return refuse(why, (uint32_t)(v & 0xff), (uint32_t)(v >> 32), (uint32_t)(v >> 8) & 0xffffffu); // final
    // ---- stage 2: every record lies inside the payload and every row's cells inside the allocation
    k->first = h.first;
    k->nrows = nrows;
    k->cells = h.cells;
    k->samples = h.samples;
    k->bytes = (2 * (u64)nrows + 1) * sizeof(u64) + h.cells * (sizeof(u64) + sizeof(int16_t));
    LH_BESIDE_CHK(hipMalloc((void **)&k->block, (size_t)k->bytes));
    LH_BESIDE_CHK(hipMemcpyAsync(k->block, off, rows1 * sizeof(u64), hipMemcpyDeviceToDevice, st));
    const u64 block = (u64)(uintptr_t)k->block;
    clk.mark();
    hipLaunchKernelGGL(k_dec_fill, wave_per_row(nrows), dim3(ROW_BLOCK), 0, st, payload, nrows, h.cells, h.bytes, block, soff, verdict);
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    hipLaunchKernelGGL(k_kept_check_samples, dim3(1), dim3(WG), 0, st, block, nrows, h.samples, verdict);
    LH_BESIDE_CHK(hipGetLastError());
    clk.mark();
    LH_BESIDE_CHK(hipMemcpyAsync(cx->h_totals, verdict, sizeof(u64), hipMemcpyDeviceToHost, st));
    LH_BESIDE_CHK(hipStreamSynchronize(st));
    v = cx->h_totals[0];
    if (v != CHECK_NONE) return refuse(why, (uint32_t)(v & 0xff), (uint32_t)(v >> 32), (uint32_t)(v >> 8) & 0xffffffu);
    return LH_OK;
}

int kept_decode(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out, bool from_device,
                float *const *ms = nullptr)
{
    if (why && why->struct_size != sizeof(lh_kept_check)) return LH_EINVAL;
    if (!buf || !out || flags != 0 || device < 0 || device >= MAX_DEVICES) return refuse(why, LH_KEPT_BAD_ARG);
    if (len < LH_KEPT_BLOB_HEADER) return refuse(why, LH_KEPT_BAD_SHORT);
    BlobHeader h;
    if (!from_device) { // the header's causes before any device call
        std::memcpy(&h, buf, sizeof h);
        const uint32_t cause = enc_header_cause(h, len);
        if (cause) return refuse(why, cause);
    }
    KeptCtx *cx = device_ctx<KeptCtx>(device);
    if (!cx) return LH_EDEVICE; // (never: the range was checked)
    lh_kept *k = new (std::nothrow) lh_kept;
    if (!k) return LH_ENOMEM;
    k->device = device;
    k->cx = cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char *src = static_cast<const unsigned char *>(buf);
    int rc;
    {
        std::lock_guard<std::mutex> g(cx->mu);
        rc = hipSetDevice(device) == hipSuccess ? LH_OK : LH_EDEVICE;
        if (!rc && from_device) { // its 64 header bytes alone come to the host
            rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
            if (!rc && (hipMemcpyAsync(cx->h_totals, src, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                        hipStreamSynchronize(st) != hipSuccess))
                rc = LH_EDEVICE;
            if (!rc) {
                std::memcpy(&h, cx->h_totals, sizeof h);
                const uint32_t cause = enc_header_cause(h, len);
                if (cause) rc = refuse(why, cause);
            }
        }
        Stages clk(ms != nullptr, st);
        if (!rc) rc = decode_block(cx, h, src + sizeof h, from_device, st, why, k, clk);
        if (rc) {
            (void)hipGetLastError();
            if (hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
            if (k->block && hipFree(k->block) != hipSuccess) (void)hipGetLastError();
        }
        if (!rc && ms) { // directory | scans | fill | samples
            static const int from[4] = {0, 1, 3, 4};
            for (int i = 0; i < 4 && !rc; i++) rc = clk.ms(from[i], from[i] + 1, ms[i]);
            if (rc && hipFree(k->block) != hipSuccess) (void)hipGetLastError();
        }
    }
    if (rc) {
        delete k;
        return rc;
    }
    *out = k;
    return LH_OK;
}

// The readers' output structs from the pointers of the C ABI, host and device forms alike
KeptOut kept_out(uint64_t *count, double *sum, uint32_t *nbuckets, uint64_t *present_bits, int16_t *pkeys, uint8_t *pvalid)
{
    return {reinterpret_cast<u64 *>(count), sum, nbuckets, reinterpret_cast<u64 *>(present_bits), pkeys, pvalid};
}
CompareOut compare_out(uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key, uint64_t *ks_below_a, uint64_t *ks_below_b,
                       double *w1, double *shift)
{
    return {reinterpret_cast<u64 *>(count_a), reinterpret_cast<u64 *>(count_b), ks, ks_key, reinterpret_cast<u64 *>(ks_below_a),
            reinterpret_cast<u64 *>(ks_below_b), w1, shift};
}
SpreadOut spread_out(uint64_t *count, double *sum, double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le)
{
    return {reinterpret_cast<u64 *>(count), sum, m2, pkeys, pvalid, reinterpret_cast<u64 *>(count_le), sum_le};
}

} // namespace

extern "C" {

int lh_kept_save_size(const lh_kept *k, size_t *bytes)
{
    if (!k || !bytes) return LH_EINVAL;
    *bytes = (size_t)(LH_KEPT_BLOB_HEADER + k->bytes);
    return LH_OK;
}

int lh_kept_save(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written)
{
    return kept_save(k, buf, cap, stream, written, false);
}

int lh_kept_save_device(lh_kept *k, void *d_buf, size_t cap, void *stream, size_t *written)
{
    return kept_save(k, d_buf, cap, stream, written, true);
}

int lh_kept_load(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out)
{
    return kept_load(device, buf, len, flags, stream, why, out, false);
}

int lh_kept_load_device(int device, const void *d_buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out)
{
    return kept_load(device, d_buf, len, flags, stream, why, out, true);
}

int lh_kept_encode_size(lh_kept *k, void *stream, size_t *bytes) { return kept_encode(k, nullptr, 0, stream, bytes, ENC_SIZE); }

int lh_kept_encode(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written)
{
    return kept_encode(k, buf, cap, stream, written, ENC_HOST);
}

int lh_kept_encode_device(lh_kept *k, void *d_buf, size_t cap, void *stream, size_t *written)
{
    return kept_encode(k, d_buf, cap, stream, written, ENC_DEVICE);
}

int lh_kept_decode(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out)
{
    return kept_decode(device, buf, len, flags, stream, why, out, false);
}

int lh_kept_decode_device(int device, const void *d_buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out)
{
    return kept_decode(device, d_buf, len, flags, stream, why, out, true);
}

int lh_tool_kept_encode_ms(lh_kept *k, void *stream, float *size_ms, float *scan_ms, float *fill_ms)
{
    if (!k || !size_ms || !scan_ms || !fill_ms) return LH_EINVAL;
    float *const ms[3] = {size_ms, scan_ms, fill_ms};
    return kept_encode(k, nullptr, 0, stream, nullptr, ENC_NOWHERE, ms);
}

int lh_tool_kept_decode_ms(int device, const void *d_buf, size_t len, void *stream, float *dir_ms, float *scan_ms, float *fill_ms,
                           float *samples_ms)
{
    if (!dir_ms || !scan_ms || !fill_ms || !samples_ms) return LH_EINVAL;
    float *const ms[4] = {dir_ms, scan_ms, fill_ms, samples_ms};
    lh_kept *k = nullptr;
    const int rc = kept_decode(device, d_buf, len, 0, stream, nullptr, &k, true, ms);
    if (rc) return rc;
    return lh_kept_release(k);
}

int lh_tool_kept_check_ms(lh_kept *k, void *stream, float *check_ms, float *samples_ms)
{
    if (!k || !check_ms || !samples_ms) return LH_EINVAL;
    KeptCtx *cx = k->cx;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> g(cx->mu);
    LH_BESIDE_CHK(hipSetDevice(k->device));
    int rc = grow_device(cx->d_tmp, cx->tmp_cap, 1, 4096);
    if (!rc) rc = grow_pinned(cx->h_totals, cx->totals_cap, 8, 8);
    if (rc) return rc;
    u64 *verdict = cx->d_tmp;
    LH_BESIDE_CHK(hipMemsetAsync(verdict, 0xff, sizeof(u64), st));
    const u64 block = (u64)(uintptr_t)k->block;
    float *const ms[2] = {check_ms, samples_ms};
    rc = steps_ms(st, 2, ms, [&](int i) {
        if (i == 0) hipLaunchKernelGGL(k_kept_check, wave_per_row(k->nrows), dim3(ROW_BLOCK), 0, st, block, k->nrows, k->cells, verdict);
        else hipLaunchKernelGGL(k_kept_check_samples, dim3(1), dim3(WG), 0, st, block, k->nrows, k->samples, verdict);
    });
    if (rc) return rc;
    LH_BESIDE_CHK(hipMemcpy(cx->h_totals, verdict, sizeof(u64), hipMemcpyDeviceToHost));
    return cx->h_totals[0] == CHECK_NONE ? LH_OK : LH_ESTATE; // (never: a handle holds what the check asks for)
}

int lh_tool_keep_count_ms(lh_snapshot *s, uint32_t first, size_t nmetrics, float *count_ms)
{
    if (!s || !count_ms || nmetrics == 0) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE;
    KeptSource q;
    int rc = source_cells(s, first, nmetrics, q);
    if (!rc) rc = source_open(s, q);
    if (rc) return rc;
    const uint32_t nrows = (uint32_t)nmetrics;
    std::lock_guard<std::mutex> g(q.cx->mu);
    rc = grow_device(q.cx->d_tmp, q.cx->tmp_cap, 2 * (size_t)nrows + 3, 4096);
    if (rc) return rc;
    u64 *off = q.cx->d_tmp, *row_count = off + nrows + 1;
    const uint32_t *ranges = ranges_from(q, first);
    float *const ms[1] = {count_ms};
    return steps_ms(q.stream, 1, ms, [&](int) {
        with_cells(q, first, [&](auto c) {
            hipLaunchKernelGGL((k_keep_count<cell_of<decltype(c)>>), wave_per_row(nrows), dim3(ROW_BLOCK), 0, q.stream, c, ranges, q.stride,
                               nrows, off, row_count);
        });
    });
}

int lh_kept_values(int device, double *D)
{
    if (!D || misaligned(D, 8) || device < 0 || device >= MAX_DEVICES) return LH_EINVAL;
    KeptCtx *cx = device_ctx<KeptCtx>(device);
    if (!cx) return LH_EDEVICE; // (never: the range was checked)
    std::lock_guard<std::mutex> g(cx->mu);
    LH_BESIDE_CHK(hipSetDevice(device));
    const int rc = ensure_table(cx->d_table, nullptr, lh::k_value_table<KeptCtx>);
    if (rc) return rc;
    LH_BESIDE_CHK(hipMemcpy(D, cx->d_table, (size_t)LH_NKEYS * sizeof(double), hipMemcpyDeviceToHost));
    return LH_OK;
}

int lh_kept_top(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                uint32_t flags, void *stream, lh_top_entry *out, size_t *n_out)
{
    return kept_select(false, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, stream, out, n_out);
}

int lh_kept_top_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                       uint32_t flags, void *stream, lh_top_entry *d_out, uint32_t *d_n_out)
{
    return kept_select_device(false, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, stream, d_out, d_n_out);
}

int lh_kept_movers(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                   uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_mover_entry *out, size_t *n_out)
{
    return kept_select(true, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, stream, out, n_out);
}

int lh_kept_movers_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                          size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                          lh_mover_entry *d_out, uint32_t *d_n_out)
{
    return kept_select_device(true, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, stream, d_out, d_n_out);
}

int lh_tool_kept_top_passes_ms(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                               uint32_t flags, void *stream, float *score_ms, float *select_ms)
{
    return kept_select_passes_ms<lh_top_entry>(false, nullptr, 0, kept, nkept, first, nmetrics, by, arg, k, flags, stream, score_ms,
                                               select_ms);
}

int lh_tool_kept_movers_passes_ms(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                                  size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream, float *score_ms,
                                  float *select_ms)
{
    return kept_select_passes_ms<lh_mover_entry>(true, base, nbase, cur, ncur, first, nmetrics, by, arg, k, flags, stream, score_ms,
                                                 select_ms);
}

int lh_kept_top_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                       uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_top_entry *out, size_t *n_out)
{
    return kept_select_series(false, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, out, n_out);
}

int lh_kept_top_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                              uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_top_entry *d_out, uint32_t *d_n_out)
{
    return kept_select_series_device(false, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, d_out, d_n_out);
}

int lh_kept_movers_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_mover_entry *out, size_t *n_out)
{
    return kept_select_series(true, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, out, n_out);
}

int lh_kept_movers_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                 size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                                 lh_mover_entry *d_out, uint32_t *d_n_out)
{
    return kept_select_series_device(true, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, d_out, d_n_out);
}

int lh_tool_kept_top_series_passes_ms(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                      size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                                      float *score_ms, float *select_ms)
{
    return kept_select_series_passes_ms<lh_top_entry>(false, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, score_ms,
                                                      select_ms);
}

int lh_tool_kept_movers_series_passes_ms(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                         size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                                         float *score_ms, float *select_ms)
{
    return kept_select_series_passes_ms<lh_mover_entry>(true, kept, nkept, win, nwin, first, nmetrics, by, arg, k, flags, stream, score_ms,
                                                        select_ms);
}

int lh_tool_kept_select_bytes(uint64_t bytes, uint64_t *previous)
{
    const u64 old = g_select_bytes.exchange(bytes ? (u64)bytes : KEPT_SELECT_BYTES, std::memory_order_relaxed);
    if (previous) *previous = old;
    return LH_OK;
}

int lh_keep(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t flags, lh_kept **out)
{
    if (!s || !out || flags != 0 || nmetrics == 0) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE;
    KeptSource q;
    int rc = source_cells(s, first, nmetrics, q);
    if (!rc) rc = source_open(s, q);
    if (rc) return rc;
    lh_kept *k = new (std::nothrow) lh_kept;
    if (!k) return LH_ENOMEM;
    k->device = q.device;
    k->cx = q.cx;
    {
        std::lock_guard<std::mutex> g(q.cx->mu);
        rc = keep(q, first, (uint32_t)nmetrics, k);
        if (rc) {
            if (hipStreamSynchronize(q.stream) != hipSuccess) (void)hipGetLastError();
            if (k->block && hipFree(k->block) != hipSuccess) (void)hipGetLastError();
        }
    }
    if (rc) {
        delete k;
        return rc;
    }
    *out = k;
    return LH_OK;
}

int lh_kept_merge(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t flags, void *stream, lh_kept **out)
{
    if (bad_list(kept, nkept, LH_MAX_KEPT) || flags != 0 || !out || nmetrics == 0) return LH_EINVAL;
    if (nmetrics > 0xffffffffu) return LH_ERANGE;
    // ---- from here on the handles are looked at
    const int device = kept[nkept - 1]->device;
    for (size_t i = 0; i + 1 < nkept; i++)
        if (kept[i]->device != device) return LH_EINVAL;
    for (size_t i = 0; i < nkept; i++) // the block lies inside every handle's: lh_kept_across' rule
        if (first < kept[i]->first || (u64)first + nmetrics > (u64)kept[i]->first + kept[i]->nrows) return LH_ERANGE;
    return born_of(device, stream, out, [&](KeptCtx *cx, hipStream_t st, lh_kept *k) {
        return merge(cx, kept, nkept, first, (uint32_t)nmetrics, st, k);
    });
}

// lh_kept_gather*'s one front end: the checks in lh_kept_merge's style and order, then -- the host form only -- every entry of the
// map against its handle's block, and the map staged on the call's stream as an id list is (born_of waits for it after a failure)
static int kept_gather(lh_kept *const *kept, size_t nkept, const uint32_t *src, bool on_device, size_t n, uint32_t first_out,
                       uint32_t flags, void *stream, lh_kept **out)
{
    if (bad_list(kept, nkept, LH_MAX_KEPT) || !src || misaligned(src, 4) || flags != 0 || !out || n == 0) return LH_EINVAL;
    if (n > 0xffffffffu || (u64)first_out + n > (1ull << 32)) return LH_ERANGE;
    // ---- from here on the handles are looked at
    int device = -1;
    int rc = one_device(kept, nkept, &device);
    if (rc) return rc;
    if (!on_device)
        for (size_t i = 0; i < nkept; i++) {
            const u64 lo = kept[i]->first, end = lo + kept[i]->nrows;
            for (size_t j = 0; j < n; j++) {
                const uint32_t r = src[i * n + j];
                if (r != LH_KEPT_NO_ROW && (r < lo || r >= end)) return LH_ERANGE;
            }
        }
    return born_of(device, stream, out, [&](KeptCtx *cx, hipStream_t st, lh_kept *k) {
        const uint32_t *d_src = nullptr;
        const int staged = stage_ids(cx->ids, rows_by_id(src, on_device), nkept * n, st, d_src);
        return staged ? staged : gather(cx, kept, nkept, d_src, (uint32_t)n, first_out, st, k);
    });
}

int lh_kept_gather(lh_kept *const *kept, size_t nkept, const uint32_t *src, size_t n, uint32_t first_out, uint32_t flags, void *stream,
                   lh_kept **out)
{
    return kept_gather(kept, nkept, src, false, n, first_out, flags, stream, out);
}

int lh_kept_gather_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_src, size_t n, uint32_t first_out, uint32_t flags,
                          void *stream, lh_kept **out)
{
    return kept_gather(kept, nkept, d_src, true, n, first_out, flags, stream, out);
}

// lh_kept_group*'s one front end: the checks in lh_kept_gather's style and order; the host form's CSR rules need no handle and are
// decided before one is looked at (they and "different devices" are both LH_EINVAL, so the documented order holds), its members
// are held to EVERY handle's block; the CSR staged on the call's stream (born_of waits for it after a failure)
static int kept_group(lh_kept *const *kept, size_t nkept, const uint64_t *goff, const uint32_t *members, bool on_device, size_t nmembers,
                      size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out)
{
    if (bad_list(kept, nkept, LH_MAX_KEPT) || !goff || misaligned(goff, 8) || (!members && nmembers > 0) || misaligned(members, 4) ||
        flags != 0 || !out || ngroups == 0)
        return LH_EINVAL;
    if (ngroups > 0xffffffffu || (u64)first_out + ngroups > (1ull << 32) || nmembers > 0xffffffffu) return LH_ERANGE;
    if (!on_device) {
        if (goff[0] != 0 || goff[ngroups] != nmembers) return LH_EINVAL;
        for (size_t g = 0; g < ngroups; g++)
            if (goff[g + 1] < goff[g]) return LH_EINVAL;
    }
    // ---- from here on the handles are looked at
    int device = -1;
    int rc = one_device(kept, nkept, &device);
    if (rc) return rc;
    if (!on_device) {
        u64 lo = 0, end = ~0ull; // the rows every handle has
        for (size_t i = 0; i < nkept; i++) {
            const u64 f = kept[i]->first, e = f + kept[i]->nrows;
            lo = f > lo ? f : lo;
            end = e < end ? e : end;
        }
        for (size_t j = 0; j < nmembers; j++)
            if (members[j] != LH_KEPT_NO_ROW && (members[j] < lo || members[j] >= end)) return LH_ERANGE;
    }
    return born_of(device, stream, out, [&](KeptCtx *cx, hipStream_t st, lh_kept *k) {
        const u64 *d_goff = reinterpret_cast<const u64 *>(goff);
        const uint32_t *d_members = members;
        const int staged = on_device ? LH_OK : stage_groups(cx->ids, d_goff, members, nmembers, ngroups, st, d_goff, d_members);
        return staged ? staged : group(cx, kept, nkept, d_goff, d_members, nmembers, (uint32_t)ngroups, first_out, st, k);
    });
}

int lh_kept_group(lh_kept *const *kept, size_t nkept, const uint64_t *goff, const uint32_t *members, size_t nmembers, size_t ngroups,
                  uint32_t first_out, uint32_t flags, void *stream, lh_kept **out)
{
    return kept_group(kept, nkept, goff, members, false, nmembers, ngroups, first_out, flags, stream, out);
}

int lh_kept_group_device(lh_kept *const *kept, size_t nkept, const uint64_t *d_goff, const uint32_t *d_members, size_t nmembers,
                         size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out)
{
    return kept_group(kept, nkept, d_goff, d_members, true, nmembers, ngroups, first_out, flags, stream, out);
}

int lh_kept_slide(lh_kept *const *add, size_t nadd, lh_kept *const *sub, size_t nsub, uint32_t first, size_t nmetrics, uint32_t flags,
                  void *stream, lh_kept_under *why, lh_kept **out)
{
    lh_kept *all[LH_MAX_KEPT];
    int device = -1;
    int rc = check_slide(add, nadd, sub, nsub, first, nmetrics, flags, why, out, all, &device);
    if (rc) return rc;
    u64 verdict = SLIDE_CLEAN;
    rc = born_of(device, stream, out, [&](KeptCtx *cx, hipStream_t st, lh_kept *k) {
        return slide(cx, all, nadd + nsub, nadd, first, (uint32_t)nmetrics, st, k, &verdict);
    });
    if (verdict != SLIDE_CLEAN && why) { // (rc is LH_ERANGE: make ended there)
        why->row = (uint32_t)(verdict >> 16);
        why->key = (int16_t)bin_to_key((uint32_t)(verdict & 0xffff));
        why->reserved0 = 0;
        why->reserved1 = 0;
    }
    return rc;
}

int lh_tool_kept_slide_passes_ms(lh_kept *const *add, size_t nadd, lh_kept *const *sub, size_t nsub, uint32_t first, size_t nmetrics,
                                 void *stream, float *count_ms, float *fill_ms)
{
    alignas(8) unsigned char own[8] = {0}; // (stands in for `out`: the handle made here is freed again)
    lh_kept *all[LH_MAX_KEPT];
    int device = -1;
    int rc = check_slide(add, nadd, sub, nsub, first, nmetrics, 0, nullptr, own, all, &device);
    if (rc) return rc;
    if (!count_ms || !fill_ms) return LH_EINVAL;
    lh_kept *made = nullptr;
    const uint32_t nrows = (uint32_t)nmetrics, NA = (uint32_t)nadd;
    rc = born_of(device, stream, &made, [&](KeptCtx *cx, hipStream_t st, lh_kept *k) -> int {
        u64 verdict = SLIDE_CLEAN;
        int r = slide(cx, all, nadd + nsub, nadd, first, nrows, st, k, &verdict); // the allocation, and d_tmp's offsets
        if (r) return r;
        if (k->cells == 0) return LH_EINVAL; // no fill pass to time
        const KeptList s = list_of(all, nadd + nsub);
        u64 *off = cx->d_tmp, *row_count = off + nrows + 1, *totals = off + 2 * (size_t)nrows + 1, *counts = k->block + 2 * (size_t)nrows + 1;
        int16_t *keys = reinterpret_cast<int16_t *>(counts + k->cells);
        float *const c_ms[1] = {count_ms}, *const f_ms[1] = {fill_ms};
        int launched = LH_OK;
        r = steps_ms(st, 1, c_ms, [&](int) {
            launched = launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_slide_count<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NA, nrows, first, off, row_count, totals + 2);
            });
        });
        if (r || launched) return r ? r : launched;
        hipLaunchKernelGGL(k_keep_scan, dim3(1), dim3(WG), 0, st, off, row_count, nrows, totals); // off[]: nnz -> offsets again
        LH_BESIDE_CHK(hipGetLastError());
        r = steps_ms(st, 1, f_ms, [&](int) { // into the handle's own arrays: the bytes they hold already
            launched = launch_rows(nrows, [&](const RowShape &sh, auto nw) {
                hipLaunchKernelGGL((k_slide_fill<decltype(nw)::value>), sh.grid, sh.block, 0, st, s, NA, nrows, first, off, keys, counts);
            });
        });
        return r ? r : launched;
    });
    if (rc) return rc;
    return lh_kept_release(made);
}

int lh_kept_release(lh_kept *k)
{
    if (!k) return LH_EINVAL;
    KeptCtx *cx = k->cx; // (lh_keep's: never null)
    {
        std::lock_guard<std::mutex> g(cx->mu);
        (void)hipSetDevice(k->device);
        if (k->busy) { // enqueued work may still read the block
            (void)hipEventSynchronize(k->busy->ev);
            unuse(cx, k->busy);
        }
        if (k->block) (void)hipFree(k->block);
        (void)hipGetLastError();
    }
    delete k;
    return LH_OK;
}

int lh_kept_hold(lh_kept *k, void *stream)
{
    if (!k) return LH_EINVAL;
    KeptCtx *cx = k->cx;
    std::lock_guard<std::mutex> g(cx->mu);
    LH_BESIDE_CHK(hipSetDevice(k->device));
    return hold(cx, &k, 1, static_cast<hipStream_t>(stream));
}

int lh_kept_info_get(const lh_kept *k, lh_kept_info *out)
{
    if (!k || !out || out->struct_size != sizeof(lh_kept_info)) return LH_EINVAL;
    out->device = k->device;
    out->first = k->first;
    out->nrows = k->nrows;
    out->cells = k->cells;
    out->samples = k->samples;
    out->bytes = k->bytes;
    return LH_OK;
}

int lh_kept_arrays(const lh_kept *k, const uint64_t **d_offsets, const int16_t **d_keys, const uint64_t **d_counts,
                   const uint64_t **d_row_count)
{
    if (!k) return LH_EINVAL;
    if (d_offsets) *d_offsets = reinterpret_cast<const uint64_t *>(k->offsets());
    if (d_keys) *d_keys = k->keys();
    if (d_counts) *d_counts = reinterpret_cast<const uint64_t *>(k->counts());
    if (d_row_count) *d_row_count = reinterpret_cast<const uint64_t *>(k->row_count());
    return LH_OK;
}

int lh_kept_across(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np, uint32_t flags,
                   void *stream, uint64_t *count, double *sum, uint32_t *nbuckets, uint64_t *present_bits, int16_t *pkeys,
                   uint8_t *pvalid)
{
    return kept_across(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, p, np, flags, stream,
                       kept_out(count, sum, nbuckets, present_bits, pkeys, pvalid), false);
}

int lh_kept_across_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                          uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets,
                          uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid)
{
    return kept_across(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, p, np, flags, stream,
                       kept_out(d_count, d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid), true);
}

int lh_kept_across_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *p, size_t np, uint32_t flags,
                       void *stream, uint64_t *count, double *sum, uint32_t *nbuckets, uint64_t *present_bits, int16_t *pkeys,
                       uint8_t *pvalid)
{
    return kept_across(kept, nkept, WHOLE_LIST, rows_by_id(ids, false), n, p, np, flags, stream,
                       kept_out(count, sum, nbuckets, present_bits, pkeys, pvalid), false);
}

int lh_kept_across_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                              uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets,
                              uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid)
{
    return kept_across(kept, nkept, WHOLE_LIST, rows_by_id(d_ids, true), n, p, np, flags, stream,
                       kept_out(d_count, d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid), true);
}

int lh_kept_compare(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                    uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                    uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift)
{
    return kept_compare_lists(base, nbase, cur, ncur, rows_from(first), nmetrics, flags, stream,
                              compare_out(count_a, count_b, ks, ks_key, ks_below_a, ks_below_b, w1, shift), false);
}

int lh_kept_compare_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                           uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks,
                           int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift)
{
    return kept_compare_lists(base, nbase, cur, ncur, rows_from(first), nmetrics, flags, stream,
                              compare_out(d_count_a, d_count_b, d_ks, d_ks_key, d_ks_below_a, d_ks_below_b, d_w1, d_shift), true);
}

int lh_kept_compare_ids(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, const uint32_t *ids, size_t n,
                        uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                        uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift)
{
    return kept_compare_lists(base, nbase, cur, ncur, rows_by_id(ids, false), n, flags, stream,
                              compare_out(count_a, count_b, ks, ks_key, ks_below_a, ks_below_b, w1, shift), false);
}

int lh_kept_compare_ids_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, const uint32_t *d_ids,
                               size_t n, uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks,
                               int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift)
{
    return kept_compare_lists(base, nbase, cur, ncur, rows_by_id(d_ids, true), n, flags, stream,
                              compare_out(d_count_a, d_count_b, d_ks, d_ks_key, d_ks_below_a, d_ks_below_b, d_w1, d_shift), true);
}

int lh_kept_count_le(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *bounds, size_t nb,
                     uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_count_le(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_count_le_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *bounds, size_t nb,
                            uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_count_le(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, bounds, nb, flags, stream, d_cum, d_total, true);
}

int lh_kept_count_le_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *bounds, size_t nb,
                         uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_count_le(kept, nkept, WHOLE_LIST, rows_by_id(ids, false), n, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_count_le_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *bounds, size_t nb,
                                uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_count_le(kept, nkept, WHOLE_LIST, rows_by_id(d_ids, true), n, bounds, nb, flags, stream, d_cum, d_total, true);
}

int lh_kept_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                   const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets,
                   uint64_t *present_bits, int16_t *pkeys, uint8_t *pvalid)
{
    return kept_across(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, p, np, flags, stream,
                       kept_out(count, sum, nbuckets, present_bits, pkeys, pvalid), false);
}

int lh_kept_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count, double *d_sum,
                          uint32_t *d_nbuckets, uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid)
{
    return kept_across(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, p, np, flags, stream,
                       kept_out(d_count, d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid), true);
}

int lh_kept_series_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                       const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets,
                       uint64_t *present_bits, int16_t *pkeys, uint8_t *pvalid)
{
    return kept_across(kept, nkept, Windows{true, win, nwin}, rows_by_id(ids, false), n, p, np, flags, stream,
                       kept_out(count, sum, nbuckets, present_bits, pkeys, pvalid), false);
}

int lh_kept_series_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                              const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count, double *d_sum,
                              uint32_t *d_nbuckets, uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid)
{
    return kept_across(kept, nkept, Windows{true, win, nwin}, rows_by_id(d_ids, true), n, p, np, flags, stream,
                       kept_out(d_count, d_sum, d_nbuckets, d_present_bits, d_pkeys, d_pvalid), true);
}

int lh_kept_heat(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                 const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_count_le(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_heat_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                        const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_count_le(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, bounds, nb, flags, stream, d_cum, d_total,
                         true);
}

int lh_kept_heat_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                     const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_count_le(kept, nkept, Windows{true, win, nwin}, rows_by_id(ids, false), n, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_heat_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                            const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_count_le(kept, nkept, Windows{true, win, nwin}, rows_by_id(d_ids, true), n, bounds, nb, flags, stream, d_cum, d_total,
                         true);
}

int lh_kept_slo(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_slo(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_slo_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                       const double *d_bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_slo(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, d_bounds, nb, flags, stream, d_cum, d_total, true);
}

int lh_kept_slo_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                    const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total)
{
    return kept_slo(kept, nkept, Windows{true, win, nwin}, rows_by_id(ids, false), n, bounds, nb, flags, stream, cum, total, false);
}

int lh_kept_slo_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                           const double *d_bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_slo(kept, nkept, Windows{true, win, nwin}, rows_by_id(d_ids, true), n, d_bounds, nb, flags, stream, d_cum, d_total, true);
}

int lh_kept_burn(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                 const double *rate, const double *bounds, const double *budget, size_t k, uint32_t flags, void *stream,
                 lh_burn_hit *out, uint64_t *n_out, uint64_t *cum, uint64_t *total)
{
    return kept_burn(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics,
                     BurnCall{rate, bounds, budget, k, out, n_out, cum, total}, flags, stream, false);
}

int lh_kept_burn_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                        const double *rate, const double *d_bounds, const double *d_budget, size_t k, uint32_t flags, void *stream,
                        lh_burn_hit *d_out, uint64_t *d_n_out, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_burn(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics,
                     BurnCall{rate, d_bounds, d_budget, k, d_out, d_n_out, d_cum, d_total}, flags, stream, true);
}

int lh_kept_burn_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                     const double *rate, const double *bounds, const double *budget, size_t k, uint32_t flags, void *stream,
                     lh_burn_hit *out, uint64_t *n_out, uint64_t *cum, uint64_t *total)
{
    return kept_burn(kept, nkept, Windows{true, win, nwin}, rows_by_id(ids, false), n,
                     BurnCall{rate, bounds, budget, k, out, n_out, cum, total}, flags, stream, false);
}

int lh_kept_burn_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                            const double *rate, const double *d_bounds, const double *d_budget, size_t k, uint32_t flags, void *stream,
                            lh_burn_hit *d_out, uint64_t *d_n_out, uint64_t *d_cum, uint64_t *d_total)
{
    return kept_burn(kept, nkept, Windows{true, win, nwin}, rows_by_id(d_ids, true), n,
                     BurnCall{rate, d_bounds, d_budget, k, d_out, d_n_out, d_cum, d_total}, flags, stream, true);
}

int lh_kept_spread(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np, uint32_t flags,
                   void *stream, uint64_t *count, double *sum, double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le,
                   double *sum_le)
{
    return kept_spread(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, p, np, flags, stream,
                       spread_out(count, sum, m2, pkeys, pvalid, count_le, sum_le), false);
}

int lh_kept_spread_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                          uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, double *d_m2, int16_t *d_pkeys,
                          uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le)
{
    return kept_spread(kept, nkept, WHOLE_LIST, rows_from(first), nmetrics, p, np, flags, stream,
                       spread_out(d_count, d_sum, d_m2, d_pkeys, d_pvalid, d_count_le, d_sum_le), true);
}

int lh_kept_spread_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *p, size_t np, uint32_t flags,
                       void *stream, uint64_t *count, double *sum, double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le,
                       double *sum_le)
{
    return kept_spread(kept, nkept, WHOLE_LIST, rows_by_id(ids, false), n, p, np, flags, stream,
                       spread_out(count, sum, m2, pkeys, pvalid, count_le, sum_le), false);
}

int lh_kept_spread_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                              uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, double *d_m2, int16_t *d_pkeys,
                              uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le)
{
    return kept_spread(kept, nkept, WHOLE_LIST, rows_by_id(d_ids, true), n, p, np, flags, stream,
                       spread_out(d_count, d_sum, d_m2, d_pkeys, d_pvalid, d_count_le, d_sum_le), true);
}

int lh_kept_spread_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2,
                          int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le)
{
    return kept_spread(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, p, np, flags, stream,
                       spread_out(count, sum, m2, pkeys, pvalid, count_le, sum_le), false);
}

int lh_kept_spread_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                                 const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count, double *d_sum,
                                 double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le)
{
    return kept_spread(kept, nkept, Windows{true, win, nwin}, rows_from(first), nmetrics, p, np, flags, stream,
                       spread_out(d_count, d_sum, d_m2, d_pkeys, d_pvalid, d_count_le, d_sum_le), true);
}

int lh_kept_spread_series_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                              const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2,
                              int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le)
{
    return kept_spread(kept, nkept, Windows{true, win, nwin}, rows_by_id(ids, false), n, p, np, flags, stream,
                       spread_out(count, sum, m2, pkeys, pvalid, count_le, sum_le), false);
}

int lh_kept_spread_series_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids,
                                     size_t n, const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count,
                                     double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le,
                                     double *d_sum_le)
{
    return kept_spread(kept, nkept, Windows{true, win, nwin}, rows_by_id(d_ids, true), n, p, np, flags, stream,
                       spread_out(d_count, d_sum, d_m2, d_pkeys, d_pvalid, d_count_le, d_sum_le), true);
}

int lh_kept_drift(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics, uint32_t flags,
                  void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key, uint64_t *ks_below_a,
                  uint64_t *ks_below_b, double *w1, double *shift)
{
    return kept_compare(kept, nkept, 0, Windows{true, win, nwin}, rows_from(first), nmetrics, flags, stream,
                        compare_out(count_a, count_b, ks, ks_key, ks_below_a, ks_below_b, w1, shift), false);
}

int lh_kept_drift_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                         uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks, int16_t *d_ks_key,
                         uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift)
{
    return kept_compare(kept, nkept, 0, Windows{true, win, nwin}, rows_from(first), nmetrics, flags, stream,
                        compare_out(d_count_a, d_count_b, d_ks, d_ks_key, d_ks_below_a, d_ks_below_b, d_w1, d_shift), true);
}

int lh_kept_drift_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                      uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                      uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift)
{
    return kept_compare(kept, nkept, 0, Windows{true, win, nwin}, rows_by_id(ids, false), n, flags, stream,
                        compare_out(count_a, count_b, ks, ks_key, ks_below_a, ks_below_b, w1, shift), false);
}

int lh_kept_drift_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                             uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks, int16_t *d_ks_key,
                             uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift)
{
    return kept_compare(kept, nkept, 0, Windows{true, win, nwin}, rows_by_id(d_ids, true), n, flags, stream,
                        compare_out(d_count_a, d_count_b, d_ks, d_ks_key, d_ks_below_a, d_ks_below_b, d_w1, d_shift), true);
}

int lh_tool_kept_compare_tile(uint32_t *bins)
{
    if (!bins) return LH_EINVAL;
    *bins = KEPT_COMPARE_TILE;
    return LH_OK;
}

int lh_tool_kept_switch(uint32_t wave_from_rows, uint32_t *previous)
{
    switch_exchange(g_wave_from, wave_from_rows, KEPT_WAVE_FROM_DEFAULT, previous);
    return LH_OK;
}

int lh_tool_kept_gather_route(uint32_t route, uint32_t *previous)
{
    if (route > LH_TOOL_GATHER_TRANSPOSED) return LH_EINVAL;
    const uint32_t old = g_gather_route.exchange(route, std::memory_order_relaxed);
    if (previous) *previous = old;
    return LH_OK;
}

int lh_tool_kept_tile(uint32_t *bins)
{
    if (!bins) return LH_EINVAL;
    *bins = KEPT_TILE;
    return LH_OK;
}

} // extern "C"
