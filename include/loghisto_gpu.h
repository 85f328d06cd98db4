/*
 * loghisto_gpu.h -- C ABI of liblhgpu.so, the MI355X (gfx950) engine behind
 * loghisto's histogram hot path.
 *
 * The reference (spacejam/loghisto, Go) has no FFI on this path: the boundary is
 * the bodies of three Go functions, which a cgo binding replaces with calls into
 * this library (the binding is shown in INTEGRATION.md):
 *
 *   (*MetricSystem).Histogram        /root/reference/metrics.go:273-295
 *       -> lh_intern (once per name) + lh_submit / lh_submit_pairs (batched)
 *   collectRawMetrics, histogram part /root/reference/metrics.go:460-463
 *       -> lh_flip            (the epoch boundary: steal the interval's cells)
 *   processHistograms + percentile   /root/reference/metrics.go:336-418
 *       -> lh_extract         (count, sum, avg, uint64(sum), percentiles)
 *   RawMetricSet.Histograms          /root/reference/metrics.go:54-60
 *       -> lh_buckets         (occupied (key,count) cells of one metric)
 *   processMetrics/addAggregates key loops + the serializers' per-key line
 *                                    /root/reference/metrics.go:483-506, 590-608,
 *                                    graphite.go:37-48, opentsdb.go:45-58
 *       -> lh_snapshot_accumulate + lh_serialize (keys, Go's %f and the wire
 *          lines assembled on the device; optional, for large name spaces)
 *   compress / decompress            /root/reference/metrics.go:316-332
 *       -> computed on device inside lh_submit*; lh_compress_device and
 *          lh_codec_tables expose the codec for parity tests.
 *
 * Conventions:
 *   - every entry point returns an int status (LH_OK == 0); nothing aborts.
 *     The Go layer logs non-zero codes through glog and carries on, exactly as
 *     it does for percentile()'s error (metrics.go:379-384).
 *   - ingest is lossless and may block (back-pressure) but never drops
 *     (metrics.go:273-295 is synchronous); only emission may be dropped, by the
 *     caller.
 *   - lh_submit* are thread-safe and copy the caller's buffer before returning
 *     (cgo rule: C may not retain Go memory).
 *   - a sample belongs to exactly one snapshot: everything submitted before
 *     lh_flip returns is in that snapshot, everything after is in the next
 *     (metrics.go:460-463).
 *   - plain pointers and sizes only; `stream` arguments are hipStream_t passed
 *     as void* (NULL = the engine's own stream).
 *
 * Bucket keys are the reference's int16 keys.  Dense rows are indexed by
 * bin = (uint16)key ^ 0x8000, so ascending bin == ascending key == ascending
 * decompressed value.
 */
#ifndef LOGHISTO_GPU_H
#define LOGHISTO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH_ABI_VERSION 7           /* 7: uint32 cells above 8 192 names (lh_config.cell_bits, lh_snapshot_cells, lh_cell_bytes;
                                      lh_counters.widenings / store_bytes): half the lines under every flush, clear, extract
                                      read and merge pack, lh_create(65 536 names) 32 GiB instead of 64; lh_snapshot_rows still
                                      hands out uint64 rows; 6: lh_extract_rows_compact / lh_expand_compact (the results of many names at 42 B instead of
                                      139 B per name); 5: lh_row_stride() (rows of lh_snapshot_rows are no longer 65 536 cells apart), the
                                      tuning / test options moved to loghisto_gpu_tuning.h, ingest falls back to the
                                      scratch-free kernel when scratch cannot be had; 4: uint16-id pairs (lh_*pairs16*) */
#define LH_NKEYS 65536            /* int16 key space (metrics.go:316)        */
#define LH_NTHRESH 70980          /* extended-key thresholds incl. sentinel  */
#define LH_MAX_PERCENTILES 32

enum {
    LH_OK = 0,
    LH_EINVAL = 1,      /* bad argument                                      */
    LH_ENOMEM = 2,      /* host or device allocation failed                  */
    LH_EDEVICE = 3,     /* HIP runtime error (see lh_last_error)             */
    LH_ENODEVICE = 4,   /* no usable gfx950 device                           */
    LH_EBUSY = 5,       /* lh_flip: every epoch buffer still has a live snapshot */
    LH_ERANGE = 6,      /* metric id >= max_metrics / table full             */
    LH_ESTATE = 7       /* call not valid in this state                      */
};

typedef struct lh_engine lh_engine;
typedef struct lh_snapshot lh_snapshot;

typedef struct lh_config {
    uint32_t struct_size;   /* sizeof(lh_config), for ABI growth              */
    int32_t  device;        /* HIP device ordinal                             */
    uint32_t max_metrics;   /* dense rows per epoch buffer (512 KiB each)     */
    uint32_t num_buffers;   /* epoch buffers, >= 2                            */
    uint32_t num_lanes;     /* host staging lanes (one HIP stream each)       */
    uint32_t max_counters;  /* counter names (metrics.go:115), 8 B each per epoch buffer; 0 = no counters */
    uint64_t lane_samples;  /* samples per pinned half-buffer of a lane       */
    uint32_t cell_bits;     /* (ABI 7) width of a bucket cell in HBM: 64 = the reference's uint64 (metrics.go:278); 32 = an
                               epoch buffer counts in uint32 cells while its interval holds fewer than 2^32 samples -- no cell
                               can wrap -- and moves to a uint64 store of its own (allocated then, kept) before a submit could
                               pass that: exact for any stream, half the HBM and half the lines per window until then;
                               0 = default: 64 up to 8 192 names, 32 above.  A struct_size without this field means 0. */
    uint32_t reserved0;     /* 0 */
} lh_config;

/* Per-metric result of processHistograms (metrics.go:336-376). */
typedef struct lh_stats {
    uint64_t count;        /* totalCount                                      */
    double   sum;          /* totalSum (fixed parallel order)  */
    double   avg;          /* sum / float64(count); NaN when count == 0       */
    uint64_t agg_sum_add;  /* uint64(totalSum), amd64 conversion (metrics.go:374) */
    uint32_t nbuckets;     /* occupied buckets                                */
    uint32_t present;      /* 1 iff the metric received a sample this epoch   */
} lh_stats;

int lh_abi_version(void);
const char *lh_strerror(int code);
/* Thread-local text of the last HIP failure seen by this thread ("" if none). */
const char *lh_last_error(void);

int lh_default_config(lh_config *cfg);
/* NewMetricSystem (metrics.go:143) calls this; Stop (metrics.go:651) -> lh_destroy. */
int lh_create(const lh_config *cfg, lh_engine **out);
int lh_destroy(lh_engine *e);

/* name -> dense metric id (idempotent, thread-safe).  Replaces the string-keyed
 * outer map of histogramCache (metrics.go:119). */
int lh_intern(lh_engine *e, const char *name, size_t len, uint32_t *id);
int lh_lookup(lh_engine *e, const char *name, size_t len, uint32_t *id); /* LH_ERANGE if unknown */
int lh_num_metrics(lh_engine *e, uint32_t *n);
/* Copies up to cap bytes of the name (no terminator); *len receives the full length. */
int lh_metric_name(lh_engine *e, uint32_t id, char *buf, size_t cap, size_t *len);

/* Host-memory ingest: Histogram(name, v[i]) for i < n (metrics.go:273). */
int lh_submit(lh_engine *e, uint32_t id, const double *v, size_t n);
/* Mixed batch: Histogram(name(ids[i]), v[i]). */
int lh_submit_pairs(lh_engine *e, const uint32_t *ids, const double *v, size_t n);
/* In-place staging of a mixed batch (the other half of SURVEY.md 8b "Ownership": "the ring is C-allocated
 * (hipHostMalloc) and Go writes into it in place"; call shape of Histogram, metrics.go:273).  lh_reserve_pairs hands
 * out the free tail of one of the engine's pinned staging buffers: *ids / *vals point at room for *granted <= want
 * pairs, which the caller fills front to back -- the only host-side store a sample ever sees; the ingest kernel
 * later reads that memory over PCIe in place -- and lh_commit_pairs(token, n) publishes the first n <= *granted of
 * them (n = 0 gives the reservation back).  Between the two calls the buffer belongs to the caller: a flip, and
 * other producers that are sent to the same buffer, wait for the commit, so a producer commits before it blocks on
 * anything else.  Every reservation is committed exactly once; commit from any thread.  ids are not validated on
 * the host: an id >= max_metrics is skipped by the kernel and reported as LH_ERANGE by the next lh_sync / lh_flip
 * / lh_extract, as for lh_submit_pairs_device. */
int lh_reserve_pairs(lh_engine *e, size_t want, uint32_t **ids, double **vals, size_t *granted, uint32_t *token);
int lh_commit_pairs(lh_engine *e, uint32_t token, size_t n);
/* Device-memory ingest for GPU-resident producers; asynchronous on `stream`.
 * Ordering contract: the kernel is enqueued on `stream` (NULL = the engine's own non-blocking
 * stream, which does NOT synchronise with the legacy default stream).  The producer of the buffers
 * must therefore either run on the same stream or be complete before the call, and the buffers must
 * stay valid until the stream reaches this point (lh_sync / lh_flip + lh_extract imply it).  A
 * caller-owned stream must outlive the next lh_flip, which records an event on it. */
int lh_submit_device(lh_engine *e, uint32_t id, const double *d_v, size_t n, void *stream);
int lh_submit_pairs_device(lh_engine *e, const uint32_t *d_ids, const double *d_v, size_t n, void *stream);
/* The same three ways in with uint16 ids: 10 bytes per pair instead of 12 (SURVEY.md 8d "mixed stream: 12 B/sample ...
 * 10 B if ids are uint16, legal for <= 65 536 names").  Every mixed-ingest kernel is a template on the id width and
 * reads the narrow ids directly (two per 4-byte load), so nothing is widened on the way: the host-fed path moves 17 %
 * fewer bytes over PCIe, the device-resident path reads 17 % fewer from HBM.  Replaces the same Go lines as the
 * uint32 forms (body of Histogram, /root/reference/metrics.go:273-295); a binding uses them whenever the engine was
 * created with max_metrics <= 65 536.  A staging buffer holds one id width at a time: a producer that switches width
 * makes the library launch what the buffer holds first.  lh_commit_pairs16 == lh_commit_pairs (the token knows). */
int lh_submit_pairs16(lh_engine *e, const uint16_t *ids, const double *v, size_t n);
int lh_reserve_pairs16(lh_engine *e, size_t want, uint16_t **ids, double **vals, size_t *granted, uint32_t *token);
int lh_commit_pairs16(lh_engine *e, uint32_t token, size_t n);
int lh_submit_pairs16_device(lh_engine *e, const uint16_t *d_ids, const double *d_v, size_t n, void *stream);
/* Counters on the device.  Counter names have their own dense id space.
 *   (*MetricSystem).Counter           /root/reference/metrics.go:251-269  -> lh_intern_counter + lh_submit_counts
 *   collectRawMetrics, counter part   /root/reference/metrics.go:425-458  -> lh_flip (steals the interval's amounts
 *                                     together with the histogram cells) + lh_counters_collect (Rates = the
 *                                     interval's amounts of the names touched, Counters = lifetime totals of every
 *                                     name ever touched; the fold into the lifetime store happens once per snapshot)
 *   processMetrics / serializers      /root/reference/metrics.go:487-493  -> lh_serialize_counters ("<name>" and
 *                                     "<name>_rate" lines, Go's %f of float64(count))
 * Same conventions as the histogram ingest: lossless, thread-safe, the caller's buffers are copied. */
int lh_intern_counter(lh_engine *e, const char *name, size_t len, uint32_t *id);
int lh_num_counters(lh_engine *e, uint32_t *n);
int lh_counter_name(lh_engine *e, uint32_t id, char *buf, size_t cap, size_t *len);
/* Counter(name(ids[i]), amounts[i]) for i < n. */
int lh_submit_counts(lh_engine *e, const uint32_t *ids, const uint64_t *amounts, size_t n);
int lh_submit_counts_device(lh_engine *e, const uint32_t *d_ids, const uint64_t *d_amounts, size_t n, void *stream);
/* Counters [first, first+n) of the snapshot: rate[i] = amount added this interval, present[i] = 1 iff the name was
 * touched this interval (metrics.go:430-433), total[i] = lifetime total after this interval, known[i] = 1 iff the
 * name has ever been touched (metrics.go:435-458).  Any output may be NULL. */
int lh_counters_collect(lh_snapshot *s, uint32_t first, size_t n, uint64_t *rate, uint8_t *present, uint64_t *total,
                        uint8_t *known);
/* lh_serialize_counters (declared after lh_line_format below) writes them as wire lines. */

/* Push partially filled staging buffers to the device (asynchronous). */
int lh_flush(lh_engine *e);
/* Wait until every sample submitted so far is in the bucket arrays. */
int lh_sync(lh_engine *e);

/* Epoch boundary (metrics.go:460-463).  Returns LH_EBUSY if no epoch buffer is
 * free; the current epoch simply keeps accumulating in that case. */
int lh_flip(lh_engine *e, lh_snapshot **out);
/* processHistograms for metrics [0, nmetrics) of the snapshot.
 *   p[np]                     percentiles in [0,1] (metrics.go:145-155)
 *   stats[nmetrics]
 *   pvals[nmetrics*np]        always exactly some decompress(key)
 *   pkeys[nmetrics*np]        (may be NULL) the selected int16 keys
 *   pvalid[nmetrics*np]       (may be NULL) 0 where the reference returns
 *                             "Invalid percentile" (metrics.go:417) or count==0 */
int lh_extract(lh_snapshot *s, const double *p, size_t np, lh_stats *stats,
               double *pvals, int16_t *pkeys, uint8_t *pvalid, size_t nmetrics);
/* Same for metrics [first, first+nmetrics): the rows a rank owns after a
 * reduce-scatter merge. */
int lh_extract_rows(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np,
                    lh_stats *stats, double *pvals, int16_t *pkeys, uint8_t *pvalid);
/* The same without the last copy: the results are handed out IN PLACE, in the engine's pinned result buffer (a
 * cgo caller wraps them as slices without copying; at 65 536 names the copy into caller arrays would cost more
 * than the scan).  The pointers point into the engine's one pinned result block, which every call that returns
 * results through it rewrites (and may re-allocate): they stay valid until the next lh_extract*, lh_buckets*,
 * lh_serialize*, lh_counters_collect, lh_lifetime, lh_format_f or lh_snapshot_merge call on this engine, or
 * lh_release of the snapshot, whichever comes first.  A host layer that needs lifetime totals or counters for the
 * same interval reads the view first (or copies what it keeps) and then makes those calls. */
typedef struct lh_extract_view {
    const lh_stats *stats;   /* [nmetrics]      */
    const double *pvals;     /* [nmetrics * np] */
    const int16_t *pkeys;    /* [nmetrics * np] */
    const uint8_t *pvalid;   /* [nmetrics * np] */
    size_t nmetrics, np;
} lh_extract_view;
int lh_extract_rows_view(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np,
                         lh_extract_view *view);
/* The COMPACT form of the same results, for large name spaces (round 6).  processHistograms emits 3 + P floats per
 * name (metrics.go:349-356, 378-385), but only count, sum and the P selected KEYS are information: avg is
 * sum / float64(count), uint64(sum) a conversion, and every percentile value is exactly decompress(key) -- the table
 * D[] that lh_codec_tables exports.  This call brings 8 + 8 + 4 + 4 + 2 P bytes per name to the host (42 B at the nine
 * default percentiles against 139 B: at 65 536 names 2.75 MB instead of 9.1 MB over PCIe, which was more than half of
 * the flip -> results latency), in place in the engine's pinned block under lh_extract_rows_view's lifetime rule.
 *   count[nmetrics], sum[nmetrics], nbuckets[nmetrics]
 *   pkeys[nmetrics * np]     the selected int16 keys (0 where the percentile has no bucket)
 *   pvalid_bits[nmetrics]    bit i set iff percentile i has a bucket (np <= LH_MAX_PERCENTILES = 32)
 * lh_expand_compact derives the full form from it ON THE HOST, bit for bit what lh_extract_rows returns for the same
 * snapshot (present = count != 0, avg = sum / float64(count), agg_sum_add = uint64(sum) with the amd64 conversion,
 * pvals = D[key]); a binding that formats keys itself reads D[] once (lh_codec_tables) and never expands.  Any of
 * stats / pvals / pkeys / pvalid may be NULL. */
typedef struct lh_extract_compact {
    const uint64_t *count;
    const double *sum;
    const uint32_t *nbuckets;
    const uint32_t *pvalid_bits;
    const int16_t *pkeys;
    size_t nmetrics, np;
} lh_extract_compact;
int lh_extract_rows_compact(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np,
                            lh_extract_compact *view);
int lh_expand_compact(lh_engine *e, const lh_extract_compact *c, lh_stats *stats, double *pvals, int16_t *pkeys,
                      uint8_t *pvalid);
/* Occupied cells of one metric, ascending key. *n receives the number of
 * occupied cells even when it exceeds cap. */
int lh_buckets(lh_snapshot *s, uint32_t id, int16_t *keys, uint64_t *counts, size_t cap, size_t *n);
/* The same for metrics [first, first+nmetrics) at once, compacted on the device: CSR arrays with
 * offsets[nmetrics+1]; metric first+i owns keys/counts[offsets[i] .. offsets[i+1]).  *total receives
 * the number of occupied cells; if it exceeds cap only offsets/total are filled (size and call again).
 * This is RawMetricSet.Histograms (metrics.go:54-60) for every name in one crossing. */
int lh_buckets_all(lh_snapshot *s, uint32_t first, size_t nmetrics, uint64_t *offsets, int16_t *keys,
                   uint64_t *counts, size_t cap, size_t *total);
/* Dense device view of the snapshot for the multi-GPU merge: row r of metric r
 * is (uint64 *)d_counts + r * lh_row_stride(), LH_NKEYS cells long (bin = key ^ 0x8000).
 * The rows are NOT back to back: lh_row_stride() > LH_NKEYS (ABI 5; rows exactly 512 KiB
 * apart put every name's occupied window on the same low address bits -- DESIGN.md 4).
 * After an in-place reduction the caller must call lh_snapshot_mark_dirty so that
 * extract/clear cover the merged cells. */
int lh_snapshot_rows(lh_snapshot *s, void **d_counts, uint32_t *nrows);
size_t lh_row_stride(void); /* in cells */
/* (ABI 7) On an engine of 32-bit cells (lh_config.cell_bits) lh_snapshot_rows first moves the snapshot to its uint64 store
 * (one pass over the occupied windows; the store is allocated the first time: LH_ENOMEM if it cannot be had), so that the
 * view above stays what it was.  lh_snapshot_cells hands out the cells as they are: row r is at
 * (char *)d_cells + r * lh_row_stride() * cell_bytes, cell_bytes = 4 or 8.  lh_cell_bytes: the width an engine's epoch
 * buffers START every interval with (4 or 8). */
int lh_snapshot_cells(lh_snapshot *s, void **d_cells, uint32_t *nrows, uint32_t *cell_bytes);
int lh_cell_bytes(lh_engine *e);
int lh_snapshot_ranges(lh_snapshot *s, void **d_ranges /* uint32[nrows][2] lo,hi bins */);
int lh_snapshot_mark_dirty(lh_snapshot *s, uint32_t first_row, uint32_t nrows, uint32_t lo_bin, uint32_t hi_bin);
/* Cells back IN: the inverse of lh_buckets / lh_buckets_all.  An interval that already exists in bucket form -- another
 * process's RawMetricSet.Histograms, name -> {int16 key -> count} (/root/reference/metrics.go:54-60), an older interval
 * of this engine (1 s -> 10 s / 60 s roll-ups), a checkpoint -- is added to the snapshot per CELL, not per sample: cells
 * are a commutative integer sum (atomic.AddUint64, /root/reference/metrics.go:278, 292), so the percentile scan, the
 * lifetime stores and lh_serialize then work on the merged interval unchanged.  No communicator, no peer engine.
 *   lh_snapshot_add_buckets             snapshot[ids[i]][keys[i]] += counts[i] for i < n.  Host arrays, copied before
 *                                       the call returns.
 *   lh_snapshot_add_buckets_csr         metric first + i gets keys / counts[offsets[i] .. offsets[i + 1]), i < nmetrics:
 *                                       exactly what lh_buckets_all hands out.  Host arrays, copied likewise.
 *   lh_snapshot_add_buckets_device,     the same two with device arrays, enqueued on the snapshot's stream
 *   lh_snapshot_add_buckets_csr_device  (lh_snapshot_stream): the producer of the arrays runs on that stream or is
 *                                       complete; the arrays stay valid until the stream passes this point.
 * Entries come in any order, keys unsorted, duplicates allowed (several entries of one cell add up); a cell wraps mod
 * 2^64 as the reference's does.  Entries with count == 0 are skipped entirely: they touch neither a cell nor a row's
 * dirty span, so nbuckets and `present` do not see them.  Every int16 is a valid key (bin = (uint16)key ^ 0x8000).
 * ALL OR NOTHING: an id >= max_metrics or first + nmetrics > max_metrics -> LH_ERANGE, offsets that are not
 * non-decreasing from offsets[0] -> LH_EINVAL, and no cell has been added.  The host forms check while they read; the
 * device forms run a pre-pass over ids / offsets / counts and read one small result back (one stream wait per call)
 * before the add is enqueued.  n == 0, an all-empty CSR or nothing but zero counts: LH_OK, nothing touched.  NULL or
 * misaligned arrays (counts and offsets 8, ids 4, keys 2 bytes) -> LH_EINVAL without touching a device.
 * The adds run on the uint64 rows of lh_snapshot_rows: a snapshot of 32-bit cells moves to its wide store first
 * (allocated then, kept; LH_ENOMEM if it cannot be had, nothing added), so any count is exact, a single cell >= 2^32
 * included.  Every touched row's [lo, hi] in lh_snapshot_ranges ends as the TIGHT union of what it was and the bins
 * added -- extract and clear cover the new cells and nothing more -- and the buffer's cell sizes count as unknown to a
 * later lh_snapshot_merge (lh_snapshot_mark_dirty, on one added cell).
 * One thread per snapshot, as for lh_snapshot_merge.  Import BEFORE lh_snapshot_accumulate if the lifetime stores are
 * to include the imported cells (it applies once per snapshot); every later lh_extract* / lh_buckets* / lh_serialize
 * sees them.  Names need to be interned only for what requires it anyway (lh_serialize). */
int lh_snapshot_add_buckets(lh_snapshot *s, const uint32_t *ids, const int16_t *keys, const uint64_t *counts, size_t n);
int lh_snapshot_add_buckets_csr(lh_snapshot *s, uint32_t first, size_t nmetrics, const uint64_t *offsets,
                                const int16_t *keys, const uint64_t *counts);
int lh_snapshot_add_buckets_device(lh_snapshot *s, const uint32_t *d_ids, const int16_t *d_keys,
                                   const uint64_t *d_counts, size_t n);
int lh_snapshot_add_buckets_csr_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const uint64_t *d_offsets,
                                       const int16_t *d_keys, const uint64_t *d_counts);
/* Counts at or below given values: the read-side counterpart of the import above, and the one query whose answers can be
 * SUMMED across intervals, ranks and processes ("how many requests finished within 250 ms", an SLO / Apdex ratio, the
 * fixed-boundary cumulative `le` buckets of a scraper).  It is the running count of percentile()'s bucket walk
 * (/root/reference/metrics.go:389-418: `sofar += *count` over the cells in ascending key order) read at a VALUE instead of
 * searched for a fraction, over the interval's cells (RawMetricSet.Histograms, metrics.go:54-60; filled by
 * atomic.AddUint64, metrics.go:278):
 *   cum[m * nb + j] = number of samples of metric first + m, in this snapshot, whose bucket key is <= the key of bounds[j]
 *   total[m]        = all of its samples (the +Inf bucket; lh_stats.count)
 * RESOLUTION IS THE BUCKET.  A bound b is mapped to the key compress(b) (metrics.go:316-322) by the arithmetic the ingest's
 * threshold table is generated with; every sample v <= b is counted (compress is monotone), and so are the samples > b that
 * share b's bucket (within 1 % of 1 + |v|, the histogram's own precision).  For b = decompress(k) the count is exactly the
 * cells with key <= k.
 *   bounds   a HOST array in both forms: nb doubles shared by all names, or, with LH_LE_PER_METRIC, nmetrics * nb doubles,
 *            row m for metric first + m (SLO thresholds differ per endpoint).  Each row non-decreasing (equal neighbours
 *            allowed); -0.0 == 0.0.  +Inf takes in everything (cum == total), -Inf nothing (0) -- an infinite SAMPLE lies
 *            in bucket 0, where the ingest puts it.  A finite bound whose extended key floor(100 Log(1 + |b|) + 0.5) exceeds
 *            32 767 (|b| >~ 1.9e142, where the reference's int16 keys wrap) saturates the same way: everything for b > 0,
 *            nothing for b < 0.
 *   LH_EINVAL, checked on the host before the snapshot or a device is touched: NULL s; nb == 0 or nb > LH_MAX_BOUNDS; NULL
 *            bounds; both outputs NULL (either one may be); a NaN bound; a decreasing row; unknown flag bits; arrays not
 *            8-byte aligned.  first + nmetrics > max_metrics -> LH_ERANGE.  nmetrics == 0 -> LH_OK, nothing written.  The rows of
 *            per-metric bounds are checked before the snapshot is looked at: bounds holds nmetrics * nb doubles whatever
 *            the call returns (an nmetrics no engine can have, above 2^32 - 1, is LH_ERANGE before a bound is read).
 * READ-ONLY: no cell, span or cell width of the snapshot changes (the kernels read lh_snapshot_cells as they are: a snapshot
 * of 32-bit cells stays one).  Works on whatever the snapshot holds: ingested, imported, merged, widened.
 * Ordering and threading as for lh_snapshot_add_buckets*: enqueued on lh_snapshot_stream(s), one thread per snapshot.
 * lh_count_le returns when the results are in the caller's arrays (host arrays that are pinned -- hipHostMalloc'ed or
 * registered -- receive them by one copy, others through a pinned block of the library's).  lh_count_le_device returns
 * after enqueueing; d_cum / d_total are device arrays that stay valid until the stream passes that point.  Per-metric
 * bounds are copied before either call returns (a device-form call may first wait for the previous per-metric call's
 * kernel, which reads that copy).  The unit's staging blocks are one set per DEVICE: calls on snapshots of different
 * engines on one device are safe from any threads but take turns, a host-form call for its whole round trip.  Counts are exact uint64 sums; a total past 2^64 wraps as the reference's would. */
#define LH_MAX_BOUNDS 64
enum { LH_LE_PER_METRIC = 1 };
int lh_count_le(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags,
                uint64_t *cum, uint64_t *total);
int lh_count_le_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *bounds, size_t nb, uint32_t flags,
                       uint64_t *d_cum, uint64_t *d_total);
/* Spread and percentile-trimmed sums per name: what statsd emits as std / mean_90 / sum_90 / count_90 / upper_90, a
 * Coda-Hale-style registry as stddev, and the "tail mean" of the slowest few per cent.  One more weighted walk of the kind
 * processHistograms does (/root/reference/metrics.go:342-346: `sum += value * float64(*count)` over the buckets), cut at the
 * bucket percentile() selects (metrics.go:406-418).  With c[b] the cells of metric first + m (RawMetricSet.Histograms,
 * metrics.go:54-60) and D[b] = decompress(key of bin b) (metrics.go:326-332), bit for bit the D[] of lh_codec_tables:
 *   count[m] = sum of c[b]                          (uint64; wraps past 2^64 as the reference's would; lh_stats.count)
 *   sum[m]   = sum of D[b] * float64(c[b])          (metrics.go:344)
 *   m2[m]    = sum of float64(c[b]) * (D[b] - mean)^2, mean = sum / float64(count): the CENTRED second moment, taken in a
 *              second walk of the row -- not a difference of raw power sums, so a name whose samples share one bucket has
 *              a spread of (numerically) zero rather than rounding noise.  count == 0: sum and m2 are 0.
 * and for each p[i], at the bucket percentile() selects -- the first bin whose inclusive prefix count reaches
 * T = min{s in [1, total] : float64(s) / float64(total) >= p} (metrics.go:413):
 *   pkeys[m * np + i], pvalid[m * np + i]   what lh_extract_rows returns for the same snapshot and p (p unsorted, repeated,
 *                                           0, 1, > 1 or NaN included: the last two have no bucket, pvalid 0)
 *   count_le[m * np + i]                    the inclusive prefix count at that bin
 *   sum_le[m * np + i]                      sum of D[b] * float64(c[b]) over the bins up to and including it
 * Where pvalid is 0 the key, count_le and sum_le are 0.  RESOLUTION IS THE BUCKET, as for lh_count_le: every sample of the
 * selected bucket is taken in, so count_le / count may exceed p by that bucket's share.
 * What a caller derives (Snapshot.spread in the Python binding does):
 *   std = sqrt(m2 / count)      mean_p = sum_le / count_le      upper_p = D[pkey]
 *   tail mean = (sum - sum_le) / (count - count_le)             (the samples above the percentile's bucket)
 * Floating-point sums are taken in a fixed order: a result does not depend on timing (it may differ in the last bits
 * between calls that cover different numbers of rows, which use differently shaped kernels, and from lh_stats.sum).
 *   np <= LH_MAX_PERCENTILES; np == 0 is allowed: moments only, the four per-percentile outputs are ignored.
 *   Any output may be NULL, but not all of them.
 *   LH_EINVAL, checked on the host before the snapshot or a device is touched: NULL s; np too large; np > 0 with NULL p;
 *            all outputs NULL; arrays not aligned to their element size.  first + nmetrics > max_metrics -> LH_ERANGE.
 *            nmetrics == 0 -> LH_OK, nothing written.
 * READ-ONLY, ordering, threading and staging as for lh_count_le*: enqueued on lh_snapshot_stream(s); lh_spread returns when
 * the results are in the caller's arrays (pinned arrays receive them by one copy each, others go through a pinned block of
 * the library's); lh_spread_device takes device arrays and returns after enqueueing (the first call on a device also
 * generates the unit's copy of D[] and waits for it once).  p is a HOST array in both forms and travels by value.  One set
 * of staging blocks per DEVICE behind a mutex: calls on snapshots of different engines take turns. */
int lh_spread(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np, uint64_t *count, double *sum,
              double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le);
int lh_spread_device(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, size_t np, uint64_t *d_count,
                     double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le,
                     double *d_sum_le);
/* The k names that lead: "which 20 endpoints have the worst p99 this interval", "which names took the most total time",
 * "which names have the most requests over 250 ms" -- answered on the device, so that k entries travel instead of the
 * results of every name.  The reference has no counterpart for the SELECTION (its consumers receive every name's
 * ProcessedMetricSet entries and sort for themselves); what is ranked is what it computes and this library already returns:
 * the outputs of processHistograms (/root/reference/metrics.go:336-376), the bucket percentile() selects
 * (metrics.go:389-418), and the running count lh_count_le reads at a value.  Nothing is summed across names and no new
 * statistic is defined.
 *   CANDIDATES  the rows of [first, first + nmetrics) with count != 0.  *n_out = min(k, candidates); entries at and beyond
 *               n_out are not written.
 *   SCORE, by `by`:
 *     LH_TOP_BY_COUNT        count (uint64, lh_stats.count)
 *     LH_TOP_BY_SUM          sum as a float64, compared numerically (-0.0 == +0.0)
 *     LH_TOP_BY_PERCENTILE   the bin of the bucket lh_extract_rows selects for p = arg; ascending bin is ascending value, so
 *                            a negative p99 ranks below a positive one
 *     LH_TOP_BY_COUNT_ABOVE  count minus the name's lh_count_le result at bounds = {arg}: the samples in buckets whose key is
 *                            > the key of arg, by lh_count_le's bound-to-key rule (+Inf: nothing is above; -Inf: everything;
 *                            a finite arg whose extended key exceeds 32 767 saturates the same way).  RESOLUTION IS THE
 *                            BUCKET, as there.
 *     arg is ignored for the first two.
 *   ORDER  one total order, so the result never depends on timing or launch shape: descending score, or ascending score with
 *          LH_TOP_ASCENDING; in BOTH directions equal scores go lowest id first.  out[0] is the leader.
 *   FIELDS  id is absolute (first + i).  count and sum are filled for every entry whatever `by` is; pkey for
 *           LH_TOP_BY_PERCENTILE only and above for LH_TOP_BY_COUNT_ABOVE only (0 otherwise); reserved is 0.  sum is taken in
 *           this unit's own fixed order: it does not depend on timing, and may differ in the last bits from lh_stats.sum and
 *           lh_spread's.
 *   LH_EINVAL, checked on the host before the snapshot or a device is touched: NULL s; k == 0 or k > LH_MAX_TOP; unknown `by`;
 *           unknown flag bits; NULL out or n_out; out not 8-byte aligned; n_out not aligned to its type (size_t in lh_top,
 *           uint32_t in lh_top_device); arg NaN for LH_TOP_BY_PERCENTILE or LH_TOP_BY_COUNT_ABOVE; arg outside [0, 1] for
 *           LH_TOP_BY_PERCENTILE (there would be no bucket to rank by).
 *   LH_ERANGE: first + nmetrics > max_metrics; an nmetrics above 2^32 - 1 before anything is looked at.
 *   nmetrics == 0 -> LH_OK with *n_out = 0.
 * READ-ONLY, ordering, threading and staging as for lh_spread*: enqueued on lh_snapshot_stream(s) (a pass that scores every
 * row, one wave per row, then an exact radix select and a sort of the winners in one workgroup); lh_top returns when the
 * entries are in `out` -- entries and n_out come back in one copy through a pinned block of the library's, whatever memory
 * `out` is, because only the first n_out entries may be written; lh_top_device takes device memory for both and returns
 * after enqueueing (the first call on a device also generates the unit's copy of D[] and waits for it once).  One set of
 * staging blocks per DEVICE behind the unit's own mutex: calls on snapshots of different engines take turns. */
#define LH_MAX_TOP 1024
enum { LH_TOP_BY_COUNT = 0, LH_TOP_BY_SUM = 1, LH_TOP_BY_PERCENTILE = 2, LH_TOP_BY_COUNT_ABOVE = 3 };
enum { LH_TOP_ASCENDING = 1 };
typedef struct lh_top_entry {   /* 32 bytes */
    uint32_t id;        /* absolute metric id (first + i), not the index inside the range */
    int16_t  pkey;      /* BY_PERCENTILE: the selected int16 key; else 0 */
    uint16_t reserved;  /* 0 */
    uint64_t count;     /* lh_stats.count of the name */
    double   sum;       /* sum of D[b] * float64(c[b]) (metrics.go:344), this unit's fixed order */
    uint64_t above;     /* BY_COUNT_ABOVE: samples in buckets whose key is > the key of arg; else 0 */
} lh_top_entry;
int lh_top(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
           lh_top_entry *out, size_t *n_out);
int lh_top_device(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags,
                  lh_top_entry *d_out, uint32_t *d_n_out);
/* How a name's distribution in one snapshot differs from its distribution in another: "which names changed against the
 * previous interval", "does the canary's latency match the baseline's", "did the deploy shift p-anything" -- answered on the
 * device, where both intervals already are (num_buffers >= 3 keeps the previous snapshot alive across a flip;
 * lh_snapshot_add_buckets* puts a stored baseline into a snapshot; lh_kept_compare* below compares intervals kept in compact
 * form without one), instead of pulling both intervals' cells to the host with
 * lh_buckets_all.  One more bucket walk of the kind percentile() does (/root/reference/metrics.go:389-418), over two rows at
 * once.  For metric first + m, with a[j] the cells of `base` and b[j] the cells of `cur` in ascending bin order (ascending bin
 * is ascending value), A_j and B_j their inclusive prefix counts and na, nb the totals:
 *   count_a[m], count_b[m]   na and nb
 *   Kolmogorov-Smirnov, decided in exact integers: X_j = |A_j nb - B_j na| (128 bits), j* = the LOWEST bin at which X_j
 *   reaches its maximum;
 *   ks_key[m]                the int16 key of bin j*
 *   ks_below_a[m], ks_below_b[m]   A_j* and B_j*
 *   ks[m]                    fabs((double)A_j* / (double)na - (double)B_j* / (double)nb), both divides IEEE
 *                            A maximum of 0 means the two normalised distributions are identical: ks = 0, the key and both
 *                            prefixes are 0 (whatever the rows' dirty spans are).  The argmax is never taken in floating point.
 *   w1[m]                    sum over the bins j of |A_j / na - B_j / nb|: the earth mover's distance in BUCKETS (100 buckets
 *                            are one e-fold, so w1 per cent is roughly the mean relative shift)
 *   shift[m]                 the same sum without the absolute value: positive means `cur` sits higher; |shift| <= w1
 * Each term of the two sums is X_j / (na nb) with the sign of A_j nb - B_j na, rounded three times (no two rounded quotients
 * cancel).  Bins outside the union of the two rows' dirty spans contribute nothing; empty bins inside it do.  Both sums are
 * taken in a fixed order: a result does not depend on timing (calls that cover different numbers of rows use differently
 * shaped kernels and may differ in the last bits).
 * A name with na == 0 or nb == 0: ks, w1 and shift are NaN, the key and both prefixes 0; the counts are still reported.
 * Totals that wrap past 2^64: the results are unspecified (nothing faults).
 *   Any output may be NULL, but not all of them.  flags must be 0.  nmetrics == 0 -> LH_OK, nothing written.
 *   LH_EINVAL, checked on the host before either snapshot or a device is touched: NULL base or cur; all outputs NULL; unknown
 *            flag bits; arrays not aligned to their element size.
 *   LH_ERANGE: an nmetrics above 2^32 - 1 before anything is looked at; first + nmetrics beyond the rows of EITHER snapshot
 *            (the two engines may have different max_metrics).
 *   base == cur is allowed: every ks, w1 and shift of a non-empty name is exactly 0.
 *   Two snapshots on different devices -> LH_EINVAL (after both were opened).
 * ORDERING: the work is enqueued on lh_snapshot_stream(cur).  When base's stream is another one (a snapshot of another
 * engine) an event recorded on base's stream is waited for by cur's first, so whatever base's stream held at the call is
 * complete before a cell of base is read.  base must NOT be released before cur's stream has passed the call
 * (lh_compare_device; lh_compare has waited already when it returns).  One thread per snapshot, as for the other readers.
 * READ-ONLY: no cell, span or cell width of either snapshot changes; the kernels read lh_snapshot_cells as they are, in all
 * four combinations of 4- and 8-byte cells (a narrow snapshot against one that an import has widened).
 * Staging as for lh_spread*: lh_compare returns when the results are in the caller's arrays (pinned arrays receive them by
 * one copy each, others go through a pinned block of the library's); lh_compare_device takes device arrays and returns after
 * enqueueing.  One set of staging blocks per DEVICE behind the unit's own mutex: calls take turns. */
int lh_compare(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t flags, uint64_t *count_a,
               uint64_t *count_b, double *ks, int16_t *ks_key, uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1,
               double *shift);
int lh_compare_device(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t flags,
                      uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks, int16_t *d_ks_key, uint64_t *d_ks_below_a,
                      uint64_t *d_ks_below_b, double *d_w1, double *d_shift);
/* The k names whose distribution moved most between two snapshots: "which 20 of my 65 536 endpoints changed most since the
 * last interval, or against the baseline", "whose p99 moved most" -- lh_compare* and lh_top* joined on the device, so that k
 * entries travel instead of eight arrays over every name (or two full extracts and a host join).  The walk is lh_compare's:
 * the bucket walk of percentile() (/root/reference/metrics.go:389-418) over two rows at once.  The reference has no
 * counterpart for the SELECTION.  Nothing is summed across names, no cell is written and no new statistic is defined: every
 * score is a value lh_compare or lh_extract_rows already returns.
 *   CANDIDATES  the rows of [first, first + nmetrics) with count_a != 0 and count_b != 0 (for the others lh_compare returns
 *               NaN, and a NaN is never ranked).  *n_out = min(k, candidates); entries at and beyond n_out are not written.
 *   SCORE, always a float64, by `by`:
 *     LH_MOVERS_BY_KS          ks[m] of lh_compare(base, cur, ...): bit-equal to it in either of its kernel shapes (a fixed
 *                              function of exact integers)
 *     LH_MOVERS_BY_W1          w1[m], bit-equal to what lh_compare returns from its wave-per-row kernel (calls of 1 024 rows
 *                              or more by default): the same steps, the same per-lane order and the same tree over the lanes
 *     LH_MOVERS_BY_SHIFT       shift[m], as w1; the SIGNED value is ranked: descending gives the names that moved up most,
 *                              LH_MOVERS_ASCENDING those that moved down most
 *     LH_MOVERS_BY_PERCENTILE  (double)((int64)bin_cur - (int64)bin_base), bin_x the bin of the bucket lh_extract_rows selects
 *                              for p = arg in that snapshot: an exact integer in BUCKETS (100 buckets are one e-fold, so
 *                              score / 100 is roughly the log ratio of the two percentile values)
 *     arg is ignored for the first three.
 *   ORDER  one total order, so the result never depends on timing or launch shape: descending score, or ascending score with
 *          LH_MOVERS_ASCENDING; in BOTH directions equal scores go lowest id first.  Scores compare numerically
 *          (-0.0 == +0.0).  out[0] is the leader.
 *   FIELDS  id is absolute (first + i).  count_a and count_b are the name's totals in base and cur, whatever `by` is.  key is
 *           lh_compare's ks_key for LH_MOVERS_BY_KS and the int16 key selected in cur for LH_MOVERS_BY_PERCENTILE; key_base
 *           the one selected in base for LH_MOVERS_BY_PERCENTILE; both 0 otherwise.
 *   LH_EINVAL, checked on the host before either snapshot or a device is touched: NULL base or cur; k == 0 or
 *           k > LH_MAX_TOP; unknown `by`; unknown flag bits; NULL out or n_out; out not 8-byte aligned; n_out not aligned to
 *           its type (size_t in lh_movers, uint32_t in lh_movers_device); LH_MOVERS_BY_PERCENTILE with arg NaN or outside
 *           [0, 1].
 *   LH_ERANGE: an nmetrics above 2^32 - 1 before anything is looked at (a cause of LH_EINVAL wins over it); first + nmetrics
 *           beyond the rows of EITHER snapshot.
 *   Two snapshots on different devices -> LH_EINVAL (after both were opened).  nmetrics == 0 -> LH_OK with *n_out = 0.
 *   base == cur is allowed: every candidate scores 0 and the lowest ids win.
 *   Totals that wrap past 2^64: the results are unspecified (nothing faults).
 * ORDERING and threading as for lh_compare*: enqueued on lh_snapshot_stream(cur), behind an event on base's stream when the
 * two differ; base must not be released before cur's stream has passed the call.  READ-ONLY in all four combinations of 4- and
 * 8-byte cells.  Staging as for lh_top*: a pass that scores every row (one wave per row) into a records block in device
 * memory, then lh_top's exact radix select and sort in one workgroup; lh_movers returns when the entries are in `out` --
 * entries and n_out come back in one copy through a pinned block of the library's; lh_movers_device takes device memory
 * for both and returns after enqueueing.  One records block per DEVICE behind the unit's own mutex: calls take turns. */
enum { LH_MOVERS_BY_KS = 0, LH_MOVERS_BY_W1 = 1, LH_MOVERS_BY_SHIFT = 2, LH_MOVERS_BY_PERCENTILE = 3 };
enum { LH_MOVERS_ASCENDING = 1 };
typedef struct lh_mover_entry {   /* 32 bytes */
    uint32_t id;        /* absolute metric id (first + i) */
    int16_t  key;       /* BY_KS: ks_key of lh_compare; BY_PERCENTILE: the key selected in cur; else 0 */
    int16_t  key_base;  /* BY_PERCENTILE: the key selected in base; else 0 */
    uint64_t count_a;   /* the name's total in base */
    uint64_t count_b;   /* ... in cur */
    double   score;     /* what was ranked */
} lh_mover_entry;
int lh_movers(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
              uint32_t flags, lh_mover_entry *out, size_t *n_out);
int lh_movers_device(lh_snapshot *base, lh_snapshot *cur, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                     uint32_t flags, lh_mover_entry *d_out, uint32_t *d_n_out);
/* Stats and percentiles of a name over SEVERAL snapshots at once: "p99 over the last 10 seconds while emitting every second",
 * or one answer over the ranks and engines of one device.  Counts add across intervals (lh_count_le) and percentiles do not:
 * a percentile over K intervals needs the K rows of cells added together and walked once.  The rows are already side by side
 * in device memory (num_buffers >= K + 1 keeps K snapshots alive; an engine has at most 16 buffers, so a list of 16 takes
 * snapshots of more than one engine, or one of them twice), so the walk of lh_compare* is taken over up to
 * LH_MAX_ACROSS rows and gives what lh_extract_rows gives, for the summed row.  Nothing is summed across names, no cell is
 * written and no new statistic is defined: the sum is over time (or ranks) for ONE name, the cell atomic.AddUint64 would have
 * left had the samples arrived in one interval (metrics.go:278, 292).
 * With c_i[b] the cells of metric first + m in snaps[i] and C[b] = sum over i of c_i[b], taken in 64 bits (two narrow cells
 * of 0xffffffff give 0x1fffffffe, not a 32-bit wrap), and D[b] bit for bit the D[] of lh_codec_tables:
 *   count[m]         sum of C[b] (uint64; wraps past 2^64 as the reference's would)
 *   sum[m]           sum of D[b] * float64(C[b]) (metrics.go:344), in one fixed order: it does not depend on timing (it may
 *                    differ in the last bits between calls that cover different numbers of rows, which use differently shaped
 *                    kernels, and from lh_stats.sum)
 *   nbuckets[m]      the number of bins with C[b] != 0
 *   present_bits[m]  bit i set iff snaps[i] holds at least one sample of the name
 *   pkeys[m * np + i], pvalid[m * np + i]   the bucket percentile() selects on C (metrics.go:389-418): the first bin whose
 *                    inclusive prefix count reaches T = min{s in [1, count] : float64(s) / float64(count) >= p[i]} -- bit
 *                    for bit what lh_extract_rows returns for a snapshot that holds C (p unsorted, repeated, 0, 1, > 1 or NaN
 *                    included: the last two have no bucket, pvalid 0 and key 0)
 *   count == 0: sum 0, nbuckets 0, present_bits 0, every pvalid and key 0.
 *   1 <= nsnaps <= LH_MAX_ACROSS.  A snapshot may appear more than once and counts that often; nsnaps == 1 gives that
 *   snapshot's own lh_extract_rows keys.  np <= LH_MAX_PERCENTILES; np == 0 is allowed: the two per-percentile outputs are
 *   ignored.  Any output may be NULL, but not all of them.  flags must be 0.  nmetrics == 0 -> LH_OK, nothing written.
 *   Totals that wrap past 2^64: count wraps, the percentile outputs are unspecified (nothing faults).
 *   LH_EINVAL, checked on the host before any snapshot or a device is touched: NULL snaps or a NULL entry; nsnaps 0 or too
 *            large; np too large; np > 0 with NULL p; all outputs NULL; unknown flag bits; arrays not aligned to their
 *            element size.
 *   LH_ERANGE: an nmetrics above 2^32 - 1 before anything is looked at (a cause of LH_EINVAL wins over it); first + nmetrics
 *            beyond the rows of ANY snapshot (the engines may have different max_metrics).
 *   Snapshots on different devices -> LH_EINVAL (after all were opened).
 * THE WINDOW IS BOUNDED BY DEVICE MEMORY, not by this call: K snapshots must be alive at once, and at 8 192 names a buffer of
 * 64-bit cells is 4 GiB, at 65 536 names a narrow one 16 GiB.  LH_MAX_ACROSS = 16 is for small and mid name counts and
 * roll-ups of 1 s into 10 s; a minute of history belongs in imports (lh_snapshot_add_buckets*).
 * ORDERING: the work is enqueued on lh_snapshot_stream(snaps[nsnaps - 1]); for every other distinct stream of the list an
 * event recorded there is waited for first.  No snapshot of the list may be released before that stream has passed the call
 * (lh_across_device; lh_across has waited already when it returns).  One thread per snapshot, as for the other readers.
 * READ-ONLY: no cell, span or cell width of any snapshot changes; every snapshot is read at its own width through
 * lh_snapshot_cells, 4 or 8 bytes, in any mixture.
 * Staging as for lh_spread*: lh_across returns when the results are in the caller's arrays (pinned arrays receive them by
 * one copy each, others go through a pinned block of the library's); lh_across_device takes device arrays and returns after
 * enqueueing (the first call on a device also generates the unit's copy of D[] and waits for it once).  p is a HOST array in
 * both forms and travels by value.  One set of staging blocks per DEVICE behind the unit's own mutex: calls take turns. */
#define LH_MAX_ACROSS 16
int lh_across(lh_snapshot *const *snaps, size_t nsnaps, uint32_t first, size_t nmetrics, const double *p, size_t np,
              uint32_t flags, uint64_t *count, double *sum, uint32_t *nbuckets, uint32_t *present_bits, int16_t *pkeys,
              uint8_t *pvalid);
int lh_across_device(lh_snapshot *const *snaps, size_t nsnaps, uint32_t first, size_t nmetrics, const double *p, size_t np,
                     uint32_t flags, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets, uint32_t *d_present_bits,
                     int16_t *d_pkeys, uint8_t *d_pvalid);
/* ROWS BY ID LIST: lh_across_ids*, lh_count_le_ids*, lh_spread_ids*.  The base forms above address names as one block
 * [first, first + nmetrics); ids are handed out in lh_intern order, so the names a caller wants together -- the k ids lh_top* or
 * lh_movers* returned, the endpoints of a dashboard, the names that have an SLO -- are almost never one block.  These forms
 * take the rows from an array of n ids instead of (first, nmetrics) and are otherwise the base form, word for word: the same
 * kernels read row ids[m] where the base form reads row first + m (one uniform load per row), nothing is summed across names
 * and no new statistic is defined.  lh_across_ids with nsnaps == 1 is the id-list form of the compact extract (count, sum,
 * nbuckets and the percentile keys of lh_extract_rows_compact).
 *   Entry m of every output describes row ids[m], bit for bit what the base form returns for that row in a call of the same
 *   kernel shape (the shape is chosen by n, the number of entries, as the base form's is by nmetrics).  Per-percentile and
 *   per-bound outputs are [n * np] / [n * nb], row m for ids[m]; with LH_LE_PER_METRIC row m of `bounds` ([n * nb]) belongs to
 *   ids[m].  ids may be in any order and may hold an id more than once -- each occurrence gets its own, equal entry -- and n is
 *   not bounded by the number of rows.  n == 0 -> LH_OK, nothing written, before any device call.
 *   HOST FORMS (lh_*_ids: ids is a host array): ids is copied before the call returns.  Every id is checked against the rows
 *   of the snapshot -- for lh_across_ids of every snapshot of the list, i.e. against the smallest number of rows: an id at or
 *   beyond it -> LH_ERANGE, nothing is enqueued and no output is written.
 *   DEVICE FORMS (lh_*_ids_device: d_ids is a device array, valid until the stream has passed the call): the call returns
 *   after enqueueing, like the base device forms -- no pre-pass and no host wait, so the ids lh_top_device has just written
 *   can be used on the same stream without a round trip.  The host never sees these ids (the stance lh_reserve_pairs takes):
 *   THE KERNEL READS NOTHING FOR AN ID AT OR BEYOND THE ROWS of the snapshot (for lh_across_ids_device: of the shortest
 *   snapshot of the list), and that entry comes out as a row that was never marked does: count / total 0, sum, m2 0,
 *   nbuckets 0, present_bits 0, every key, pvalid, count_le, sum_le and cum 0.
 *   LH_EINVAL, decided on the host before a snapshot or a device is touched: every cause the base form has; ids NULL with
 *            n > 0; ids not 4-byte aligned.
 *   LH_ERANGE: n above 2^32 - 1, before anything is looked at (a cause of LH_EINVAL wins over it); a host form's bad id.
 *   READ-ONLY, ordering, threading, staging and the fixed order of every floating-point sum are the base form's: the same
 *   context and mutex per unit and device, the work on the same stream (for a list of snapshots behind the others' streams), a
 *   host form's id list copied into a block of the unit's that only grows. */
/* lh_across over rows ids[0 .. n) */
int lh_across_ids(lh_snapshot *const *snaps, size_t nsnaps, const uint32_t *ids, size_t n, const double *p, size_t np,
                  uint32_t flags, uint64_t *count, double *sum, uint32_t *nbuckets, uint32_t *present_bits, int16_t *pkeys,
                  uint8_t *pvalid);
/* lh_across_device over rows d_ids[0 .. n), a device array */
int lh_across_ids_device(lh_snapshot *const *snaps, size_t nsnaps, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                         uint32_t flags, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets, uint32_t *d_present_bits,
                         int16_t *d_pkeys, uint8_t *d_pvalid);
/* lh_count_le over rows ids[0 .. n); per-metric bounds hold a row per entry */
int lh_count_le_ids(lh_snapshot *s, const uint32_t *ids, size_t n, const double *bounds, size_t nb, uint32_t flags,
                    uint64_t *cum, uint64_t *total);
/* lh_count_le_device over rows d_ids[0 .. n), a device array (bounds stay a host array) */
int lh_count_le_ids_device(lh_snapshot *s, const uint32_t *d_ids, size_t n, const double *bounds, size_t nb, uint32_t flags,
                           uint64_t *d_cum, uint64_t *d_total);
/* lh_spread over rows ids[0 .. n) */
int lh_spread_ids(lh_snapshot *s, const uint32_t *ids, size_t n, const double *p, size_t np, uint64_t *count, double *sum,
                  double *m2, int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le);
/* lh_spread_device over rows d_ids[0 .. n), a device array */
int lh_spread_ids_device(lh_snapshot *s, const uint32_t *d_ids, size_t n, const double *p, size_t np, uint64_t *d_count,
                         double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le,
                         double *d_sum_le);
/* INTERVALS KEPT IN COMPACT FORM ON THE DEVICE: lh_keep, lh_kept_*.  lh_across* needs all K intervals alive as dense epoch
 * buffers, and an engine has at most 16 of them (4 GiB each at 8 192 names).  An interval's OCCUPIED cells are small -- a few
 * hundred (int16 key, uint64 count) pairs per name, RawMetricSet.Histograms (/root/reference/metrics.go:54-60) -- so a minute of
 * 1 s intervals fits where two dense buffers do not.  lh_keep copies the occupied cells of rows [first, first + nmetrics) of a
 * snapshot into device memory the handle owns; lh_kept_across* then gives lh_across*' outputs over a LIST of up to LH_MAX_KEPT
 * handles without any dense buffer.  The sum is over time for ONE name: nothing is summed across names, no cell of a snapshot is
 * written and no new statistic is defined -- every output is what lh_extract_rows would return for the cells atomic.AddUint64
 * would have left had the samples arrived in one interval (metrics.go:278; the walks: metrics.go:336-418).
 *   lh_keep           The handle's arrays are exactly what lh_buckets_all hands out for the same rows, in DEVICE memory:
 *                     offsets[nrows + 1] from 0, keys ascending by bin (bin = (uint16)key ^ 0x8000), uint64 counts -- so
 *                     lh_snapshot_add_buckets_csr_device(s2, first, nrows, d_offsets, d_keys, d_counts) restores the interval
 *                     unchanged -- plus row_count[nrows], each row's sum of cells (wrapping).  Counted, prefix-summed and
 *                     compacted on the device, on lh_snapshot_stream(s); only the two grand totals come back, to size ONE exact
 *                     allocation.  Returns when the copy is complete: the snapshot may be released at once, and the handle
 *                     depends on neither the snapshot nor the engine afterwards (it survives lh_destroy).  READ-ONLY on the
 *                     snapshot: a narrow snapshot stays narrow.  A handle never changes after creation.  A block without an
 *                     occupied cell gives a valid handle with cells == 0.  flags must be 0.
 *                     LH_EINVAL: NULL s or out, flags != 0, nmetrics == 0.  LH_ERANGE: first + nmetrics beyond the snapshot's
 *                     rows.  LH_ENOMEM: the allocation failed; *out is untouched and nothing is leaked.
 *   lh_kept_release   frees the handle; waits first for enqueued work that still reads it: every lh_kept_across*_device call
 *                     that listed it, on whichever streams (each such call chains one event behind the earlier ones), and
 *                     whatever lh_kept_hold covered.
 *   lh_kept_info_get  out->struct_size = sizeof(lh_kept_info) on entry.  cells: occupied cells held; samples: the sum of
 *                     row_count (wrapping); bytes: the allocation, exactly (2 * nrows + 1) * 8 + cells * 10 -- the four arrays.
 *   lh_kept_arrays    the four device arrays (any pointer may be NULL), valid until lh_kept_release; with cells == 0 the keys
 *                     and counts arrays are empty.  Work of the caller's own that reads them is NOT guarded by itself:
 *   lh_kept_hold      everything enqueued on `stream` (a hipStream_t of the handle's device; NULL: its null stream) up to now
 *                     counts as a reader of the handle: lh_kept_release waits for it.  Call it right AFTER enqueueing work
 *                     that reads lh_kept_arrays' pointers, lh_snapshot_add_buckets_csr_device on them for one.  LH_EINVAL:
 *                     NULL k.
 *   lh_kept_across, lh_kept_across_device, lh_kept_across_ids, lh_kept_across_ids_device
 *                     lh_across* / lh_across_ids* over handles: the same outputs, definitions and error order, with
 *                     C[b] = the sum over the listed handles of the name's cell b, taken in 64 bits.  Differences:
 *                     1 <= nkept <= LH_MAX_KEPT; present_bits is uint64_t (bit i: kept[i] holds a cell of the name); `first` and
 *                     ids are ABSOLUTE row numbers (metric ids), and [first, first + nmetrics) must lie inside EVERY handle's
 *                     block [first_i, first_i + nrows_i), else LH_ERANGE; a host id outside some handle's block -> LH_ERANGE,
 *                     nothing enqueued, nothing written; a DEVICE id outside some handle's block yields the empty entry and the
 *                     kernel reads nothing for it (the stance of the *_ids_device forms above).  A handle may be listed more
 *                     than once and counts that often.  nmetrics == 0 / n == 0 -> LH_OK before any handle is looked at.
 *                     Handles on different devices -> LH_EINVAL.  Totals that wrap past 2^64: count wraps, the percentile
 *                     outputs are unspecified (nothing faults).
 *                     ORDERING: the work goes on `stream` (a hipStream_t of the handles' device; NULL: its null stream).  Host
 *                     forms return with the results in the caller's arrays (pinned arrays by one copy each); device forms
 *                     return after enqueueing, and the outputs and d_ids stay valid until the stream has passed the call.  p is
 *                     a HOST array in all forms and travels by value, as does the list of handles.  sum is taken in one fixed
 *                     order and does not depend on timing.  One set of staging blocks per DEVICE behind the unit's own mutex:
 *                     calls take turns.
 *   lh_kept_merge     CONSOLIDATION: one new handle of rows [first, first + nmetrics) out of 1 .. LH_MAX_KEPT handles -- sixty
 *                     1 s handles into one of a minute, sixty of those into one of an hour; lh_kept_across* takes any mix.
 *                     *out holds exactly what lh_keep would return for a snapshot whose cells are C[b] = the sum over the
 *                     listed handles of the name's cell b in 64 bits, wrapping (the cell atomic.AddUint64 would have left had
 *                     the samples arrived in one interval, metrics.go:278; the pairs of RawMetricSet.Histograms,
 *                     metrics.go:54-60): per row the union of the handles' bins ascending by bin, a bin whose sum wraps to 0
 *                     not listed (it is not an occupied cell), row_count[m] the wrapping sum of the row's cells, samples the
 *                     sum of those; the same single allocation, layout and bytes.  A handle listed twice counts twice;
 *                     nkept == 1 is a slice, or a copy.  Nothing is summed across names; no snapshot, engine or listed handle
 *                     is written.  The work goes on `stream` (a hipStream_t of the handles' device; NULL: its null stream) and
 *                     is complete on return, like lh_keep's (the allocation's size is known only after the count pass); the
 *                     new handle depends on none of the listed ones.  The rows of the call choose between the reader's two
 *                     kernel shapes, which give identical bytes.  flags must be 0.  Checked on the host, in this order, before
 *                     any handle is looked at -- LH_EINVAL: NULL or misaligned list, a NULL entry, nkept == 0 or
 *                     > LH_MAX_KEPT, flags != 0, NULL out, nmetrics == 0; LH_ERANGE: nmetrics > 0xffffffff -- then LH_EINVAL:
 *                     handles on different devices; LH_ERANGE: [first, first + nmetrics) not inside EVERY handle's block
 *                     (lh_kept_across' rule).  LH_ENOMEM: the allocation failed.  *out is untouched on any failure.
 *   lh_kept_slide     A ROLLING WINDOW ADVANCED EXACTLY: new window = old window + newest interval - oldest interval, as one new
 *                     handle of rows [first, first + nmetrics) -- a process that emits the last minute every second reads one
 *                     merged handle and two small ones a tick, where lh_kept_merge would read all sixty.  With A[b] = the sum over
 *                     the `add` list of the name's cell b and S[b] = the same sum over `sub`, both in 64 bits, wrapping
 *                     (lh_kept_merge's C[b], once per side), *out holds exactly what lh_keep would return for a snapshot whose
 *                     cells are A[b] - S[b]: per row the bins ascending, a bin whose difference is 0 not listed, row_count[m] =
 *                     (the wrapping sum of the add handles' row_count[m]) - (the same over sub), wrapping, samples the wrapping
 *                     sum of those; the same single allocation, layout and bytes as every other handle.  Cells are unsigned
 *                     integer counts (atomic.AddUint64, metrics.go:278), so the result is bit for bit lh_kept_merge's of the
 *                     window's handles and nothing drifts however long the window runs; every reader, lh_kept_save* and
 *                     lh_kept_merge take it like any other handle.  1 <= nadd, 0 <= nsub, nadd + nsub <= LH_MAX_KEPT; with
 *                     nsub == 0 `sub` may be NULL and the result is byte-identical to lh_kept_merge(add, nadd, ...).  A handle
 *                     may appear several times, and on both sides, where it cancels.
 *                     UNDERFLOW: if S[b] > A[b] for any cell of the rows asked for -- decided on the wrapped sums -- the call
 *                     returns LH_ERANGE: *out is untouched and nothing is leaked (no block is allocated), and *why -- optional;
 *                     why->struct_size = sizeof(lh_kept_under) on entry -- names the violating cell of the LOWEST ROW, in it the
 *                     LOWEST BIN (bin = (uint16)key ^ 0x8000), whatever the timing and the kernel shape.  The corner where the
 *                     adds wrapped past 2^64 and a legitimate subtrahend then looks too large is refused like any other
 *                     underflow.  *why is written by an underflow refusal only.
 *                     Checked on the host, in this order, before any handle is looked at -- LH_EINVAL: NULL or misaligned add,
 *                     nadd == 0, sub NULL or misaligned with nsub > 0, a NULL entry in either list, nadd + nsub > LH_MAX_KEPT,
 *                     flags != 0, NULL out, why non-NULL with why->struct_size != sizeof(lh_kept_under), nmetrics == 0;
 *                     LH_ERANGE: nmetrics > 0xffffffff -- then LH_EINVAL: handles on different devices; LH_ERANGE (*why left
 *                     as it was): [first, first + nmetrics) not inside EVERY handle's block.  LH_ENOMEM, LH_EDEVICE, the stream,
 *                     the two kernel shapes, the unit's mutex and "complete on return" as for lh_kept_merge: the listed handles
 *                     are only read, and the new handle depends on none of them.
 *   lh_kept_gather*   KEPT ROWS RE-MAPPED PER HANDLE, SUMMED INTO ONE: history that came from somewhere else -- another process of a
 *                     fleet, the same process before a restart, a rank that owns another block of names -- interned its names in
 *                     another order, so row r does not mean the same name in every handle and no reader, lh_kept_merge or
 *                     lh_kept_slide can take such a list as it is.  `src` is handle-major: src[i * n + j] is the ABSOLUTE row number
 *                     of kept[i] that feeds output row first_out + j (ids are absolute everywhere in the family);
 *                     LH_KEPT_NO_ROW: handle i has nothing for that row.  *out is a new handle of rows [first_out, first_out + n)
 *                     that holds exactly what lh_keep would return for a snapshot whose row first_out + j has cells C[b] = the
 *                     sum over i of cell b of row src[i * n + j] of kept[i], in 64 bits, wrapping: bins ascending, a bin whose sum
 *                     wraps to 0 not listed, row_count the wrapping sum of the source rows' row_count entries, samples the
 *                     wrapping sum of those; the same single allocation, layout and bytes as every other handle, so every
 *                     reader, lh_kept_merge, lh_kept_slide and lh_kept_save* take it as they are.  The same source row may feed
 *                     several output rows, and a handle may be listed several times, with different maps.
 *                     1 <= nkept <= LH_MAX_KEPT.  With src[i * n + j] = first + j for all i the bytes are lh_kept_merge(kept,
 *                     nkept, first, n)'s; with nkept == 1 it is a pure row permutation, selection or duplication and no cell
 *                     changes (a route without the tile; identical bytes); the gather of a list equals lh_kept_merge of the nkept
 *                     one-handle gathers.  Row 0xffffffff of a handle cannot be named: the value is LH_KEPT_NO_ROW.
 *                     ONE DELIBERATE DIFFERENCE FROM THE READERS, which make an entry empty if its row lies outside ANY handle's
 *                     block: here a LH_KEPT_NO_ROW entry, and in the device form any row outside handle i's block, makes handle i's
 *                     segment empty for that output row and nothing else.  Nothing is read for it.
 *                     Checked on the host, in lh_kept_merge's style and order, before any handle is looked at -- LH_EINVAL: a NULL or
 *                     misaligned list or src, a NULL entry, nkept == 0 or > LH_MAX_KEPT, flags != 0, NULL out, n == 0; LH_ERANGE:
 *                     n > 0xffffffff or first_out + n > 2^32 -- then LH_EINVAL: handles on different devices; the host form only:
 *                     LH_ERANGE if some src value is neither LH_KEPT_NO_ROW nor inside its handle's block (nothing is enqueued).
 *                     LH_ENOMEM and LH_EDEVICE as for lh_kept_merge; *out is untouched on any failure and nothing is leaked.
 *                     The work goes on `stream`, is complete on return and runs under the unit's mutex; the listed handles are
 *                     only read and the new handle depends on none of them.  The host form copies src (nkept * n * 4 bytes) to the
 *                     device on the call's stream, as the id lists travel; the device form reads the caller's device array, which
 *                     must stay valid and unchanged until the call returns.  The two kernel shapes give identical bytes.
 *                     OUT OF SCOPE: more than LH_MAX_KEPT handles a call (gather in groups, then lh_kept_merge); many-to-one
 *                     roll-ups of names within one handle; names inside the blob (loghisto_amd.keptfile.pack_names is a sidecar);
 *                     a cross-rank collective; retuning the shape switch.
 *   lh_kept_group*    MANY KEPT ROWS SUMMED INTO ONE ROW, BY GROUP: the roll-up across names -- the p99 of a service over all its
 *                     endpoints, hosts or status codes, a fleet total beside the per-endpoint rows; Prometheus' sum by (label).  It
 *                     is where lh_kept_gather*'s out-of-scope item "many-to-one roll-ups of names within one handle" went.  The
 *                     groups are a CSR over row numbers: group g has the members members[goff[g] .. goff[g + 1]), ABSOLUTE row
 *                     numbers as everywhere in the family, LH_KEPT_NO_ROW: nothing.  *out is a new handle of rows [first_out,
 *                     first_out + ngroups) that holds exactly what lh_keep would return for a snapshot whose row first_out + g has
 *                     cells C[b] = the sum over the handles i and over the members r of group g of cell b of row r of kept[i], in
 *                     64 bits, wrapping: bins ascending, a bin whose sum wraps to 0 not listed, row_count the wrapping sum of the
 *                     source rows' row_count entries, samples the wrapping sum of those; the same single allocation, layout and
 *                     bytes as every other handle, so every reader, lh_kept_merge, lh_kept_slide, lh_kept_save* and lh_lines* take
 *                     it as they are.  A row may be a member of several groups (per service, and "everything": the normal case); a
 *                     row that appears several times in one group counts that often, and a handle listed twice counts twice; an
 *                     empty group gives an empty row; a call in which no cell survives gives a valid handle with cells == 0.
 *                     1 <= nkept <= LH_MAX_KEPT; there is no limit on the sources of a group.
 *                     THREE EQUIVALENCES ARE THE WHOLE DEFINITION:
 *                     1. With ngroups singleton groups, goff[g] = g and members[g] = src[g]: the bytes are lh_kept_gather's for the
 *                        list with that one map repeated for every handle.  With members[g] = first + g, they are lh_kept_merge's.
 *                     2. A call whose largest group has G members, with nkept x G <= LH_MAX_KEPT: the bytes are lh_kept_gather's
 *                        for the list in which every handle stands G times.  The copies are G consecutive entries per handle.  Copy
 *                        c is mapped to member c of each group.  LH_KEPT_NO_ROW stands where the group is shorter.
 *                     3. Any partition of every group's member list into pieces: the bytes are lh_kept_merge's over the handles
 *                        that lh_kept_group gives for each piece.
 *                     THE ROW RULE is lh_kept_gather's deliberate difference from the readers, not the readers' rule: a
 *                     LH_KEPT_NO_ROW member contributes nothing, and in the device form a member outside handle i's block
 *                     contributes nothing for handle i alone; nothing is read for it.
 *                     Checked on the host, in lh_kept_gather's style and order, before any handle is looked at -- LH_EINVAL: a NULL
 *                     or misaligned list, goff or members (members may be NULL only with nmembers == 0), a NULL entry, nkept == 0
 *                     or > LH_MAX_KEPT, flags != 0, NULL out, ngroups == 0; LH_ERANGE: ngroups > 0xffffffff, first_out + ngroups >
 *                     2^32 or nmembers > 0xffffffff -- then LH_EINVAL: handles on different devices; then, the host form only:
 *                     LH_EINVAL if goff[0] != 0, goff decreases somewhere or goff[ngroups] != nmembers; LH_ERANGE if a member is
 *                     neither LH_KEPT_NO_ROW nor inside EVERY handle's block.  Nothing is enqueued on a refusal and *out is
 *                     untouched on any failure.  The host form copies goff and members to the device on the call's stream, as src
 *                     and the id lists travel.  The device form's arrays are any bytes: entry g reads a = min(goff[g], nmembers)
 *                     and b = min(goff[g + 1], nmembers) and is empty if b <= a; both passes apply the same clamp, and nothing is
 *                     stored beyond a row's place whatever the arrays hold by the second pass; they must stay valid until the
 *                     call returns.  The stream, "complete on return", the unit's mutex, LH_ENOMEM / LH_EDEVICE and "the new handle
 *                     depends on none of the listed ones" as for lh_kept_merge.  Up to 64 sources (handles x members) of a group
 *                     take lh_kept_gather's open and turns, one source a lane; more go through the same tile in chunks of 64.  The
 *                     two kernel shapes give identical bytes; the switch takes the call's OUTPUT rows.
 *                     OUT OF SCOPE: spreading ONE group over several workgroups (a single group of every name runs in one
 *                     workgroup; profiles/kept_group.txt has it); more than LH_MAX_KEPT handles a call; readers over groups without
 *                     materialising the handle; a different member list per handle (gather first, then group); weights; retuning
 *                     the shape switch. */
typedef struct lh_kept lh_kept;     /* one interval's occupied cells of rows [first, first + nrows), in device memory the handle owns */
#define LH_MAX_KEPT 64
typedef struct lh_kept_info {
    uint32_t struct_size;            /* sizeof(lh_kept_info) */
    int32_t device;
    uint32_t first, nrows;
    uint64_t cells, samples, bytes;
} lh_kept_info;
int lh_keep(lh_snapshot *s, uint32_t first, size_t nmetrics, uint32_t flags, lh_kept **out);
int lh_kept_release(lh_kept *k);
int lh_kept_info_get(const lh_kept *k, lh_kept_info *out);
int lh_kept_arrays(const lh_kept *k, const uint64_t **d_offsets, const int16_t **d_keys, const uint64_t **d_counts,
                   const uint64_t **d_row_count);
int lh_kept_hold(lh_kept *k, void *stream);
int lh_kept_across(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                   uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets, uint64_t *present_bits,
                   int16_t *pkeys, uint8_t *pvalid);
int lh_kept_across_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                          uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets,
                          uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid);
int lh_kept_across_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *p, size_t np,
                       uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets, uint64_t *present_bits,
                       int16_t *pkeys, uint8_t *pvalid);
int lh_kept_across_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                              uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, uint32_t *d_nbuckets,
                              uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid);
int lh_kept_merge(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t flags, void *stream,
                  lh_kept **out);
#define LH_KEPT_NO_ROW 0xffffffffu
int lh_kept_gather(lh_kept *const *kept, size_t nkept, const uint32_t *src, size_t n, uint32_t first_out, uint32_t flags,
                   void *stream, lh_kept **out);
int lh_kept_gather_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_src, size_t n, uint32_t first_out,
                          uint32_t flags, void *stream, lh_kept **out);
int lh_kept_group(lh_kept *const *kept, size_t nkept, const uint64_t *goff, const uint32_t *members, size_t nmembers,
                  size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out);
int lh_kept_group_device(lh_kept *const *kept, size_t nkept, const uint64_t *d_goff, const uint32_t *d_members, size_t nmembers,
                         size_t ngroups, uint32_t first_out, uint32_t flags, void *stream, lh_kept **out);
typedef struct lh_kept_under {
    uint32_t struct_size;            /* sizeof(lh_kept_under) == 16 */
    uint32_t row;                    /* ABSOLUTE row number (metric id) of the first cell that would go below zero */
    int16_t key;                     /* its bucket key */
    uint16_t reserved0;              /* written as 0 */
    uint32_t reserved1;              /* written as 0 */
} lh_kept_under;
int lh_kept_slide(lh_kept *const *add, size_t nadd, lh_kept *const *sub, size_t nsub, uint32_t first, size_t nmetrics,
                  uint32_t flags, void *stream, lh_kept_under *why, lh_kept **out);
/* KEPT INTERVALS SAVED AND LOADED: lh_kept_save*, lh_kept_load*, lh_kept_values.  A handle is otherwise born from a live snapshot
 * (lh_keep) or from handles of the same device (lh_kept_merge): the history dies with the process and cannot change devices.  A
 * BLOB carries one handle to a file, to another process, rank or device; a process that only QUERIES history -- a dashboard
 * backend, a fleet aggregator, a restart -- needs no engine: lh_kept_load* and the lh_kept_* readers.  The names that belong to
 * the ids are not in the blob (store lh_metric_name's output beside it); no checksum, and verbatim: lh_kept_encode* below writes the compact form.
 *   THE BLOB (format version 1; little-endian; part of this interface) is a 64-byte header followed by the handle's single
 *   allocation VERBATIM, lh_kept_info.bytes long:
 *       offset  0  uint8[8]  magic "LHKEPT\x1a\n" (LH_KEPT_BLOB_MAGIC)
 *               8  uint32    format version, 1 (LH_KEPT_BLOB_VERSION)
 *              12  uint32    header size, 64 (LH_KEPT_BLOB_HEADER)
 *              16  uint32    LH_NKEYS, 65 536
 *              20  uint32    first
 *              24  uint32    nrows
 *              28  uint32    reserved, 0
 *              32  uint64    cells
 *              40  uint64    samples
 *              48  uint64    bytes = (2 * nrows + 1) * 8 + cells * 10
 *              56  uint8[8]  reserved, 0
 *              64  uint64 offsets[nrows + 1] | uint64 row_count[nrows] | uint64 counts[cells] | int16 keys[cells]
 *   lh_kept_save_size *bytes = 64 + lh_kept_info.bytes.  LH_EINVAL: NULL k or bytes.
 *   lh_kept_save      writes the blob of k into HOST memory buf[0 .. cap), pageable or pinned; *written (may be NULL) = its size.
 *   lh_kept_save_device  the same into DEVICE memory of the handle's device (what a rank hands to RCCL); any alignment.
 *                     Both: the copies go on `stream` (a hipStream_t of the handle's device; NULL: its null stream) and the save is
 *                     COMPLETE on return; under the unit's mutex; the handle is only read.  LH_EINVAL: NULL k or buf.  LH_ERANGE:
 *                     cap below the blob's size -- below LH_KEPT_BLOB_MIN (the smallest blob there is: one row, no cell) before
 *                     the handle is looked at --, nothing written, *written untouched.
 *   lh_kept_load      a NEW handle on `device` from a blob in HOST memory buf[0 .. len): an ordinary lh_kept with the exact
 *                     allocation, layout and bytes lh_keep would give -- every reader, lh_kept_merge, lh_kept_arrays,
 *                     lh_kept_hold and lh_kept_release take it, in any mix with other handles of that device.
 *   lh_kept_load_device  the same from a blob in the memory of `device` itself; only its 64 header bytes come to the host.
 *                     Both: a blob is UNTRUSTED, and every lh_kept_* kernel loops and scatters by the handle's arrays, so the load
 *                     PROVES on the device what lh_keep guarantees before a handle exists: the block is copied into its exact
 *                     allocation and checked there on `stream` (a hipStream_t of `device`; NULL: its null stream), a wave per row;
 *                     the check reads nothing outside the copied block whatever the bytes say, and the verdict does not depend on
 *                     timing.  Like lh_keep and lh_kept_merge a load is complete on return, under the unit's mutex.  flags must
 *                     be 0.  Any refusal is LH_EINVAL: *out untouched, nothing leaked (the stream waited for, the block freed),
 *                     and *why -- optional; why->struct_size = sizeof(lh_kept_check) on entry, anything else is LH_EINVAL with
 *                     nothing written -- says which: cause, and for the device's causes row and index (0 otherwise).
 *                     Decided on the HOST, before any device call (lh_kept_load_device: NULL arguments, flags and len < 64
 *                     before any device call, the rest once the header has come over), in this order:
 *                       LH_KEPT_BAD_ARG          NULL buf or out, flags != 0, device < 0 or beyond the unit's 64 slots
 *                       LH_KEPT_BAD_SHORT        len < 64
 *                       LH_KEPT_BAD_MAGIC, LH_KEPT_BAD_VERSION, LH_KEPT_BAD_HEADER_SIZE
 *                       LH_KEPT_BAD_NKEYS        the blob's LH_NKEYS is not this library's
 *                       LH_KEPT_BAD_NROWS        nrows == 0
 *                       LH_KEPT_BAD_FIRST        first + nrows > 2^32
 *                       LH_KEPT_BAD_CELLS        cells > nrows * LH_NKEYS
 *                       LH_KEPT_BAD_BYTES        bytes != (2 * nrows + 1) * 8 + cells * 10
 *                       LH_KEPT_BAD_LENGTH       len != 64 + bytes
 *                       LH_KEPT_BAD_RESERVED     a reserved byte that is not 0
 *                     Decided on the DEVICE, with bin = (uint16)key ^ 0x8000; row m's cells are [offsets[m], offsets[m + 1]):
 *                       LH_KEPT_BAD_OFFSET_FIRST   offsets[0] != 0                                          (row 0, index 0)
 *                       LH_KEPT_BAD_OFFSET_ORDER   not offsets[m] <= offsets[m + 1] <= cells                (row m, index 0)
 *                       LH_KEPT_BAD_ROW_LENGTH     offsets[m + 1] - offsets[m] > LH_NKEYS                   (row m, index 0)
 *                       LH_KEPT_BAD_OFFSET_LAST    offsets[nrows] != cells                          (row nrows - 1, index 0)
 *                       LH_KEPT_BAD_KEY_ORDER      cell i > 0 of row m: bin(i - 1) >= bin(i) -- within the row only: its first
 *                                                  key may lie below the previous row's last        (row m, index i in the row)
 *                       LH_KEPT_BAD_ZERO_COUNT     cell i of row m has count 0                               (row m, index i)
 *                       LH_KEPT_BAD_ROW_COUNT      row_count[m] is not the wrapping sum of the row's counts
 *                                                                                    (row m, index = the row's number of cells)
 *                       LH_KEPT_BAD_SAMPLES        samples is not the wrapping sum of row_count         (row = nrows, index 0)
 *                     A row with one of the four offset causes is not walked: no cell of it is read or reported.  Of all
 *                     violations the one reported is that of the LOWEST ROW, in it the LOWEST INDEX, there the LOWEST CAUSE CODE.
 *                     LH_ENOMEM: the allocation failed.  LH_EDEVICE: a HIP error.
 *   lh_kept_values    D[LH_NKEYS] (host, 8-byte aligned): decompress() by bin, the value table the lh_kept_* readers weigh cells
 *                     with on `device`, generated there on first use -- bit-equal to lh_codec_tables' D.  What a process without
 *                     an engine turns pkeys into values with: D[(uint16)key ^ 0x8000].  LH_EINVAL: NULL or misaligned D, device
 *                     < 0 or beyond the unit's 64 slots. */
#define LH_KEPT_BLOB_MAGIC "LHKEPT\x1a\n"
#define LH_KEPT_BLOB_VERSION 1
#define LH_KEPT_BLOB_HEADER 64
#define LH_KEPT_BLOB_MIN (LH_KEPT_BLOB_HEADER + 24) /* one row, no cell */
enum {
    LH_KEPT_BAD_ARG = 1,
    LH_KEPT_BAD_SHORT = 2,
    LH_KEPT_BAD_MAGIC = 3,
    LH_KEPT_BAD_VERSION = 4,
    LH_KEPT_BAD_HEADER_SIZE = 5,
    LH_KEPT_BAD_NKEYS = 6,
    LH_KEPT_BAD_NROWS = 7,
    LH_KEPT_BAD_FIRST = 8,
    LH_KEPT_BAD_CELLS = 9,
    LH_KEPT_BAD_BYTES = 10,
    LH_KEPT_BAD_LENGTH = 11,
    LH_KEPT_BAD_RESERVED = 12,
    LH_KEPT_BAD_OFFSET_FIRST = 16,
    LH_KEPT_BAD_OFFSET_ORDER = 17,
    LH_KEPT_BAD_ROW_LENGTH = 18,
    LH_KEPT_BAD_OFFSET_LAST = 19,
    LH_KEPT_BAD_KEY_ORDER = 20,
    LH_KEPT_BAD_ZERO_COUNT = 21,
    LH_KEPT_BAD_ROW_COUNT = 22,
    LH_KEPT_BAD_SAMPLES = 23
};
typedef struct lh_kept_check {
    uint32_t struct_size;            /* sizeof(lh_kept_check) */
    uint32_t cause;                  /* LH_KEPT_BAD_* */
    uint32_t row, index;             /* row within the block (0 = the handle's `first`), cell within the row */
} lh_kept_check;
int lh_kept_save_size(const lh_kept *k, size_t *bytes);
int lh_kept_save(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written);
int lh_kept_save_device(lh_kept *k, void *d_buf, size_t cap, void *stream, size_t *written);
int lh_kept_load(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out);
int lh_kept_load_device(int device, const void *d_buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why,
                        lh_kept **out);
int lh_kept_values(int device, double *D /* LH_NKEYS */);
/* KEPT INTERVALS IN A COMPACT BLOB: lh_kept_encode*, lh_kept_decode*.  The verbatim blob above costs 10 bytes a cell and 16 a row on
 * every file, wire and PCIe copy; the ENCODED blob carries the same handle in a per-row encoding -- counts at the narrowest width
 * that holds the row's largest, bins as byte deltas -- made and taken apart on the device, a wave per row.  A decoded handle is
 * byte for byte the handle that was encoded, so nothing else in the family changes.  lh_kept_load* refuses an encoded blob
 * (LH_KEPT_BAD_MAGIC) and lh_kept_decode* a verbatim one.  No checksum, no names, no entropy coding.
 *   THE ENCODED BLOB (format version 1; little-endian; part of this interface):
 *       offset  0  uint8[8]  magic "LHKENC\x1a\n" (LH_KEPT_ENC_MAGIC)
 *               8  uint32    format version, 1 (LH_KEPT_ENC_VERSION)
 *              12  uint32    header size, 64
 *              16  uint32    LH_NKEYS, 65 536
 *              20  uint32    first
 *              24  uint32    nrows
 *              28  uint32    reserved, 0
 *              32  uint64    cells, the total over all rows
 *              40  uint64    samples, the wrapping sum of every count
 *              48  uint64    bytes, the length of everything behind the header
 *              56  uint8[8]  reserved, 0
 *              64  THE ROW DIRECTORY  uint32 desc[nrows], padded with one zero uint32 when nrows is odd: D = 8 * ceil(nrows / 2)
 *                  bytes.  desc[m] = n | cw << 20 | km << 24: n (bits 0-16) the row's cells, 0 .. 65 536; cw (bits 20-21) the
 *                  count width, 1 << cw bytes; km (bit 24) the key mode; every other bit 0.  A row without a cell has desc == 0
 *                  and no record.
 *          64 + D  THE ROW RECORDS in row order, each S(m) bytes long and 8-aligned; nothing else is stored -- no offsets, no
 *                  row_count (the wrapping sum of the row's counts).  A record of n >= 1 cells:
 *                    counts  n values of 1 << cw bytes, zero-padded to a multiple of 8
 *                    keys    zero-padded to a multiple of 8; with bin = (uint16)key ^ 0x8000,
 *                            km 0: uint16 bin[0], then n - 1 bytes d[i] = bin[i] - bin[i - 1] - 1 (gaps of 1 .. 256)
 *                            km 1: uint16 bin[n]
 *                  Every multi-byte value is naturally aligned.
 *   CANONICAL: one handle has exactly one encoding.  cw is the least width that holds the row's largest count; km is 1 exactly
 *   when some gap of the row exceeds 256; every pad byte is 0.
 *   SIZE: for n >= 1, S(m) <= 8 n + (2 n + 6), hence bytes <= D + 10 * cells + 6 * nrows and LH_KEPT_ENC_BOUND(nrows, cells) is the
 *   capacity that always suffices -- never above the verbatim blob's 64 + 10 * cells + 16 * nrows + 8.
 *   lh_kept_encode_size  *bytes = the exact size of k's encoded blob: the encoder's first pass and its scan run on `stream`, the
 *                     total alone comes to the host.  LH_EINVAL: NULL k or bytes.
 *   lh_kept_encode    writes the encoded blob of k into HOST memory buf[0 .. cap), pageable or pinned; *written (may be NULL) = its
 *                     size.  Encoded on the device into a block of the exact size, then ONE copy to the host.
 *   lh_kept_encode_device  the same into DEVICE memory of the handle's device, at any alignment (an address that is not
 *                     8-aligned is served through the unit's own block and one device copy).
 *                     Both: three kernels on `stream` (a hipStream_t of the handle's device; NULL: its null stream) -- a wave per
 *                     row finds desc[m] and S(m), one scan gives the records' offsets, a wave per row writes the record, every pad
 *                     byte included: what buf held before does not show.  COMPLETE on return; under the unit's mutex; the handle
 *                     is only read.  LH_EINVAL: NULL k or buf.  LH_ERANGE: cap below LH_KEPT_ENC_MIN (the smallest encoded blob
 *                     there is: one row, no cell) before the handle is looked at, then cap below the exact size, known after
 *                     the first pass: nothing written, *written untouched.
 *   lh_kept_decode    a NEW handle on `device` from an encoded blob in HOST memory buf[0 .. len): allocation, layout and bytes
 *                     are exactly those of the handle that was encoded.
 *   lh_kept_decode_device  the same from an encoded blob in the memory of `device` itself, at any alignment; only its 64 header
 *                     bytes come to the host.
 *                     Both: an encoded blob is UNTRUSTED like a verbatim one: the kernels are safe on arbitrary bytes and the
 *                     verdict does not depend on timing.  flags must be 0; complete on return, under the unit's mutex.  Any
 *                     refusal is LH_EINVAL, *out untouched, nothing leaked, *why as for lh_kept_load (struct_size first).
 *                     STAGE 0, on the HOST before any device call (lh_kept_decode_device: the arguments and len < 64 before any
 *                     device call, the rest once the header has come over), lh_kept_load's causes in lh_kept_load's order:
 *                       LH_KEPT_BAD_ARG, LH_KEPT_BAD_SHORT, LH_KEPT_BAD_MAGIC, LH_KEPT_BAD_VERSION, LH_KEPT_BAD_HEADER_SIZE,
 *                       LH_KEPT_BAD_NKEYS, LH_KEPT_BAD_NROWS, LH_KEPT_BAD_FIRST, LH_KEPT_BAD_CELLS
 *                       LH_KEPT_BAD_BYTES        bytes not a multiple of 8, below D, or above D + 10 * cells + 6 * nrows
 *                       LH_KEPT_BAD_LENGTH       len != 64 + bytes
 *                       LH_KEPT_BAD_RESERVED
 *                     STAGE 1, the directory alone, a thread per descriptor:
 *                       LH_KEPT_BAD_ENC_DESC     a reserved bit, n > 65 536, or n == 0 with desc != 0        (row m, index 0)
 *                       LH_KEPT_BAD_ENC_TOTALS   the sum of n is not cells, or D + the sum of S(m) not bytes (row nrows, index 0)
 *                       LH_KEPT_BAD_ENC_PAD      the pad word behind an odd nrows is not 0                 (row nrows, index 0)
 *                     A stage-1 refusal is final: the records are read only behind a sound directory, by which every record lies
 *                     inside the payload and every row's cells inside the handle's exact allocation, whatever the bytes say.
 *                     STAGE 2, a wave per row, cell i of row m:
 *                       LH_KEPT_BAD_ENC_KEY_RANGE  km 0: bin[i] above 65 535                                 (row m, index i)
 *                       LH_KEPT_BAD_KEY_ORDER      km 1: bin[i - 1] >= bin[i]                                (row m, index i)
 *                       LH_KEPT_BAD_ZERO_COUNT     a count of 0                                              (row m, index i)
 *                       LH_KEPT_BAD_ENC_PAD        a pad byte of the record that is not 0                    (row m, index n)
 *                       LH_KEPT_BAD_ENC_WIDTH      cw or km is not the canonical one                         (row m, index n)
 *                       LH_KEPT_BAD_SAMPLES        samples is not the wrapping sum of the counts      (row = nrows, index 0)
 *                     Of all violations of a stage the one reported is that of the LOWEST ROW, in it the LOWEST INDEX, there the
 *                     LOWEST CAUSE CODE.  LH_ENOMEM: an allocation failed.  LH_EDEVICE: a HIP error. */
#define LH_KEPT_ENC_MAGIC "LHKENC\x1a\n"
#define LH_KEPT_ENC_VERSION 1
#define LH_KEPT_ENC_MIN (LH_KEPT_BLOB_HEADER + 8) /* one row, no cell */
#define LH_KEPT_ENC_BOUND(nrows, cells) \
    (LH_KEPT_BLOB_HEADER + 8 * (((uint64_t)(nrows) + 1) / 2) + 10 * (uint64_t)(cells) + 6 * (uint64_t)(nrows))
/* lh_kept_check.cause of an encoded blob: the LH_KEPT_BAD_* above, and */
#define LH_KEPT_BAD_ENC_DESC 32
#define LH_KEPT_BAD_ENC_TOTALS 33
#define LH_KEPT_BAD_ENC_KEY_RANGE 34
#define LH_KEPT_BAD_ENC_PAD 35
#define LH_KEPT_BAD_ENC_WIDTH 36
int lh_kept_encode_size(lh_kept *k, void *stream, size_t *bytes);
int lh_kept_encode(lh_kept *k, void *buf, size_t cap, void *stream, size_t *written);
int lh_kept_encode_device(lh_kept *k, void *d_buf, size_t cap, void *stream, size_t *written);
int lh_kept_decode(int device, const void *buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why, lh_kept **out);
int lh_kept_decode_device(int device, const void *d_buf, size_t len, uint32_t flags, void *stream, lh_kept_check *why,
                          lh_kept **out);
/* DISTRIBUTION SHIFT BETWEEN KEPT INTERVALS: lh_compare* over handles, so that the baseline -- the same minute an hour ago, the
 * interval before the deploy, yesterday's roll-up -- need not be alive as a dense snapshot, nor be poured back into one.  With
 *   a[j] = the sum over the `base` list of the name's cell j, b[j] = the same sum over the `cur` list, both in 64 bits
 * (lh_kept_across' C[b], once per side), every output is lh_compare's, word for word, for two snapshots that hold those cells:
 * count_a / count_b (the wrapping sums of the handles' row_count entries), the argmax of X_j in exact 128-bit integers with the
 * lowest bin among equals (ks_key, ks_below_a, ks_below_b), ks as the fixed function of the two prefixes, w1 and shift over every
 * bin from the lowest to the highest occupied one of the two sides (empty bins between them included, as inside lh_compare's
 * union span), NaN with key and prefixes 0 for a name without samples on a side, exact zeros for identical normalised
 * distributions, wrapped totals unspecified (nothing faults).  The totals are known before a cell is read, so a row is walked
 * once, over its occupied stretches only; w1 and shift are taken in one fixed order, the same in both kernel shapes (which
 * agree bit for bit), and differ from lh_compare's in the last bits only.
 *   1 <= nbase, 1 <= ncur, nbase + ncur <= LH_MAX_KEPT: ONE handle per lane of a wave, and the two lists travel by value in the
 *   kernel's arguments.  Longer windows go through lh_kept_merge first.  A handle may appear more than once in a list and
 *   counts that often; a handle may appear in both lists; identical lists give exact zeros for every non-empty name.
 *   `first` and ids are ABSOLUTE row numbers, as for lh_kept_across*.  Any output may be NULL, but not all.  flags must be 0.
 *   Checked on the host, in this order, before any handle is looked at -- LH_EINVAL: (ids forms: NULL ids with n > 0,
 *   misaligned ids,) a NULL or misaligned list, nbase == 0, ncur == 0, nbase + ncur > LH_MAX_KEPT, a NULL entry, flags != 0,
 *   all outputs NULL, an output not aligned to its element; LH_ERANGE: nmetrics > 0xffffffff; nmetrics == 0 / n == 0 -> LH_OK,
 *   nothing looked at -- then LH_EINVAL: handles of the two lists on different devices; LH_ERANGE, nothing enqueued and nothing
 *   written: [first, first + nmetrics), or a HOST id, outside the block of ANY handle of either list.  A DEVICE id outside some
 *   handle's block yields the entry of two empty sides (counts 0, NaN, key and prefixes 0); nothing is read for it.
 *   ORDERING and staging as for lh_kept_across*: the work goes on `stream`; host forms return with the results in the caller's
 *   arrays (pinned arrays by one copy each); device forms return after enqueueing, with ALL handles of both lists guarded
 *   against lh_kept_release until the stream has passed the call.  READ-ONLY. */
int lh_kept_compare(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                    uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                    uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift);
int lh_kept_compare_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                           size_t nmetrics, uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b,
                           double *d_ks, int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1,
                           double *d_shift);
int lh_kept_compare_ids(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, const uint32_t *ids, size_t n,
                        uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                        uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift);
int lh_kept_compare_ids_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, const uint32_t *d_ids,
                               size_t n, uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks,
                               int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1,
                               double *d_shift);
/* COUNTS AT OR BELOW VALUES, SPREAD AND TRIMMED SUMS OVER KEPT INTERVALS: lh_count_le* and lh_spread* over handles, the two
 * per-name readers whose natural windows -- the last hour's SLO ratio and `le` buckets, the last minute's std / mean_90 / sum_90 /
 * upper_90 -- exist only as handles.  With C[b] = the sum over the listed handles of the name's cell b, in 64 bits wrapping
 * (lh_kept_across' C; a handle listed twice counts twice), every output is, word for word, what lh_count_le / lh_spread return
 * for a snapshot whose cells are C (the walks: metrics.go:342-346 and 389-418): no dense buffer is alive or
 * filled, nothing is summed across names, no new statistic is defined, and no handle, snapshot or engine is written.  The outputs
 * are per-name columns in device memory in the device forms, which lh_lines* turns into wire lines as they are.
 *   lh_kept_count_le, lh_kept_count_le_device, lh_kept_count_le_ids, lh_kept_count_le_ids_device
 *                     cum[m * nb + j] = the sum of C[b] over the bins whose key is <= the key of bounds[j]; total[m] = the
 *                     wrapping sum of the handles' row_count entries (no cell is read for it).  The bound-to-key rule, +-Inf,
 *                     -0.0 and the saturation beyond the int16 key range are lh_count_le's; counts are exact uint64 sums that
 *                     wrap past 2^64.  bounds is ONE HOST array of nb doubles shared by all names, which travels by value beside
 *                     the list of handles.  flags must be 0: LH_LE_PER_METRIC is NOT supported here and returns LH_EINVAL -- a
 *                     row of bounds per name would need a block in device memory guarded across streams, which is why the
 *                     list itself travels by value.  One walk of the row, over its occupied stretches only.  (A row of bounds
 *                     per name over kept intervals is lh_kept_slo*, further down, which takes the rows as the ids are taken.)
 *                     Checked on the host before any handle is looked at -- LH_EINVAL: (ids forms: NULL ids with n > 0,
 *                     misaligned ids,) a NULL or misaligned list, nkept == 0 or > LH_MAX_KEPT, a NULL entry, nb == 0 or
 *                     nb > LH_MAX_BOUNDS, NULL bounds, both outputs NULL (either one may be), flags != 0, arrays not 8-byte
 *                     aligned, a NaN bound, a decreasing row of bounds (equal neighbours are allowed; -0.0 == 0.0); then
 *                     LH_ERANGE: nmetrics > 0xffffffff.  (The bounds being one shared row, every cause of LH_EINVAL comes before
 *                     that LH_ERANGE.)
 *   lh_kept_spread, lh_kept_spread_device, lh_kept_spread_ids, lh_kept_spread_ids_device
 *                     count, sum, m2 and, per p[i], pkeys, pvalid, count_le, sum_le: lh_spread's definitions -- m2 the CENTRED
 *                     second moment about sum / float64(count), taken in a second walk; the percentile's bucket the first bin
 *                     whose inclusive prefix reaches T (metrics.go:413); D[] bit for bit lh_codec_tables'.  count is the wrapping
 *                     sum of the handles' row_count entries, so the thresholds are known before a cell is read.  count == 0:
 *                     every output of the name is 0.  np <= LH_MAX_PERCENTILES; np == 0 is allowed: moments only, the four
 *                     per-percentile outputs are ignored.  Any output may be NULL, but not all.  flags must be 0.  Totals that
 *                     wrap past 2^64: count wraps, the other outputs are unspecified (nothing faults).  Every floating-point sum
 *                     is taken in ONE fixed order, the same in both kernel shapes, which therefore agree BIT FOR BIT on every
 *                     output (lh_spread's own two shapes agree to rounding only); sum, m2 and sum_le differ from lh_spread's on
 *                     a snapshot of the same cells in the last bits only.
 *                     Checked on the host before any handle is looked at -- LH_EINVAL: (ids forms as above,) a NULL or
 *                     misaligned list, nkept == 0 or > LH_MAX_KEPT, a NULL entry, flags != 0, np too large, np > 0 with NULL p,
 *                     all outputs NULL, arrays not aligned to their element size; then LH_ERANGE: nmetrics > 0xffffffff.
 *   Both families, as lh_kept_across*: nmetrics == 0 / n == 0 -> LH_OK before any handle is looked at, nothing written; then
 *   LH_ERANGE, nothing enqueued and nothing written, unless [first, first + nmetrics) -- `first` and ids are ABSOLUTE row numbers
 *   -- or every HOST id lies inside EVERY handle's block; LH_EINVAL for handles on different devices.  A DEVICE id outside some
 *   handle's block yields the empty entry (all zeros), and nothing is read for it.  ORDERING and staging as for lh_kept_across*:
 *   the work goes on `stream` (a hipStream_t of the handles' device; NULL: its null stream); host forms return with the results
 *   in the caller's arrays (pinned arrays by one copy each, others through a pinned block of the library's); device forms return
 *   after enqueueing, with ALL listed handles under one hold, so that lh_kept_release waits for the call.  bounds and p are HOST
 *   arrays in all forms.  The rows of a call choose between the reader's two kernel shapes (lh_tool_kept_switch). */
int lh_kept_count_le(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *bounds, size_t nb,
                     uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_count_le_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *bounds, size_t nb,
                            uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_count_le_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *bounds, size_t nb,
                         uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_count_le_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *bounds,
                                size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_spread(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                   uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2, int16_t *pkeys, uint8_t *pvalid,
                   uint64_t *count_le, double *sum_le);
int lh_kept_spread_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, const double *p, size_t np,
                          uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, double *d_m2, int16_t *d_pkeys,
                          uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le);
int lh_kept_spread_ids(lh_kept *const *kept, size_t nkept, const uint32_t *ids, size_t n, const double *p, size_t np,
                       uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2, int16_t *pkeys, uint8_t *pvalid,
                       uint64_t *count_le, double *sum_le);
int lh_kept_spread_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *d_ids, size_t n, const double *p, size_t np,
                              uint32_t flags, void *stream, uint64_t *d_count, double *d_sum, double *d_m2, int16_t *d_pkeys,
                              uint8_t *d_pvalid, uint64_t *d_count_le, double *d_sum_le);
/* PER-WINDOW READS OF KEPT INTERVALS: lh_kept_across* and lh_kept_count_le* for MANY sub-lists of one list of handles in ONE call
 * and one launch -- the p99 of each of the last 60 seconds for the 20 endpoints a dashboard shows (a sparkline), the last minute
 * at 5 s or 10 s resolution, a rolling 10 s p99 stepped by 1 s, a latency heat map (counts per `le` band per second) -- where one
 * lh_kept_* call per window pays the unit's mutex, a launch, an id copy and a hold each time.  Nothing is summed across names and no
 * new statistic is defined: every output is one that an existing reader returns for a sub-list.
 *   WINDOWS.  win is a HOST array of 2 * nwin values, 1 <= nwin <= LH_MAX_WINDOWS.  Window w is the slice
 *   kept[win[2w] .. win[2w+1]) of the list: half open, with 0 <= lo < hi <= nkept.  Windows may overlap, repeat and come in any
 *   order.  The windows travel by value, as the list, p and bounds do.
 *   LAYOUT, window-major: entry (w, m) lies at index e = w * n + m (n: nmetrics, or the ids' n); pkeys / pvalid lie at
 *   e * np + i; cum lies at e * nb + j.  Window w's block of every output is therefore a per-name column that lh_lines* takes as
 *   it is.
 *   CONTRACT -- this is the whole definition:
 *   - Window w's block of every output of lh_kept_series* is byte for byte what lh_kept_across* (the same form, the same rows or
 *     ids, p, np) writes for the list (kept + lo_w, hi_w - lo_w).
 *   - The one exception is present_bits: bit i means kept[i] of the WHOLE list, which is the slice call's value shifted left by
 *     lo_w.
 *   - Window w's block of lh_kept_heat* is byte for byte lh_kept_count_le*'s cum / total for that slice.
 *   - This includes sum: it is taken in the same fixed order, the same in both kernel shapes and independent of timing.
 *   - A handle listed twice counts twice.
 *   - A name with no sample in a window has the empty entry there.
 *   - Totals that wrap past 2^64: lh_kept_series* behaves as lh_kept_across* does; lh_kept_heat*'s cum and total stay exact modulo
 *     2^64, as lh_kept_count_le*'s are.
 *   - A DEVICE id outside the block of some handle of window w yields the empty entry in that window, and nothing is read for it.
 *   CHECKS on the host, before any handle is looked at, in this order.  LH_EINVAL: (ids forms) NULL ids with n > 0, or misaligned
 *   ids; a NULL or misaligned list; nkept == 0 or > LH_MAX_KEPT; a NULL entry; NULL or misaligned win; nwin == 0 or
 *   > LH_MAX_WINDOWS; a window with lo >= hi or hi > nkept; flags != 0; the family's own argument rules, exactly as
 *   lh_kept_across* / lh_kept_count_le* have them (np, NULL p, NaN or decreasing bounds, nb limits, all outputs NULL, alignment).
 *   Then LH_ERANGE: nmetrics > 0xffffffff.  Then nmetrics == 0 / n == 0 -> LH_OK with nothing written.  After the host checks,
 *   in this order: LH_EINVAL for handles on different devices; LH_ERANGE, with nothing enqueued and nothing written, unless the
 *   rows or every HOST id lie inside EVERY listed handle's block, whether or not a window names the handle.  No output is written
 *   on any refusal.
 *   ORDERING, staging and lifetime as for lh_kept_across*: the work goes on `stream`, under the unit's mutex; host forms bring
 *   nwin * n entries back through the unit's staging block and are complete on return; device forms return after enqueueing,
 *   with ALL listed handles under one hold; READ-ONLY.  One window per blockIdx.y of the reader's two kernel shapes, which give
 *   identical bytes; the switch between them (lh_tool_kept_switch) takes the ENTRIES of a call, nwin * n, not its rows.
 *   OUT OF SCOPE: sharing cell reads between overlapping windows; a tile-free fast path for one-handle windows (it would have to
 *   reproduce sum's order bit for bit); spread / compare / top per window; more than LH_MAX_KEPT handles per call. */
#define LH_MAX_WINDOWS 128
int lh_kept_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                   const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets,
                   uint64_t *present_bits, int16_t *pkeys, uint8_t *pvalid);
int lh_kept_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count, double *d_sum,
                          uint32_t *d_nbuckets, uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid);
int lh_kept_series_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                       const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, uint32_t *nbuckets,
                       uint64_t *present_bits, int16_t *pkeys, uint8_t *pvalid);
int lh_kept_series_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                              const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count, double *d_sum,
                              uint32_t *d_nbuckets, uint64_t *d_present_bits, int16_t *d_pkeys, uint8_t *d_pvalid);
int lh_kept_heat(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                 const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_heat_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                        const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_heat_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                     const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_heat_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                            const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
/* SPREAD AND COMPARE PER WINDOW OF KEPT INTERVALS: lh_kept_spread* and lh_kept_compare* for MANY windows of one list of handles in ONE
 * call and one launch.  This lifts spread / compare per window from the out-of-scope list of the block above; top per window stays
 * out (it needs a select per window).  lh_kept_spread_series*: the std, mean_90, sum_90 and upper_90 of each of the last 60 seconds,
 * or of the minute at 10 s resolution -- the statsd-style emit at a resolution chosen afterwards.  lh_kept_drift*: "when did it
 * start" -- the KS distance, earth mover's distance and shift of every second against a fixed baseline such as the minute before the
 * deploy, of each second against the second before it, of a rolling 10 s window against the 10 s before it.  Nothing is summed
 * across names and no new statistic is defined: every output is one that lh_kept_spread* / lh_kept_compare* returns for sub-lists.
 *   SPREAD WINDOWS.  win is lh_kept_series*' HOST array of 2 * nwin values under its rules: half-open slices [lo, hi) of the list
 *   with 0 <= lo < hi <= nkept, 1 <= nwin <= LH_MAX_WINDOWS, which may overlap, repeat and come in any order.
 *   DRIFT WINDOWS.  win is a HOST array of 4 * nwin uint32 values, 1 <= nwin <= LH_MAX_WINDOWS.  Window w compares
 *   base = kept[win[4w] .. win[4w+1]) with cur = kept[win[4w+2] .. win[4w+3]): both are slices of the ONE list, each with
 *   0 <= lo < hi <= nkept, and (base_hi - base_lo) + (cur_hi - cur_lo) <= LH_MAX_KEPT.  The two slices may overlap, coincide and
 *   stand in either order in the list.  A fixed baseline is the same base slice in every window.  Both kinds of windows travel by
 *   value.
 *   LAYOUT, window-major, as for lh_kept_series*: entry (w, m) lies at index e = w * n + m (n: nmetrics, or the ids' n);
 *   per-percentile outputs lie at e * np + i.
 *   CONTRACT -- this is the whole definition:
 *   - Window w's block of every output of lh_kept_spread_series* is byte for byte what lh_kept_spread* (the same form, the same
 *     rows or ids, p, np) writes for the list (kept + lo_w, hi_w - lo_w).
 *   - This includes sum, m2 and sum_le: they are taken in the same fixed order, the same in both kernel shapes.
 *   - Wrapped totals behave as lh_kept_spread*'s do; np == 0 is allowed; a handle listed twice counts twice.
 *   - Window w's block of every output of lh_kept_drift* is byte for byte what lh_kept_compare* (the same form, the same rows or
 *     ids) writes for the lists (kept + base_lo, base_hi - base_lo) and (kept + cur_lo, cur_hi - cur_lo).
 *   - This covers all eight outputs, w1 and shift among them, in both kernel shapes.
 *   - A name with no samples on one side of a window has NaN distances with key and prefixes 0 in that window, and only there.
 *   - Identical slices give exact zeros for non-empty names.
 *   - A DEVICE id outside the block of some handle of window w yields, in that window only, the all-zero entry of
 *     lh_kept_spread_series* or the entry of two empty sides of lh_kept_drift* (the window's two slices count), and nothing is read
 *     for it.
 *   CHECKS on the host, before any handle is looked at, in lh_kept_series*' order.  LH_EINVAL: the ids and list rules; NULL or
 *   misaligned win; nwin == 0 or > LH_MAX_WINDOWS; a slice with lo >= hi or hi > nkept; a drift window whose two slices hold more
 *   than LH_MAX_KEPT handles together; flags != 0; the family's own argument rules, exactly as lh_kept_spread* / lh_kept_compare*
 *   have them.  Then LH_ERANGE: nmetrics > 0xffffffff.  Then nmetrics == 0 / n == 0 -> LH_OK with nothing written.  After the host
 *   checks, in this order: LH_EINVAL for handles on different devices; LH_ERANGE, with nothing enqueued and nothing written, unless
 *   the rows or every HOST id lie inside EVERY listed handle's block, whether or not a window names the handle.  No output is
 *   written on any refusal.
 *   ORDERING, staging, hold and lifetime as for lh_kept_series*: host forms bring nwin * n entries back through the unit's staging
 *   block and are complete on return; device forms return after enqueueing, with ALL listed handles under one hold; READ-ONLY.  One
 *   window per blockIdx.y of the parents' two kernel shapes, which give identical bytes; the switch takes the ENTRIES, nwin * n.
 *   OUT OF SCOPE: top and movers per window; sharing cell reads between overlapping windows; more than LH_MAX_KEPT handles per
 *   call; LH_LE_PER_METRIC. */
int lh_kept_spread_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2,
                          int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le);
int lh_kept_spread_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                 size_t nmetrics, const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count,
                                 double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le,
                                 double *d_sum_le);
int lh_kept_spread_series_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                              const double *p, size_t np, uint32_t flags, void *stream, uint64_t *count, double *sum, double *m2,
                              int16_t *pkeys, uint8_t *pvalid, uint64_t *count_le, double *sum_le);
int lh_kept_spread_series_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids,
                                     size_t n, const double *p, size_t np, uint32_t flags, void *stream, uint64_t *d_count,
                                     double *d_sum, double *d_m2, int16_t *d_pkeys, uint8_t *d_pvalid, uint64_t *d_count_le,
                                     double *d_sum_le);
int lh_kept_drift(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                  uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                  uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift);
int lh_kept_drift_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                         uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks, int16_t *d_ks_key,
                         uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift);
int lh_kept_drift_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                      uint32_t flags, void *stream, uint64_t *count_a, uint64_t *count_b, double *ks, int16_t *ks_key,
                      uint64_t *ks_below_a, uint64_t *ks_below_b, double *w1, double *shift);
int lh_kept_drift_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                             uint32_t flags, void *stream, uint64_t *d_count_a, uint64_t *d_count_b, double *d_ks,
                             int16_t *d_ks_key, uint64_t *d_ks_below_a, uint64_t *d_ks_below_b, double *d_w1, double *d_shift);
/* THE K NAMES THAT LEAD, AND THE K THAT MOVED MOST, OVER KEPT INTERVALS: lh_top* and lh_movers* over handles, the two readers that
 * SELECT across names, for the windows that exist only as handles -- "which 20 of my 65 536 endpoints have the worst p99 over the
 * last minute", "whose distribution moved most against the same minute an hour ago" -- so that k entries travel instead of the
 * per-name readers' arrays over every name, and no dense buffer is filled.  With C[b] = the sum over the list of the name's cell b,
 * in 64 bits wrapping (lh_kept_across' C; a handle listed twice counts twice), nothing is summed across names and no new statistic
 * is defined: every ranked value is one an lh_kept_* reader above returns for the same lists.  lh_top_entry, lh_mover_entry,
 * LH_TOP_*, LH_MOVERS_* and LH_MAX_TOP are lh_top's and lh_movers'.
 *   lh_kept_top, lh_kept_top_device
 *                     lh_top's CANDIDATES, SCORE, ORDER and FIELDS, word for word, for a snapshot whose cells are C.  count is the
 *                     wrapping sum of the handles' row_count entries (no cell is read for it), and a row is a candidate iff that
 *                     count != 0.  sum is BIT-EQUAL to lh_kept_across' sum for the same list and row (the same step in the same
 *                     order, in both kernel shapes).  LH_TOP_BY_PERCENTILE ranks the bin of the bucket lh_kept_across selects for
 *                     p = arg, and pkey is its pkeys entry.  LH_TOP_BY_COUNT_ABOVE ranks count minus lh_kept_count_le's cum at
 *                     bounds = {arg}: the same bound-to-key rule, +-Inf and saturation.  A name whose total wraps past 2^64 has
 *                     count and its candidate status as defined; its other fields and its rank are unspecified (nothing faults).
 *   lh_kept_movers, lh_kept_movers_device
 *                     lh_movers' definitions for a[j] / b[j] = C over the `base` / `cur` list (lh_kept_compare's two sides).
 *                     CANDIDATES: the rows with count_a != 0 and count_b != 0.  The LH_MOVERS_BY_KS, _BY_W1 and _BY_SHIFT scores
 *                     are BIT-EQUAL to lh_kept_compare's ks, w1 and shift for the same lists (its walk; its two shapes agree bit
 *                     for bit, so these do), and for BY_KS key is its ks_key.  LH_MOVERS_BY_PERCENTILE:
 *                     score = (double)((int64)bin_cur - (int64)bin_base), each bin the one lh_kept_across selects for p = arg over
 *                     that side's list; key / key_base are the two pkeys.  1 <= nbase, 1 <= ncur, nbase + ncur <= LH_MAX_KEPT, as
 *                     for lh_kept_compare; longer windows go through lh_kept_merge first.  Identical lists give score 0 for every
 *                     candidate, and the lowest ids win.  Wrapped totals: unspecified (nothing faults).
 *   There are no _ids forms: the candidates of a selection are a range.  `first` is an ABSOLUTE row number, and ids are absolute.
 *   ORDER OF THE CHECKS.  On the host, before any handle is looked at -- LH_EINVAL: a NULL or misaligned list; a wrong list length
 *   (top: nkept == 0 or > LH_MAX_KEPT; movers: nbase == 0, ncur == 0 or nbase + ncur > LH_MAX_KEPT); a NULL entry; unknown `by`;
 *   unknown flag bits (LH_TOP_ASCENDING / LH_MOVERS_ASCENDING are the known ones); lh_top's / lh_movers' rules for arg (NaN for
 *   BY_PERCENTILE and BY_COUNT_ABOVE, outside [0, 1] for BY_PERCENTILE); k == 0 or k > LH_MAX_TOP; NULL out or n_out, out not
 *   8-byte aligned, n_out not aligned to its type (size_t in the host forms, uint32_t in the device forms); then LH_ERANGE:
 *   nmetrics > 0xffffffff.  nmetrics == 0: the host forms write *n_out = 0 and return LH_OK before any handle is looked at; the
 *   device forms look at the handles' devices only (LH_EINVAL for more than one), zero d_n_out on `stream` and return LH_OK.
 *   Then the handles are looked at -- LH_EINVAL: handles on different devices; LH_ERANGE, nothing enqueued and nothing written:
 *   [first, first + nmetrics) not inside EVERY handle's block (both lists).  Entries at and beyond n_out are never written.
 *   ORDERING, staging and lifetime: the work goes on `stream` (a hipStream_t of the handles' device; NULL: its null stream): a
 *   score pass over every row in one of the reader's two kernel shapes (lh_tool_kept_switch; identical bytes), then lh_top's exact
 *   radix select and sort in one workgroup.  Host forms return with the first n_out entries in `out`; entries and n_out come back
 *   in one copy through a pinned block of the library's, whatever memory `out` is.  Device forms take device memory for both and
 *   return after enqueueing, with ALL listed handles (both lists) under ONE hold, so that lh_kept_release waits for the call; the
 *   unit's records block is guarded by an event, so a call on another stream waits for it on the device.  READ-ONLY: no handle,
 *   snapshot or engine is written.  One records block per DEVICE behind the unit's own mutex: calls take turns. */
int lh_kept_top(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                uint32_t flags, void *stream, lh_top_entry *out, size_t *n_out);
int lh_kept_top_device(lh_kept *const *kept, size_t nkept, uint32_t first, size_t nmetrics, uint32_t by, double arg, size_t k,
                       uint32_t flags, void *stream, lh_top_entry *d_out, uint32_t *d_n_out);
int lh_kept_movers(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first, size_t nmetrics,
                   uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_mover_entry *out, size_t *n_out);
int lh_kept_movers_device(lh_kept *const *base, size_t nbase, lh_kept *const *cur, size_t ncur, uint32_t first,
                          size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                          lh_mover_entry *d_out, uint32_t *d_n_out);
/* TOP-K PER WINDOW OF KEPT INTERVALS: lh_kept_top* and lh_kept_movers* for MANY windows of one list of handles in ONE call -- which
 * 20 endpoints had the worst p99 in each of the last 60 seconds, which 20 moved most in each second against the minute before the
 * deploy, and from when on a given name appears among them -- where one lh_kept_top* / lh_kept_movers* call per window pays the
 * unit's mutex, a hold, two launches and, in the host form, a round trip each time.  This lifts top and movers per window from the
 * out-of-scope lists of the two blocks above (lh_kept_series* and lh_kept_spread_series* / lh_kept_drift*): the select per window
 * they waited for is one select workgroup per window.
 *   WINDOWS.  lh_kept_top_series* takes lh_kept_series*' HOST array of 2 * nwin values under its rules: half-open [lo, hi),
 *   0 <= lo < hi <= nkept, 1 <= nwin <= LH_MAX_WINDOWS; windows may overlap, repeat and come in any order.
 *   lh_kept_movers_series* takes lh_kept_drift*'s 4 * nwin values {base_lo, base_hi, cur_lo, cur_hi} under its rules: both are
 *   slices of the one list, they may overlap, coincide and stand in either order, and the two slices hold at most LH_MAX_KEPT
 *   handles together.
 *   LAYOUT.  n_out is an array of nwin counts: size_t in the host forms, uint32_t in the device forms.  Window w's entries lie at
 *   out[w * k .. w * k + n_out[w]).  Entries of a window's block at and beyond n_out[w] are never written.
 *   CONTRACT -- this is the whole definition:
 *   - Window w's block of out and n_out[w] are byte for byte what lh_kept_top* (the same form, the same first, nmetrics, by, arg, k,
 *     flags) writes for the list (kept + lo_w, hi_w - lo_w).
 *   - For lh_kept_movers_series* they are what lh_kept_movers* writes for base = (kept + base_lo, base_hi - base_lo) and
 *     cur = (kept + cur_lo, cur_hi - cur_lo).
 *   - This holds for sum and score, in both kernel shapes.
 *   - A window with no candidate has n_out[w] = 0, and nothing of its block is written.
 *   - A handle listed twice counts twice.
 *   - Wrapped totals behave as the parents' do.
 *   - Nothing is summed across names and no new statistic is defined.
 *   CHECKS on the host, before any handle is looked at, in lh_kept_top*'s order with the windows' term behind the list's rules --
 *   LH_EINVAL: a NULL or misaligned list; nkept == 0 or > LH_MAX_KEPT; a NULL entry; NULL or misaligned win; nwin == 0 or
 *   > LH_MAX_WINDOWS; a slice with lo >= hi or hi > nkept; a movers window whose two slices hold more than LH_MAX_KEPT handles
 *   together; unknown `by`; unknown flag bits; lh_top's / lh_movers' rules for arg; k == 0 or k > LH_MAX_TOP; NULL out or n_out, out
 *   not 8-byte aligned, n_out not aligned to its type.  Then LH_ERANGE: nmetrics > 0xffffffff.  nmetrics == 0: the host forms write
 *   nwin zeros to n_out and return LH_OK before any handle is looked at; the device forms look at the handles' devices only
 *   (LH_EINVAL for more than one), zero nwin counts on `stream` and return LH_OK.  Then the handles are looked at, as for the other
 *   window forms -- LH_EINVAL: handles on different devices; LH_ERANGE, nothing enqueued and nothing written: [first, first +
 *   nmetrics) not inside EVERY listed handle's block, whether or not a window names the handle.  No output is written on any
 *   refusal.  There are no _ids forms, as for the parents.
 *   ORDERING, staging and hold: the work goes on `stream`, under the unit's mutex: the parents' score pass with one window per
 *   blockIdx.y (the shape switch, lh_tool_kept_switch, takes the ENTRIES, nwin * nmetrics; identical bytes in both shapes), then
 *   lh_top's exact radix select and sort with one workgroup per window.  The records of a call go to ONE block of at most 64 MiB:
 *   the two passes run over chunks of consecutive windows that fit (a call of up to 8 192 names is one chunk at any nwin, 65 536
 *   names take 25 windows a chunk), one behind the other on `stream`.  Host forms bring nwin * k entries and nwin counts back in
 *   ONE copy through the unit's pinned block (at most 4 MiB + 512 B), then copy n_out[w] entries per window to the caller, and are
 *   complete on return.  Device forms return after enqueueing, with ALL listed handles under one hold; the records block is
 *   guarded by the unit's event as for lh_kept_top*.  READ-ONLY.
 *   OUT OF SCOPE: sharing cell reads between overlapping windows; a select that spreads ONE window over several workgroups; _ids
 *   forms; more than LH_MAX_KEPT handles a call. */
int lh_kept_top_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                       uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_top_entry *out, size_t *n_out);
int lh_kept_top_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                              uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_top_entry *d_out,
                              uint32_t *d_n_out);
int lh_kept_movers_series(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                          uint32_t by, double arg, size_t k, uint32_t flags, void *stream, lh_mover_entry *out, size_t *n_out);
int lh_kept_movers_series_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first,
                                 size_t nmetrics, uint32_t by, double arg, size_t k, uint32_t flags, void *stream,
                                 lh_mover_entry *d_out, uint32_t *d_n_out);
/* PER-NAME BOUNDS AND BURN-RATE ALERTS OVER KEPT INTERVALS: lh_kept_slo*, lh_kept_burn*.  A real SLO has its own threshold per
 * endpoint: lh_kept_slo* is lh_kept_heat* with a ROW OF BOUNDS PER ENTRY (lh_count_le's LH_LE_PER_METRIC layout), which the entry
 * points above keep refusing; lh_kept_burn* is the multi-window burn-rate rule over one bound and one error budget per entry -- the
 * names whose bad fraction exceeds rate x budget in the short window AND in the long one -- of which k records travel, not every
 * name's counts.  Nothing is summed across names and no new statistic is defined: every count is one lh_kept_heat* returns.
 *   THE PER-ENTRY ARRAYS are the ids' kind of argument.  A host form takes HOST arrays, checks them, copies them to the device on
 *   `stream` (a pinned block and a device block of the unit's, under its mutex) and waits before it returns, after a failure too.
 *   A device form takes DEVICE arrays, 8-byte aligned, on the handles' device, which the kernel reads behind `stream`; the host
 *   never sees them, and the kernel is safe on any bytes: each bound is taken on its own, so a decreasing device row is simply
 *   answered bound by bound, and a NaN bound takes in no bin and gives cum 0.
 *   WINDOWS, rows, ids and `stream` exactly as for lh_kept_heat*; the whole list is the one window [0, nkept).
 *   lh_kept_slo, lh_kept_slo_device, lh_kept_slo_ids, lh_kept_slo_ids_device
 *     bounds is [n * nb] doubles, row m for entry m (row first + m, or ids[m]), 1 <= nb <= LH_MAX_BOUNDS; flags must be 0.
 *     cum[(w * n + m) * nb + j] and total[w * n + m]; either may be NULL, not both.
 *     CONTRACT -- this is the whole definition:
 *     - Entry (w, m) of cum and total is byte for byte what lh_kept_heat_ids* writes for window w and the one row of entry m with
 *       bounds + m * nb, nb.
 *     - This holds in both kernel shapes, which agree exactly: only integers are involved.
 *     - total is exact modulo 2^64, as lh_kept_heat*'s is, and so is cum.
 *     - A DEVICE id outside some handle's block gives the empty entry in that window.
 *     CHECKS on the host, before any handle is looked at, in lh_kept_heat*'s order.  LH_EINVAL: the ids, list and window rules;
 *     nb == 0 or nb > LH_MAX_BOUNDS; NULL bounds; both outputs NULL; flags != 0; arrays not 8-byte aligned.  Then LH_ERANGE:
 *     n > 0xffffffff, before a bound is read, as for lh_count_le (bounds holds n * nb doubles whatever the call returns, and no
 *     caller has 2^32 rows of them).  Then n == 0 -> LH_OK with nothing written.  Then, host forms only, every row of bounds by
 *     lh_count_le's rule -- LH_EINVAL for a NaN or a decreasing row (equal neighbours allowed; -0.0 == 0.0).  Then the handles, as
 *     for lh_kept_heat*: LH_EINVAL for more than one device, LH_ERANGE for rows or HOST ids outside some listed handle's block.
 *   lh_kept_burn, lh_kept_burn_device, lh_kept_burn_ids, lh_kept_burn_ids_device
 *     rate[nwin]: HOST doubles in all forms, which travel by value like the windows.  bounds[n]: one bound per entry.  budget[n]:
 *     the allowed bad fraction per entry, e.g. 0.001.  flags must be 0.  With cum and total as lh_kept_slo* defines them for nb = 1,
 *     for window w and entry m:
 *         bad   = total - cum
 *         t     = rate[w] * budget[m]                              one rounded product
 *         fires = total != 0 && (double)bad > t * (double)total    a second rounded product; strict
 *     in IEEE doubles, the conversions the language's uint64 -> double, nothing contracted.  Entry m is REPORTED iff it fires in
 *     EVERY window of the call.  out receives the records {entry = m, row = first + m or ids[m]} of the reported entries in
 *     ascending m: the first min(*n_out, k) are written and the rest of out is left untouched; *n_out (uint64) is the number of
 *     reported entries whatever k is; k == 0 with NULL out is a count-only call.  cum / total (optional, [nwin * n]) have exactly
 *     lh_kept_slo*'s bytes for nb = 1.  Device forms take device pointers for out, n_out, cum and total; host forms bring the
 *     records and the count back in one copy.  The result depends on neither timing nor the kernel shape: an entry that does not
 *     fire adds 1 to an integer word of its m, and ONE workgroup then walks m in ascending order.
 *     A NaN in a device budget never fires (the comparison is false); a device id outside a handle's block never fires (its total
 *     is 0 there).  Firing is unspecified once a total has wrapped past 2^64; cum and total stay exact modulo 2^64.
 *     CHECKS on the host, before any handle is looked at.  LH_EINVAL: the ids, list and window rules; flags != 0; NULL rate, bounds,
 *     budget or n_out; k > 0 with NULL out; rate, bounds, budget, n_out, cum or total not 8-byte aligned, out not 4-byte aligned; a
 *     NaN or negative rate (all forms).  Then LH_ERANGE: n > 0xffffffff, before a bound or a budget is read.  Then n == 0 -> LH_OK
 *     with nothing written, n_out included.  Then, host forms only, LH_EINVAL for a NaN or negative budget or a NaN bound.  Then
 *     the handles as above.  No output is written on any refusal.
 *   ORDERING, hold and lifetime as for lh_kept_heat*: the work goes on `stream` under the unit's mutex; host forms are complete on
 *   return; device forms return after enqueueing with ALL listed handles under one hold.  lh_kept_burn*'s n words of scratch come
 *   from the records block of lh_kept_top*, guarded by the unit's event, and are zeroed on `stream`.  READ-ONLY.  The shape switch
 *   (lh_tool_kept_switch) takes the ENTRIES of a call, nwin * n.
 *   OUT OF SCOPE: sharing cell reads between overlapping windows; more than LH_MAX_KEPT handles a call; per-name bounds for
 *   lh_kept_top*'s count-above; an OR or a per-pair rule across windows (make two calls); retuning the shape switch; any change to
 *   the snapshot-side lh_count_le. */
typedef struct { uint32_t entry, row; } lh_burn_hit;
int lh_kept_slo(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_slo_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                       const double *d_bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_slo_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                    const double *bounds, size_t nb, uint32_t flags, void *stream, uint64_t *cum, uint64_t *total);
int lh_kept_slo_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                           const double *d_bounds, size_t nb, uint32_t flags, void *stream, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_burn(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                 const double *rate, const double *bounds, const double *budget, size_t k, uint32_t flags, void *stream,
                 lh_burn_hit *out, uint64_t *n_out, uint64_t *cum, uint64_t *total);
int lh_kept_burn_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, uint32_t first, size_t nmetrics,
                        const double *rate, const double *d_bounds, const double *d_budget, size_t k, uint32_t flags,
                        void *stream, lh_burn_hit *d_out, uint64_t *d_n_out, uint64_t *d_cum, uint64_t *d_total);
int lh_kept_burn_ids(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *ids, size_t n,
                     const double *rate, const double *bounds, const double *budget, size_t k, uint32_t flags, void *stream,
                     lh_burn_hit *out, uint64_t *n_out, uint64_t *cum, uint64_t *total);
int lh_kept_burn_ids_device(lh_kept *const *kept, size_t nkept, const uint32_t *win, size_t nwin, const uint32_t *d_ids, size_t n,
                            const double *rate, const double *d_bounds, const double *d_budget, size_t k, uint32_t flags,
                            void *stream, lh_burn_hit *d_out, uint64_t *d_n_out, uint64_t *d_cum, uint64_t *d_total);
/* WIRE LINES FOR ANY PER-NAME COLUMNS: lh_names_*, lh_lines*.  The reference's serializers do not care where a key came from:
 *   GraphiteProtocol    /root/reference/graphite.go:37-48    formats every key -> float64 pair of the set
 *   OpenTSDBProtocol    /root/reference/opentsdb.go:45-58    likewise
 *   ProcessedMetricSet  /root/reference/metrics.go:62-66     map[string]float64: gauges and whatever a subscriber added too
 * lh_serialize (K6, below) is that loop for the keys processMetrics makes.  lh_lines* is that loop for ARBITRARY columns that
 * already lie in device memory -- the arrays the readers above return from their _device forms (count_le's cum / total, spread's
 * m2 / sum_le / pkeys, the records of lh_top_device, lh_across' count / sum / pkeys): each per-name key / value pair becomes
 * one line, assembled and formatted on the device as K6 does it.  No statistic is defined and nothing is summed across names.
 *   NAMES.  A unit beside the engine cannot see the engine's name table: an lh_names handle holds a device copy of the names
 *   [0, lh_num_metrics) at the time of lh_names_create, fetched through lh_metric_name, on device `device` (the engine's
 *   lh_config.device).  lh_names_refresh appends the names interned since (*count, may be NULL: the names held).  The engine
 *   must be alive for create and refresh only; lh_lines* never touches it.  A name longer than 16 MiB - 8 KiB, or more than
 *   4 GiB of names -> LH_ERANGE from create / refresh.
 *   LINES.  One line per (entry, column):  prefix  key  sep  %f  suffix  with key = fmt.Sprintf(label, name) and the value
 *   printed as Go's %f prints a float64 (as lh_serialize).  LH_FMT_UNDERSCORE_TO_DOT is applied to the whole key, name and
 *   label text alike (graphite.go:42), as lh_serialize does.  Lines are entry-major, columns in the order given; no trailing
 *   NUL.  prefix + sep + suffix + all labels: at most 4 KiB.
 *   VALUES.  A source element becomes a float64 the way the reference converts a count, float64(count) (metrics.go:349):
 *     LH_OP_VALUE       a
 *     LH_OP_RATIO       a / b, an IEEE divide
 *     LH_OP_SQRT_RATIO  sqrt(a / b), correctly rounded
 *     LH_OP_DIFF        a - b: in uint64 (wrapping), then converted, when both elements are integers; in float64 otherwise
 *   LH_COL_KEY (an int16 bucket key, printed as its value D[(uint16)key ^ 0x8000], D bit for bit lh_codec_tables' D) is allowed
 *   for `a` under LH_OP_VALUE only.  NaN prints as "NaN", +-Inf as "+Inf" / "-Inf", as Go does; with LH_LINES_SKIP_NAN a
 *   NaN line is omitted instead (lh_compare returns NaN for a name that is empty on one side).
 *   WHICH ENTRIES EMIT.  Entry m's name is first + m, or (lh_lines_ids*) the uint32 at (char *)d_ids + m * id_stride -- so the
 *   `id` field of lh_top_entry / lh_mover_entry records is used directly with id_stride 32.  An entry whose
 *   d_row_count element (at byte stride row_count_stride; usually the count / total array a reader returned) is 0 emits nothing,
 *   as lh_serialize omits names without samples; d_row_count NULL: every entry emits.  A column's line is omitted where
 *   valid[m * valid_stride] == 0.  An id at or beyond the names held emits nothing (the host never sees device ids: the
 *   stance of the *_ids_device forms above).  first + n beyond the names held -> LH_ERANGE.
 *   EVERYTHING DATA-SHAPED IS DEVICE MEMORY IN ALL FOUR FORMS: columns, valid arrays, row counts and ids are the outputs of
 *   the readers' _device forms, valid until `stream` has passed the call.  The work goes on `stream` (a hipStream_t; usually
 *   lh_snapshot_stream(s), so that it runs behind the reader that fills the columns); NULL: the null stream of the handle's
 *   device.
 *   TEXT.  Host forms (lh_lines, lh_lines_ids): lh_serialize's size-then-call protocol -- *len always receives the byte
 *   count; when it exceeds cap, or out is NULL, nothing is written and the status is LH_OK.  They return when the text is
 *   in `out`.  Device forms (lh_lines_device, lh_lines_ids_device) return after enqueueing and never wait for their own work:
 *   *d_len (8-byte aligned device memory) always receives the total, d_out is written only when the total fits cap (d_out
 *   may be NULL to size).
 *   LH_EINVAL, decided on the host before the handle is dereferenced or a device is touched: nm, cols, fmt (or one of its
 *            three pieces) or len / d_len NULL; ncols 0 or above LH_MAX_COLUMNS; an unknown type, op or flag bit; a non-zero
 *            reserved field; a label without exactly one %s (or with a % that is neither %s nor %%); prefix + sep + suffix +
 *            labels above 4 KiB; `a` NULL; an op other than LH_OP_VALUE with b NULL; LH_COL_KEY anywhere but `a` under
 *            LH_OP_VALUE; a, b, d_row_count or their strides not a multiple of the element size (8 / 8 / 4 / 2 bytes for
 *            F64 / U64 / U32 / KEY); d_ids NULL with n > 0; d_ids or id_stride not a multiple of 4; len / d_len misaligned.
 *   LH_ERANGE: n above 2^32 - 1 (a cause of LH_EINVAL wins over it); a block of names the handle does not hold.
 *   n == 0 -> LH_OK with *len = 0 before any device call (a device form enqueues the one store of *d_len = 0).
 *   THREADING.  One mutex per handle, held for the length of a call.  The handle's blocks -- descriptors, labels, line
 *   lengths, workgroup offsets, the host forms' text -- only grow and are guarded by an event across streams: a device-form
 *   call returns while they are in use, and the next call (or lh_names_refresh, before it replaces the name table) waits
 *   for that event before it rewrites them.  lh_names_destroy waits for it too. */
typedef struct lh_names lh_names;
struct lh_line_format;             /* the wire format's pieces: defined with lh_serialize below */
int lh_names_create(lh_engine *e, int device, lh_names **out);
int lh_names_refresh(lh_names *nm, uint32_t *count);
int lh_names_destroy(lh_names *nm);

#define LH_MAX_COLUMNS 128
enum { LH_COL_F64 = 0, LH_COL_U64 = 1, LH_COL_U32 = 2, LH_COL_KEY = 3 };
enum { LH_OP_VALUE = 0, LH_OP_RATIO = 1, LH_OP_SQRT_RATIO = 2, LH_OP_DIFF = 3 };
enum { LH_LINES_SKIP_NAN = 1 };
typedef struct lh_column {            /* 64 bytes */
    const char *label;                /* Go format with exactly one %s ("%s_std"); "%%" is a literal % (as lh_serialize) */
    const void *a;                    /* DEVICE memory; element of entry m at (char *)a + m * a_stride */
    const void *b;                    /* likewise; NULL for LH_OP_VALUE */
    const uint8_t *valid;             /* DEVICE, may be NULL: entry m's line is omitted when valid[m * valid_stride] == 0 */
    uint64_t a_stride;                /* BYTES */
    uint64_t b_stride;
    uint64_t valid_stride;
    uint8_t a_type;                   /* LH_COL_* */
    uint8_t b_type;
    uint8_t op;                       /* LH_OP_* */
    uint8_t reserved0;                /* 0 */
    uint32_t reserved1;               /* 0 */
} lh_column;
int lh_lines(lh_names *nm, uint32_t first, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride,
             const lh_column *cols, size_t ncols, const struct lh_line_format *fmt, uint32_t flags, void *stream,
             char *out, size_t cap, size_t *len);
int lh_lines_ids(lh_names *nm, const uint32_t *d_ids, uint64_t id_stride, size_t n, const uint64_t *d_row_count,
                 uint64_t row_count_stride, const lh_column *cols, size_t ncols, const struct lh_line_format *fmt, uint32_t flags,
                 void *stream, char *out, size_t cap, size_t *len);
int lh_lines_device(lh_names *nm, uint32_t first, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride,
                    const lh_column *cols, size_t ncols, const struct lh_line_format *fmt, uint32_t flags, void *stream,
                    char *d_out, size_t cap, uint64_t *d_len);
int lh_lines_ids_device(lh_names *nm, const uint32_t *d_ids, uint64_t id_stride, size_t n, const uint64_t *d_row_count,
                        uint64_t row_count_stride, const lh_column *cols, size_t ncols, const struct lh_line_format *fmt,
                        uint32_t flags, void *stream, char *d_out, size_t cap, uint64_t *d_len);
/* K4 -- multi-GPU merge of a snapshot across the ranks of an RCCL communicator (one process per GPU).
 * Ingest is data-parallel: every rank buckets its own slice of the stream for ALL names; the only
 * exchange is this integer SUM of the occupied window of the uint64 bucket matrix at the flip
 * (cells are a commutative sum, metrics.go:278, 292).  The reference is single-process: no counterpart.
 *   comm   ncclComm_t (as void*) created by the caller with the RCCL named by lh_set_rccl_library
 *   plan   LH_MERGE_ALLREDUCE: every rank ends with every merged row;
 *          LH_MERGE_REDUCE_SCATTER: rank r ends with the merged rows of a contiguous block of names and
 *          extracts those with lh_extract_rows.  The blocks tile [0, nrows) in rank order and hold equal numbers of
 *          PACKED CELLS, not of names (names ranked by frequency would otherwise put every wide window into block 0
 *          and pad the other blocks up to it): use the returned [first, last)
 *   first_owned / last_owned  receive the [first, last) rows holding merged data on this rank
 * Runs on the snapshot's stream; dirty ranges are merged first (one MIN all-reduce on (lo, ~hi)), then every
 * row's own merged window travels, packed back to back; the window plan (prefix sums, block sizes) is computed
 * on the device and only two totals come back to size the collective.  Extract/clear stay exact. */
enum { LH_MERGE_ALLREDUCE = 0, LH_MERGE_REDUCE_SCATTER = 1 };
int lh_snapshot_merge(lh_snapshot *s, void *comm, int nranks, int rank, int plan, uint32_t nrows,
                      uint32_t *first_owned, uint32_t *last_owned);
/* What the last lh_snapshot_merge on this engine moved.  Every row travels with its OWN merged window
 * [lo_r, hi_r] (packed back to back), so an outlier sample widens one row, never the matrix -- and, when the wire word
 * is uint32, at its own cell width: 8, 16 or 32 bits, the narrowest that holds nranks x (the largest cell any rank
 * has in that row; all-reduced with the dirty ranges), so that the uint32 SUM of the collective never carries from one
 * cell of a word into the next.  Most names of a skewed stream hold small counts per interval: config 4's windows
 * (65 536 Zipf names, 8 ranks) travel at ~1.1 bytes per cell instead of 4. */
typedef struct lh_merge_info {
    uint64_t packed_cells;   /* sum over rows of the merged window widths, in cells                          */
    uint64_t send_bytes;     /* bytes handed to the collective (reduce-scatter: nranks x largest block)      */
    uint64_t recv_bytes;     /* bytes this rank ends up with                                                  */
    uint32_t widest_row;     /* widest merged window, in cells                                                */
    uint32_t occupied_rows;  /* rows with at least one cell on some rank                                      */
    uint64_t padded_words;   /* reduce-scatter: nranks x largest owner block, in wire words (>= packed_words; the
                              * ratio is what the equal-block collective costs over the packed matrix);
                              * all-reduce: packed_words */
    uint32_t cell_bytes;     /* the wire word: 8 (one cell per word), or 4 when no merged cell of the interval can
                              * reach 2^32 (nranks x the largest per-rank sample count of the interval < 2^32)  */
    uint32_t rows_8bit;      /* occupied rows that travelled at 8 bits per cell (4 cells per word) ...          */
    /* Device time of the merge's steps, HIP events on the snapshot stream (lh_snapshot_merge_info waits for the
     * last one): dirty-range all-reduce (with the pass over the rows' largest cells), window plan, pack, the
     * collective, unpack; span = first event to last, host round trip for the plan totals included. */
    float ranges_ms, plan_ms, pack_ms, collective_ms, unpack_ms, span_ms;
    uint64_t packed_words;   /* sum over rows of ceil(window cells x bits / 32) (uint32 words), or packed_cells */
    uint32_t rows_16bit;     /* ... and at 16 bits per cell (2 per word); the other occupied rows: one per word  */
    uint32_t reserved;
} lh_merge_info;
int lh_snapshot_merge_info(lh_snapshot *s, lh_merge_info *out);
/* Path (or soname) of the RCCL shared object the communicator comes from; default "librccl.so".
 * Process-wide; call before the first lh_snapshot_merge. */
int lh_set_rccl_library(const char *path);
/* K6 -- the interval's histogram keys as wire text, assembled and formatted on the device.
 * Replaces, for the histogram part of a ProcessedMetricSet, one fmt.Sprintf + map insert per key:
 *   processMetrics    /root/reference/metrics.go:495-499   <name>_count, _sum, _avg, percentile labels
 *   addAggregates     /root/reference/metrics.go:590-608   <name>_agg_avg, _agg_count, _agg_sum
 *   GraphiteProtocol  /root/reference/graphite.go:37-48    "cockroach.<host>.<key, _ -> .> %f %d\n"
 *   OpenTSDBProtocol  /root/reference/opentsdb.go:45-58    "put <key> %d %f host=<host>\n"
 * One line per key:  prefix  key  sep  value  suffix  with value printed as Go's %f prints a float64
 * (exact decimal expansion, 6 fractional digits, round-half-even, "NaN", "+Inf", "-Inf") and
 * key = fmt.Sprintf(label, name).  Lines are metric-major for metrics [first, first+nmetrics) that have
 * samples in this interval, keys in the order _count, _sum, _avg, labels[0..np), then (with
 * LH_SER_AGGREGATES, for names whose lifetime count is > 0) _agg_avg, _agg_count, _agg_sum; keys whose
 * percentile is invalid (metrics.go:379-384) are omitted.  Go's map iteration order is random, so this
 * is one of the orders the reference can produce.
 *   labels[np]  Go format strings holding exactly one %s ("%s_99.9"); "%%" is a literal %
 *   fmt         NUL-terminated pieces; LH_FMT_UNDERSCORE_TO_DOT applies graphite.go:42 to the key
 *   out/cap     host buffer; *len receives the byte count even when it exceeds cap, in which case
 *               nothing is written (size and call again).  No trailing NUL.
 * Every name in the range must have been interned.  prefix+sep+suffix+labels are limited to 2 KiB. */
typedef struct lh_line_format {
    const char *prefix;     /* "cockroach.<host>."        | "put "              */
    const char *sep;        /* " "                        | " <unix time> "     */
    const char *suffix;     /* " <unix time>\n"           | " host=<host>\n"    */
    uint32_t    flags;      /* LH_FMT_UNDERSCORE_TO_DOT   | 0                   */
    uint32_t    reserved;
} lh_line_format;
enum { LH_FMT_UNDERSCORE_TO_DOT = 1 };
enum { LH_SER_AGGREGATES = 1 };
int lh_serialize(lh_snapshot *s, uint32_t first, size_t nmetrics, const double *p, const char *const *labels,
                 size_t np, const lh_line_format *fmt, uint32_t flags, char *out, size_t cap, size_t *len);
/* One line per exported key, counter-major: "<prefix><name><sep>%f<suffix>" for every known counter and
 * "<prefix><name>_rate<sep>%f<suffix>" for those touched this interval (same lh_line_format and size-then-call
 * protocol as lh_serialize). */
int lh_serialize_counters(lh_snapshot *s, uint32_t first, size_t n, const lh_line_format *fmt, char *out, size_t cap,
                          size_t *len);
/* processHistograms' lifetime side effect (metrics.go:359-376) for every row of the snapshot, kept in
 * HBM: life_sum[m] += uint64(totalSum_m) (amd64 conversion, wrapping add), life_count[m] += count_m.
 * Applied at most once per snapshot; later calls return LH_OK without effect. */
int lh_snapshot_accumulate(lh_snapshot *s);
/* The lifetime stores of metrics [first, first+n) (histogramCountStore, metrics.go:127). */
int lh_lifetime(lh_engine *e, uint32_t first, size_t n, uint64_t *count, uint64_t *sum);
/* Go's %f of n float64 values, formatted on the device (parity tests of the formatter):
 * value i occupies out[i*slot .. i*slot + lens[i]); slot must be >= 336. */
int lh_format_f(lh_engine *e, const double *v, size_t n, char *out, size_t slot, uint32_t *lens);
/* Stream on which the snapshot's extract/clear work is ordered (hipStream_t). */
int lh_snapshot_stream(lh_snapshot *s, void **stream);
/* Returns the snapshot's buffer to the pool (cleared asynchronously). */
int lh_release(lh_snapshot *s);

/* Self-metrics of the engine (exposed by the host layer as gauges through
 * RegisterGaugeFunc, metrics.go:299).  Monotonic since lh_create. */
typedef struct lh_counters {
    uint64_t samples_single;       /* through k_ingest_single                           */
    uint64_t samples_small;        /* mixed, single-pass LDS kernel (<= 32 names)       */
    uint64_t samples_partitioned;  /* mixed, partition + LDS reduce                     */
    uint64_t samples_direct;       /* mixed, one global atomic per sample (small launches) */
    uint64_t launches;             /* ingest launches of any kind                       */
    uint64_t flips;                /* successful lh_flip calls                          */
    uint64_t flips_busy;           /* lh_flip calls that returned LH_EBUSY              */
    uint64_t extracts;             /* lh_extract / lh_extract_rows calls                */
    uint64_t backpressure_waits;   /* submitters that had to wait for a staging half-buffer */
    uint64_t window_misses;        /* samples the single-pass kernel sent to global atomics */
    uint32_t small_path_disabled;  /* 1 while adaptive dispatch routes few-name streams through the partitioned path */
    uint32_t regions_disabled;     /* 1 while a name-clustered stream keeps the mixed ingest on the exact-layout scatter */
    uint64_t scratch_bytes;        /* HBM scratch of the partitioned mixed ingest: the engine's shared block (the host-fed
                                      lanes' own small blocks, LH_OPT_LANE_SCRATCH_BLOCKS, are not counted) */
    uint64_t sublaunches;          /* partitioned sub-launches (a large launch is cut so the scratch stays bounded) */
    uint64_t samples_partitioned_v2; /* of samples_partitioned: through the survey + 2-byte-record path          */
    uint64_t counter_events;         /* (id, amount) events through lh_submit_counts*                               */
    uint64_t region_overflows;       /* records the region scatter counted through the exact out-of-window path     */
    uint64_t samples_partitioned_v3; /* of samples_partitioned: through the 8 193 .. 65 536-name path               */
    uint64_t window_log2;            /* that path's second-level window width (log2 bins) for the next call         */
    uint64_t records_level1;         /* that path: 4-byte records its first level wrote (samples no hot window took)  */
    uint64_t records_level2;         /* ... records its second level forwarded to the reduce pass                     */
    uint64_t level2_overflows;       /* ... records that found a second-level region full (exact path)                */
    uint64_t reduce_window_misses;   /* ... records outside their window in the reduce pass (exact path)              */
    uint64_t surveys_reused;         /* calls that ran on an earlier call's survey (LH_OPT_SURVEY_EVERY)              */
    uint64_t scratch_alloc_failures; /* scratch blocks of the mixed ingest that could not be allocated (ABI 5)         */
    uint64_t samples_fallback;       /* samples that therefore went through the scratch-free kernel: exact, slower     */
    uint64_t survey_stale_pairs;     /* pairs a kept survey's hot windows no longer took (the values moved under it: the
                                        launch reports them, the next call surveys again)                              */
    uint64_t lane_scratch_bytes;     /* (ABI 6) HBM the host-fed lanes' launches hold beside scratch_bytes: their scratch
                                        blocks (up to LH_OPT_LANE_SCRATCH_BLOCKS of them, ~0.2 GiB each at 65 536 names;
                                        LH_OPT_SCRATCH_CAP_BYTES bounds the shared block only) and the two sets of survey
                                        tables the lanes share                                                         */
    uint64_t widenings;              /* (ABI 7) epoch buffers of 32-bit cells that moved to uint64 cells (an interval about to
                                        hold 2^32 samples, a merge whose sums may pass it, lh_snapshot_rows)                */
    uint64_t store_bytes;            /* (ABI 7) HBM of the epoch buffers' cell stores, wide stores of narrow engines included */
} lh_counters;
int lh_get_counters(lh_engine *e, lh_counters *out);

/* Settings.  Every option only chooses among EXACT kernel paths or sizes a buffer: no option (and no environment
 * variable -- the library never calls getenv) can change a result.  Takes effect for later calls; not synchronised
 * with concurrent submits (set options before the producers start).  These are the operational ones; the keys that
 * only exist to steer the mixed ingest's path choice in tests and tuning runs (generation switches, size thresholds,
 * window widths, the allocation-failure hook) live in loghisto_gpu_tuning.h and are not part of the drop-in contract.
 *   LH_OPT_EXTRACT_ZERO_COPY  0 / 1: small extract results (<= 32 KiB) are stored by the kernel straight into pinned
 *                             host memory (default 1); a value >= 4096 also sets that size limit (measured: beyond
 *                             32 KiB the copy engine wins -- 1 024 names, 158 KB: 48 us by copy, 95 us by stores)
 *   LH_OPT_SCRATCH_CAP_BYTES  upper bound of the mixed ingest's SHARED scratch block (default 1.5 GiB, >= 64 MiB); the
 *                             host-fed lanes' own blocks are bounded by LH_OPT_LANE_SCRATCH_BLOCKS x a lane-sized launch's
 *                             need and reported as lh_counters.lane_scratch_bytes
 *   LH_OPT_SUBLAUNCH_PAIRS    largest partitioned sub-launch, 2^22 .. 2^30 pairs, rounded down to a power of two
 *                             (default 2^29; a sub-launch is halved until its scratch fits the cap).
 *                             Engines with more than 8 192 names (two scatter levels: ~1.2 GB of chunk pools and
 *                             ~0.35 ms of fixed work per launch) are NOT cut by default -- a 1e9-pair launch over
 *                             65 536 names takes a 9 GB block -- unless one of these two options was set, and then
 *                             not below 2^28 pairs.  A block that cannot be had never fails a call: the sub-launch goes
 *                             through the scratch-free kernel (lh_counters.scratch_alloc_failures / samples_fallback)
 *   LH_OPT_SURVEY_EVERY       33 .. 65 536 names: a call may run on the survey of an earlier call (hot names, region
 *                             sizes, per-partition ranking stay in the scratch block) until this many calls have used
 *                             it (default 32; 1 = every call surveys).  Only while the stream looks the same: a survey
 *                             is also repeated when the window width or scatter shape changed, when anything else used
 *                             the block, or when more than 2 % of the pairs of the calls completed since took an
 *                             overflow / window-miss path or stayed out of the hot windows that took them when the
 *                             survey was new (the stream's values moved: lh_counters.survey_stale_pairs).  A stale
 *                             survey costs speed -- one call's worth -- never exactness
 *   LH_OPT_LANE_SCRATCH_BLOCKS  0 .. 16 (default 0 since round 6; 16 before): 0 = a host-fed mixed launch (lh_submit_pairs*,
 *                             lh_commit_pairs*: one staging half-buffer, at most 2^22 pairs) takes the direct path -- one
 *                             link-bound pass through a per-workgroup LDS table of cells, no scratch: 0.89 - 0.90 of the
 *                             link at every name count.  n > 0 = such launches run partitioned in one of n scratch blocks
 *                             of their own (first generation up to 8 192 names; above, the third generation on survey
 *                             tables the lanes share), one lane's later passes beside another lane's read (0.84 - 0.87 of
 *                             the link up to 8 192 names, 0.75 - 0.78 above; lh_counters.lane_scratch_bytes)
 *   LH_OPT_LANE_ZERO_COPY     0 / 1: the ingest kernels read the pinned staging buffers of lh_submit* / lh_reserve_pairs
 *                             in place over PCIe (default 1) instead of after a hipMemcpyAsync into HBM (0)
 *   LH_OPT_MERGE_NARROW_CELLS 0 / 1 (default 1): lh_snapshot_merge over more than one rank sends a row at 8 or 16 bits per
 *                             cell when nranks x its largest per-rank cell fits (lh_merge_info); 0 = every cell a whole
 *                             word.  A rank that sets 0 makes every rank of that merge send whole words (the bound
 *                             is all-reduced): ranks need not agree */
enum {
    LH_OPT_EXTRACT_ZERO_COPY = 5,
    LH_OPT_SCRATCH_CAP_BYTES = 6,
    LH_OPT_SUBLAUNCH_PAIRS = 7,
    LH_OPT_LANE_ZERO_COPY = 15,
    LH_OPT_SURVEY_EVERY = 16,
    LH_OPT_LANE_SCRATCH_BLOCKS = 18,
    LH_OPT_MERGE_NARROW_CELLS = 22
};
int lh_set_option(lh_engine *e, int option, uint64_t value);

/* Codec access for parity tests. */
/* key[i] = compress(d_v[i]) on device (metrics.go:316-322). */
int lh_compress_device(lh_engine *e, const double *d_v, int16_t *d_keys, size_t n, void *stream);
/* Same arithmetic but through the device restatement of Go's math.Log instead of
 * the fast path + threshold table (cross-check of the two device routes). */
int lh_compress_device_golog(lh_engine *e, const double *d_v, int16_t *d_keys, size_t n, void *stream);
/* Copies the device-generated tables to host: Tx[LH_NTHRESH] (thresholds in
 * x = 1+|v| space) and D[LH_NKEYS] (decompress by bin).  Either may be NULL. */
int lh_codec_tables(lh_engine *e, double *Tx, double *D);
/* max |v_log_f32(m) - log2(m)| over all 2^23 fp32 mantissas m in [1,2): the
 * measured bound the fast path's guard band rests on. */
int lh_selftest_vlog(lh_engine *e, double *max_abs_err);

#ifdef __cplusplus
}
#endif
#endif /* LOGHISTO_GPU_H */
