// lh_lines.hip -- lh_names_* and lh_lines* (include/loghisto_gpu.h): wire lines for any per-name columns that already lie in
// device memory, formatted on the device.  The reference's serializers do not care where a key came from:
//   GraphiteProtocol   /root/reference/graphite.go:37-48   "cockroach.<host>.<key, _ -> .> %f %d\n" for every key of the set
//   OpenTSDBProtocol   /root/reference/opentsdb.go:45-58   "put <key> %d %f host=<host>\n"
//   ProcessedMetricSet /root/reference/metrics.go:62-66    map[string]float64: gauges and whatever a subscriber added included
// This is that loop for the columns the readers beside the engine return (lh_count_le*, lh_spread*, lh_top*, lh_compare*,
// lh_movers*, lh_across*): one line per (entry, column), key = Sprintf(label, name), value by Go's %f.  It defines no
// statistic and sums nothing across names; the four ops are what turns the readers' arrays into the keys their header
// comments name (std = sqrt(m2 / count), mean_90 = sum_le / count_le, upper_90 = decompress(key), above = total - cum).
//
// Built BESIDE the engine, on its public C ABI only (lh_beside.h): it sees neither the engine's name table nor its value
// table, so a handle (lh_names) carries a device copy of the names, fetched through lh_num_metrics / lh_metric_name, and the
// unit's own D[] (lh::k_value_table, bit for bit lh_codec_tables' D).  It reads no snapshot at all.
//
// K6's structure (lh_kernels_fmt.hip) on the new inputs, one THREAD per line, three launches on the call's stream:
//   k_lines_len     the line's value and its length (fmt_f<false>), 0 for a line that is not emitted; per-workgroup totals
//   k_lines_scan    one workgroup: the exclusive scan of the workgroup totals, the grand total to boff[nblocks] and *d_len
//   k_lines_write   the text: a workgroup's lines are staged in LDS at the 16-byte phase their first byte has in the output
//                   and copied out with 16-byte stores; a workgroup whose lines exceed the staging area writes them straight
//                   to HBM.  Nothing is written when the total exceeds cap.
// line_value() is the one place a line's value is computed; both passes call it, so their bytes agree.  The descriptors
// (64 bytes a column, up to 128 of them: more than the kernel-argument space) and the labels travel in the handle's device
// block, through a pinned copy on the call's stream.  The formatter is lh_fmt.h, the one K6 formats with.
// tools/lines_bench.py measures it against lh_serialize over the same lines (profiles/lines.txt: 65 536 names x 15 keys, the
// three kernels 84 us against K6's 71 us, 1.18 x per output byte; most of the difference is in the length pass).
#include "../../include/loghisto_gpu.h"
#include "lh_beside.h"
#include "lh_codec.h"
#include "lh_fmt.h"
#include "lh_wave.h"

#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <string>
#include <vector>

namespace {

using namespace lh; // (lh_wave.h)
using namespace lh::beside;
using lh::fmt::BLOCK;

static_assert(sizeof(lh_column) == 64, "lh_column is 64 bytes");

constexpr uint32_t STAGE_LDS = 36864;   // staging bytes of one workgroup (256 lines x 144 B), as K6
constexpr uint32_t BLOB_MAX = 4096;     // prefix + sep + suffix + all labels
constexpr uint32_t NAME_LEN_MAX = (1u << 24) - 2 * BLOB_MAX; // a workgroup's 256 line lengths sum in 32 bits
constexpr uint32_t F_DOTS = 1, F_SKIP_NAN = 2, F_BY_ID = 4;

// a column as the kernels read it
struct DevCol {
    const char *a, *b;
    const uint8_t *valid;
    uint64_t a_stride, b_stride, valid_stride;
    uint8_t a_type, b_type, op, pad0;
    uint16_t pre_off, pre_len, post_off, post_len; // the label around %s, in the blob
    uint32_t pad1;
};
static_assert(sizeof(DevCol) == 64, "a descriptor is 64 bytes");

struct LinesArgs {
    const char *names;          // the handle's table: name id is names[name_off[id] .. name_off[id + 1])
    const uint32_t *name_off;
    const char *ids;            // F_BY_ID: entry m's name is *(uint32_t *)(ids + m * id_stride)
    const char *row_count;      // may be null
    const DevCol *cols;
    const char *blob;
    const double *D;            // null unless a column is LH_COL_KEY
    uint64_t id_stride, row_count_stride;
    uint32_t held, first, n, ncols, blob_len, flags;
    uint16_t prefix_off, prefix_len, sep_off, sep_len, suffix_off, suffix_len;
};

// ---- the value of a line ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_int(uint32_t type) { return type == LH_COL_U64 || type == LH_COL_U32; }
__device__ __forceinline__ u64 load_int(const char *p, uint32_t type)
{
    return type == LH_COL_U64 ? *reinterpret_cast<const u64 *>(p) : (u64) * reinterpret_cast<const uint32_t *>(p);
}
// float64(element) (metrics.go:349 for a count); a key goes through D[]
__device__ __forceinline__ double load_f64(const char *p, uint32_t type, const double *__restrict__ D)
{
    if (type == LH_COL_F64) return *reinterpret_cast<const double *>(p);
    if (type == LH_COL_KEY) return D[(uint32_t)(*reinterpret_cast<const uint16_t *>(p)) ^ 0x8000u];
    return (double)load_int(p, type);
}
// Which name entry m prints, false when the entry emits nothing: an id at or beyond the names held, a row count of 0.
__device__ __forceinline__ bool entry_name(const LinesArgs &a, uint32_t m, uint32_t *id)
{
    const uint32_t r = (a.flags & F_BY_ID) ? *reinterpret_cast<const uint32_t *>(a.ids + (uint64_t)m * a.id_stride) : a.first + m;
    *id = r;
    if (r >= a.held) return false;
    return !a.row_count || *reinterpret_cast<const u64 *>(a.row_count + (uint64_t)m * a.row_count_stride) != 0;
}
// The value of entry m's line for column c; false when the line is omitted (valid == 0, or a NaN under LH_LINES_SKIP_NAN).
// The ONE place a value is computed: the length pass and the write pass both call it.
__device__ __forceinline__ bool line_value(const LinesArgs &a, const DevCol &c, uint32_t m, double *v)
{
    if (c.valid && c.valid[(uint64_t)m * c.valid_stride] == 0) return false;
    const char *pa = c.a + (uint64_t)m * c.a_stride;
    double x;
    if (c.op == LH_OP_VALUE) {
        x = load_f64(pa, c.a_type, a.D);
    } else {
        const char *pb = c.b + (uint64_t)m * c.b_stride;
        if (c.op == LH_OP_DIFF && is_int(c.a_type) && is_int(c.b_type)) {
            x = (double)(load_int(pa, c.a_type) - load_int(pb, c.b_type)); // uint64, wrapping
        } else {
            const double fa = load_f64(pa, c.a_type, a.D), fb = load_f64(pb, c.b_type, a.D);
            if (c.op == LH_OP_DIFF) x = fa - fb;
            else if (c.op == LH_OP_RATIO) x = fa / fb;                     // an IEEE divide (-fno-fast-math)
            else x = __dsqrt_rn(fa / fb);                                  // correctly rounded
        }
    }
    *v = x;
    return !((a.flags & F_SKIP_NAN) && x != x);
}

__device__ __forceinline__ void line_of(const LinesArgs &a, uint64_t L, uint32_t *m, uint32_t *j)
{
    *m = (uint32_t)(L / a.ncols);
    *j = (uint32_t)(L - (uint64_t)*m * a.ncols);
}

// ---- pass 1: line lengths and per-workgroup totals ----------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_lines_len(const LinesArgs a, uint32_t *__restrict__ lens, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t s_w[lh::fmt::WAVES];
    const uint64_t L = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t nlines = (uint64_t)a.n * a.ncols;
    uint32_t len = 0;
    if (L < nlines) {
        uint32_t m, j, id;
        line_of(a, L, &m, &j);
        if (entry_name(a, m, &id)) {
            const DevCol &c = a.cols[j];
            double v;
            if (line_value(a, c, m, &v))
                len = a.prefix_len + c.pre_len + (a.name_off[id + 1] - a.name_off[id]) + c.post_len + a.sep_len + a.suffix_len +
                      lh::fmt::fmt_f<false>(v, nullptr);
        }
        lens[L] = len;
    }
    uint32_t total;
    (void)lh::fmt::block_excl_scan(len, s_w, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// ---- pass 2: exclusive scan of the workgroup totals; boff[nblocks] = *d_len = all bytes --------------------------------
__global__ __launch_bounds__(1024) void k_lines_scan(const uint32_t *__restrict__ bsum, uint64_t *__restrict__ boff, uint32_t nblocks,
                                                     uint64_t *__restrict__ d_len)
{
    __shared__ uint64_t s_w[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nblocks ? bsum[i] : 0;
        const uint64_t inc = wave_scan_incl_u64(v);
        __syncthreads();
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint64_t wb = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            if (w < (int)wave) wb += s_w[w];
            tot += s_w[w];
        }
        if (i < nblocks) boff[i] = carry + wb + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        boff[nblocks] = carry;
        if (d_len) *d_len = carry;
    }
}

// ---- pass 3: the text ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_lines_write(const LinesArgs a, const uint32_t *__restrict__ lens,
                                                       const uint64_t *__restrict__ boff, uint32_t nblocks, char *__restrict__ out,
                                                       uint64_t cap)
{
    __shared__ __attribute__((aligned(16))) char s_stage[STAGE_LDS + 16];
    __shared__ char s_blob[BLOB_MAX];
    __shared__ uint32_t s_w[lh::fmt::WAVES];
    using lh::fmt::put_bytes;

    if (boff[nblocks] > cap) return; // uniform over the grid: the text does not fit, nothing is written

    for (uint32_t i = threadIdx.x; i < a.blob_len; i += BLOCK) s_blob[i] = a.blob[i];

    const uint64_t L = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint64_t nlines = (uint64_t)a.n * a.ncols;
    const uint32_t len = L < nlines ? lens[L] : 0;
    uint32_t total;
    const uint32_t excl = lh::fmt::block_excl_scan(len, s_w, &total); // also orders the s_blob fill before its use
    const uint64_t base = boff[blockIdx.x];
    const uint32_t phase = (uint32_t)(((uintptr_t)out + base) & 15u); // the same 16-byte phase in LDS and in the output
    const bool staged = total + phase <= STAGE_LDS;
    if (len) {
        uint32_t m, j, id;
        line_of(a, L, &m, &j);
        (void)entry_name(a, m, &id);
        const DevCol &c = a.cols[j];
        char *p = staged ? s_stage + phase + excl : out + base + excl;
        p = put_bytes(p, s_blob + a.prefix_off, a.prefix_len);
        p = put_bytes(p, s_blob + c.pre_off, c.pre_len);
        const uint32_t n0 = a.name_off[id], n1 = a.name_off[id + 1];
        if (a.flags & F_DOTS) { // strings.Replace(metric, "_", ".", -1), graphite.go:42 (the label's text: on the host)
            for (uint32_t i = n0; i < n1; i++) {
                const char ch = a.names[i];
                *p++ = ch == '_' ? '.' : ch;
            }
        } else {
            p = put_bytes(p, a.names + n0, n1 - n0);
        }
        p = put_bytes(p, s_blob + c.post_off, c.post_len);
        p = put_bytes(p, s_blob + a.sep_off, a.sep_len);
        double v = 0;
        (void)line_value(a, c, m, &v);
        p += lh::fmt::fmt_f<true>(v, p);
        (void)put_bytes(p, s_blob + a.suffix_off, a.suffix_len);
    }
    if (!staged) return; // uniform: the lines went straight to HBM
    __syncthreads();
    const char *src = s_stage + phase;
    char *dst = out + base;
    const uint32_t head = total < ((16u - phase) & 15u) ? total : ((16u - phase) & 15u);
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t nvec = (total - head) >> 4;
    const uint4 *vs = reinterpret_cast<const uint4 *>(src + head);
    uint4 *vd = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t i = threadIdx.x; i < nvec; i += BLOCK) vd[i] = vs[i];
    const uint32_t done = head + (nvec << 4);
    if (threadIdx.x < total - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

// ---- host side: the argument checks (no handle, no device) --------------------------------------------------------------
// label = pre "%s" post with "%%" -> '%'; exactly one %s (lh_serialize's rule)
bool split_label(const char *label, std::string *pre, std::string *post)
{
    int seen = 0;
    std::string *cur = pre;
    for (const char *c = label; *c; c++) {
        if (c[0] == '%' && c[1] == 's') {
            if (seen++) return false;
            cur = post;
            c++;
        } else if (c[0] == '%' && c[1] == '%') {
            *cur += '%';
            c++;
        } else if (c[0] == '%') {
            return false;
        } else {
            *cur += *c;
        }
    }
    return seen == 1;
}

// a call's descriptors and blob as they travel to the device
struct Staged {
    std::vector<DevCol> cols;
    std::string blob;
    uint16_t prefix_off = 0, prefix_len = 0, sep_off = 0, sep_len = 0, suffix_off = 0, suffix_len = 0;
    bool keys = false; // a column is LH_COL_KEY: the call needs D[]
    void put(const std::string &s, bool is_key, bool dots, uint16_t *off, uint16_t *len)
    {
        *off = (uint16_t)blob.size();
        *len = (uint16_t)s.size();
        for (char ch : s) blob += (is_key && dots && ch == '_') ? '.' : ch;
    }
};

uintptr_t type_bytes(uint32_t type) { return type == LH_COL_U32 ? 4 : type == LH_COL_KEY ? 2 : 8; }

struct Rows {
    uint32_t first = 0;
    const uint32_t *d_ids = nullptr;
    uint64_t id_stride = 0;
    bool by_id = false;
};

// every cause of LH_EINVAL, then LH_ERANGE for n: decided before the handle is dereferenced or a device touched
int check_args(const lh_names *nm, const Rows &rows, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride,
               const lh_column *cols, size_t ncols, const lh_line_format *f, uint32_t flags, const void *len, uintptr_t len_align,
               Staged &st)
{
    if (!nm || !cols || !f || !len || misaligned(len, len_align) || ncols == 0 || ncols > LH_MAX_COLUMNS || (flags & ~(uint32_t)LH_LINES_SKIP_NAN)) return LH_EINVAL;
    if (!f->prefix || !f->sep || !f->suffix) return LH_EINVAL;
    if (rows.by_id && ((!rows.d_ids && n > 0) || misaligned(rows.d_ids, 4) || (rows.id_stride & 3))) return LH_EINVAL;
    if (misaligned(d_row_count, 8) || (row_count_stride & 7)) return LH_EINVAL;
    const bool dots = (f->flags & LH_FMT_UNDERSCORE_TO_DOT) != 0;
    size_t raw = std::strlen(f->prefix) + std::strlen(f->sep) + std::strlen(f->suffix);
    if (raw > BLOB_MAX) return LH_EINVAL;
    st.put(f->prefix, false, dots, &st.prefix_off, &st.prefix_len);
    st.put(f->sep, false, dots, &st.sep_off, &st.sep_len);
    st.put(f->suffix, false, dots, &st.suffix_off, &st.suffix_len);
    st.cols.resize(ncols);
    for (size_t j = 0; j < ncols; j++) {
        const lh_column &c = cols[j];
        if (!c.label || !c.a || c.reserved0 || c.reserved1) return LH_EINVAL;
        if (c.a_type > LH_COL_KEY || c.b_type > LH_COL_U32 || c.op > LH_OP_DIFF) return LH_EINVAL; // KEY is for `a` only ...
        if (c.a_type == LH_COL_KEY && c.op != LH_OP_VALUE) return LH_EINVAL;                       // ... under VALUE only
        if (misaligned(c.a, type_bytes(c.a_type)) || (c.a_stride & (type_bytes(c.a_type) - 1))) return LH_EINVAL;
        if (c.op != LH_OP_VALUE) {
            if (!c.b || misaligned(c.b, type_bytes(c.b_type)) || (c.b_stride & (type_bytes(c.b_type) - 1))) return LH_EINVAL;
        }
        raw += std::strlen(c.label);
        if (raw > BLOB_MAX) return LH_EINVAL;
        std::string pre, post;
        if (!split_label(c.label, &pre, &post)) return LH_EINVAL;
        DevCol &d = st.cols[j];
        d.a = static_cast<const char *>(c.a);
        d.b = c.op != LH_OP_VALUE ? static_cast<const char *>(c.b) : nullptr;
        d.valid = c.valid;
        d.a_stride = c.a_stride;
        d.b_stride = c.b_stride;
        d.valid_stride = c.valid_stride;
        d.a_type = c.a_type;
        d.b_type = c.b_type;
        d.op = c.op;
        d.pad0 = 0;
        d.pad1 = 0;
        st.put(pre, true, dots, &d.pre_off, &d.pre_len);
        st.put(post, true, dots, &d.post_off, &d.post_len);
        st.keys = st.keys || c.a_type == LH_COL_KEY;
    }
    if (n > 0xffffffffull) return LH_ERANGE;
    return LH_OK;
}

} // namespace

// ---- the handle ------------------------------------------------------------------------------------------------------
// `mu` is held for the length of a call (a host form's wait included).  The blocks only grow; `guard` is behind the last
// device-form call's work, which reads them -- and the name table -- after the call has returned.
struct lh_names {
    std::mutex mu;
    lh_engine *e = nullptr; // used by create and refresh only
    int device = -1;
    std::vector<char> h_bytes;    // the names held, back to back ...
    std::vector<uint32_t> h_off;  // ... and where each begins: held + 1 entries
    char *d_bytes = nullptr;
    uint32_t *d_off = nullptr;
    size_t d_bytes_cap = 0, d_off_cap = 0;
    uint32_t held = 0;
    double *d_table = nullptr;    // D[LH_NKEYS], on the first call with an LH_COL_KEY column
    unsigned char *h_call = nullptr, *d_call = nullptr; // the descriptors, then the blob (pinned; in HBM)
    size_t h_call_cap = 0, d_call_cap = 0;
    uint32_t *d_lens = nullptr, *d_bsum = nullptr;
    uint64_t *d_boff = nullptr;
    size_t lens_cap = 0, bsum_cap = 0, boff_cap = 0;
    char *d_text = nullptr;       // the host forms' text
    size_t text_cap = 0;
    uint64_t *h_total = nullptr;  // pinned
    EventGuard guard;
};

namespace {

// (nm->mu held, the device current) the names interned since, appended
int fetch_names(lh_names *nm)
{
    uint32_t have = 0;
    int rc = lh_num_metrics(nm->e, &have);
    if (rc) return rc;
    if (have <= nm->held && nm->d_off) return LH_OK;
    std::vector<char> bytes = nm->h_bytes;
    std::vector<uint32_t> off = nm->h_off;
    if (off.empty()) off.push_back(0);
    std::vector<char> buf(256);
    for (uint32_t id = nm->held; id < have; id++) {
        size_t len = 0;
        rc = lh_metric_name(nm->e, id, buf.data(), buf.size(), &len);
        if (!rc && len > buf.size()) {
            buf.resize(len);
            rc = lh_metric_name(nm->e, id, buf.data(), buf.size(), &len);
        }
        if (rc) return rc;
        if (len > NAME_LEN_MAX || bytes.size() + len > 0xffffffffull) return LH_ERANGE;
        bytes.insert(bytes.end(), buf.data(), buf.data() + len);
        off.push_back((uint32_t)bytes.size());
    }
    rc = nm->guard.host_wait(); // a device-form call may still read the table
    if (rc) return rc;
    const size_t old_bytes_cap = nm->d_bytes_cap, old_off_cap = nm->d_off_cap;
    rc = grow_device(nm->d_bytes, nm->d_bytes_cap, bytes.size() ? bytes.size() : 1, 65536);
    if (!rc) rc = grow_device(nm->d_off, nm->d_off_cap, off.size(), 1024);
    if (rc) { // a block that failed to grow is gone: the handle holds nothing until a refresh succeeds
        nm->held = 0;
        nm->h_bytes.clear();
        nm->h_off.clear();
        return rc;
    }
    // a block that moved takes everything, one that stayed the appended part
    const size_t b0 = nm->d_bytes_cap == old_bytes_cap ? nm->h_bytes.size() : 0;
    const size_t o0 = nm->d_off_cap == old_off_cap ? nm->h_off.size() : 0;
    if (bytes.size() > b0) LH_BESIDE_CHK(hipMemcpy(nm->d_bytes + b0, bytes.data() + b0, bytes.size() - b0, hipMemcpyHostToDevice));
    LH_BESIDE_CHK(hipMemcpy(nm->d_off + o0, off.data() + o0, (off.size() - o0) * sizeof(uint32_t), hipMemcpyHostToDevice));
    nm->h_bytes.swap(bytes);
    nm->h_off.swap(off);
    nm->held = have;
    return LH_OK;
}

// after a failure behind the first enqueue: the stream may still read the blocks
int settle(int rc, hipStream_t st)
{
    if (rc && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
    return rc;
}

// (nm->mu held, the device current, the guard waited for) the call's three passes on `st`; the write pass only with `out`
int enqueue_sizes(lh_names *nm, const Staged &sg, const Rows &rows, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride,
                  uint32_t flags, const lh_line_format *f, hipStream_t st, LinesArgs &a, uint32_t &nb, uint64_t *d_len)
{
    const size_t ncols = sg.cols.size(), desc_bytes = ncols * sizeof(DevCol), call_bytes = desc_bytes + sg.blob.size();
    const uint64_t nlines = (uint64_t)n * ncols;
    if (nlines > (uint64_t)0x7fffffff * BLOCK) return LH_ERANGE; // the grid
    nb = (uint32_t)((nlines + BLOCK - 1) / BLOCK);
    int rc = grow_pinned(nm->h_call, nm->h_call_cap, call_bytes, 16384);
    if (!rc) rc = grow_device(nm->d_call, nm->d_call_cap, call_bytes, 16384);
    if (!rc) rc = grow_device(nm->d_lens, nm->lens_cap, nlines, 65536);
    if (!rc) rc = grow_device(nm->d_bsum, nm->bsum_cap, nb, 1024);
    if (!rc) rc = grow_device(nm->d_boff, nm->boff_cap, (size_t)nb + 1, 1024);
    if (!rc && sg.keys) rc = ensure_table(nm->d_table, st, lh::k_value_table<lh_names>);
    if (rc) return rc;
    std::memcpy(nm->h_call, sg.cols.data(), desc_bytes);
    std::memcpy(nm->h_call + desc_bytes, sg.blob.data(), sg.blob.size());
    LH_BESIDE_CHK(hipMemcpyAsync(nm->d_call, nm->h_call, call_bytes, hipMemcpyHostToDevice, st));
    a.names = nm->d_bytes;
    a.name_off = nm->d_off;
    a.ids = reinterpret_cast<const char *>(rows.d_ids);
    a.row_count = reinterpret_cast<const char *>(d_row_count);
    a.cols = reinterpret_cast<const DevCol *>(nm->d_call);
    a.blob = reinterpret_cast<const char *>(nm->d_call + desc_bytes);
    a.D = sg.keys ? nm->d_table : nullptr;
    a.id_stride = rows.id_stride;
    a.row_count_stride = row_count_stride;
    a.held = nm->held;
    a.first = rows.first;
    a.n = (uint32_t)n;
    a.ncols = (uint32_t)ncols;
    a.blob_len = (uint32_t)sg.blob.size();
    a.flags = ((f->flags & LH_FMT_UNDERSCORE_TO_DOT) ? F_DOTS : 0u) | ((flags & LH_LINES_SKIP_NAN) ? F_SKIP_NAN : 0u) |
              (rows.by_id ? F_BY_ID : 0u);
    a.prefix_off = sg.prefix_off; a.prefix_len = sg.prefix_len;
    a.sep_off = sg.sep_off; a.sep_len = sg.sep_len;
    a.suffix_off = sg.suffix_off; a.suffix_len = sg.suffix_len;
    hipLaunchKernelGGL(k_lines_len, dim3(nb), dim3(BLOCK), 0, st, a, nm->d_lens, nm->d_bsum);
    hipLaunchKernelGGL(k_lines_scan, dim3(1), dim3(1024), 0, st, nm->d_bsum, nm->d_boff, nb, d_len);
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

int enqueue_write(lh_names *nm, const LinesArgs &a, uint32_t nb, hipStream_t st, char *d_out, size_t cap)
{
    hipLaunchKernelGGL(k_lines_write, dim3(nb), dim3(BLOCK), 0, st, a, nm->d_lens, nm->d_boff, nb, d_out, (uint64_t)cap);
    LH_BESIDE_CHK(hipGetLastError());
    return LH_OK;
}

// (nm->mu held) the device made current; LH_ERANGE for a block of names the handle does not hold
int open_call(lh_names *nm, const Rows &rows, size_t n)
{
    LH_BESIDE_CHK(hipSetDevice(nm->device));
    if (!rows.by_id && (n > nm->held || rows.first > nm->held - n)) return LH_ERANGE;
    return nm->guard.host_wait(); // an earlier device-form call may still read the blocks this one rewrites
}

int lines_host(lh_names *nm, const Rows &rows, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride, const lh_column *cols,
               size_t ncols, const lh_line_format *f, uint32_t flags, void *stream, char *out, size_t cap, size_t *len)
{
    Staged sg;
    int rc = check_args(nm, rows, n, d_row_count, row_count_stride, cols, ncols, f, flags, len, alignof(size_t), sg);
    if (rc) return rc;
    if (n == 0) {
        *len = 0;
        return LH_OK;
    }
    std::lock_guard<std::mutex> g(nm->mu);
    rc = open_call(nm, rows, n);
    if (rc) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    LinesArgs a;
    uint32_t nb = 0;
    rc = enqueue_sizes(nm, sg, rows, n, d_row_count, row_count_stride, flags, f, st, a, nb, nullptr);
    if (rc) return settle(rc, st);
    hipError_t e = hipMemcpyAsync(nm->h_total, nm->d_boff + nb, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return settle(LH_EDEVICE, st);
    }
    const uint64_t total = *nm->h_total;
    *len = (size_t)total;
    if (!out || total > cap || total == 0) return LH_OK;
    rc = grow_device(nm->d_text, nm->text_cap, (size_t)total, 1 << 20);
    if (!rc) rc = enqueue_write(nm, a, nb, st, nm->d_text, (size_t)total);
    if (rc) return settle(rc, st);
    e = hipMemcpyAsync(out, nm->d_text, (size_t)total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return settle(LH_EDEVICE, st);
    }
    return LH_OK;
}

int lines_device(lh_names *nm, const Rows &rows, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride, const lh_column *cols,
                 size_t ncols, const lh_line_format *f, uint32_t flags, void *stream, char *d_out, size_t cap, uint64_t *d_len)
{
    Staged sg;
    int rc = check_args(nm, rows, n, d_row_count, row_count_stride, cols, ncols, f, flags, d_len, 8, sg);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(nm->mu);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) { // (*d_len always receives the total: the one device call of an empty call)
        LH_BESIDE_CHK(hipSetDevice(nm->device));
        LH_BESIDE_CHK(hipMemsetAsync(d_len, 0, sizeof(uint64_t), st));
        return LH_OK;
    }
    rc = open_call(nm, rows, n);
    if (!rc) rc = nm->guard.create();
    if (rc) return rc;
    LinesArgs a;
    uint32_t nb = 0;
    rc = enqueue_sizes(nm, sg, rows, n, d_row_count, row_count_stride, flags, f, st, a, nb, d_len);
    if (!rc) rc = enqueue_write(nm, a, nb, st, d_out, d_out ? cap : 0); // (no d_out: cap 0, written only when nothing emits)
    if (!rc) rc = nm->guard.record(st);
    return settle(rc, st);
}

} // namespace

extern "C" {

int lh_names_create(lh_engine *e, int device, lh_names **out)
{
    if (!e || !out || device < 0 || device >= MAX_DEVICES) return LH_EINVAL;
    *out = nullptr;
    lh_names *nm = new (std::nothrow) lh_names;
    if (!nm) return LH_ENOMEM;
    nm->e = e;
    nm->device = device;
    int rc = LH_OK;
    {
        std::lock_guard<std::mutex> g(nm->mu);
        const hipError_t err = hipSetDevice(device);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            rc = LH_EDEVICE;
        }
        if (!rc && hipHostMalloc((void **)&nm->h_total, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            nm->h_total = nullptr;
            rc = LH_ENOMEM;
        }
        if (!rc) rc = fetch_names(nm);
    }
    if (rc) {
        (void)lh_names_destroy(nm);
        return rc;
    }
    *out = nm;
    return LH_OK;
}

int lh_names_refresh(lh_names *nm, uint32_t *count)
{
    if (!nm) return LH_EINVAL;
    std::lock_guard<std::mutex> g(nm->mu);
    LH_BESIDE_CHK(hipSetDevice(nm->device));
    const int rc = fetch_names(nm);
    if (count) *count = nm->held;
    return rc;
}

int lh_names_destroy(lh_names *nm)
{
    if (!nm) return LH_EINVAL;
    {
        std::lock_guard<std::mutex> g(nm->mu);
        if (hipSetDevice(nm->device) == hipSuccess) {
            (void)nm->guard.host_wait();
            void *dev[] = {nm->d_bytes, nm->d_off, nm->d_table, nm->d_call, nm->d_lens, nm->d_bsum, nm->d_boff, nm->d_text};
            for (void *p : dev)
                if (p) (void)hipFree(p);
            if (nm->h_call) (void)hipHostFree(nm->h_call);
            if (nm->h_total) (void)hipHostFree(nm->h_total);
            if (nm->guard.ev) (void)hipEventDestroy(nm->guard.ev);
        }
        (void)hipGetLastError();
    }
    delete nm;
    return LH_OK;
}

int lh_lines(lh_names *nm, uint32_t first, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride, const lh_column *cols,
             size_t ncols, const lh_line_format *fmt, uint32_t flags, void *stream, char *out, size_t cap, size_t *len)
{
    Rows rows;
    rows.first = first;
    return lines_host(nm, rows, n, d_row_count, row_count_stride, cols, ncols, fmt, flags, stream, out, cap, len);
}

int lh_lines_ids(lh_names *nm, const uint32_t *d_ids, uint64_t id_stride, size_t n, const uint64_t *d_row_count,
                 uint64_t row_count_stride, const lh_column *cols, size_t ncols, const lh_line_format *fmt, uint32_t flags, void *stream,
                 char *out, size_t cap, size_t *len)
{
    Rows rows;
    rows.d_ids = d_ids;
    rows.id_stride = id_stride;
    rows.by_id = true;
    return lines_host(nm, rows, n, d_row_count, row_count_stride, cols, ncols, fmt, flags, stream, out, cap, len);
}

int lh_lines_device(lh_names *nm, uint32_t first, size_t n, const uint64_t *d_row_count, uint64_t row_count_stride,
                    const lh_column *cols, size_t ncols, const lh_line_format *fmt, uint32_t flags, void *stream, char *d_out, size_t cap,
                    uint64_t *d_len)
{
    Rows rows;
    rows.first = first;
    return lines_device(nm, rows, n, d_row_count, row_count_stride, cols, ncols, fmt, flags, stream, d_out, cap, d_len);
}

int lh_lines_ids_device(lh_names *nm, const uint32_t *d_ids, uint64_t id_stride, size_t n, const uint64_t *d_row_count,
                        uint64_t row_count_stride, const lh_column *cols, size_t ncols, const lh_line_format *fmt, uint32_t flags,
                        void *stream, char *d_out, size_t cap, uint64_t *d_len)
{
    Rows rows;
    rows.d_ids = d_ids;
    rows.id_stride = id_stride;
    rows.by_id = true;
    return lines_device(nm, rows, n, d_row_count, row_count_stride, cols, ncols, fmt, flags, stream, d_out, cap, d_len);
}

} // extern "C"
