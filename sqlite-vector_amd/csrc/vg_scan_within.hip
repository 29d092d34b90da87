// vg_scan_within.hip - range scans: every row within a distance of the query (vg_scan_within, include/vectorgpu.h).
//
// The kernels are the VG_SQ_WITHIN instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h; ScanFamily, vg_pick.h): the plain scan's loads,
// arithmetic and summation order with a fixed threshold in place of the converging k-th best - compare, ballot, and only for the rare
// batch with a match a key parked in the wavefront's LDS queue, flushed in bursts (vg_within_offer / vg_within_flush).  A translation
// unit of their own, like vg_scan_ex.hip: the plain kernels keep their register budget.  One load policy (non-temporal).
//
// Host side: [count | capacity keys] in device memory; the count keeps counting past the capacity, so ONE more launch into a buffer of
// the counted size answers an overflow - a partial answer is never returned.  The unsigned order of the keys is the contract order
// (distance, scan position): up to VG_WITHIN_HOST_SORT keys are sorted on the host behind the copy, more by a device radix sort
// (vg_select.hip) so that a `limit` below the match count brings only `limit` keys across the host link.
//
// The result path - radius rounding, the sort's buffers, "count keys on the device -> held, sorted, cut to limit", the readers of a held
// result - is here ONCE and serves the batch form (vg_multi_within.hip) too; each form keeps its own held result on the handle.
// So is the single scan itself (vg_within_run): the masked range scan (vg_scan_within_masked.hip) is this code with its own kernel
// table and ScanArgs.mask set, and leaves its result where vg_scan_within leaves its own; the labeled range scans
// (vg_rowpred.hip) are the masked one over a bitmap of their own making.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// ------------------------------------------------------------------------------------------------ the result path

extern "C" int vg_select_temp_bytes(long long n, size_t *bytes);                                                  // vg_select.hip
extern "C" int vg_select_sort_keys(const uint64_t *keys, long long n, uint64_t *keys_sorted, void *temp, size_t temp_bytes, hipStream_t stream);

// the largest float not above the radius: the device then compares floats and `d <= r` decides what (double)d <= radius decides
float vg_within_radius(double radius) {
    float r = (float)radius;
    if ((double)r > radius) r = std::nextafterf(r, -INFINITY);
    return r;
}

static int ensure_within_sort(vg_corpus *c, int64_t n) {
    if (c->within_sort_cap >= n) return VG_OK;
    if (c->d_within_sorted) hipFree(c->d_within_sorted);
    if (c->d_within_temp) hipFree(c->d_within_temp);
    c->d_within_sorted = nullptr; c->d_within_temp = nullptr; c->within_sort_cap = 0;
    if (vg_select_temp_bytes(n, &c->within_temp_bytes) != 0) return vg_fail(VG_ERR_HIP, "radix sort temp-size query failed");
    HIP_TRY(hipMalloc(&c->d_within_sorted, (size_t)n * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(&c->d_within_temp, c->within_temp_bytes ? c->within_temp_bytes : 16));
    c->within_sort_cap = n;
    return VG_OK;
}

int vg_within_collect(vg_corpus *c, const unsigned long long *dev_keys, int64_t count, int64_t limit, std::vector<uint64_t> *dst, bool *pending) {
    if (count <= 0) { dst->clear(); return VG_OK; }
    if (count <= VG_WITHIN_HOST_SORT) {
        dst->resize((size_t)count);
        HIP_TRY(hipMemcpyAsync(dst->data(), dev_keys, (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        *pending = true;
        return VG_OK;
    }
    const int64_t held = (limit > 0) ? std::min<int64_t>(limit, count) : count;
    int rc = ensure_within_sort(c, count);
    if (rc != VG_OK) return rc;
    if (vg_select_sort_keys(reinterpret_cast<const uint64_t *>(dev_keys), count, c->d_within_sorted, c->d_within_temp, c->within_temp_bytes, c->stream) != 0)
        return vg_fail(VG_ERR_HIP, "device key sort failed: %s", hipGetErrorString(hipGetLastError()));
    dst->resize((size_t)held);
    HIP_TRY(hipMemcpyAsync(dst->data(), c->d_within_sorted, (size_t)held * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                  // (the sort buffers serve the next result)
    return VG_OK;
}
void vg_within_finish(std::vector<uint64_t> *dst, int64_t count, int64_t limit) {
    if (count <= 0 || count > VG_WITHIN_HOST_SORT) return;
    std::sort(dst->begin(), dst->end());
    if (limit > 0 && limit < count) dst->resize((size_t)limit);
}

static bool held_range(const char *who, const std::vector<uint64_t> &held, int64_t first, int64_t n) {
    if (first >= 0 && first + n <= (int64_t)held.size()) return true;
    vg_fail(VG_ERR_INVALID, "%s: rows %lld..%lld of %lld held", who, (long long)first, (long long)(first + n), (long long)held.size());
    return false;
}
int vg_within_held_keys(const char *who, const std::vector<uint64_t> &held, int64_t first, int64_t n, uint64_t *out_keys) {
    if (n < 0) n = 0;
    if (!held_range(who, held, first, n)) return VG_ERR_INVALID;
    if (n > 0) memcpy(out_keys, held.data() + first, (size_t)n * sizeof(uint64_t));
    return VG_OK;
}
int vg_within_held_rows(const vg_corpus *c, const char *who, const std::vector<uint64_t> &held, int64_t first, int64_t n, int64_t *out_rowids,
                        double *out_dist) {
    if (n < 0) n = 0;
    if (!held_range(who, held, first, n)) return VG_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = held[(size_t)(first + i)];
        if (out_rowids) out_rowids[i] = vg_corpus_rowid_at(c, (int64_t)vg_key_position(key));
        if (out_dist) out_dist[i] = (double)vg_key_distance(key);
    }
    return VG_OK;
}

// ------------------------------------------------------------------------------------------------ the single range scan

// one launch of the form's within kernel into c->d_within ([count | cap keys]); the count lands in the pinned c->h_keys[0] behind it
static int launch_within(vg_corpus *c, const VgWithinForm &f, int metric, float r, int64_t cap) {
    int acc = vg_metric_to_acc(metric);
    VgShape s;
    vg_plain_scan_shape(c, metric, &s);
    int rc = vg_half_cosine_acc(c, s, &acc);                 // the plain scan's cached-norm cosine: the same floats
    if (rc != VG_OK) return rc;
    scan_fn_t fn = f.pick(c->vtype, acc, s.U, s.long_rows);
    if (!fn) return vg_fail(VG_ERR_UNSUPPORTED, "%s: no kernel for this type / metric", f.who);

    const long long blocks = vg_within_scan_blocks(c, c->n_rows, s);
    ScanArgs a = vg_scan_args(c, metric, acc, s, c->d_query, 0);
    a.emit = c->d_within;
    a.within_r = r;
    a.within_cap = (unsigned long long)cap;
    if (f.rows == VG_ROWS_MASK) a.mask = c->d_mask;
    if (f.rows == VG_ROWS_BITMAP) a.mask = c->d_label_bits;  // (a row predicate's bitmap, built on this stream in front of the scan)
    a.store_lds_off = (int)((vg_query_lds_bytes(c, s) + 255) / 256 * 256);     // the wavefronts' key queues behind the query
    const size_t smem = (size_t)a.store_lds_off + VG_WITHIN_LDS_BYTES;

    HIP_TRY(hipMemsetAsync(c->d_within, 0, sizeof(unsigned long long), c->stream));
    hipEvent_t *evs = vg_prof_slot(c, 0);
    if (evs) hipEventRecord(evs[0], c->stream);
    if ((rc = vg_launch_scan_kernel(fn, blocks, smem, c->stream, a)) != VG_OK) return rc;
    if (evs) { hipEventRecord(evs[2], c->stream); hipEventRecord(evs[3], c->stream); }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_keys, c->d_within, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->within_launches;
    return VG_OK;
}

static int ensure_within_buffer(vg_corpus *c, int64_t cap) {
    if (c->within_cap >= cap) return VG_OK;
    if (c->d_within) { hipFree(c->d_within); c->d_within = nullptr; c->within_cap = 0; }
    HIP_TRY(hipMalloc(&c->d_within, ((size_t)cap + 1) * sizeof(unsigned long long)));
    c->within_cap = cap;
    return VG_OK;
}

int vg_within_begin(vg_corpus *c, const char *who, int metric, const void *query, double radius, int64_t *out_matches, int64_t *out_held) {
    if (out_matches) *out_matches = 0;
    if (out_held) *out_held = 0;
    if (!c || !query) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    c->within_keys.clear();
    c->within_matches = 0;
    c->within_launches = 0;
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (radius != radius) return vg_fail(VG_ERR_INVALID, "%s: the radius is NaN", who);
    return VG_OK;
}

// a single range scan of any form (VgWithinForm, vg_internal.h): argument checks, launch, the overflow protocol, the held result
int vg_within_run(vg_corpus *c, const VgWithinForm &f, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                  int64_t *out_held) {
    int rcb = vg_within_begin(c, f.who, metric, query, radius, out_matches, out_held);
    if (rcb != VG_OK) return rcb;
    if (f.rows == VG_ROWS_MASK && c->mask_count < 0) return vg_fail(VG_ERR_INVALID, "%s: no row mask set", f.who);
    if (f.needs_values && !c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", f.who);
    if (f.needs_labels && !c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", f.who);
    if (int rcm = vg_metric_check(c->vtype, metric, f.who)) return rcm;
    if (c->n_rows == 0 || (f.rows == VG_ROWS_MASK && c->mask_count == 0)) return VG_OK;      // nothing can match: no launch
    HIP_TRY(hipSetDevice(c->device));
    c->enqueued = false;                                     // (the pinned key buffer is this scan's landing zone now)
    const float r = vg_within_radius(radius);
    int64_t cap = c->within_cap_init > 0 ? c->within_cap_init : (int64_t)VG_WITHIN_INITIAL_CAP;
    cap = std::max<int64_t>(std::min<int64_t>(cap, c->n_rows), c->within_cap);      // (a buffer an earlier scan grew is kept)
    int rc = ensure_within_buffer(c, cap);
    if (rc != VG_OK) return rc;
    memset(c->h_query, 0, (size_t)c->stride);
    memcpy(c->h_query, query, (size_t)c->dim * c->es);
    HIP_TRY(hipMemcpyAsync(c->d_query, c->h_query, (size_t)c->stride, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_within(c, f, metric, r, cap)) != VG_OK) return rc;
    int64_t count = (int64_t)c->h_keys[0];
    if (count > cap) {                                       // overflow: the count IS the size needed - grow, launch once more
        cap = count;
        if ((rc = ensure_within_buffer(c, cap)) != VG_OK) return rc;
        if ((rc = launch_within(c, f, metric, r, cap)) != VG_OK) return rc;
        if ((int64_t)c->h_keys[0] != count) return vg_fail(VG_ERR_HIP, "%s: two launches counted %lld and %lld rows", f.who, (long long)count, (long long)c->h_keys[0]);
    }
    vg_collect_timing(c);
    bool pending = false;
    if ((rc = vg_within_collect(c, c->d_within + 1, count, limit, &c->within_keys, &pending)) != VG_OK) return rc;
    if (pending) HIP_TRY(hipStreamSynchronize(c->stream));
    vg_within_finish(&c->within_keys, count, limit);
    c->within_matches = count;
    if (out_matches) *out_matches = count;
    if (out_held) *out_held = (int64_t)c->within_keys.size();
    return VG_OK;
}

extern "C" int vg_scan_within(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                              int64_t *out_held) {
    const VgWithinForm form = vg_within_form("vg_scan_within", vg_pick_scan<ScanFamily<VG_SQ_WITHIN, true, true>>, VG_ROWS_ALL);
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}

extern "C" int vg_scan_within_keys(const vg_corpus *c, int64_t first, int64_t n, uint64_t *out_keys) {
    if (!c || (n > 0 && !out_keys)) return vg_fail(VG_ERR_INVALID, "vg_scan_within_keys: NULL argument");
    if (n <= 0) return VG_OK;
    return vg_within_held_keys("vg_scan_within_keys", c->within_keys, first, n, out_keys);
}

extern "C" int vg_scan_within_fetch(const vg_corpus *c, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist) {
    if (!c) return vg_fail(VG_ERR_INVALID, "vg_scan_within_fetch: NULL argument");
    if (n <= 0) return VG_OK;
    return vg_within_held_rows(c, "vg_scan_within_fetch", c->within_keys, first, n, out_rowids, out_dist);
}

extern "C" int vg_within_set_initial_capacity(vg_corpus *c, int64_t keys) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    c->within_cap_init = keys > 0 ? keys : 0;
    if (c->d_within) { hipSetDevice(c->device); hipFree(c->d_within); c->d_within = nullptr; c->within_cap = 0; }   // (the next scan starts from that size)
    return VG_OK;
}

extern "C" int vg_within_last_launches(const vg_corpus *c) { return c ? c->within_launches : 0; }
