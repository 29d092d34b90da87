// vg_scan_masked.hip - masked scans: the k nearest rows among an allowed set (vg_scan_topk_masked, include/vectorgpu.h).
//
// The row mask is a bitmap over scan positions on the corpus handle (bit p & 63 of word p >> 6 = the row at position p may be returned;
// bits behind the last row are zero), set once and read by any number of masked scans.  The kernels are the VG_SQ_MASKED
// instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h; ScanFamily, vg_pick.h): the plain top-k scan's launch shape, loads, arithmetic, candidate
// lists and merge - plus one scalar load of mask bits per batch, fetched one step ahead of the row prefetch, so that a batch without an
// allowed row reads no rows and a row whose bit is clear is never offered to a list.  A translation unit of their own, like
// vg_scan_ex.hip and vg_scan_within.hip: the plain kernels keep their register budget.  One load policy (non-temporal).
//
// Only the masked scans read the mask: vg_scan_topk_masked here, vg_scan_topk_batch_masked in vg_multi_masked.hip, and the masked range
// scans (vg_scan_within_masked.hip, vg_multi_within.hip).  Order: ascending (distance, scan position) whatever the handle's tie_order.
// Also the home of vg_fused_run / launch_fused, the form-driven single-query routine the paged scans (vg_scan_after.hip) share with
// the masked scan: it serves every VgFusedForm, masked or not.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// ------------------------------------------------------------------------------------------------ the mask on the handle

// mask_host (ceil(n_rows / 64) words, tail bits clear) -> d_mask; the scan that follows runs on the same stream
int vg_mask_upload(vg_corpus *c) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (int64_t)c->mask_host.size();
    if (words == 0) return VG_OK;
    if (c->mask_cap_words < words) {
        if (c->d_mask) { hipFree(c->d_mask); c->d_mask = nullptr; c->mask_cap_words = 0; }
        HIP_TRY(hipMalloc(&c->d_mask, (size_t)words * sizeof(uint64_t)));
        c->mask_cap_words = words;
    }
    HIP_TRY(hipMemcpyAsync(c->d_mask, c->mask_host.data(), (size_t)words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                // (the host words may change right behind this call)
    return VG_OK;
}

// the handle's mask becomes `words` (already sized and tail-cleared); a failed upload leaves no mask
static int install_mask(vg_corpus *c, std::vector<uint64_t> &words) {
    int64_t count = 0;
    for (uint64_t w : words) count += __builtin_popcountll(w);
    c->mask_host.swap(words);
    c->mask_count = count;
    int rc = vg_mask_upload(c);
    if (rc != VG_OK) vg_drop_mask(c);
    return rc;
}

extern "C" int vg_corpus_set_mask_bits(vg_corpus *c, const uint64_t *words, int64_t n_bits) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    if (n_bits < 0 || (n_bits > 0 && !words)) return vg_fail(VG_ERR_INVALID, "vg_corpus_set_mask_bits: bad words pointer / bit count");
    if (n_bits > c->n_rows) return vg_fail(VG_ERR_INVALID, "vg_corpus_set_mask_bits: %lld bits for %lld rows", (long long)n_bits, (long long)c->n_rows);
    std::vector<uint64_t> w((size_t)((c->n_rows + 63) / 64), 0ull);
    const int64_t full = n_bits / 64;
    if (full > 0) memcpy(w.data(), words, (size_t)full * sizeof(uint64_t));
    if (n_bits % 64) w[(size_t)full] = words[full] & ((1ull << (n_bits % 64)) - 1ull);      // bits behind n_bits: zero
    return install_mask(c, w);
}

extern "C" int vg_corpus_set_mask_rowids(vg_corpus *c, const int64_t *rowids, int64_t n, int64_t *out_set) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    if (out_set) *out_set = 0;
    if (n < 0 || (n > 0 && !rowids)) return vg_fail(VG_ERR_INVALID, "vg_corpus_set_mask_rowids: bad rowids pointer / count");
    if (!c->rowids.empty() && !c->rowids_ascending)
        return vg_fail(VG_ERR_UNSUPPORTED, "vg_corpus_set_mask_rowids: the corpus' rowids are not ascending (no rowid lookup); set the mask by scan position");
    std::vector<uint64_t> w((size_t)((c->n_rows + 63) / 64), 0ull);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t p = vg_corpus_find_rowid(c, rowids[i]);              // (rowids not held are ignored, duplicates set a set bit)
        if (p >= 0) w[(size_t)(p >> 6)] |= 1ull << (p & 63);
    }
    int rc = install_mask(c, w);
    if (rc == VG_OK && out_set) *out_set = c->mask_count;
    return rc;
}

extern "C" int vg_corpus_clear_mask(vg_corpus *c) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    vg_drop_mask(c);
    return VG_OK;
}

extern "C" int64_t vg_corpus_mask_count(const vg_corpus *c) { return c ? c->mask_count : -1; }

// ------------------------------------------------------------------------------------------------ the scan

// One routine for every fused top-k variant that differs from the masked scan only in its kernel table and a ScanArgs field (3.11 of
// DESIGN.md): VgFusedForm names the table, where ScanArgs.mask comes from (the user's mask, then required, or a row predicate's
// bitmap), whether ScanArgs.floor is set (the paged scans of vg_scan_after.hip; the floor key travels in the 8 bytes behind the query,
// one upload) and the result: grouped (vg_scan_grouped.hip: ScanArgs.labels, the label-deduping merge, labels in the result) or capped
// (vg_scan_capped.hip: the grouped path with the cap in ScanArgs.within_cap, which no top-k kernel reads, and the capped merge).
// the form's kernel + the plain scan's merge; the k winners land in the pinned c->h_keys (copied behind the merge)
static int launch_fused(vg_corpus *c, const VgFusedForm &f, int metric, int k) {
    int acc = vg_metric_to_acc(metric);
    VgShape s;
    vg_plain_scan_shape(c, metric, &s);
    int rc = vg_half_cosine_acc(c, s, &acc);                 // the plain scan's cached-norm cosine: the same floats
    if (rc != VG_OK) return rc;
    scan_fn_t fn = f.pick(c->vtype, acc, s.U, s.long_rows);
    if (!fn) return vg_fail(VG_ERR_UNSUPPORTED, "%s: no kernel for this type / metric", f.who);

    const long long blocks = vg_plain_scan_blocks(c, c->n_rows, s);      // the launch shape of the plain top-k scan
    ScanArgs a = vg_scan_args(c, metric, acc, s, c->d_query, k);
    a.cand = c->d_cand;
    const bool grouped = f.result.with_labels();
    if (f.rows == VG_ROWS_MASK) a.mask = c->d_mask;
    if (f.rows == VG_ROWS_BITMAP) a.mask = c->d_label_bits;  // (a row predicate's bitmap, built on this stream in front of the scan)
    if (f.after) a.floor = reinterpret_cast<const uint64_t *>(c->d_query + c->stride);
    if (grouped) a.labels = c->d_labels;
    const int cap = f.result.kind == VG_RESULT_CAPPED ? std::min(f.result.per_label, k) : 0;   // (more than k of one label cannot be returned)
    if (cap > 0) a.within_cap = (unsigned long long)cap;
    const size_t smem = std::max<size_t>(vg_query_lds_bytes(c, s), (size_t)VG_PUBLISH_LDS_BYTES);

    hipEvent_t *evs = vg_prof_slot(c, VG_EVF_MERGE);
    if (evs) hipEventRecord(evs[0], c->stream);
    if ((rc = vg_launch_scan_kernel(fn, blocks, smem, c->stream, a)) != VG_OK) return rc;
    if (evs) hipEventRecord(evs[2], c->stream);
    int rcm = cap > 0   ? vg_launch_merge_capped(c->d_cand, (int)blocks, k, cap, c->d_labels, c->d_keys, c->stream)
              : grouped ? vg_launch_merge_grouped(c->d_cand, (int)blocks, k, c->d_labels, c->d_keys, c->stream)
                        : vg_launch_merge_one(c->d_cand, (int)blocks, k, c->d_keys, c->stream);
    if (evs) hipEventRecord(evs[3], c->stream);
    if (rcm != 0) return vg_fail(VG_ERR_HIP, "%s: merge launch failed: %s", f.who, hipGetErrorString((hipError_t)rcm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_keys, c->d_keys, grouped ? VG_KEYS_BYTES : VG_WAVE * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VG_OK;
}

// packed keys (distance image << 32 | position local to this corpus), ascending: the form a multi-shard caller merges.  `floor`: the
// smallest key admitted (read by an after form only)
int vg_fused_run(vg_corpus *c, const VgFusedForm &f, int metric, const void *query, int k, uint64_t floor, uint64_t *out_keys, int *out_count,
                 uint32_t *out_labels) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", f.who);
    *out_count = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", f.who);
    if (k > VG_MAX_FUSED_K) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (%s scans use the fused list only)", f.who, VG_MAX_FUSED_K, f.noun);
    if (!out_keys || (f.result.with_labels() && !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", f.who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (f.rows == VG_ROWS_MASK && c->mask_count < 0) return vg_fail(VG_ERR_INVALID, "%s: no row mask set", f.who);
    if (f.needs_values && !c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", f.who);
    if (f.needs_labels && !c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", f.who);
    if (int rcm = vg_metric_check(c->vtype, metric, f.who)) return rcm;
    if ((f.rows == VG_ROWS_MASK && c->mask_count == 0) || c->n_rows == 0) return VG_OK;      // an empty mask: no launch
    if (f.after && floor == VG_EMPTY_KEY) return VG_OK;      // nothing is behind the cursor: no launch
    HIP_TRY(hipSetDevice(c->device));
    c->enqueued = false;                                    // (the pinned key buffer is this scan's landing zone now)
    memset(c->h_query, 0, (size_t)c->stride);
    memcpy(c->h_query, query, (size_t)c->dim * c->es);
    if (f.after) memcpy(c->h_query + c->stride, &floor, sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(c->d_query, c->h_query, (size_t)c->stride + (f.after ? sizeof(uint64_t) : 0), hipMemcpyHostToDevice, c->stream));
    int rc = launch_fused(c, f, metric, k);
    if (rc != VG_OK) return rc;
    vg_collect_timing(c);
    int cnt = 0;
    const uint32_t *h_labels = reinterpret_cast<const uint32_t *>(c->h_keys + VG_WAVE);      // (grouped forms: the labels behind the keys)
    while (cnt < k && c->h_keys[cnt] != VG_EMPTY_KEY) {
        out_keys[cnt] = c->h_keys[cnt];
        if (f.result.with_labels()) out_labels[cnt] = h_labels[cnt];
        ++cnt;
    }
    *out_count = cnt;
    return VG_OK;
}

// the masked kernel table as a plain function: the fallback of the masked batch (vg_multi_masked.hip) names it in its form
scan_fn_t vg_pick_scan_masked(int vtype, int acc, int U, bool long_rows) { return vg_pick_scan<ScanFamily<VG_SQ_MASKED, true, true>>(vtype, acc, U, long_rows); }

extern "C" int vg_scan_topk_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, int *out_count) {
    const VgFusedForm form = vg_fused_form("vg_scan_topk_masked", "masked", vg_pick_scan_masked, VG_ROWS_MASK);
    return vg_fused_run(c, form, metric, query, k, 0ull, out_keys, out_count);
}

extern "C" int vg_scan_topk_masked(vg_corpus *c, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                   int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_masked: NULL argument");
    *out_count = 0;
    if (k >= 1 && k <= VG_MAX_FUSED_K && (!out_rowids || !out_dist)) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_masked: NULL output");
    uint64_t keys[VG_WAVE];
    int cnt = 0;
    int rc = vg_scan_topk_masked_keys(c, metric, query, k, keys, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, nullptr, 1, k, &cnt, out_rowids, out_dist, nullptr);
    *out_count = cnt;
    return VG_OK;
}

void vg_keys_to_rows(const vg_corpus *c, const uint64_t *keys, const uint32_t *labels, int nq, int k, const int *counts, int64_t *out_rowids,
                     double *out_dist, uint32_t *out_labels) {
    for (int i = 0; i < nq; ++i)
        for (int j = 0; j < counts[i]; ++j) {
            const size_t at = (size_t)i * k + j;
            out_dist[at] = (double)vg_key_distance(keys[at]);
            out_rowids[at] = vg_corpus_rowid_at(c, (int64_t)vg_key_position(keys[at]));
            if (labels) out_labels[at] = labels[at];
        }
}
