// vg_rowpred.hip - row predicates: the single and the range forms of the labeled, the label-set and the valued scans
// (vg_scan_topk_labeled, vg_scan_topk_*labelset, vg_scan_topk_*valued*, vg_scan_within_labeled / _labelset / _valued,
// include/vectorgpu.h).
//
// A predicate (VgRowPred, vg_internal.h) says which rows a query may see as a condition over the columns the handle holds: a uint32
// label per scan position (vg_corpus_set_labels), an int64 value per scan position (vg_corpus_set_values).  None of these scans has
// scan instances of its own: vg_pred_bits_kernel turns the condition into a bitmap in a scratch buffer the handle owns, d_label_bits -
// NOT the user's row mask, which is neither read nor written - and the masked kernels run with ScanArgs.mask pointing at it
// (VG_ROWS_BITMAP): the masked, masked grouped or masked capped table through vg_fused_run, the masked range kernels through
// vg_within_run, so what those tables leave out stays refused.  A scan is two launches on the corpus stream (a label set: its upload
// in front) and one wait; the bitmap pass reads 4 or 8 bytes per row, the scan then only the batches that hold an allowed row.  Also
// the fallback of the batches (vg_multi_labeled.hip, vg_multi_labelset.hip, vg_multi_valued.hip, vg_multi_within.hip).
#include "vg_internal.h"

#include "vg_device.h"

// ------------------------------------------------------------------------------------------------ the bitmap

// "does the row at `at` pass?", one functor per kind; `at` is always a row of the corpus
struct PredLabel {
    const uint32_t *labels; uint32_t label;          // (VG_LABEL_NONE is never asked for: the host refuses it)
    __device__ bool operator()(long long at) const { return labels[at] == label; }
};
struct PredLabelset {                                // a binary search in the sorted set; a row without a label passes in neither mode
    const uint32_t *labels; const uint32_t *set; int n_set; int exclude;
    __device__ bool operator()(long long at) const {
        const uint32_t lab = labels[at];
        int lo = 0, hi = n_set;                      // the first element >= lab
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (set[mid] < lab) lo = mid + 1; else hi = mid;
        }
        const bool found = lo < n_set && set[lo] == lab;
        return (lab != VG_LABEL_NONE) && (found != (exclude != 0));
    }
};
struct PredValue {                                   // the closed interval, signed 64-bit; use_label: the row must also carry `label`
    const int64_t *values; long long lo, hi; int use_label; const uint32_t *labels; uint32_t label;
    __device__ bool operator()(long long at) const {
        const long long v = values[at];
        bool hit = v >= lo && v <= hi;
        if (use_label) hit = hit && labels[at] == label;
        return hit;
    }
};

// One wavefront covers 64 rows: every lane asks the predicate about its row, the wavefront ballots, and one lane stores the word (an
// ordinary vector store).  A row behind the last one asks about row 0 and does not pass: the bits behind n_rows stay clear.
template <class Pred>
__global__ __launch_bounds__(256) void vg_pred_bits_kernel(Pred pred, long long n_rows, uint64_t *bits, long long n_words) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long w = wave; w < n_words; w += nwaves) {
        const long long row = w * VG_WAVE + lane;
        const bool pass = pred(row < n_rows ? row : 0);
        const unsigned long long m = __ballot((row < n_rows) && pass);
        if (lane == 0) bits[w] = m;
    }
}

int vg_lset_reserve(vg_corpus *c, size_t bytes) {
    if (c->lset_bytes >= bytes) return VG_OK;
    if (c->d_lset) { hipFree(c->d_lset); c->d_lset = nullptr; c->lset_bytes = 0; }
    const size_t want = std::max<size_t>(bytes, 4096);
    HIP_TRY(hipMalloc(&c->d_lset, want));
    c->lset_bytes = want;
    return VG_OK;
}

// a caller's set: a bad pointer / count, VG_LABEL_NONE in it (the message set in `who`'s name)
static bool labelset_ok(const char *who, const uint32_t *labels, int64_t n) {
    if (n < 0 || (n > 0 && !labels)) { vg_fail(VG_ERR_INVALID, "%s: bad label-set pointer / count", who); return false; }
    if (std::find(labels, labels + n, (uint32_t)VG_LABEL_NONE) != labels + n) { vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", who); return false; }
    return true;
}

static void sort_distinct(std::vector<uint32_t> *v) {
    std::sort(v->begin(), v->end());
    v->erase(std::unique(v->begin(), v->end()), v->end());
}

bool vg_labelset_normalise(const char *who, const uint32_t *labels, int64_t n, std::vector<uint32_t> *out) {
    out->clear();
    if (!labelset_ok(who, labels, n)) return false;
    out->assign(labels, labels + n);
    sort_distinct(out);
    return true;
}

int vg_pred_refusal(const vg_corpus *c, const char *who, const VgRowPred &pred, bool needs_labels_for_grouping) {
    if (pred.kind == VG_PRED_VALUE && !c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", who);
    const bool reads_labels = pred.kind != VG_PRED_VALUE || pred.use_label;
    if ((reads_labels || needs_labels_for_grouping) && !c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", who);
    if (pred.kind == VG_PRED_LABELSET) return labelset_ok(who, pred.set, pred.n_set) ? VG_OK : VG_ERR_INVALID;
    if (pred.use_label && pred.label == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", who);
    return VG_OK;
}

bool vg_pred_allows_nothing(const VgRowPred &pred) {
    if (pred.kind == VG_PRED_VALUE) return pred.lo > pred.hi;
    return pred.kind == VG_PRED_LABELSET && pred.n_set == 0 && !pred.exclude;
}

template <class Pred> static void launch_bits(vg_corpus *c, const Pred &pred, int64_t words) {
    const long long blocks = std::min<long long>((words + 3) / 4, 4096);          // 4 wavefronts a workgroup, grid-stride beyond
    hipLaunchKernelGGL(vg_pred_bits_kernel<Pred>, dim3((unsigned)blocks), dim3(256), 0, c->stream, pred, (long long)c->n_rows, c->d_label_bits,
                       (long long)words);
}

int vg_pred_bits_enqueue(vg_corpus *c, const VgRowPred &pred) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (c->n_rows + 63) / 64;
    if (words == 0) return VG_OK;
    if (pred.kind == VG_PRED_LABELSET) {
        c->lset_host.assign(pred.set, pred.set + pred.n_set);
        sort_distinct(&c->lset_host);
        if (c->lset_host.size() > 0x7FFFFFFFull) return vg_fail(VG_ERR_UNSUPPORTED, "a label set of more than 2^31 - 1 labels");
    }
    if (c->label_bits_cap_words < words) {
        if (c->d_label_bits) { hipFree(c->d_label_bits); c->d_label_bits = nullptr; c->label_bits_cap_words = 0; }
        HIP_TRY(hipMalloc(&c->d_label_bits, (size_t)words * sizeof(uint64_t)));
        c->label_bits_cap_words = words;
    }
    if (pred.kind == VG_PRED_LABEL) {
        launch_bits(c, PredLabel{c->d_labels, pred.label}, words);
    } else if (pred.kind == VG_PRED_VALUE) {
        launch_bits(c, PredValue{c->d_values, (long long)pred.lo, (long long)pred.hi, pred.use_label ? 1 : 0, c->d_labels, pred.label}, words);
    } else {
        const size_t n = c->lset_host.size();
        int rc = vg_lset_reserve(c, n * sizeof(uint32_t));
        if (rc != VG_OK) return rc;
        // (the upload's source is the handle's: it does not move before the scan behind this call has waited for the stream)
        if (n > 0) HIP_TRY(hipMemcpyAsync(c->d_lset, c->lset_host.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        launch_bits(c, PredLabelset{c->d_labels, c->d_lset, (int)n, pred.exclude ? 1 : 0}, words);
    }
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// ------------------------------------------------------------------------------------------------ the host paths

VgFusedForm vg_pred_form(const char *who, const VgRowPred &pred, VgResult result) {
    vg_pick_scan_fn_t pick = result.kind == VG_RESULT_CAPPED    ? vg_pick_scan_capped_masked
                             : result.kind == VG_RESULT_GROUPED ? vg_pick_scan_grouped_masked
                                                                : vg_pick_scan_masked;
    VgFusedForm f = vg_fused_form(who, pred.noun, pick, VG_ROWS_BITMAP, result);
    f.needs_labels = f.needs_labels || pred.kind != VG_PRED_VALUE || pred.use_label;
    f.needs_values = pred.kind == VG_PRED_VALUE;
    return f;
}

int vg_pred_topk_keys(vg_corpus *c, const char *who, VgResult result, const VgRowPred &pred, int metric, const void *query, int k,
                      uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", who);
    if (k > VG_WAVE_HOST) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (%s scans use the fused list only)", who, VG_WAVE_HOST, pred.noun);
    if (!out_keys || (result.with_labels() && !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    int rc = vg_pred_refusal(c, who, pred, result.with_labels());
    if (rc != VG_OK) return rc;
    if ((rc = vg_metric_check(c->vtype, metric, who)) != VG_OK) return rc;
    if (c->n_rows == 0 || vg_pred_allows_nothing(pred)) return VG_OK;          // no row can be returned: no launch
    if ((rc = vg_pred_bits_enqueue(c, pred)) != VG_OK) return rc;
    return vg_fused_run(c, vg_pred_form(who, pred, result), metric, query, k, 0ull, out_keys, out_count, out_labels);
}

int vg_pred_topk_rows(vg_corpus *c, const char *who, VgResult result, const VgRowPred &pred, int metric, const void *query, int k,
                      int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_HOST && (!out_rowids || !out_dist || (result.with_labels() && !out_labels))) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    uint64_t keys[VG_WAVE_HOST];
    uint32_t labs[VG_WAVE_HOST];
    int cnt = 0;
    int rc = vg_pred_topk_keys(c, who, result, pred, metric, query, k, keys, labs, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, result.with_labels() ? labs : nullptr, 1, k, &cnt, out_rowids, out_dist, out_labels);
    *out_count = cnt;
    return VG_OK;
}

int vg_pred_within(vg_corpus *c, const char *who, const VgRowPred &pred, int metric, const void *query, double radius, int64_t limit,
                   int64_t *out_matches, int64_t *out_held) {
    int rc = vg_within_begin(c, who, metric, query, radius, out_matches, out_held);
    if (rc != VG_OK) return rc;
    if ((rc = vg_pred_refusal(c, who, pred, false)) != VG_OK) return rc;
    if ((rc = vg_metric_check(c->vtype, metric, who)) != VG_OK) return rc;
    if (c->n_rows == 0 || vg_pred_allows_nothing(pred)) return VG_OK;          // no row can match: no launch
    if ((rc = vg_pred_bits_enqueue(c, pred)) != VG_OK) return rc;
    VgWithinForm form = vg_within_form(who, vg_pick_scan_within_masked, VG_ROWS_BITMAP);
    form.needs_labels = pred.kind != VG_PRED_VALUE || pred.use_label;
    form.needs_values = pred.kind == VG_PRED_VALUE;
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}

// ------------------------------------------------------------------------------------------------ the entry points

extern "C" int vg_scan_topk_labeled_keys(vg_corpus *c, int metric, const void *query, int k, uint32_t label, uint64_t *out_keys,
                                         int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_labeled", vg_result_plain(), vg_pred_label(label), metric, query, k, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_labeled(vg_corpus *c, int metric, const void *query, int k, uint32_t label, int64_t *out_rowids,
                                    double *out_dist, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_labeled", vg_result_plain(), vg_pred_label(label), metric, query, k, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_within_labeled(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, uint32_t label,
                                      int64_t *out_matches, int64_t *out_held) {
    return vg_pred_within(c, "vg_scan_within_labeled", vg_pred_label(label), metric, query, radius, limit, out_matches, out_held);
}

extern "C" int vg_scan_topk_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                          int exclude, uint64_t *out_keys, int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_labelset", vg_result_plain(), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                                     int64_t *out_rowids, double *out_dist, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_labelset", vg_result_plain(), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_grouped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                                  int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_grouped_labelset", vg_result_grouped(), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                             int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_grouped_labelset", vg_result_grouped(), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                                 int64_t n_labels, int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_labelset: per_label must be at least 1");
    return vg_pred_topk_keys(c, "vg_scan_topk_capped_labelset", vg_result_capped(per_label), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_labelset(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                            int64_t n_labels, int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels,
                                            int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_labelset: per_label must be at least 1");
    return vg_pred_topk_rows(c, "vg_scan_topk_capped_labelset", vg_result_capped(per_label), vg_pred_labelset(labels, n_labels, exclude), metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_within_labelset(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, const uint32_t *labels,
                                       int64_t n_labels, int exclude, int64_t *out_matches, int64_t *out_held) {
    return vg_pred_within(c, "vg_scan_within_labelset", vg_pred_labelset(labels, n_labels, exclude), metric, query, radius, limit, out_matches, out_held);
}

extern "C" int vg_scan_topk_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint64_t *out_keys,
                                        int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_valued", vg_result_plain(), vg_pred_value(lo, hi), metric, query, k, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, int64_t *out_rowids,
                                   double *out_dist, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_valued", vg_result_plain(), vg_pred_value(lo, hi), metric, query, k, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued_labeled_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                                uint64_t *out_keys, int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_valued_labeled", vg_result_plain(), vg_pred_value_labeled(lo, hi, label), metric, query, k, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued_labeled(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                           int64_t *out_rowids, double *out_dist, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_valued_labeled", vg_result_plain(), vg_pred_value_labeled(lo, hi, label), metric, query, k, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_grouped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint64_t *out_keys,
                                                uint32_t *out_labels, int *out_count) {
    return vg_pred_topk_keys(c, "vg_scan_topk_grouped_valued", vg_result_grouped(), vg_pred_value(lo, hi), metric, query, k, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, int64_t *out_rowids,
                                           double *out_dist, uint32_t *out_labels, int *out_count) {
    return vg_pred_topk_rows(c, "vg_scan_topk_grouped_valued", vg_result_grouped(), vg_pred_value(lo, hi), metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                               uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_valued: per_label must be at least 1");
    return vg_pred_topk_keys(c, "vg_scan_topk_capped_valued", vg_result_capped(per_label), vg_pred_value(lo, hi), metric, query, k, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_valued(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_valued: per_label must be at least 1");
    return vg_pred_topk_rows(c, "vg_scan_topk_capped_valued", vg_result_capped(per_label), vg_pred_value(lo, hi), metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_within_valued(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t lo, int64_t hi,
                                     int64_t *out_matches, int64_t *out_held) {
    return vg_pred_within(c, "vg_scan_within_valued", vg_pred_value(lo, hi), metric, query, radius, limit, out_matches, out_held);
}
