// vg_scan_valued.hip - value-range scans, single forms: the k nearest rows whose int64 value lies in [lo, hi] (vg_scan_topk_valued,
// vg_scan_topk_valued_labeled, vg_scan_topk_grouped_valued, vg_scan_topk_capped_valued, vg_scan_within_valued, include/vectorgpu.h).
//
// The label-set single scan (vg_scan_labelset.hip) with another predicate: vg_value_bits_kernel turns (values, lo, hi) - and, for the
// conjunction, (labels, label) - into the bitmap the labeled scans build for one label, in the same scratch buffer, d_label_bits, NOT
// the user's row mask, which is neither read nor written; the masked single kernels run with ScanArgs.mask pointing at it: no scan
// instances of its own.  The top-k forms run the masked table, the grouped and capped forms the masked grouped / capped tables, the
// range form the masked range kernels through vg_within_run - so what those tables leave out stays refused.  Also the fallback of the
// valued batch (vg_multi_valued.hip).
#include "vg_internal.h"

#include "vg_device.h"

// One wavefront covers 64 rows: every lane compares the value of its row with the closed interval (signed 64-bit), the wavefront
// ballots, and one lane stores the word (an ordinary vector store).  A row behind the last one reads row 0 and is not allowed: the
// bits behind n_rows stay clear.  use_label: the row must also carry `label`.
__global__ __launch_bounds__(256) void vg_value_bits_kernel(const int64_t *values, long long n_rows, long long lo, long long hi, int use_label,
                                                            const uint32_t *labels, uint32_t label, uint64_t *bits, long long n_words) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long w = wave; w < n_words; w += nwaves) {
        const long long row = w * VG_WAVE + lane;
        const long long at = row < n_rows ? row : 0;
        const long long v = values[at];
        bool hit = (row < n_rows) && v >= lo && v <= hi;
        if (use_label) hit = hit && labels[at] == label;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) bits[w] = m;
    }
}

int vg_value_bits_enqueue(vg_corpus *c, int64_t lo, int64_t hi, int use_label, uint32_t label) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (c->n_rows + 63) / 64;
    if (words == 0) return VG_OK;
    if (c->label_bits_cap_words < words) {
        if (c->d_label_bits) { hipFree(c->d_label_bits); c->d_label_bits = nullptr; c->label_bits_cap_words = 0; }
        HIP_TRY(hipMalloc(&c->d_label_bits, (size_t)words * sizeof(uint64_t)));
        c->label_bits_cap_words = words;
    }
    const long long blocks = std::min<long long>((words + 3) / 4, 4096);          // 4 wavefronts a workgroup, grid-stride beyond
    hipLaunchKernelGGL(vg_value_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (const int64_t *)c->d_values, (long long)c->n_rows,
                       (long long)lo, (long long)hi, use_label ? 1 : 0, (const uint32_t *)c->d_labels, label, c->d_label_bits, (long long)words);
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// ------------------------------------------------------------------------------------------------ the scans

// what allows a row: the interval, and - use_label - one label
struct ValueCond { int64_t lo, hi; int use_label; uint32_t label; };

// per_label < 0: the top-k forms; 0: grouped; >= 1: capped
static VgFusedForm valued_form(const char *who, int per_label, bool grouped) {
    if (per_label > 0) return VgFusedForm{who, vg_pick_scan_capped_masked, false, false, true, true, per_label, true, true};
    if (grouped) return VgFusedForm{who, vg_pick_scan_grouped_masked, false, false, true, true, 0, true, true};
    return VgFusedForm{who, vg_pick_scan_masked, false, false, true, false, 0, true, true};
}

// the checks the fused routine does not know, then the bitmap and the scan
static int valued_keys(vg_corpus *c, const VgFusedForm &form, int metric, const void *query, int k, const ValueCond &v, uint64_t *out_keys,
                       uint32_t *out_labels, int *out_count) {
    const char *who = form.who;
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", who);
    if (k > VG_WAVE_HOST) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (valued scans use the fused list only)", who, VG_WAVE_HOST);
    if (!out_keys || (form.grouped && !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (!c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", who);
    if ((v.use_label || form.grouped) && !c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", who);
    if (v.use_label && v.label == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", who);
    if (c->n_rows == 0 || v.lo > v.hi) return VG_OK;          // an empty interval allows no row: no launch
    int rc = vg_value_bits_enqueue(c, v.lo, v.hi, v.use_label, v.label);
    if (rc != VG_OK) return rc;
    return vg_fused_run(c, form, metric, query, k, 0ull, out_keys, out_count, out_labels);
}

static int valued_rows(vg_corpus *c, const VgFusedForm &form, int metric, const void *query, int k, const ValueCond &v, int64_t *out_rowids,
                       double *out_dist, uint32_t *out_labels, int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_HOST && (!out_rowids || !out_dist || (form.grouped && !out_labels))) return vg_fail(VG_ERR_INVALID, "%s: NULL output", form.who);
    uint64_t keys[VG_WAVE_HOST];
    uint32_t labs[VG_WAVE_HOST];
    int cnt = 0;
    int rc = valued_keys(c, form, metric, query, k, v, keys, labs, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, form.grouped ? labs : nullptr, 1, k, &cnt, out_rowids, out_dist, out_labels);
    *out_count = cnt;
    return VG_OK;
}

extern "C" int vg_scan_topk_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint64_t *out_keys,
                                        int *out_count) {
    return valued_keys(c, valued_form("vg_scan_topk_valued", -1, false), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, int64_t *out_rowids,
                                   double *out_dist, int *out_count) {
    return valued_rows(c, valued_form("vg_scan_topk_valued", -1, false), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued_labeled_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                                uint64_t *out_keys, int *out_count) {
    return valued_keys(c, valued_form("vg_scan_topk_valued_labeled", -1, false), metric, query, k, ValueCond{lo, hi, 1, label}, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_valued_labeled(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                           int64_t *out_rowids, double *out_dist, int *out_count) {
    return valued_rows(c, valued_form("vg_scan_topk_valued_labeled", -1, false), metric, query, k, ValueCond{lo, hi, 1, label}, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_grouped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint64_t *out_keys,
                                                uint32_t *out_labels, int *out_count) {
    return valued_keys(c, valued_form("vg_scan_topk_grouped_valued", 0, true), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, int64_t *out_rowids,
                                           double *out_dist, uint32_t *out_labels, int *out_count) {
    return valued_rows(c, valued_form("vg_scan_topk_grouped_valued", 0, true), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                               uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_valued: per_label must be at least 1");
    return valued_keys(c, valued_form("vg_scan_topk_capped_valued", per_label, true), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_valued(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_valued: per_label must be at least 1");
    return valued_rows(c, valued_form("vg_scan_topk_capped_valued", per_label, true), metric, query, k, ValueCond{lo, hi, 0, 0u}, out_rowids, out_dist, out_labels, out_count);
}

// what vg_within_run checks, in its order, in front of the checks only this form knows (vg_scan_within_labeled.hip does the same): a
// refusal or an answer without a launch must leave the handle as vg_within_run would
extern "C" int vg_scan_within_valued(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t lo, int64_t hi,
                                     int64_t *out_matches, int64_t *out_held) {
    const VgWithinForm form = {"vg_scan_within_valued", vg_pick_scan_within_masked, false, true, true};
    if (out_matches) *out_matches = 0;
    if (out_held) *out_held = 0;
    if (!c || !query) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    c->within_keys.clear();
    c->within_matches = 0;
    c->within_launches = 0;
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (radius != radius) return vg_fail(VG_ERR_INVALID, "%s: the radius is NaN", form.who);
    if (!c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", form.who);
    if (c->n_rows == 0 || lo > hi) return VG_OK;              // an empty interval allows no row: no launch
    int rc = vg_value_bits_enqueue(c, lo, hi, 0, 0u);
    if (rc != VG_OK) return rc;
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}
