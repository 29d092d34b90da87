// vg_scan_labelset.hip - label-set scans, single forms: the k nearest rows whose label is in a SET of labels - or, with `exclude`, is
// a label and NOT in it (vg_scan_topk_labelset, vg_scan_topk_grouped_labelset, vg_scan_topk_capped_labelset, include/vectorgpu.h).
//
// The labeled single scan (vg_scan_labeled.hip) with a set in place of one label: the host sorts and de-duplicates the set and uploads
// it into a scratch buffer the handle owns (d_lset), vg_labelset_bits_kernel turns (labels, set, exclude) into the bitmap the labeled
// scan builds for one label - in the same scratch buffer, d_label_bits, NOT the user's row mask, which is neither read nor written -
// and the masked single kernels run with ScanArgs.mask pointing at it: no scan instances of its own.  The top-k form runs the masked
// table (VgFusedForm.labeled), the grouped and capped forms the masked grouped / capped tables (.labeled with .grouped / .per_label),
// so what those tables leave out stays refused.  Also the fallback of the label-set batch (vg_multi_labelset.hip).
#include "vg_internal.h"

#include "vg_device.h"

// One wavefront covers 64 rows: every lane binary-searches the label of its row in the sorted set, the wavefront ballots, and one lane
// stores the word (an ordinary vector store).  A row behind the last one, and a row without a label, is allowed in neither mode: the
// bits behind n_rows stay clear.  An empty set: nothing is found - no row allowed, or with `exclude` every labeled row.
__global__ __launch_bounds__(256) void vg_labelset_bits_kernel(const uint32_t *labels, long long n_rows, const uint32_t *set, int n_set,
                                                               int exclude, uint64_t *bits, long long n_words) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long w = wave; w < n_words; w += nwaves) {
        const long long row = w * VG_WAVE + lane;
        const uint32_t lab = labels[row < n_rows ? row : 0];
        int lo = 0, hi = n_set;                                  // the first element >= lab
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (set[mid] < lab) lo = mid + 1; else hi = mid;
        }
        const bool found = lo < n_set && set[lo] == lab;
        const bool hit = (row < n_rows) && (lab != VG_LABEL_NONE) && (found != (exclude != 0));
        const unsigned long long m = __ballot(hit);
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

bool vg_labelset_normalise(const char *who, const uint32_t *labels, int64_t n, std::vector<uint32_t> *out) {
    out->clear();
    if (n < 0 || (n > 0 && !labels)) { vg_fail(VG_ERR_INVALID, "%s: bad label-set pointer / count", who); return false; }
    out->assign(labels, labels + n);
    std::sort(out->begin(), out->end());
    out->erase(std::unique(out->begin(), out->end()), out->end());
    if (!out->empty() && out->back() == VG_LABEL_NONE) { vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", who); return false; }
    return true;
}

int vg_labelset_bits_enqueue(vg_corpus *c, const uint32_t *sorted, int64_t n, int exclude) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (c->n_rows + 63) / 64;
    if (words == 0) return VG_OK;
    if (n > 0x7FFFFFFFll) return vg_fail(VG_ERR_UNSUPPORTED, "a label set of more than 2^31 - 1 labels");
    if (c->label_bits_cap_words < words) {
        if (c->d_label_bits) { hipFree(c->d_label_bits); c->d_label_bits = nullptr; c->label_bits_cap_words = 0; }
        HIP_TRY(hipMalloc(&c->d_label_bits, (size_t)words * sizeof(uint64_t)));
        c->label_bits_cap_words = words;
    }
    int rc = vg_lset_reserve(c, (size_t)n * sizeof(uint32_t));
    if (rc != VG_OK) return rc;
    if (n > 0) {
        // (the upload's source is the handle's: it does not move before the scan behind this call has waited for the stream)
        if (sorted != c->lset_host.data()) c->lset_host.assign(sorted, sorted + n);
        HIP_TRY(hipMemcpyAsync(c->d_lset, c->lset_host.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    const long long blocks = std::min<long long>((words + 3) / 4, 4096);          // 4 wavefronts a workgroup, grid-stride beyond
    hipLaunchKernelGGL(vg_labelset_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->d_labels, (long long)c->n_rows,
                       (const uint32_t *)c->d_lset, (int)n, exclude ? 1 : 0, c->d_label_bits, (long long)words);
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// ------------------------------------------------------------------------------------------------ the scans

// per_label < 0: the top-k form; 0: grouped; >= 1: capped
static VgFusedForm labelset_form(int per_label, bool grouped) {
    if (per_label > 0) return VgFusedForm{"vg_scan_topk_capped_labelset", vg_pick_scan_capped_masked, false, false, true, true, per_label, true};
    if (grouped) return VgFusedForm{"vg_scan_topk_grouped_labelset", vg_pick_scan_grouped_masked, false, false, true, true, 0, true};
    return VgFusedForm{"vg_scan_topk_labelset", vg_pick_scan_masked, false, false, true, false, 0, true};
}

// the checks the fused routine does not know, then the bitmap and the scan
static int labelset_keys(vg_corpus *c, const VgFusedForm &form, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                         int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    const char *who = form.who;
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", who);
    if (k > VG_WAVE_HOST) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (label-set scans use the fused list only)", who, VG_WAVE_HOST);
    if (!out_keys || (form.grouped && !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (!c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", who);
    std::vector<uint32_t> set;
    if (!vg_labelset_normalise(who, labels, n_labels, &set)) return VG_ERR_INVALID;
    if (c->n_rows == 0 || (set.empty() && !exclude)) return VG_OK;          // an empty set allows no row: no launch
    c->lset_host.swap(set);
    int rc = vg_labelset_bits_enqueue(c, c->lset_host.data(), (int64_t)c->lset_host.size(), exclude);
    if (rc != VG_OK) return rc;
    return vg_fused_run(c, form, metric, query, k, 0ull, out_keys, out_count, out_labels);
}

static int labelset_rows(vg_corpus *c, const VgFusedForm &form, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                         int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_HOST && (!out_rowids || !out_dist || (form.grouped && !out_labels))) return vg_fail(VG_ERR_INVALID, "%s: NULL output", form.who);
    uint64_t keys[VG_WAVE_HOST];
    uint32_t labs[VG_WAVE_HOST];
    int cnt = 0;
    int rc = labelset_keys(c, form, metric, query, k, labels, n_labels, exclude, keys, labs, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, form.grouped ? labs : nullptr, 1, k, &cnt, out_rowids, out_dist, out_labels);
    *out_count = cnt;
    return VG_OK;
}

extern "C" int vg_scan_topk_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                          int exclude, uint64_t *out_keys, int *out_count) {
    return labelset_keys(c, labelset_form(-1, false), metric, query, k, labels, n_labels, exclude, out_keys, nullptr, out_count);
}
extern "C" int vg_scan_topk_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                                     int64_t *out_rowids, double *out_dist, int *out_count) {
    return labelset_rows(c, labelset_form(-1, false), metric, query, k, labels, n_labels, exclude, out_rowids, out_dist, nullptr, out_count);
}
extern "C" int vg_scan_topk_grouped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                                  int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    return labelset_keys(c, labelset_form(0, true), metric, query, k, labels, n_labels, exclude, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                             int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count) {
    return labelset_rows(c, labelset_form(0, true), metric, query, k, labels, n_labels, exclude, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                                 int64_t n_labels, int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_labelset: per_label must be at least 1");
    return labelset_keys(c, labelset_form(per_label, true), metric, query, k, labels, n_labels, exclude, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_labelset(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                            int64_t n_labels, int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels,
                                            int *out_count) {
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_capped_labelset: per_label must be at least 1");
    return labelset_rows(c, labelset_form(per_label, true), metric, query, k, labels, n_labels, exclude, out_rowids, out_dist, out_labels, out_count);
}
