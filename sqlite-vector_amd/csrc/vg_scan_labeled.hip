// vg_scan_labeled.hip - labeled scans, single form: the k nearest rows that carry one label (vg_scan_topk_labeled, include/vectorgpu.h).
//
// The labels are a uint32 per scan position on the corpus handle (vg_corpus_set_labels, vg_corpus.hip).  A single labeled scan is two
// launches on the corpus stream and one wait: vg_label_bits_kernel turns (labels, label) into a bitmap in a scratch buffer the handle
// owns - NOT the user's row mask, which is neither read nor written - and the single masked kernels (vg_scan_masked.hip, long rows
// included) run with ScanArgs.mask pointing at it: no scan instances of its own.  The bitmap pass reads 4 bytes per row, the scan
// then only the batches that hold a row of the label.  Also the fallback of the labeled batch (vg_multi_labeled.hip).
#include "vg_internal.h"

#include "vg_device.h"

// One wavefront covers 64 rows: compare, ballot, and one lane stores the word (an ordinary vector store).  Rows behind the last one
// compare false, so the bits behind n_rows stay clear; VG_LABEL_NONE is never asked for (the host refuses it), so such rows match no one.
__global__ __launch_bounds__(256) void vg_label_bits_kernel(const uint32_t *labels, long long n_rows, uint32_t label, uint64_t *bits,
                                                            long long n_words) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long w = wave; w < n_words; w += nwaves) {
        const long long row = w * VG_WAVE + lane;
        const bool hit = (row < n_rows) && (labels[row < n_rows ? row : 0] == label);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) bits[w] = m;
    }
}

int vg_label_bits_enqueue(vg_corpus *c, uint32_t label) {
    HIP_TRY(hipSetDevice(c->device));
    const int64_t words = (c->n_rows + 63) / 64;
    if (words == 0) return VG_OK;
    if (c->label_bits_cap_words < words) {
        if (c->d_label_bits) { hipFree(c->d_label_bits); c->d_label_bits = nullptr; c->label_bits_cap_words = 0; }
        HIP_TRY(hipMalloc(&c->d_label_bits, (size_t)words * sizeof(uint64_t)));
        c->label_bits_cap_words = words;
    }
    const long long blocks = std::min<long long>((words + 3) / 4, 4096);          // 4 wavefronts a workgroup, grid-stride beyond
    hipLaunchKernelGGL(vg_label_bits_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, c->d_labels, (long long)c->n_rows, label,
                       c->d_label_bits, (long long)words);
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

static const VgFusedForm labeled_form = {"vg_scan_topk_labeled", vg_pick_scan_masked, false, false, true};

extern "C" int vg_scan_topk_labeled_keys(vg_corpus *c, int metric, const void *query, int k, uint32_t label, uint64_t *out_keys,
                                         int *out_count) {
    const char *who = labeled_form.who;
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", who);
    if (k > VG_WAVE_HOST) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (labeled scans use the fused list only)", who, VG_WAVE_HOST);
    if (!out_keys) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (!c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", who);
    if (label == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", who);
    if (c->n_rows == 0) return VG_OK;
    int rc = vg_label_bits_enqueue(c, label);
    if (rc != VG_OK) return rc;
    return vg_fused_run(c, labeled_form, metric, query, k, 0ull, out_keys, out_count);
}

extern "C" int vg_scan_topk_labeled(vg_corpus *c, int metric, const void *query, int k, uint32_t label, int64_t *out_rowids,
                                    double *out_dist, int *out_count) {
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_labeled: NULL argument");
    *out_count = 0;
    if (k >= 1 && k <= VG_WAVE_HOST && (!out_rowids || !out_dist)) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_labeled: NULL output");
    uint64_t keys[VG_WAVE_HOST];
    int cnt = 0;
    int rc = vg_scan_topk_labeled_keys(c, metric, query, k, label, keys, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, nullptr, 1, k, &cnt, out_rowids, out_dist, nullptr);
    *out_count = cnt;
    return VG_OK;
}
