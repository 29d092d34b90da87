// vg_scan_capped.hip - capped scans: the k nearest rows, at most m of one label (vg_scan_topk_capped, include/vectorgpu.h) - rows are
// chunks, the label is the document a chunk belongs to, the caller wants the 20 nearest chunks but no more than 3 of any document.
//
// Contract: take every row with a finite distance and a label other than VG_LABEL_NONE (masked form: whose mask bit is set), order
// them by the 64-bit scan key = (distance, scan position), walk that order and keep a row iff fewer than m rows of its label have been
// kept, return the first k rows kept.  m = 1 is the grouped contract (vg_scan_grouped.hip), m >= k with every row labeled the plain
// top-k.
//
// The kernels are the VG_SQ_GROUPED | VG_SQ_CAPPED instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h), without
// VG_SQ_MASKED and with it: the grouped scan's launch shape, loads, label prefetch and arithmetic; only the list routine differs
// (vg_list_offer_capped, vg_device.h: the label's worst kept row is replaced once m of its rows are kept).  The workgroup's 16
// lists (vg_block_publish_capped) and the per-workgroup lists in HBM (vg_merge_capped_kernel, below) merge through that same
// routine; lists stay keys-only in HBM, the final merge gathers labels[position], and one copy brings back k keys and k labels.
// A translation unit of their own, and a merge kernel of their own: every other kernel keeps its code.
//
// The host side is the grouped scan's (vg_scan_masked.hip: vg_fused_run with VgFusedForm.grouped and .per_label); this unit hands
// it its kernel tables and the merge, and holds the entry points and the host merge of several corpora's lists (vg_merge_keys_capped).
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// Not in the tables: the shapes the grouped tables leave out (f16 cosine / dot at 6 chunks per lane, rows of 2049 .. 3072 halves:
// vg_scan_grouped.hip) - the capped instances of those shapes spill like their grouped twins.  No other capped instance uses
// scratch (DESIGN.md 3.17 lists every instance against its twin).
static bool capped_shape_spills(int vtype, int acc, int U, bool long_rows) {
    return vtype == VG_TYPE_F16 && U == 6 && !long_rows && (acc == A_COS || acc == A_COSN || acc == A_DOT);
}
scan_fn_t vg_pick_scan_capped(int vtype, int acc, int U, bool long_rows) {
    if (capped_shape_spills(vtype, acc, U, long_rows)) return nullptr;
    return vg_pick_scan<ScanFamily<VG_SQ_GROUPED | VG_SQ_CAPPED, true, true>>(vtype, acc, U, long_rows);
}
scan_fn_t vg_pick_scan_capped_masked(int vtype, int acc, int U, bool long_rows) {
    if (capped_shape_spills(vtype, acc, U, long_rows)) return nullptr;
    return vg_pick_scan<ScanFamily<VG_SQ_GROUPED | VG_SQ_CAPPED | VG_SQ_MASKED, true, true>>(vtype, acc, U, long_rows);
}

// ------------------------------------------------------------------------------------------------ the final merge

// vg_merge_grouped_kernel (vg_scan_grouped.hip) with the cap: one workgroup of 16 wavefronts over nlists <= 256 sorted lists of 64
// keys, wavefront w takes lists w, w + 16, ... - all their keys first, then all their labels - offers them list by list to its own
// capped list, and the 16 lists merge through LDS like a scan workgroup's (vg_block_publish_capped).  out: 64 keys, then 64 labels.
// A kernel of its own, not a parameter of the grouped one: sharing a body moved that kernel's code.
// (vg_merge_capped_batch_kernel, vg_multi_capped.hip, is these statements behind a per-query offset: a change here belongs there too)
#define VG_CMERGE_PER_WAVE (VG_SEL_MAX_HEADS / VG_WAVES_PER_BLOCK)
__global__ __launch_bounds__(VG_BLOCK) void vg_merge_capped_kernel(const uint64_t *cand, int nlists, int k, int m, const uint32_t *labels, uint64_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[VG_WAVES_PER_BLOCK * VG_WAVE * 12];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    uint64_t keys[VG_CMERGE_PER_WAVE];
    uint32_t labs[VG_CMERGE_PER_WAVE];
#pragma unroll
    for (int i = 0; i < VG_CMERGE_PER_WAVE; ++i) {
        const int l = wave + i * VG_WAVES_PER_BLOCK;
        keys[i] = (l < nlists && lane < k) ? cand[(long long)l * VG_WAVE + lane] : VG_EMPTY_KEY;
    }
#pragma unroll
    for (int i = 0; i < VG_CMERGE_PER_WAVE; ++i) labs[i] = (keys[i] != VG_EMPTY_KEY) ? labels[(uint32_t)keys[i]] : 0xFFFFFFFFu;
    uint64_t mine = VG_EMPTY_KEY, thr = VG_EMPTY_KEY;
    uint32_t mlab = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < VG_CMERGE_PER_WAVE; ++i) vg_list_offer_capped(keys[i], labs[i], keys[i] != VG_EMPTY_KEY, mine, mlab, thr, lane, k, m);
    vg_block_publish_capped(smem, mine, mlab, k, m, VG_WAVES_PER_BLOCK, out, reinterpret_cast<uint32_t *>(out + VG_WAVE));
}

int vg_launch_merge_capped(const uint64_t *dev_cand, int nlists, int k, int per_label, const uint32_t *dev_labels, uint64_t *dev_out, hipStream_t stream) {
    if (nlists > VG_SEL_MAX_HEADS || per_label < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(vg_merge_capped_kernel, dim3(1), dim3(VG_BLOCK), 0, stream, dev_cand, nlists, k, per_label, dev_labels, dev_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the scans

static VgFusedForm capped_form(bool masked, int per_label) {
    if (masked) return vg_fused_form("vg_scan_topk_capped_masked", "capped", vg_pick_scan_capped_masked, VG_ROWS_MASK, vg_result_capped(per_label));
    return vg_fused_form("vg_scan_topk_capped", "capped", vg_pick_scan_capped, VG_ROWS_ALL, vg_result_capped(per_label));
}

static int capped_keys(vg_corpus *c, bool masked, int metric, const void *query, int k, int per_label, uint64_t *out_keys, uint32_t *out_labels,
                       int *out_count) {
    const VgFusedForm form = capped_form(masked, per_label);
    if (out_count) *out_count = 0;
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "%s: per_label must be at least 1", form.who);
    return vg_fused_run(c, form, metric, query, k, 0ull, out_keys, out_count, out_labels);
}

static int capped_rows(vg_corpus *c, bool masked, int metric, const void *query, int k, int per_label, int64_t *out_rowids, double *out_dist,
                       uint32_t *out_labels, int *out_count) {
    const char *who = capped_form(masked, per_label).who;
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k >= 1 && k <= VG_MAX_FUSED_K && per_label >= 1 && (!out_rowids || !out_dist || !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    uint64_t keys[VG_WAVE];
    uint32_t labels[VG_WAVE];
    int cnt = 0;
    int rc = capped_keys(c, masked, metric, query, k, per_label, keys, labels, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, labels, 1, k, &cnt, out_rowids, out_dist, out_labels);
    *out_count = cnt;
    return VG_OK;
}

extern "C" int vg_scan_topk_capped(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t *out_rowids, double *out_dist,
                                   uint32_t *out_labels, int *out_count) {
    return capped_rows(c, false, metric, query, k, per_label, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_masked(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t *out_rowids,
                                          double *out_dist, uint32_t *out_labels, int *out_count) {
    return capped_rows(c, true, metric, query, k, per_label, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, uint64_t *out_keys,
                                        uint32_t *out_labels, int *out_count) {
    return capped_keys(c, false, metric, query, k, per_label, out_keys, out_labels, out_count);
}
extern "C" int vg_scan_topk_capped_masked_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, uint64_t *out_keys,
                                               uint32_t *out_labels, int *out_count) {
    return capped_keys(c, true, metric, query, k, per_label, out_keys, out_labels, out_count);
}

// ------------------------------------------------------------------------------------------------ the host merge

// vg_merge_keys_grouped (vg_scan_grouped.hip) with the cap: one label can live in several lists (shards), so the lists' rows of a
// label compete - the four-step contract over the union of the lists, by (distance image, GLOBAL position = pos_offsets[list] +
// position).  Exact for lists that are capped top-k answers of their own rows.
extern "C" int vg_merge_keys_capped(const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets,
                                    int k, int per_label, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (!keys || !labels || !out_keys || !out_labels || !out_count) return vg_fail(VG_ERR_INVALID, "vg_merge_keys_capped: NULL argument");
    if (n_lists < 1 || list_len < 1 || k < 1 || per_label < 1)
        return vg_fail(VG_ERR_INVALID, "vg_merge_keys_capped: n_lists, list_len, k and per_label must be at least 1");
    return vg_merge_keys_by_label("vg_merge_keys_capped", keys, labels, n_lists, list_len, pos_offsets, k, per_label, out_keys, out_labels, out_count);
}
