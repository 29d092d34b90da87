// vg_scan_grouped.hip - grouped scans: the k nearest LABELS, each represented by its best row (vg_scan_topk_grouped,
// include/vectorgpu.h) - rows are chunks, the label is the document a chunk belongs to, the caller wants the k nearest documents.
//
// Contract: take every row with a finite distance and a label other than VG_LABEL_NONE (masked form: whose mask bit is set), order
// them by the 64-bit scan key = (distance, scan position), keep the first row of each label, return the first k rows kept.
//
// The kernels are the VG_SQ_GROUPED instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h), without VG_SQ_MASKED (all rows)
// and with it (the rows the handle's mask allows): the plain / the masked scan's launch shape, loads and arithmetic, plus one dword
// per row - the label, riding with the batch prefetch - and a candidate list that stays distinct by label (vg_list_offer_grouped,
// vg_device.h).  The workgroup's 16 lists and the per-workgroup lists in HBM merge through that same routine: a rank-select over
// keys would return two rows of one label.  Lists stay keys-only in HBM; the final merge (vg_merge_grouped_kernel, below) gathers a
// key's label as labels[position], runs on the corpus stream, and one device-to-host copy brings back k keys and k labels.
// A translation unit of their own: every other kernel keeps its code and its register budget.
//
// The host side is the masked scan's (vg_scan_masked.hip: vg_fused_run with VgFusedForm.grouped); this unit hands it its kernel
// tables and the merge, and holds the entry points and the host merge of several corpora's lists (vg_merge_keys_grouped).
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// Not in the tables: f16 cosine (either accumulation) and dot at 6 chunks per lane - rows of 2049 .. 3072 halves, the only rows the
// planner gives that shape.  These instances do not fit 128 VGPRs (neither do their plain twins): their spills sit in the Inf / NaN
// path, and the reload behind it puts a vmcnt(0) - the whole prefetch - in front of every batch's offer.  A grouped scan keeps the
// plain scan's shape so that its floats are scan_distances' (the long-row kernel has no cached-norm cosine), so such a scan is
// VG_ERR_UNSUPPORTED ("no kernel for this type / metric"), not slow.
static bool grouped_shape_spills(int vtype, int acc, int U, bool long_rows) {
    return vtype == VG_TYPE_F16 && U == 6 && !long_rows && (acc == A_COS || acc == A_COSN || acc == A_DOT);
}
scan_fn_t vg_pick_scan_grouped(int vtype, int acc, int U, bool long_rows) {
    if (grouped_shape_spills(vtype, acc, U, long_rows)) return nullptr;
    return vg_pick_scan<ScanFamily<VG_SQ_GROUPED, true, true>>(vtype, acc, U, long_rows);
}
scan_fn_t vg_pick_scan_grouped_masked(int vtype, int acc, int U, bool long_rows) {
    if (grouped_shape_spills(vtype, acc, U, long_rows)) return nullptr;
    return vg_pick_scan<ScanFamily<VG_SQ_GROUPED | VG_SQ_MASKED, true, true>>(vtype, acc, U, long_rows);
}

// ------------------------------------------------------------------------------------------------ the final merge

// One workgroup of 16 wavefronts over nlists <= 256 sorted lists of 64 keys: wavefront w takes lists w, w + 16, ... - all their keys
// first, then all their labels (two memory round trips per wavefront, not two per list), offered list by list to its own grouped
// list - and the 16 lists merge through LDS like a scan workgroup's (vg_block_publish_grouped).  out: 64 keys, then 64 labels.
// (vg_merge_grouped_batch_kernel, vg_multi_grouped.hip, is these statements behind a per-query offset: a change here belongs there too)
#define VG_GMERGE_PER_WAVE (VG_SEL_MAX_HEADS / VG_WAVES_PER_BLOCK)
__global__ __launch_bounds__(VG_BLOCK) void vg_merge_grouped_kernel(const uint64_t *cand, int nlists, int k, const uint32_t *labels, uint64_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[VG_WAVES_PER_BLOCK * VG_WAVE * 12];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    uint64_t keys[VG_GMERGE_PER_WAVE];
    uint32_t labs[VG_GMERGE_PER_WAVE];
#pragma unroll
    for (int i = 0; i < VG_GMERGE_PER_WAVE; ++i) {
        const int l = wave + i * VG_WAVES_PER_BLOCK;
        keys[i] = (l < nlists && lane < k) ? cand[(long long)l * VG_WAVE + lane] : VG_EMPTY_KEY;
    }
#pragma unroll
    for (int i = 0; i < VG_GMERGE_PER_WAVE; ++i) labs[i] = (keys[i] != VG_EMPTY_KEY) ? labels[(uint32_t)keys[i]] : 0xFFFFFFFFu;
    uint64_t mine = VG_EMPTY_KEY, thr = VG_EMPTY_KEY;
    uint32_t mlab = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < VG_GMERGE_PER_WAVE; ++i) vg_list_offer_grouped(keys[i], labs[i], keys[i] != VG_EMPTY_KEY, mine, mlab, thr, lane, k);
    vg_block_publish_grouped(smem, mine, mlab, k, VG_WAVES_PER_BLOCK, out, reinterpret_cast<uint32_t *>(out + VG_WAVE));
}

int vg_launch_merge_grouped(const uint64_t *dev_cand, int nlists, int k, const uint32_t *dev_labels, uint64_t *dev_out, hipStream_t stream) {
    if (nlists > VG_SEL_MAX_HEADS) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(vg_merge_grouped_kernel, dim3(1), dim3(VG_BLOCK), 0, stream, dev_cand, nlists, k, dev_labels, dev_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the scans

static VgFusedForm grouped_form(bool masked) {
    if (masked) return vg_fused_form("vg_scan_topk_grouped_masked", "grouped", vg_pick_scan_grouped_masked, VG_ROWS_MASK, vg_result_grouped());
    return vg_fused_form("vg_scan_topk_grouped", "grouped", vg_pick_scan_grouped, VG_ROWS_ALL, vg_result_grouped());
}

static int grouped_rows(vg_corpus *c, bool masked, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                        uint32_t *out_labels, int *out_count) {
    const VgFusedForm form = grouped_form(masked);
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    *out_count = 0;
    if (k >= 1 && k <= VG_MAX_FUSED_K && (!out_rowids || !out_dist || !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", form.who);
    uint64_t keys[VG_WAVE];
    uint32_t labels[VG_WAVE];
    int cnt = 0;
    int rc = vg_fused_run(c, form, metric, query, k, 0ull, keys, &cnt, labels);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, labels, 1, k, &cnt, out_rowids, out_dist, out_labels);
    *out_count = cnt;
    return VG_OK;
}

extern "C" int vg_scan_topk_grouped(vg_corpus *c, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                    uint32_t *out_labels, int *out_count) {
    return grouped_rows(c, false, metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_masked(vg_corpus *c, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist,
                                           uint32_t *out_labels, int *out_count) {
    return grouped_rows(c, true, metric, query, k, out_rowids, out_dist, out_labels, out_count);
}
extern "C" int vg_scan_topk_grouped_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, uint32_t *out_labels,
                                         int *out_count) {
    return vg_fused_run(c, grouped_form(false), metric, query, k, 0ull, out_keys, out_count, out_labels);
}
extern "C" int vg_scan_topk_grouped_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys,
                                                uint32_t *out_labels, int *out_count) {
    return vg_fused_run(c, grouped_form(true), metric, query, k, 0ull, out_keys, out_count, out_labels);
}

// ------------------------------------------------------------------------------------------------ the host merge

// The core of vg_merge_keys_grouped (cap = 1) and vg_merge_keys_capped (vg_scan_capped.hip; cap = per_label), which check their own
// arguments: the labeled keys of all lists ordered by (distance image, GLOBAL position = pos_offsets[list] + position), the first k
// of them kept that find fewer than `cap` rows of their label kept.  `who`: the caller, named by the one refusal of its own.
int vg_merge_keys_by_label(const char *who, const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets,
                           int k, int cap, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    struct Ent { uint32_t img; int64_t gpos; uint32_t label; };
    std::vector<Ent> all;
    for (int l = 0; l < n_lists; ++l)
        for (int j = 0; j < list_len; ++j) {
            const uint64_t key = keys[(size_t)l * list_len + j];
            if (key == VG_KEY_EMPTY) break;                  // (a list is ascending and padded at its end)
            const uint32_t lab = labels[(size_t)l * list_len + j];
            if (lab == VG_LABEL_NONE) continue;
            const int64_t g = (pos_offsets ? pos_offsets[l] : 0) + (int64_t)vg_key_position(key);
            if (g < 0 || g > 0xFFFFFFFFll) return vg_fail(VG_ERR_UNSUPPORTED, "%s: a global position does not fit a key's 32 bits", who);
            all.push_back(Ent{(uint32_t)(key >> 32), g, lab});
        }
    std::sort(all.begin(), all.end(), [](const Ent &a, const Ent &b) { return a.img != b.img ? a.img < b.img : a.gpos < b.gpos; });
    std::vector<std::pair<uint32_t, int>> seen;              // (label, rows kept of it), sorted by label
    int cnt = 0;
    for (size_t i = 0; i < all.size() && cnt < k; ++i) {
        auto it = std::lower_bound(seen.begin(), seen.end(), std::make_pair(all[i].label, 0));
        if (it == seen.end() || it->first != all[i].label) it = seen.insert(it, std::make_pair(all[i].label, 0));
        if (it->second >= cap) continue;
        ++it->second;
        out_keys[cnt] = ((uint64_t)all[i].img << 32) | (uint64_t)all[i].gpos;
        out_labels[cnt] = all[i].label;
        ++cnt;
    }
    *out_count = cnt;
    return VG_OK;
}

// The label-deduping twin of vg_merge_keys: one label can live in several lists (shards), so the lists' first rows of a label
// compete - the three-step contract over the union of the lists.
extern "C" int vg_merge_keys_grouped(const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets,
                                     int k, uint64_t *out_keys, uint32_t *out_labels, int *out_count) {
    if (out_count) *out_count = 0;
    if (!keys || !labels || !out_keys || !out_labels || !out_count) return vg_fail(VG_ERR_INVALID, "vg_merge_keys_grouped: NULL argument");
    if (n_lists < 1 || list_len < 1 || k < 1) return vg_fail(VG_ERR_INVALID, "vg_merge_keys_grouped: n_lists, list_len and k must be at least 1");
    return vg_merge_keys_by_label("vg_merge_keys_grouped", keys, labels, n_lists, list_len, pos_offsets, k, 1, out_keys, out_labels, out_count);
}
