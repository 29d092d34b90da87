// vg_multi_capped.hip - capped batch scans: the k nearest ROWS, at most m of one label, for each of many queries
// (vg_scan_topk_batch_capped, include/vectorgpu.h) - "the 20 nearest chunks, no more than 3 of any document, for these 64 requests".
//
// Host side of the capped form of the multi-query scan (vg_scan_multi.h, VG_MQ_GROUPED | VG_MQ_CAPPED) and the home of its unmasked
// kernel instances (f32 / uint8 / int8 x L2 / cosine / dot / L1 x U in {1, 2, 3} at 4 queries per pass, {4, 6} at 2); the masked
// family compiles next to it in vg_multi_capped_masked.hip.  The batch itself is vg_fused_batch_run (vg_multi_masked.hip) with a
// capped result: the grouped batch's slices, back-to-back passes, one copy of keys and labels and one wait,
// with the cap in ScanArgs.within_cap and the capped merge per query (vg_merge_capped_batch_kernel, below).  Query i gets what the
// single capped scan (vg_scan_capped.hip) is contracted to return for it; one cap serves the whole batch.  Shapes without a
// multi-query form (f16 / bf16, long rows, an instance left out of a table): one single capped scan per query - a shape that scan
// refuses (f16 cosine / dot over rows of 2049 .. 3072 halves) is refused here too.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// (every unmasked instance compiles without scratch and without spills; the masked table leaves some out: vg_multi_capped_masked.hip.
//  A shape whose instance is nullptr goes to the fallback and vg_batch_capped_plan reports 0 for it)
static scan_fn_t pick_multi_capped(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_GROUPED | VG_MQ_CAPPED>>(vtype, acc, U, NQ); }
static scan_fn_t pick_multi_capped_masked(int vtype, int acc, int U, int NQ) { return vg_pick_multi_capped_masked(vtype, acc, U, NQ); }

// ------------------------------------------------------------------------------------------------ the final merge, batch launch

// vg_merge_grouped_batch_kernel (vg_multi_grouped.hip) with the cap: workgroup n merges query n's nlists <= 256 lists - cand is
// [NQ][nlists][64] keys - through vg_list_offer_capped / vg_block_publish_capped and writes 64 keys, then 64 labels, at its own
// offset (VG_KEYS_BYTES per query).  A kernel of its own, not a parameter of the grouped one: sharing a body moved the existing
// kernels' code.
// Bodies to keep in step: a change to the statements below belongs in vg_merge_grouped_batch_kernel and in vg_merge_capped_kernel
// (vg_scan_capped.hip) too, and the other way round.
#define VG_CMERGE_BATCH_PER_WAVE (VG_SEL_MAX_HEADS / VG_WAVES_PER_BLOCK)
__global__ __launch_bounds__(VG_BLOCK) void vg_merge_capped_batch_kernel(const uint64_t *cand, int nlists, int k, int m, const uint32_t *labels, uint64_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[VG_WAVES_PER_BLOCK * VG_WAVE * 12];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    cand += (long long)blockIdx.x * nlists * VG_WAVE;
    out += (long long)blockIdx.x * (VG_KEYS_BYTES / sizeof(uint64_t));
    uint64_t keys[VG_CMERGE_BATCH_PER_WAVE];
    uint32_t labs[VG_CMERGE_BATCH_PER_WAVE];
#pragma unroll
    for (int i = 0; i < VG_CMERGE_BATCH_PER_WAVE; ++i) {
        const int l = wave + i * VG_WAVES_PER_BLOCK;
        keys[i] = (l < nlists && lane < k) ? cand[(long long)l * VG_WAVE + lane] : VG_EMPTY_KEY;
    }
#pragma unroll
    for (int i = 0; i < VG_CMERGE_BATCH_PER_WAVE; ++i) labs[i] = (keys[i] != VG_EMPTY_KEY) ? labels[(uint32_t)keys[i]] : 0xFFFFFFFFu;
    uint64_t mine = VG_EMPTY_KEY, thr = VG_EMPTY_KEY;
    uint32_t mlab = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < VG_CMERGE_BATCH_PER_WAVE; ++i) vg_list_offer_capped(keys[i], labs[i], keys[i] != VG_EMPTY_KEY, mine, mlab, thr, lane, k, m);
    vg_block_publish_capped(smem, mine, mlab, k, m, VG_WAVES_PER_BLOCK, out, reinterpret_cast<uint32_t *>(out + VG_WAVE));
}

int vg_launch_merge_capped_batch(const uint64_t *dev_cand, int nlists, int k, int per_label, const uint32_t *dev_labels, uint64_t *dev_out, int nq,
                                 hipStream_t stream) {
    if (nlists > VG_SEL_MAX_HEADS || nq < 1 || per_label < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(vg_merge_capped_batch_kernel, dim3(nq), dim3(VG_BLOCK), 0, stream, dev_cand, nlists, k, per_label, dev_labels, dev_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the scans

static VgFusedBatchForm capped_batch_form(bool masked, int per_label) {
    if (masked) return VgFusedBatchForm{"vg_scan_topk_batch_capped_masked", pick_multi_capped_masked, VG_QROWS_MASK,
                                        vg_fused_form("vg_scan_topk_capped_masked", "capped", vg_pick_scan_capped_masked, VG_ROWS_MASK, vg_result_capped(per_label))};
    return VgFusedBatchForm{"vg_scan_topk_batch_capped", pick_multi_capped, VG_QROWS_ALL,
                            vg_fused_form("vg_scan_topk_capped", "capped", vg_pick_scan_capped, VG_ROWS_ALL, vg_result_capped(per_label))};
}

extern "C" int vg_batch_capped_plan(const vg_corpus *c, int metric, int masked, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, masked ? pick_multi_capped_masked : pick_multi_capped, out_queries_per_pass, out_lpr, out_u);
}

// (the order of the answers: NULL arguments and nq, then - with the counts zeroed - k, per_label, the outputs, the handle)
static int capped_batch_keys(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, int per_label, uint64_t *out_keys,
                             uint32_t *out_labels, int *out_counts) {
    const VgFusedBatchForm form = capped_batch_form(masked, per_label);
    if (!c || !queries || !out_counts) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", form.who);
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", form.who);
    if (per_label < 1) return vg_fail(VG_ERR_INVALID, "%s: per_label must be at least 1", form.who);
    return vg_fused_batch_run(c, form, metric, queries, nq, k, nullptr, out_keys, out_counts, nullptr, out_labels);
}

static int capped_batch_rows(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, int per_label, int64_t *out_rowids,
                             double *out_dist, uint32_t *out_labels, int *out_counts) {
    return vg_batch_rows_from_keys(c, capped_batch_form(masked, per_label).who, !c || !queries || !out_counts, nq, k,
                                   k >= 1 && k <= VG_MAX_FUSED_K && per_label >= 1, true, out_rowids, out_dist, out_labels, out_counts,
                                   [&](uint64_t *keys, uint32_t *labels) {
        return capped_batch_keys(c, masked, metric, queries, nq, k, per_label, keys, labels, out_counts);
    });
}

extern "C" int vg_scan_topk_batch_capped(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label, int64_t *out_rowids,
                                         double *out_dist, uint32_t *out_labels, int *out_counts) {
    return capped_batch_rows(c, false, metric, queries, nq, k, per_label, out_rowids, out_dist, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_capped_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label, int64_t *out_rowids,
                                                double *out_dist, uint32_t *out_labels, int *out_counts) {
    return capped_batch_rows(c, true, metric, queries, nq, k, per_label, out_rowids, out_dist, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_capped_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label, uint64_t *out_keys,
                                              uint32_t *out_labels, int *out_counts) {
    return capped_batch_keys(c, false, metric, queries, nq, k, per_label, out_keys, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_capped_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label, uint64_t *out_keys,
                                                     uint32_t *out_labels, int *out_counts) {
    return capped_batch_keys(c, true, metric, queries, nq, k, per_label, out_keys, out_labels, out_counts);
}
