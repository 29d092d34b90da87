// vg_multi_grouped.hip - grouped batch scans: the k nearest LABELS, each by its best row, for each of many queries
// (vg_scan_topk_batch_grouped, include/vectorgpu.h).
//
// Host side of the grouped form of the multi-query scan (vg_scan_multi.h, VG_MQ_GROUPED) and the home of its unmasked kernel
// instances (f32 / uint8 / int8 x L2 / cosine / dot / L1 x U in {1, 2, 3} at 4 queries per pass, {4, 6} at 2); the masked family
// compiles next to it in vg_multi_grouped_masked.hip.  The batch itself is vg_fused_batch_run (vg_multi_masked.hip) with a grouped
// form: slices, back-to-back passes, the label-deduping merge per query (vg_merge_grouped_batch_kernel, below), one
// copy of keys and labels, one wait.  Query i gets what the single grouped scan is contracted to return for it.  Shapes without a
// multi-query form (f16 / bf16, long rows): one single grouped scan per query (vg_scan_grouped.hip) - a shape that scan refuses
// (f16 cosine / dot over rows of 2049 .. 3072 halves) is refused here too.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// (every unmasked instance compiles without scratch and without spills; the masked table leaves four out: vg_multi_grouped_masked.hip.
//  A shape whose instance is nullptr goes to the fallback and vg_batch_grouped_plan reports 0 for it)
static scan_fn_t pick_multi_grouped(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_GROUPED>>(vtype, acc, U, NQ); }
static scan_fn_t pick_multi_grouped_masked(int vtype, int acc, int U, int NQ) { return vg_pick_multi_grouped_masked(vtype, acc, U, NQ); }

// ------------------------------------------------------------------------------------------------ the final merge, batch launch

// vg_merge_grouped_kernel (vg_scan_grouped.hip) with a grid of NQ: workgroup n merges query n's nlists <= 256 lists - cand is
// [NQ][nlists][64] keys - and writes 64 keys, then 64 labels, at its own offset (VG_KEYS_BYTES per query).  The same statements
// behind two offsets, in a kernel of its own: the single-query kernel keeps its grid of 1, its output layout and its code.
// Two bodies to keep in step: a change to the statements below belongs in vg_merge_grouped_kernel too, and the other way round.
// (vg_merge_capped_batch_kernel, vg_multi_capped.hip, is these statements with the cap handed to the list routines: a third one)
#define VG_GMERGE_BATCH_PER_WAVE (VG_SEL_MAX_HEADS / VG_WAVES_PER_BLOCK)
__global__ __launch_bounds__(VG_BLOCK) void vg_merge_grouped_batch_kernel(const uint64_t *cand, int nlists, int k, const uint32_t *labels, uint64_t *out) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[VG_WAVES_PER_BLOCK * VG_WAVE * 12];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    cand += (long long)blockIdx.x * nlists * VG_WAVE;
    out += (long long)blockIdx.x * (VG_KEYS_BYTES / sizeof(uint64_t));
    uint64_t keys[VG_GMERGE_BATCH_PER_WAVE];
    uint32_t labs[VG_GMERGE_BATCH_PER_WAVE];
#pragma unroll
    for (int i = 0; i < VG_GMERGE_BATCH_PER_WAVE; ++i) {
        const int l = wave + i * VG_WAVES_PER_BLOCK;
        keys[i] = (l < nlists && lane < k) ? cand[(long long)l * VG_WAVE + lane] : VG_EMPTY_KEY;
    }
#pragma unroll
    for (int i = 0; i < VG_GMERGE_BATCH_PER_WAVE; ++i) labs[i] = (keys[i] != VG_EMPTY_KEY) ? labels[(uint32_t)keys[i]] : 0xFFFFFFFFu;
    uint64_t mine = VG_EMPTY_KEY, thr = VG_EMPTY_KEY;
    uint32_t mlab = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 0; i < VG_GMERGE_BATCH_PER_WAVE; ++i) vg_list_offer_grouped(keys[i], labs[i], keys[i] != VG_EMPTY_KEY, mine, mlab, thr, lane, k);
    vg_block_publish_grouped(smem, mine, mlab, k, VG_WAVES_PER_BLOCK, out, reinterpret_cast<uint32_t *>(out + VG_WAVE));
}

int vg_launch_merge_grouped_batch(const uint64_t *dev_cand, int nlists, int k, const uint32_t *dev_labels, uint64_t *dev_out, int nq, hipStream_t stream) {
    if (nlists > VG_SEL_MAX_HEADS || nq < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(vg_merge_grouped_batch_kernel, dim3(nq), dim3(VG_BLOCK), 0, stream, dev_cand, nlists, k, dev_labels, dev_out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the scans

static VgFusedBatchForm grouped_batch_form(bool masked) {
    if (masked) return VgFusedBatchForm{"vg_scan_topk_batch_grouped_masked", pick_multi_grouped_masked, VG_QROWS_MASK,
                                        vg_fused_form("vg_scan_topk_grouped_masked", "grouped", vg_pick_scan_grouped_masked, VG_ROWS_MASK, vg_result_grouped())};
    return VgFusedBatchForm{"vg_scan_topk_batch_grouped", pick_multi_grouped, VG_QROWS_ALL,
                            vg_fused_form("vg_scan_topk_grouped", "grouped", vg_pick_scan_grouped, VG_ROWS_ALL, vg_result_grouped())};
}

extern "C" int vg_batch_grouped_plan(const vg_corpus *c, int metric, int masked, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, masked ? pick_multi_grouped_masked : pick_multi_grouped, out_queries_per_pass, out_lpr, out_u);
}

static int grouped_batch_keys(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, uint64_t *out_keys,
                              uint32_t *out_labels, int *out_counts) {
    return vg_fused_batch_run(c, grouped_batch_form(masked), metric, queries, nq, k, nullptr, out_keys, out_counts, nullptr, out_labels);
}

static int grouped_batch_rows(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                              double *out_dist, uint32_t *out_labels, int *out_counts) {
    return vg_batch_rows_from_keys(c, grouped_batch_form(masked).who, !c || !queries || !out_counts, nq, k, k >= 1 && k <= VG_MAX_FUSED_K, true,
                                   out_rowids, out_dist, out_labels, out_counts, [&](uint64_t *keys, uint32_t *labels) {
        return grouped_batch_keys(c, masked, metric, queries, nq, k, keys, labels, out_counts);
    });
}

extern "C" int vg_scan_topk_batch_grouped(vg_corpus *c, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                          double *out_dist, uint32_t *out_labels, int *out_counts) {
    return grouped_batch_rows(c, false, metric, queries, nq, k, out_rowids, out_dist, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_grouped_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                                 double *out_dist, uint32_t *out_labels, int *out_counts) {
    return grouped_batch_rows(c, true, metric, queries, nq, k, out_rowids, out_dist, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_grouped_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, uint64_t *out_keys,
                                               uint32_t *out_labels, int *out_counts) {
    return grouped_batch_keys(c, false, metric, queries, nq, k, out_keys, out_labels, out_counts);
}
extern "C" int vg_scan_topk_batch_grouped_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, uint64_t *out_keys,
                                                      uint32_t *out_labels, int *out_counts) {
    return grouped_batch_keys(c, true, metric, queries, nq, k, out_keys, out_labels, out_counts);
}
