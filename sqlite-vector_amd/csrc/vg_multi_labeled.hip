// vg_multi_labeled.hip - labeled batch scans: the k nearest rows of ITS label for each of many queries (vg_scan_topk_batch_labeled,
// include/vectorgpu.h).
//
// Host side of the labeled form of the multi-query scan (vg_scan_multi.h, VG_MQ_LABELED) and the home of its 60 kernel instances
// (f32 / uint8 / int8 x L2 / cosine / dot / L1 x U in {1, 2, 3} at 4 queries per pass, {4, 6} at 2).  The batch itself is
// vg_fused_batch_run (vg_multi_masked.hip) with a labeled form: slices, back-to-back passes, one copy of the keys, one wait.  What is
// this unit's own: the queries are ordered by label (stable) before they are cut into passes - a pass' queries then share as few
// distinct labels as possible, which is what lets a pass skip the batches of rows that carry none of them - and the results are
// scattered back to caller order.  A pad query of a ragged last pass carries VG_LABEL_NONE and matches nothing.  Shapes without a
// multi-query form (f16 / bf16, long rows): one single labeled scan per query (vg_rowpred.hip), one bitmap per distinct label.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

static scan_fn_t pick_multi_labeled(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_LABELED>>(vtype, acc, U, NQ); }

extern "C" int vg_batch_labeled_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, pick_multi_labeled, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_scan_topk_batch_labeled_keys(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                               uint64_t *out_keys, int *out_counts) {
    const VgFusedBatchForm form = {"vg_scan_topk_batch_labeled", pick_multi_labeled, VG_QROWS_LABEL,
                                   vg_pred_form("vg_scan_topk_labeled", vg_pred_label(0u), vg_result_plain())};
    if (!c || !queries || !out_counts || !query_labels) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", form.who);
    // queries in label order (stable: equal labels keep caller order); everything else - argument checks included - is the shared routine's
    const std::vector<int> order = vg_stable_order(nq, [&](int x, int y) { return query_labels[x] < query_labels[y]; });
    std::vector<uint32_t> sl((size_t)nq);
    for (int i = 0; i < nq; ++i) sl[(size_t)i] = query_labels[order[(size_t)i]];
    return vg_ordered_batch(c, queries, nq, k, order, out_keys, out_counts, [&](const void *sq, uint64_t *skeys, int *scounts) {
        int rc = vg_fused_batch_run(c, form, metric, sq, nq, k, nullptr, skeys, scounts, sl.data());
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        return rc;
    });
}

extern "C" int vg_scan_topk_batch_labeled(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                          int64_t *out_rowids, double *out_dist, int *out_counts) {
    return vg_batch_rows_from_keys(c, "vg_scan_topk_batch_labeled", !c || !queries || !out_counts || !query_labels, nq, k,
                                   k >= 1 && k <= VG_MAX_FUSED_K, false, out_rowids, out_dist, nullptr, out_counts, [&](uint64_t *keys, uint32_t *) {
        return vg_scan_topk_batch_labeled_keys(c, metric, queries, nq, query_labels, k, keys, out_counts);
    });
}
