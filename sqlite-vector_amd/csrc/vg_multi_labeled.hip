// vg_multi_labeled.hip - labeled batch scans: the k nearest rows of ITS label for each of many queries (vg_scan_topk_batch_labeled,
// include/vectorgpu.h).
//
// Host side of the labeled form of the multi-query scan (vg_scan_multi.h, VG_MQ_LABELED) and the home of its 60 kernel instances
// (f32 / uint8 / int8 x L2 / cosine / dot / L1 x U in {1, 2, 3} at 4 queries per pass, {4, 6} at 2).  The batch itself is
// vg_fused_batch_run (vg_multi_masked.hip) with a labeled form: slices, back-to-back passes, one copy of the keys, one wait.  What is
// this unit's own: the queries are ordered by label (stable) before they are cut into passes - a pass' queries then share as few
// distinct labels as possible, which is what lets a pass skip the batches of rows that carry none of them - and the results are
// scattered back to caller order.  A pad query of a ragged last pass carries VG_LABEL_NONE and matches nothing.  Shapes without a
// multi-query form (f16 / bf16, long rows): one single labeled scan per query (vg_scan_labeled.hip), one bitmap per distinct label.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

#include <numeric>

static scan_fn_t pick_multi_labeled(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_LABELED>>(vtype, acc, U, NQ); }

extern "C" int vg_batch_labeled_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, pick_multi_labeled, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_scan_topk_batch_labeled_keys(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                               uint64_t *out_keys, int *out_counts) {
    const VgFusedBatchForm form = {"vg_scan_topk_batch_labeled", pick_multi_labeled, {"vg_scan_topk_labeled", vg_pick_scan_masked, false, false, true}};
    if (!c || !queries || !out_counts || !query_labels) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", form.who);
    // queries in label order (stable: equal labels keep caller order); everything else - argument checks included - is the shared routine's
    std::vector<int> order((size_t)nq);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return query_labels[x] < query_labels[y]; });
    const size_t row_bytes = (size_t)c->dim * c->es;
    std::vector<uint8_t> sq((size_t)nq * row_bytes);
    std::vector<uint32_t> sl((size_t)nq);
    for (int i = 0; i < nq; ++i) {
        memcpy(sq.data() + (size_t)i * row_bytes, (const uint8_t *)queries + (size_t)order[(size_t)i] * row_bytes, row_bytes);
        sl[(size_t)i] = query_labels[order[(size_t)i]];
    }
    const bool k_ok = k >= 1 && k <= VG_MAX_FUSED_K;
    std::vector<uint64_t> skeys(k_ok ? (size_t)nq * k : 1);
    std::vector<int> scounts((size_t)nq, 0);
    int rc = vg_fused_batch_run(c, form, metric, sq.data(), nq, k, nullptr, out_keys ? skeys.data() : nullptr, scounts.data(), sl.data());
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (rc != VG_OK) return rc;
    for (int i = 0; i < nq; ++i) {
        const int dst = order[(size_t)i];
        out_counts[dst] = scounts[(size_t)i];
        memcpy(out_keys + (size_t)dst * k, skeys.data() + (size_t)i * k, (size_t)scounts[(size_t)i] * sizeof(uint64_t));
    }
    return VG_OK;
}

extern "C" int vg_scan_topk_batch_labeled(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                          int64_t *out_rowids, double *out_dist, int *out_counts) {
    if (!c || !queries || !out_counts || !query_labels) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_batch_labeled: NULL argument");
    const bool k_ok = k >= 1 && k <= VG_MAX_FUSED_K;
    if (nq >= 1) for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (nq >= 1 && k_ok && (!out_rowids || !out_dist)) return vg_fail(VG_ERR_INVALID, "vg_scan_topk_batch_labeled: NULL output");
    std::vector<uint64_t> keys((nq >= 1 && k_ok) ? (size_t)nq * k : 1);
    int rc = vg_scan_topk_batch_labeled_keys(c, metric, queries, nq, query_labels, k, keys.data(), out_counts);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys.data(), nullptr, nq, k, out_counts, out_rowids, out_dist, nullptr);
    return VG_OK;
}
