// vg_multi_after.hip - paged batch scans: for each of nq queries the next k rows behind its own cursor (vg_scan_topk_batch_after,
// include/vectorgpu.h), over all rows or over the rows the handle's mask allows.
//
// Holds the instances of the floor forms of the multi-query scan (vg_scan_multi.h: VG_MQ_AFTER without and with VG_MQ_MASKED) and the
// batch entry points.  The
// host side is the masked batch's (vg_multi_masked.hip: vg_fused_batch_run - plan, slices, launches, merge, the fallback); this unit
// hands it its kernel tables and one floor key per query, which go up behind each slice's queries.  The plan is vg_multi_plan's (4
// queries per pass with up to 3 chunks per lane, 2 with 4 or 6; f32 / uint8 / int8); f16 / bf16 and long rows are answered by one
// single paged scan per query (vg_scan_after.hip).
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

static VgFusedBatchForm batch_form(bool masked) {
    VgFusedBatchForm f = masked ? VgFusedBatchForm{"vg_scan_topk_batch_after_masked", vg_pick_multi<MultiFamily<VG_MQ_AFTER | VG_MQ_MASKED>>, VG_QROWS_MASK,
                                                   vg_fused_form("vg_scan_topk_after_masked", "masked", vg_pick_scan_after_masked, VG_ROWS_MASK)}
                                : VgFusedBatchForm{"vg_scan_topk_batch_after", vg_pick_multi<MultiFamily<VG_MQ_AFTER>>, VG_QROWS_ALL,
                                                   vg_fused_form("vg_scan_topk_after", "paged", vg_pick_scan_after, VG_ROWS_ALL)};
    f.single.after = true;
    return f;
}

// Query i's answer must be the single form's bit for bit - a cursor taken from a single page or from vg_scan_distances is fed to the
// batch form and the floor compares KEYS.  uint8 / int8 arithmetic is exact under any lane decomposition; f32 sums are not: an f32
// shape whose multi-query launch shape differs from the plain scan's would rank by another float.  Such shapes take the fallback
// (one single paged scan per query), like f16 / bf16 and long rows.
static bool multi_floats_are_the_single_scans(const vg_corpus *c, int metric) {
    if (c->vtype != VG_TYPE_F32) return true;
    VgShape m{}, p{};
    if (vg_multi_plan(c, metric, &m) == 0) return true;      // (the fallback anyway)
    vg_plain_scan_shape(c, metric, &p);
    return !p.long_rows && m.lpr_log2 == p.lpr_log2 && m.U == p.U;
}

int vg_after_floor_batch_run(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, const uint64_t *floors,
                             uint64_t *out_keys, int *out_counts) {
    const VgFusedBatchForm form = batch_form(masked);
    if (c && queries && out_counts && floors && out_keys && nq >= 1 && vg_metric_to_acc(metric) >= 0 && !multi_floats_are_the_single_scans(c, metric)) {
        const size_t row_bytes = (size_t)c->dim * c->es;
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        for (int i = 0; i < nq; ++i) {
            int rc = vg_fused_run(c, form.single, metric, (const uint8_t *)queries + (size_t)i * row_bytes, k, floors[i],
                                  out_keys + (size_t)i * (k > 0 ? k : 0), &out_counts[i]);
            if (rc != VG_OK) return rc;
        }
        return VG_OK;
    }
    return vg_fused_batch_run(c, form, metric, queries, nq, k, floors, out_keys, out_counts);
}

static int batch_after_keys(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                            uint64_t *out_keys, int *out_counts) {
    const char *who = batch_form(masked).who;
    if (!after_keys) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", who);
    std::vector<uint64_t> floors((size_t)nq);
    for (int i = 0; i < nq; ++i) {
        if (after_keys[i] == VG_KEY_EMPTY) return vg_fail(VG_ERR_INVALID, "%s: after_keys[%d] is the empty key", who, i);
        floors[(size_t)i] = after_keys[i] + 1ull;
    }
    return vg_after_floor_batch_run(c, masked, metric, queries, nq, k, floors.data(), out_keys, out_counts);
}

static int batch_after_rows(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, const double *after_dists,
                            const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    const char *who = batch_form(masked).who;
    return vg_batch_rows_from_keys(c, who, !c || !queries || !out_counts || !after_dists || !after_rowids, nq, k, k >= 1 && k <= VG_MAX_FUSED_K, false,
                                   out_rowids, out_dist, nullptr, out_counts, [&](uint64_t *keys, uint32_t *) {
        if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", who);
        std::vector<uint64_t> floors((size_t)nq, VG_KEY_EMPTY);
        for (int i = 0; i < nq; ++i) {
            if (after_dists[i] != after_dists[i]) return vg_fail(VG_ERR_INVALID, "%s: the distance of cursor %d is NaN", who, i);
            const int64_t P = vg_corpus_rows_upto_rowid(c, after_rowids[i]);
            if (P == -2) return vg_fail(VG_ERR_UNSUPPORTED, "%s: the corpus' rowids are not ascending (no rowid order); page by key (the _keys form)", who);
            int empty = 0;
            int rc = vg_after_floor(after_dists[i], (uint32_t)P, &floors[(size_t)i], &empty);      // (an exhausted cursor: VG_KEY_EMPTY, nothing admitted)
            if (rc != VG_OK) return rc;
        }
        return vg_after_floor_batch_run(c, masked, metric, queries, nq, k, floors.data(), keys, out_counts);
    });
}

extern "C" int vg_scan_topk_batch_after(vg_corpus *c, int metric, const void *queries, int nq, int k, const double *after_dists,
                                        const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return batch_after_rows(c, false, metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts);
}
extern "C" int vg_scan_topk_batch_after_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                             uint64_t *out_keys, int *out_counts) {
    return batch_after_keys(c, false, metric, queries, nq, k, after_keys, out_keys, out_counts);
}
extern "C" int vg_scan_topk_batch_after_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, const double *after_dists,
                                               const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return batch_after_rows(c, true, metric, queries, nq, k, after_dists, after_rowids, out_rowids, out_dist, out_counts);
}
extern "C" int vg_scan_topk_batch_after_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                                    uint64_t *out_keys, int *out_counts) {
    return batch_after_keys(c, true, metric, queries, nq, k, after_keys, out_keys, out_counts);
}
