// vg_scan_within_labeled.hip - labeled range scans, single forms: every row of a label - or of a set of labels - within a distance
// of the query (vg_scan_within_labeled, vg_scan_within_labelset, include/vectorgpu.h).
//
// Host code only, no scan instances of its own: the bitmap "rows that carry the label" (vg_label_bits_enqueue, vg_scan_labeled.hip) or
// "rows whose label is in / not in the set" (vg_labelset_bits_enqueue, vg_scan_labelset.hip) is enqueued into the handle's scratch
// buffer d_label_bits - NOT the user's row mask, which is neither read nor written - and the single range scan (vg_within_run,
// vg_scan_within.hip) runs the masked range kernels of vg_scan_within_masked.hip with ScanArgs.mask pointing at it: launch shape,
// overflow protocol, result path and the held result (vg_scan_within_fetch / _keys) are the single range scan's.  Also the fallback of
// the labeled batch range scan (vg_multi_within.hip).
#include "vg_internal.h"

// what vg_within_run checks, in its order, in front of the checks only these forms know: a refusal or an answer without a launch
// (an empty allowed set) must leave the handle as vg_within_run would.  VG_OK: go on
static int labeled_within_checks(vg_corpus *c, const char *who, int metric, const void *query, double radius, int64_t *out_matches, int64_t *out_held) {
    if (out_matches) *out_matches = 0;
    if (out_held) *out_held = 0;
    if (!c || !query) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    c->within_keys.clear();
    c->within_matches = 0;
    c->within_launches = 0;
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (radius != radius) return vg_fail(VG_ERR_INVALID, "%s: the radius is NaN", who);
    if (!c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", who);
    return VG_OK;
}

extern "C" int vg_scan_within_labeled(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, uint32_t label,
                                      int64_t *out_matches, int64_t *out_held) {
    const VgWithinForm form = {"vg_scan_within_labeled", vg_pick_scan_within_masked, false, true};
    int rc = labeled_within_checks(c, form.who, metric, query, radius, out_matches, out_held);
    if (rc != VG_OK) return rc;
    if (label == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: VG_LABEL_NONE names no row", form.who);
    if (c->n_rows == 0) return VG_OK;
    if ((rc = vg_label_bits_enqueue(c, label)) != VG_OK) return rc;
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}

extern "C" int vg_scan_within_labelset(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, const uint32_t *labels,
                                       int64_t n_labels, int exclude, int64_t *out_matches, int64_t *out_held) {
    const VgWithinForm form = {"vg_scan_within_labelset", vg_pick_scan_within_masked, false, true};
    int rc = labeled_within_checks(c, form.who, metric, query, radius, out_matches, out_held);
    if (rc != VG_OK) return rc;
    std::vector<uint32_t> set;
    if (!vg_labelset_normalise(form.who, labels, n_labels, &set)) return VG_ERR_INVALID;
    if (c->n_rows == 0 || (set.empty() && !exclude)) return VG_OK;          // an empty set allows no row: no launch
    c->lset_host.swap(set);
    if ((rc = vg_labelset_bits_enqueue(c, c->lset_host.data(), (int64_t)c->lset_host.size(), exclude)) != VG_OK) return rc;
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}
