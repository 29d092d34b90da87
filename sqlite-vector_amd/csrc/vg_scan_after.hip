// vg_scan_after.hip - paged scans: the next k rows behind a (distance, rowid) cursor (vg_scan_topk_after, include/vectorgpu.h).
//
// Every scan kernel ranks rows by one 64-bit key, sortable(distance) << 32 | scan position (vg_make_key), and the fused top-k result
// is ascending in that key.  "The k rows behind a cursor" is therefore "the top-k among keys >= a floor": the kernels are the VG_SQ_AFTER
// instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h) without VG_SQ_MASKED (all rows) and with it (the rows the handle's
// mask allows) - the plain / the masked scan's loops, loads, arithmetic, lists and merge plus one wave-uniform 64-bit value and one
// compare in the offer.  A translation unit of their own: every other kernel keeps its register budget.
//
// The host side is the masked scan's (vg_scan_masked.hip: vg_fused_run - argument checks, upload, launch shape, merge, result);
// this unit hands it its kernel tables, derives the floor from the cursor (vg_after_floor) and holds the entry points.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

#include <cfloat>

scan_fn_t vg_pick_scan_after(int vtype, int acc, int U, bool long_rows) { return vg_pick_scan<ScanFamily<VG_SQ_AFTER, true, true>>(vtype, acc, U, long_rows); }
scan_fn_t vg_pick_scan_after_masked(int vtype, int acc, int U, bool long_rows) {
    return vg_pick_scan<ScanFamily<VG_SQ_AFTER | VG_SQ_MASKED, true, true>>(vtype, acc, U, long_rows);
}

// ------------------------------------------------------------------------------------------------ the floor

// The smallest key behind the cursor (after_dist, "the first `first_pos_behind` scan positions are not behind it at that distance").
// f = the smallest float >= after_dist.  When the cursor's distance IS that float, rows holding it are behind the cursor from position
// first_pos_behind on; otherwise every row holding f is.  Pure host arithmetic.
extern "C" int vg_after_floor(double after_dist, uint32_t first_pos_behind, uint64_t *out_floor, int *out_empty) {
    if (!out_floor || !out_empty) return vg_fail(VG_ERR_INVALID, "vg_after_floor: NULL output");
    *out_floor = VG_KEY_EMPTY;
    *out_empty = 1;
    if (after_dist != after_dist) return vg_fail(VG_ERR_INVALID, "vg_after_floor: the cursor's distance is NaN");
    if (after_dist > (double)FLT_MAX) return VG_OK;          // +Inf included: no finite float is larger, and +Inf never enters a result
    const double D = after_dist + 0.0;                       // -0.0 -> 0.0: no row holds -0.0 (vg_clamp), and their images differ
    float f = (float)D;                                      // to nearest (-Inf below -FLT_MAX) ...
    if ((double)f < D) f = nextafterf(f, INFINITY);          // ... then up: the double rounded towards +Inf
    f += 0.0f;
    *out_floor = ((double)f == D) ? vg_make_key(f, first_pos_behind) : vg_make_key(f, 0u);
    *out_empty = 0;
    return VG_OK;
}

// rows held with rowid <= `rowid` (a lower bound over ascending rowids, not an exact find: the cursor's row need not exist any more)
int64_t vg_corpus_rows_upto_rowid(const vg_corpus *c, int64_t rowid) {
    if (c->rowids.empty()) {
        if (rowid < c->rowid_base) return 0;
        const uint64_t diff = (uint64_t)rowid - (uint64_t)c->rowid_base;
        return diff >= (uint64_t)c->n_rows ? c->n_rows : (int64_t)diff + 1;
    }
    if (!c->rowids_ascending) return -2;
    return (int64_t)(std::upper_bound(c->rowids.begin(), c->rowids.end(), rowid) - c->rowids.begin());
}

// (distance, rowid) cursor -> floor key over this corpus' positions; *empty: nothing can be behind it
static int cursor_floor(const vg_corpus *c, const char *who, double after_dist, int64_t after_rowid, uint64_t *floor, int *empty) {
    if (after_dist != after_dist) return vg_fail(VG_ERR_INVALID, "%s: the cursor's distance is NaN", who);
    const int64_t P = vg_corpus_rows_upto_rowid(c, after_rowid);
    if (P == -2) return vg_fail(VG_ERR_UNSUPPORTED, "%s: the corpus' rowids are not ascending (no rowid order); page by key (the _keys form)", who);
    return vg_after_floor(after_dist, (uint32_t)P, floor, empty);      // (P <= n_rows < 2^32)
}

// ------------------------------------------------------------------------------------------------ the scans

static VgFusedForm after_form(bool masked) {
    VgFusedForm f = masked ? vg_fused_form("vg_scan_topk_after_masked", "masked", vg_pick_scan_after_masked, VG_ROWS_MASK)
                           : vg_fused_form("vg_scan_topk_after", "paged", vg_pick_scan_after, VG_ROWS_ALL);
    f.after = true;
    return f;
}

int vg_after_floor_run(vg_corpus *c, bool masked, int metric, const void *query, int k, uint64_t floor, uint64_t *out_keys, int *out_count) {
    return vg_fused_run(c, after_form(masked), metric, query, k, floor, out_keys, out_count);   // (a floor of VG_KEY_EMPTY: no launch)
}

static int after_keys(vg_corpus *c, bool masked, int metric, const void *query, int k, uint64_t after_key, uint64_t *out_keys, int *out_count) {
    if (out_count) *out_count = 0;
    if (after_key == VG_KEY_EMPTY) return vg_fail(VG_ERR_INVALID, "%s: after_key is the empty key", after_form(masked).who);
    return vg_after_floor_run(c, masked, metric, query, k, after_key + 1ull, out_keys, out_count);
}

static int after_rows(vg_corpus *c, bool masked, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                      int64_t *out_rowids, double *out_dist, int *out_count) {
    const char *who = after_form(masked).who;
    if (!c || !query || !out_count) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    *out_count = 0;
    if (k >= 1 && k <= VG_MAX_FUSED_K && (!out_rowids || !out_dist)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    uint64_t floor = VG_KEY_EMPTY;
    int empty = 0;
    int rc = cursor_floor(c, who, after_dist, after_rowid, &floor, &empty);
    if (rc != VG_OK) return rc;
    uint64_t keys[VG_WAVE];
    int cnt = 0;
    rc = vg_after_floor_run(c, masked, metric, query, k, empty ? VG_KEY_EMPTY : floor, keys, &cnt);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys, nullptr, 1, k, &cnt, out_rowids, out_dist, nullptr);
    *out_count = cnt;
    return VG_OK;
}

extern "C" int vg_scan_topk_after(vg_corpus *c, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                  int64_t *out_rowids, double *out_dist, int *out_count) {
    return after_rows(c, false, metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count);
}
extern "C" int vg_scan_topk_after_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t after_key, uint64_t *out_keys,
                                       int *out_count) {
    return after_keys(c, false, metric, query, k, after_key, out_keys, out_count);
}
extern "C" int vg_scan_topk_after_masked(vg_corpus *c, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                         int64_t *out_rowids, double *out_dist, int *out_count) {
    return after_rows(c, true, metric, query, k, after_dist, after_rowid, out_rowids, out_dist, out_count);
}
extern "C" int vg_scan_topk_after_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t after_key, uint64_t *out_keys,
                                              int *out_count) {
    return after_keys(c, true, metric, query, k, after_key, out_keys, out_count);
}
