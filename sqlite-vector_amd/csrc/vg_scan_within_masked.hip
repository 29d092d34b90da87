// vg_scan_within_masked.hip - masked range scans: every ALLOWED row within a distance of the query (vg_scan_within_masked,
// include/vectorgpu.h).
//
// The kernels are the VG_SQ_WITHIN | VG_SQ_MASKED instances of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h): the masked pipeline -
// the mask bits of a batch one step ahead of its row prefetch, the zero chunk and no arithmetic for a batch without an allowed row -
// with the range scan's offer (a row matches when its bit is set, d <= r and d is finite) and the range scan's tail (flush the
// wavefront's queue; no list, no publish).  A translation unit of their own: every other kernel keeps its register budget.
//
// The host side is the single range scan's (vg_scan_within.hip: vg_within_run - launch, the overflow protocol, the result path, the
// held result read by vg_scan_within_fetch / _keys); this form hands it its kernel table and asks for ScanArgs.mask to be set.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// the kernel table as a plain function: the range forms of the row predicates (vg_rowpred.hip) run these kernels over a label bitmap
scan_fn_t vg_pick_scan_within_masked(int vtype, int acc, int U, bool long_rows) {
    return vg_pick_scan<ScanFamily<VG_SQ_WITHIN | VG_SQ_MASKED, true, true>>(vtype, acc, U, long_rows);
}

extern "C" int vg_scan_within_masked(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                                     int64_t *out_held) {
    const VgWithinForm form = vg_within_form("vg_scan_within_masked", vg_pick_scan_within_masked, VG_ROWS_MASK);
    return vg_within_run(c, form, metric, query, radius, limit, out_matches, out_held);
}
