// vg_scan_ex.hip - the VG_SQ_EX instances of vg_scan_kernel (vg_scan.h; ScanFamily<VG_SQ_EX, ...>, vg_pick.h): the plain scan with what tie_order = reference
// needs on top - a start threshold from the pass over the rows in front, the candidate stream, "top-k + store" for the prefix pass
// (vg_reforder.hip).  A translation unit of their own: compile time, and the plain kernels keep their register budget.
// One load policy (non-temporal): the prefix pass is small and the emitting main pass runs only while ties are around.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

// the EX kernel for (element type, accumulation kind, chunks per lane), nullptr if there is none
// (no long-row kernel: a long-row scan neither emits nor stores a prefix - vg_api.hip, launch_scan)
scan_fn_t vg_pick_scan_kernel_ex(int vtype, int acc, int U) { return vg_pick_scan<ScanFamily<VG_SQ_EX, true, false>>(vtype, acc, U, false); }
