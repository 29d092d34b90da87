// vg_scan_ex.hip - the EX = true instantiations of vg_scan_kernel (vg_scan.h): the plain scan with what tie_order = reference
// needs on top - a start threshold from the pass over the rows in front, the candidate stream, "top-k + store" for the prefix pass
// (vg_reforder.hip).  A translation unit of their own: compile time, and the plain kernels keep their register budget.
// One load policy (non-temporal): the prefix pass is small and the emitting main pass runs only while ties are around.
#include "vg_internal.h"

#include "vg_scan.h"
#include "vg_pick.h"

struct ExFamily {
    static const bool has_long = false;                      // (a long-row scan neither emits nor stores a prefix: vg_api.hip, launch_scan)
    template <int VT, int ACC, int U> static scan_fn_t fn() { return vg_scan_kernel<VT, ACC, U, true, true>; }
};

// the EX kernel for (element type, accumulation kind, chunks per lane), nullptr if there is none
scan_fn_t vg_pick_scan_kernel_ex(int vtype, int acc, int U) { return vg_pick_scan<ExFamily>(vtype, acc, U, false); }
