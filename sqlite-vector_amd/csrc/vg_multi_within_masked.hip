// vg_multi_within_masked.hip - the kernels of the masked batch range scan (vg_scan_within_batch_masked, include/vectorgpu.h).
//
// Only the kernel table: the instances of vg_scan_multi_within_masked_kernel (vg_scan_multi_within_masked.h) the multi-query ladder
// names, in a translation unit of their own so that they compile next to the others.  Everything on the host - slices, the one key
// budget, "a pass that overflowed runs once more as a whole", the held per-query results, the fallback - is vg_multi_within.hip's,
// which asks this unit for the kernel and sets ScanArgs.mask.
#include "vg_internal.h"

#include "vg_scan_multi_within_masked.h"
#include "vg_pick.h"

struct MultiWithinMaskedFamily {
    template <int VT, int ACC, int U, int NQ> static scan_fn_t fn() { return vg_scan_multi_within_masked_kernel<VT, ACC, U, NQ, true>; }
};

scan_fn_t vg_pick_multi_within_masked(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiWithinMaskedFamily>(vtype, acc, U, NQ); }
