// vg_multi_within_labeled.hip - the kernels of the labeled batch range scan (vg_scan_within_batch_labeled, include/vectorgpu.h).
//
// Only the kernel table: the VG_MQ_LABELED | VG_MQ_WITHIN instances of the multi-query scan (vg_scan_multi.h) the multi-query ladder
// names, in a translation unit of their own so that they compile next to the others.  Everything on the host - the label order,
// slices, the one key budget, "a pass that overflowed runs once more as a whole", the held per-query results, the fallback - is
// vg_multi_within.hip's, which asks this unit for the kernel and sets ScanArgs.labels.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

scan_fn_t vg_pick_multi_within_labeled(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_LABELED | VG_MQ_WITHIN>>(vtype, acc, U, NQ); }
