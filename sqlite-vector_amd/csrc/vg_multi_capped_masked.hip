// vg_multi_capped_masked.hip - the masked family of the capped multi-query scan (vg_scan_multi.h, VG_MQ_GROUPED | VG_MQ_CAPPED |
// VG_MQ_MASKED): the k nearest rows, at most m of one label, among the rows the handle's mask allows, for each query of a pass.  Only
// the kernel table lives here - a translation unit of its own, so that its instances compile next to the unmasked family's
// (vg_multi_capped.hip), which holds the host side of both.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// Left out of the table for their registers: at 6 chunks per lane and 2 queries per pass the cosine instances of
// all three types and the f32 L2 instance spill, like their grouped twins (vg_multi_grouped_masked.hip) - the mask pipeline's words
// on top of the label and the two mlab registers.  A getter that is not instantiated compiles no kernel: such a shape is nullptr
// here, vg_batch_capped_plan reports 0 and the batch takes one single masked capped scan per query.
struct CappedMaskedFamily {
    template <int VT, int ACC, int U, int NQ> static scan_fn_t fn() {
        if constexpr (U == 6 && (ACC == A_COS || (VT == T_F32 && ACC == A_L2))) return nullptr;
        else return vg_scan_multi_kernel<VT, ACC, U, NQ, VG_MQ_GROUPED | VG_MQ_CAPPED | VG_MQ_MASKED>;
    }
};

scan_fn_t vg_pick_multi_capped_masked(int vtype, int acc, int U, int NQ) { return vg_pick_multi<CappedMaskedFamily>(vtype, acc, U, NQ); }
