// vg_multi.hip - host side of the multi-query scan (vg_scan_multi.h): shape choice, kernel table, launch.  Holds the instances of
// its plain top-k form (MultiFamily<0>); each other form's instances are in a unit of their own (vg_multi_masked.hip,
// vg_multi_after.hip, vg_multi_within.hip, vg_multi_within_masked.hip, vg_multi_within_labeled.hip), so that the 60 instances per form compile next to each other
// and to vg_api.hip's, not after them.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// (queries per pass, launch shape) of the multi-query scan for this corpus / metric; 0 when there is none
static int multi_plan(const vg_corpus *c, int metric, VgShape *s) {
    const int acc = vg_metric_to_acc(metric);
    if (acc < 0) return 0;
    // f16 / bf16 scans are bound by their f64 accumulation (the reference's arithmetic), not by HBM: two queries per
    // pass measured 0.75x - 1.2x of two single scans (and spill at U = 3), so they keep the single-query kernel
    if (c->vtype == VG_TYPE_F16 || c->vtype == VG_TYPE_BF16) return 0;
    vg_choose_shape(c->nch, c->vtype, acc, s, 3);
    if (!s->long_rows && s->U <= 3) return 4;
    vg_choose_shape(c->nch, c->vtype, acc, s, 6);
    if (!s->long_rows && (s->U == 4 || s->U == 6)) return 2;
    return 0;
}

int vg_multi_queries_per_pass(const vg_corpus *c, int metric) {
    VgShape s;
    return multi_plan(c, metric, &s);
}

// the same plan with its launch shape: what the masked multi-query scan (vg_multi_masked.hip) is launched with too
int vg_multi_plan(const vg_corpus *c, int metric, VgShape *s) { return multi_plan(c, metric, s); }

// NQ = vg_multi_queries_per_pass() queries (zero-padded rows of the corpus stride, back to back at dev_queries) against
// the corpus in ONE pass; dev_cand: NQ * (<= 256) * 64 keys of scratch; dev_out_keys: NQ x 64 keys.  Asynchronous on
// `stream`.  Returns -1 when the shape has no multi-query kernel, VG_OK or an error code otherwise.
int vg_launch_scan_multi(vg_corpus *c, int metric, const uint8_t *dev_queries, int k, uint64_t *dev_cand, uint64_t *dev_out_keys,
                         hipStream_t stream) {
    if (k < 1 || k > VG_MAX_FUSED_K) return -1;
    VgShape s;
    const int NQ = multi_plan(c, metric, &s);
    if (NQ == 0) return -1;
    const int acc = vg_metric_to_acc(metric);
    scan_fn_t fn = vg_pick_multi<MultiFamily<0>>(c->vtype, acc, s.U, NQ);
    if (!fn) return -1;
    const long long blocks = vg_percu_scan_blocks(c, c->n_rows, s);
    if (c->append_pending && stream != c->stream) HIP_TRY(hipStreamWaitEvent(stream, c->append_ev, 0));
    ScanArgs a = vg_scan_args(c, metric, acc, s, dev_queries, k);
    a.cand = dev_cand;
    const size_t smem = std::max<size_t>((size_t)NQ * c->nch * 16, (size_t)VG_PUBLISH_LDS_BYTES);
    int rc = vg_launch_scan_kernel(fn, blocks, smem, stream, a);
    if (rc != VG_OK) return rc;
    rc = vg_launch_merge(dev_cand, (int)blocks, k, dev_out_keys, NQ, stream);
    if (rc != 0) return vg_fail(VG_ERR_HIP, "merge launch failed: %s", hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipGetLastError());
    return VG_OK;
}
