// vg_multi_valued.hip - value-range batch scans: for each of many queries the k nearest rows whose value lies in ITS interval - and,
// with query labels, that carry ITS label (vg_scan_topk_batch_valued, include/vectorgpu.h).
//
// A membership form of vg_fused_batch_run (VgMemberForm, vg_internal.h) like the label-set batch, whose passes it shares: the
// VG_MQ_LABELSET instances of vg_multi_labelset.hip, unchanged - they read one membership dword per row and never a label or a value.
// What is this unit's own:
//   * the queries are ordered by (label, lo, hi), stable, before they are cut into groups and passes: requests with one condition are
//     neighbours, share passes and their skip, and share ONE comparison in the pre-pass; the results are scattered back to caller order;
//   * every membership group of up to 32 queries uploads its DISTINCT conditions into the handle's d_lset:
//     [nd | nd x {lo, hi, label, use_label, query mask, 0}] - lo and hi as two dwords each, low half first, VG_VALUE_COND_DWORDS = 8
//     dwords a condition; query mask: bit j set when query j of the group asks under the condition;
//   * vg_value_member_kernel runs once per group, in stream order in front of the group's passes: it reads values[row] once - and
//     labels[row] when a condition of the group names a label - and writes ONE dword per row into d_member.
// Shapes without a multi-query form (f16 / bf16, long rows): one single valued scan per query (vg_rowpred.hip) in that same
// order, the bitmap rebuilt only where the condition changes.
#include "vg_internal.h"

#include "vg_device.h"

#define VG_VALUE_GROUP 32               // queries per membership dword: at most that many distinct conditions in a table
#define VG_VALUE_COND_DWORDS 8

// d_member[row] for one group.  `grp`: [nd | the conditions], staged into LDS by every workgroup (at most 1 KiB).  One thread a row,
// grid-stride; per condition one signed 64-bit interval test (and one label compare), the condition's query mask OR-ed in on a hit.
__global__ __launch_bounds__(256) void vg_value_member_kernel(const int64_t *values, const uint32_t *labels, long long n_rows, const uint32_t *grp,
                                                              int nd, int any_label, uint32_t *member) {
    __shared__ uint32_t tab[VG_VALUE_GROUP * VG_VALUE_COND_DWORDS];
    for (int i = threadIdx.x; i < nd * VG_VALUE_COND_DWORDS; i += blockDim.x) tab[i] = grp[1 + i];
    __syncthreads();
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += stride) {
        const long long v = values[row];
        const uint32_t lab = any_label ? labels[row] : 0u;
        uint32_t word = 0u;
        for (int d = 0; d < nd; ++d) {
            const uint32_t *e = tab + d * VG_VALUE_COND_DWORDS;
            const long long lo = (long long)(((unsigned long long)e[1] << 32) | e[0]);
            const long long hi = (long long)(((unsigned long long)e[3] << 32) | e[2]);
            const bool hit = v >= lo && v <= hi && (e[5] == 0u || lab == e[4]);
            if (hit) word |= e[6];
        }
        member[row] = word;
    }
}

int vg_value_member_enqueue(vg_corpus *c, size_t at, int nd, int any_label) {
    if (nd < 0 || nd > VG_VALUE_GROUP) return vg_fail(VG_ERR_INVALID, "vg_value_member_enqueue: %d conditions in a group of %d", nd, VG_VALUE_GROUP);
    int rc = vg_member_reserve(c);
    if (rc != VG_OK) return rc;
    const long long blocks = std::min<long long>((c->n_rows + 255) / 256, 2048);
    hipLaunchKernelGGL(vg_value_member_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, (const int64_t *)c->d_values,
                       (const uint32_t *)c->d_labels, (long long)c->n_rows, (const uint32_t *)c->d_lset + at, nd, any_label ? 1 : 0, c->d_member);
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// ---- the valued batch as a membership form: the conditions of the queries AS HANDED OVER to vg_fused_batch_run (ordered)
struct VgValuedBatch { const int64_t *los; const int64_t *his; const uint32_t *labels; };      // labels: nullptr - no conjunction

static bool same_cond(const VgValuedBatch *v, int x, int y) {
    return v->los[x] == v->los[y] && v->his[x] == v->his[y] && (!v->labels || v->labels[x] == v->labels[y]);
}

static int valued_pack_group(const void *ctx, const char *who, int g0, int g1, std::vector<uint32_t> *data, int *nd, size_t *total) {
    const VgValuedBatch *v = (const VgValuedBatch *)ctx;
    (void)who;
    const size_t head = data->size();
    data->push_back(0u);
    int n = 0;
    for (int i = g0; i < g1; ++i) {
        if (i > g0 && same_cond(v, i, i - 1)) { (*data)[data->size() - 2] |= 1u << (i - g0); continue; }
        const uint64_t lo = (uint64_t)v->los[i], hi = (uint64_t)v->his[i];
        const uint32_t e[VG_VALUE_COND_DWORDS] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32),
                                                  v->labels ? v->labels[i] : 0u, v->labels ? 1u : 0u, 1u << (i - g0), 0u};
        data->insert(data->end(), e, e + VG_VALUE_COND_DWORDS);
        ++n;
    }
    (*data)[head] = (uint32_t)n;
    *nd = n;
    *total = v->labels ? 1 : 0;                              // (what member_enqueue gets back: a condition of the group names a label)
    return VG_OK;
}

static int valued_member_step(vg_corpus *c, const void *ctx, size_t at, int nd, size_t total) {
    (void)ctx;
    return vg_value_member_enqueue(c, at, nd, (int)total);
}

// the fallback: one bitmap per run of equal conditions; an empty interval has no rows - no launch, count 0
static int valued_bits_step(vg_corpus *c, const void *ctx, int i, bool *skip) {
    const VgValuedBatch *v = (const VgValuedBatch *)ctx;
    if (v->los[i] > v->his[i]) { *skip = true; return VG_OK; }
    if (i > 0 && same_cond(v, i, i - 1)) return VG_OK;       // (the query in front was not skipped: its interval is this one)
    return vg_pred_bits_enqueue(c, v->labels ? vg_pred_value_labeled(v->los[i], v->his[i], v->labels[i]) : vg_pred_value(v->los[i], v->his[i]));
}

extern "C" int vg_batch_valued_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, vg_pick_multi_labelset, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_scan_topk_batch_valued_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const int64_t *los, const int64_t *his,
                                              const uint32_t *query_labels, uint64_t *out_keys, int *out_counts) {
    // (the handle must hold values; labels only where the queries name one, which is checked below)
    const VgFusedBatchForm form = {"vg_scan_topk_batch_valued", vg_pick_multi_labelset, VG_QROWS_MEMBER,
                                   vg_pred_form("vg_scan_topk_valued", vg_pred_value(0, 0), vg_result_plain())};
    if (!c || !queries || !out_counts || !los || !his) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", form.who);
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", form.who);
    if (k > VG_MAX_FUSED_K) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (valued scans use the fused list only)", form.who, VG_MAX_FUSED_K);
    if (!out_keys) return vg_fail(VG_ERR_INVALID, "%s: NULL output", form.who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (!c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", form.who);
    if (query_labels) {
        if (!c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", form.who);
        for (int i = 0; i < nq; ++i)
            if (query_labels[i] == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: query %d: VG_LABEL_NONE names no row", form.who, i);
    }
    if (int rcm = vg_metric_check(c->vtype, metric, form.who)) return rcm;
    // the queries in (label, lo, hi) order (stable: equal conditions keep caller order)
    const std::vector<int> order = vg_stable_order(nq, [&](int x, int y) {
        if (query_labels && query_labels[x] != query_labels[y]) return query_labels[x] < query_labels[y];
        if (los[x] != los[y]) return los[x] < los[y];
        return his[x] < his[y];
    });
    std::vector<int64_t> slo((size_t)nq), shi((size_t)nq);
    std::vector<uint32_t> slab(query_labels ? (size_t)nq : 0);
    for (int i = 0; i < nq; ++i) {
        const int src = order[(size_t)i];
        slo[(size_t)i] = los[src];
        shi[(size_t)i] = his[src];
        if (query_labels) slab[(size_t)i] = query_labels[src];
    }
    const VgValuedBatch vb = {slo.data(), shi.data(), query_labels ? slab.data() : nullptr};
    const VgMemberForm member = {&vb, valued_pack_group, valued_member_step, valued_bits_step};
    return vg_ordered_batch(c, queries, nq, k, order, out_keys, out_counts, [&](const void *sq, uint64_t *skeys, int *scounts) {
        return vg_fused_batch_run(c, form, metric, sq, nq, k, nullptr, skeys, scounts, nullptr, nullptr, &member);
    });
}

extern "C" int vg_scan_topk_batch_valued(vg_corpus *c, int metric, const void *queries, int nq, int k, const int64_t *los, const int64_t *his,
                                         const uint32_t *query_labels, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return vg_batch_rows_from_keys(c, "vg_scan_topk_batch_valued", !c || !queries || !out_counts || !los || !his, nq, k,
                                   k >= 1 && k <= VG_MAX_FUSED_K, false, out_rowids, out_dist, nullptr, out_counts, [&](uint64_t *keys, uint32_t *) {
        return vg_scan_topk_batch_valued_keys(c, metric, queries, nq, k, los, his, query_labels, keys, out_counts);
    });
}
