// vg_multi_labelset.hip - label-set batch scans: for each of many queries the k nearest rows whose label is in (exclude: is a label
// and not in) ITS set of labels (vg_scan_topk_batch_labelset, include/vectorgpu.h).
//
// Host side of the label-set form of the multi-query scan (vg_scan_multi.h, VG_MQ_LABELSET), the home of its 60 kernel instances -
// those of the labeled form: f32 / uint8 / int8 x L2 / cosine / dot / L1 x U in {1, 2, 3} at 4 queries per pass, {4, 6} at 2 - and of
// the membership pre-pass in front of them.  The batch itself is vg_fused_batch_run (vg_multi_masked.hip) with a label-set form.
// What is this unit's own:
//   * the queries are ordered by their normalised (sorted, de-duplicated) sets, lexicographically and stable, before they are cut
//     into groups and passes: requests with one set are neighbours, share passes and their skip, and share ONE search in the pre-pass;
//     the results are scattered back to caller order;
//   * the queries are cut into membership groups of up to 32 (VG_LSET_GROUP; a multiple of every queries-per-pass, and a slice of
//     vg_fused_batch_run is a multiple of it).  Every group's DISTINCT sets go up once, for the whole batch, into the handle's
//     d_lset: per group [nd + 1 offsets | nd query masks | the nd sets back to back] - query mask d has bit j set when query j of the
//     group asks under set d;
//   * vg_labelset_member_kernel runs once per group, in stream order in front of the group's passes: it reads labels[row] once and
//     writes ONE dword per row into d_member - bit j: query j of the group may see the row, exclusion folded in, 0 for a row without
//     a label.  n_rows dwords whatever the batch: a later group refills it behind the passes of the one in front.  The passes then
//     read 4 bytes per row of a batch they visit where the labeled form reads its label - and no set at all.
// Where the sets are searched: a group whose distinct sets hold at most VG_LSET_LDS_MAX labels in all (8192: 32 KiB + the offsets and
// masks) is staged into LDS by every workgroup and searched there; a larger group is searched in global memory, where the upper
// levels of every search stay in the cache (DESIGN.md 3.20 has the sizes both were tested at).
// Shapes without a multi-query form (f16 / bf16, long rows): one single label-set scan per query (vg_rowpred.hip) in that same
// order, the bitmap rebuilt only where the set changes.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

#define VG_LSET_GROUP 32
#define VG_LSET_LDS_MAX 8192
static_assert(VG_LSET_GROUP == 32, "a membership word is a dword");

// d_member[row] for one group.  `grp`: [nd + 1 offsets | nd query masks | sets], `total` = offsets[nd] labels in the sets.  One
// thread a row, grid-stride; per distinct set one binary search (the first element >= the label), and the set's query mask is OR-ed
// in when the label was found - with `exclude`, when it was not.  IN_LDS: the whole of `grp` is copied into LDS first.
template <bool IN_LDS>
__global__ __launch_bounds__(256) void vg_labelset_member_kernel(const uint32_t *labels, long long n_rows, const uint32_t *grp, int nd, int total,
                                                                  int exclude, uint32_t *member) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t *g = grp;
    if constexpr (IN_LDS) {
        const int words = 2 * nd + 1 + total;
        for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = grp[i];
        __syncthreads();
        g = lds;
    }
    const uint32_t *off = g, *qmask = g + nd + 1, *sets = g + 2 * nd + 1;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += stride) {
        const uint32_t lab = labels[row];
        uint32_t word = 0u;
        if (lab != VG_MQ_LABEL_NONE) {
            for (int d = 0; d < nd; ++d) {
                uint32_t lo = off[d];
                const uint32_t end = off[d + 1];
                uint32_t hi = end;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sets[mid] < lab) lo = mid + 1; else hi = mid;
                }
                const bool found = lo < end && sets[lo] == lab;
                if (found != (exclude != 0)) word |= qmask[d];
            }
        }
        member[row] = word;
    }
}

int vg_member_reserve(vg_corpus *c) {
    if (c->member_cap < c->n_rows) {
        if (c->d_member) { hipFree(c->d_member); c->d_member = nullptr; c->member_cap = 0; }
        HIP_TRY(hipMalloc(&c->d_member, (size_t)c->n_rows * sizeof(uint32_t)));
        c->member_cap = c->n_rows;
    }
    return VG_OK;
}

int vg_labelset_member_enqueue(vg_corpus *c, size_t at, int nd, size_t total, int exclude) {
    int rcm = vg_member_reserve(c);
    if (rcm != VG_OK) return rcm;
    const long long blocks = std::min<long long>((c->n_rows + 255) / 256, 2048);
    const bool in_lds = total <= VG_LSET_LDS_MAX;
    const size_t smem = in_lds ? (size_t)(2 * nd + 1 + total) * sizeof(uint32_t) : 0;
    hipLaunchKernelGGL(in_lds ? vg_labelset_member_kernel<true> : vg_labelset_member_kernel<false>, dim3((unsigned)blocks), dim3(256), smem, c->stream,
                       (const uint32_t *)c->d_labels, (long long)c->n_rows, (const uint32_t *)c->d_lset + at, nd, (int)total, exclude ? 1 : 0,
                       c->d_member);
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// ---- the label-set batch as a membership form of vg_fused_batch_run (VgMemberForm, vg_internal.h; ctx: a VgLabelsetBatch)

// the DISTINCT sets of queries [g0, g1) - equal sets are neighbours: [nd + 1 offsets | nd query masks | the sets]
static int labelset_pack_group(const void *ctx, const char *who, int g0, int g1, std::vector<uint32_t> *data, int *nd, size_t *total) {
    const VgLabelsetBatch *lsets = (const VgLabelsetBatch *)ctx;
    std::vector<uint32_t> off(1, 0u), qmask, sets;
    for (int i = g0; i < g1; ++i) {
        const uint32_t *si = lsets->flat + lsets->offsets[i];
        const size_t ni = (size_t)(lsets->offsets[i + 1] - lsets->offsets[i]);
        const size_t np = i > g0 ? (size_t)(lsets->offsets[i] - lsets->offsets[i - 1]) : 0;
        if (i > g0 && ni == np && std::equal(si, si + ni, lsets->flat + lsets->offsets[i - 1])) { qmask.back() |= 1u << (i - g0); continue; }
        sets.insert(sets.end(), si, si + ni);
        if (sets.size() > 0x7FFFFFFFull) return vg_fail(VG_ERR_UNSUPPORTED, "%s: the sets of 32 queries hold more than 2^31 - 1 labels", who);
        off.push_back((uint32_t)sets.size());
        qmask.push_back(1u << (i - g0));
    }
    *nd = (int)qmask.size();
    *total = sets.size();
    data->insert(data->end(), off.begin(), off.end());
    data->insert(data->end(), qmask.begin(), qmask.end());
    data->insert(data->end(), sets.begin(), sets.end());
    return VG_OK;
}

static int labelset_member_step(vg_corpus *c, const void *ctx, size_t at, int nd, size_t total) {
    return vg_labelset_member_enqueue(c, at, nd, total, ((const VgLabelsetBatch *)ctx)->exclude);
}

// the fallback: one bitmap per run of equal sets; an empty allowed set has no rows - no launch, count 0
static int labelset_bits_step(vg_corpus *c, const void *ctx, int i, bool *skip) {
    const VgLabelsetBatch *lsets = (const VgLabelsetBatch *)ctx;
    const uint32_t *si = lsets->flat + lsets->offsets[i];
    const int64_t ni = lsets->offsets[i + 1] - lsets->offsets[i];
    if (ni == 0 && !lsets->exclude) { *skip = true; return VG_OK; }
    const int64_t np = i > 0 ? lsets->offsets[i] - lsets->offsets[i - 1] : -1;
    if (ni != np || !std::equal(si, si + ni, lsets->flat + lsets->offsets[i - 1])) return vg_pred_bits_enqueue(c, vg_pred_labelset(si, ni, lsets->exclude));
    return VG_OK;
}

static scan_fn_t pick_multi_labelset(int vtype, int acc, int U, int NQ) { return vg_pick_multi<MultiFamily<VG_MQ_LABELSET>>(vtype, acc, U, NQ); }
// the same table as a plain function: the valued batch (vg_multi_valued.hip) runs these instances over its own membership dwords
scan_fn_t vg_pick_multi_labelset(int vtype, int acc, int U, int NQ) { return pick_multi_labelset(vtype, acc, U, NQ); }

extern "C" int vg_batch_labelset_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, pick_multi_labelset, out_queries_per_pass, out_lpr, out_u);
}

extern "C" int vg_scan_topk_batch_labelset_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                                const int64_t *set_offsets, int exclude, uint64_t *out_keys, int *out_counts) {
    const VgFusedBatchForm form = {"vg_scan_topk_batch_labelset", pick_multi_labelset, VG_QROWS_MEMBER,
                                   vg_pred_form("vg_scan_topk_labelset", vg_pred_labelset(nullptr, 0, exclude), vg_result_plain())};
    if (!c || !queries || !out_counts || !set_offsets) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", form.who);
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", form.who);
    if (k > VG_MAX_FUSED_K) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (label-set scans use the fused list only)", form.who, VG_MAX_FUSED_K);
    if (set_offsets[0] < 0) return vg_fail(VG_ERR_INVALID, "%s: set_offsets[0] is negative", form.who);
    for (int i = 0; i < nq; ++i)
        if (set_offsets[i + 1] < set_offsets[i]) return vg_fail(VG_ERR_INVALID, "%s: set_offsets decrease at query %d", form.who, i);
    if (set_offsets[nq] > set_offsets[0] && !set_labels) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", form.who);
    // every query's set, normalised; then the queries in set order (stable: equal sets keep caller order)
    std::vector<std::vector<uint32_t>> sets((size_t)nq);
    for (int i = 0; i < nq; ++i)
        if (!vg_labelset_normalise(form.who, set_labels + set_offsets[i], set_offsets[i + 1] - set_offsets[i], &sets[(size_t)i])) return VG_ERR_INVALID;
    const std::vector<int> order = vg_stable_order(nq, [&](int x, int y) { return sets[(size_t)x] < sets[(size_t)y]; });
    std::vector<uint32_t> flat;
    std::vector<int64_t> offs((size_t)nq + 1, 0);
    for (int i = 0; i < nq; ++i) {
        const std::vector<uint32_t> &s = sets[(size_t)order[(size_t)i]];
        flat.insert(flat.end(), s.begin(), s.end());
        offs[(size_t)i + 1] = (int64_t)flat.size();
    }
    const VgLabelsetBatch ls = {flat.data(), offs.data(), exclude ? 1 : 0};
    const VgMemberForm member = {&ls, labelset_pack_group, labelset_member_step, labelset_bits_step};
    return vg_ordered_batch(c, queries, nq, k, order, out_keys, out_counts, [&](const void *sq, uint64_t *skeys, int *scounts) {
        return vg_fused_batch_run(c, form, metric, sq, nq, k, nullptr, skeys, scounts, nullptr, nullptr, &member);
    });
}

extern "C" int vg_scan_topk_batch_labelset(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                           const int64_t *set_offsets, int exclude, int64_t *out_rowids, double *out_dist, int *out_counts) {
    return vg_batch_rows_from_keys(c, "vg_scan_topk_batch_labelset", !c || !queries || !out_counts || !set_offsets, nq, k,
                                   k >= 1 && k <= VG_MAX_FUSED_K, false, out_rowids, out_dist, nullptr, out_counts, [&](uint64_t *keys, uint32_t *) {
        return vg_scan_topk_batch_labelset_keys(c, metric, queries, nq, k, set_labels, set_offsets, exclude, keys, out_counts);
    });
}
