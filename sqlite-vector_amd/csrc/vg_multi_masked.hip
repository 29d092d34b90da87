// vg_multi_masked.hip - masked batch scans: the k nearest ALLOWED rows for many queries (vg_scan_topk_batch_masked, include/vectorgpu.h).
// Also the home of vg_fused_batch_run, the form-driven batch routine the paged batch scans (vg_multi_after.hip) share with it: the
// fused_* / launch_fused_* routines below serve every VgFusedBatchForm, masked or not.
//
// Host side of the masked form of the multi-query scan (vg_scan_multi.h, VG_MQ_MASKED): kernel table, launch, and the batch entry points.  The plan is
// the multi-query scan's (vg_multi_plan: 4 queries per pass with up to 3 chunks per lane, 2 with 4 or 6; f32 / uint8 / int8 rows that
// fit the register-resident shapes); a pass reads the batches of rows that hold an allowed row, once, for all its queries.  Shapes
// without a multi-query form (f16 / bf16, long rows) are answered by nq single masked scans (vg_scan_masked.hip): same contract, no
// sharing.  A translation unit of its own, like vg_multi.hip: its kernel instances compile next to the others, not after them.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// (queries per pass, launch shape, kernel) of the masked multi-query scan; 0 queries per pass: the fallback serves the shape
static int fused_multi_plan(const vg_corpus *c, int metric, VgShape *s, scan_fn_t *fn, vg_pick_multi_fn_t pick = vg_pick_multi<MultiFamily<VG_MQ_MASKED>>) {
    const int NQ = vg_multi_plan(c, metric, s);
    if (NQ == 0) return 0;
    scan_fn_t f = pick(c->vtype, vg_metric_to_acc(metric), s->U, NQ);
    if (fn) *fn = f;
    return f ? NQ : 0;
}

int vg_batch_plan_report(const vg_corpus *c, int metric, vg_pick_multi_fn_t pick, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    if (int rcm = vg_metric_check(c->vtype, metric, "batch plan")) return rcm;
    VgShape s{};
    const int NQ = fused_multi_plan(c, metric, &s, nullptr, pick);
    if (NQ == 0) vg_plain_scan_shape(c, metric, &s);          // the fallback's shape: the form's single scan has the plain scan's
    if (out_queries_per_pass) *out_queries_per_pass = NQ;
    if (out_lpr) *out_lpr = s.long_rows ? VG_WAVE : (1 << s.lpr_log2);
    if (out_u) *out_u = s.long_rows ? 0 : s.U;
    return VG_OK;
}

extern "C" int vg_batch_masked_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return vg_batch_plan_report(c, metric, vg_pick_multi<MultiFamily<VG_MQ_MASKED>>, out_queries_per_pass, out_lpr, out_u);
}

// NQ queries (zero-padded rows of the corpus stride, back to back at dev_queries) against the allowed rows in ONE pass; dev_cand:
// NQ * (<= 256) * 64 keys of scratch; dev_out_keys: NQ x 64 keys.  Asynchronous on the corpus stream.  One launcher for every form
// (VgFusedBatchForm, vg_internal.h): the masked batch, and the paged batches of vg_multi_after.hip (dev_floors: NQ keys).
// A grouped form (vg_multi_grouped.hip): the lists merge through the label-deduping merge and dev_out_keys receives, per query, 64
// keys followed by their 64 labels (VG_KEYS_BYTES).  A capped form (vg_multi_capped.hip): the cap, clamped to k, travels in
// ScanArgs.within_cap - which no other top-k instance reads - and the lists merge through the capped batch merge; everything else
// is the grouped form's.  A membership form (VG_QROWS_MEMBER: vg_multi_labelset.hip, vg_multi_valued.hip): ScanArgs.labels is the
// membership buffer of the pass' group and `member_shift`, the pass' bit offset inside that group, travels in ScanArgs.within_cap.
static int launch_fused_multi(vg_corpus *c, const VgFusedBatchForm &f, int metric, scan_fn_t fn, int NQ, const VgShape &s,
                               const uint8_t *dev_queries, const uint64_t *dev_floors, const uint32_t *dev_qlabels, int k, uint64_t *dev_cand,
                               uint64_t *dev_out_keys, int member_shift = 0) {
    const long long blocks = vg_percu_scan_blocks(c, c->n_rows, s);
    ScanArgs a = vg_scan_args(c, metric, vg_metric_to_acc(metric), s, dev_queries, k);
    a.cand = dev_cand;
    const VgResult &res = f.single.result;
    if (f.rows == VG_QROWS_MASK) a.mask = c->d_mask;
    if (f.single.after) a.floor = dev_floors;
    if (f.rows == VG_QROWS_LABEL) { a.labels = c->d_labels; a.qlabels = dev_qlabels; }
    if (f.rows == VG_QROWS_MEMBER) { a.labels = c->d_member; a.within_cap = (unsigned long long)member_shift; }
    if (res.with_labels()) a.labels = c->d_labels;
    const int cap = res.kind == VG_RESULT_CAPPED ? std::min(res.per_label, k) : 0;   // (more than k of one label cannot be returned)
    if (cap > 0) a.within_cap = (unsigned long long)cap;
    const size_t smem = std::max<size_t>((size_t)NQ * c->nch * 16, (size_t)VG_PUBLISH_LDS_BYTES);
    hipEvent_t *evs = vg_prof_slot(c, VG_EVF_MERGE);          // one slot of the profiling ring per pass
    if (evs) hipEventRecord(evs[0], c->stream);
    int rc = vg_launch_scan_kernel(fn, blocks, smem, c->stream, a);
    if (rc != VG_OK) return rc;
    if (evs) hipEventRecord(evs[2], c->stream);
    rc = cap > 0          ? vg_launch_merge_capped_batch(dev_cand, (int)blocks, k, cap, c->d_labels, dev_out_keys, NQ, c->stream)
         : res.with_labels() ? vg_launch_merge_grouped_batch(dev_cand, (int)blocks, k, c->d_labels, dev_out_keys, NQ, c->stream)
                             : vg_launch_merge(dev_cand, (int)blocks, k, dev_out_keys, NQ, c->stream);
    if (evs) hipEventRecord(evs[3], c->stream);
    if (rc != 0) return vg_fail(VG_ERR_HIP, "%s: merge launch failed: %s", f.who, hipGetErrorString((hipError_t)rc));
    HIP_TRY(hipGetLastError());
    return VG_OK;
}

// queries go up in slices of this many (a multiple of every queries-per-pass): the device staging area does not grow with the batch
#define VG_FUSED_SLICE 256
// a label-set form: queries per membership word (vg_multi_labelset.hip) - a multiple of every queries-per-pass, and it divides a slice
#define VG_MEMBER_GROUP 32
static_assert(VG_FUSED_SLICE % VG_MEMBER_GROUP == 0, "a slice is whole membership groups");

// nq queries, NQ per pass; every pass of every slice is enqueued back to back on the corpus stream, one wait at the end
static int fused_batch_multi(vg_corpus *c, const VgFusedBatchForm &f, int metric, scan_fn_t fn, int NQ, const VgShape &s, const void *queries,
                              int nq, const uint64_t *floors, const uint32_t *qlabels, int k, uint64_t *out_keys, int *out_counts,
                              uint32_t *out_labels, const VgMemberForm *member) {
    const int ngroups = (nq + NQ - 1) / NQ, nq_pad = ngroups * NQ;
    const int slice = std::min(nq_pad, VG_FUSED_SLICE);
    const bool qlab = f.rows == VG_QROWS_LABEL, members = f.rows == VG_QROWS_MEMBER, grouped = f.single.result.with_labels();   // qlab: a label per query goes up with the queries
    // (a membership form: the table of every membership group of VG_MEMBER_GROUP queries - its DISTINCT conditions, equal ones are
    //  neighbours - goes up once, in front of everything; the form packs it (VgMemberForm.pack_group).  A pad query is in no mask)
    struct MemberGroup { size_t at; int nd; size_t total; };
    std::vector<MemberGroup> mgroups;
    std::vector<uint32_t> mdata;
    if (members) {
        for (int g0 = 0; g0 < nq; g0 += VG_MEMBER_GROUP) {
            MemberGroup mg{mdata.size(), 0, 0};
            int rcp = member->pack_group(member->ctx, f.who, g0, std::min(nq, g0 + VG_MEMBER_GROUP), &mdata, &mg.nd, &mg.total);
            if (rcp != VG_OK) return rcp;
            mgroups.push_back(mg);
        }
        int rcl = vg_lset_reserve(c, mdata.size() * sizeof(uint32_t));
        if (rcl != VG_OK) return rcl;
    }
    // (an after form: the slice's floor keys sit behind its queries in d_bq and go up with them; a pad slot admits nothing.  A labeled
    //  form: the slice's query labels, behind those; a pad slot carries VG_LABEL_NONE and matches nothing)
    const size_t fl_off = (size_t)slice * c->stride;
    const size_t lb_off = fl_off + (f.single.after ? (size_t)slice * sizeof(uint64_t) : 0);
    // (a grouped form: a query's 64 keys are followed by their 64 labels, so its pitch in d_bkeys is VG_KEYS_BYTES)
    const size_t kpitch = grouped ? VG_KEYS_BYTES / sizeof(uint64_t) : 64;
    const size_t qbytes = lb_off + (qlab ? (size_t)slice * sizeof(uint32_t) : 0), keybytes = (size_t)nq_pad * kpitch * sizeof(uint64_t);
    VG_TRY(vg_dev_reserve(&c->d_bq, &c->bq_bytes, qbytes));
    VG_TRY(vg_dev_reserve(&c->d_bkeys, &c->bkeys_bytes, keybytes));
    // zero-padded rows of the corpus stride; pad queries are zero.  The whole batch stays on the host until the wait: a slice's copy
    // is ordered behind the passes of the slice in front of it by the stream, its source must not move before it ran
    std::vector<uint8_t> hq((size_t)nq_pad * c->stride, 0);
    const size_t row_bytes = (size_t)c->dim * c->es;
    for (int i = 0; i < nq; ++i) memcpy(hq.data() + (size_t)i * c->stride, (const uint8_t *)queries + (size_t)i * row_bytes, row_bytes);
    std::vector<uint64_t> hf(f.single.after ? (size_t)nq_pad : 0, VG_KEY_EMPTY);
    if (f.single.after) for (int i = 0; i < nq; ++i) hf[(size_t)i] = floors[i];
    std::vector<uint32_t> hl(qlab ? (size_t)nq_pad : 0, VG_LABEL_NONE);
    if (qlab) for (int i = 0; i < nq; ++i) hl[(size_t)i] = qlabels[i];
    int rc = VG_OK;
    if (members) {                                                    // (mdata, like hq, stays where it is until the wait)
        hipError_t e = hipMemcpyAsync(c->d_lset, mdata.data(), mdata.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) rc = vg_fail(VG_ERR_HIP, "%s: label-set upload failed: %s", f.who, hipGetErrorString(e));
    }
    for (int q0 = 0; q0 < nq_pad && rc == VG_OK; q0 += slice) {
        const int nqs = std::min(slice, nq_pad - q0);
        hipError_t e = hipMemcpyAsync(c->d_bq, hq.data() + (size_t)q0 * c->stride, (size_t)nqs * c->stride, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && f.single.after)
            e = hipMemcpyAsync((uint8_t *)c->d_bq + fl_off, hf.data() + q0, (size_t)nqs * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && qlab)
            e = hipMemcpyAsync((uint8_t *)c->d_bq + lb_off, hl.data() + q0, (size_t)nqs * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) { rc = vg_fail(VG_ERR_HIP, "%s: query upload failed: %s", f.who, hipGetErrorString(e)); break; }
        for (int g = 0; g < nqs && rc == VG_OK; g += NQ) {
            // (a label-set form: the first pass of a membership group is preceded by the group's pre-pass; a slice is whole groups)
            if (members && (q0 + g) % VG_MEMBER_GROUP == 0) {
                const MemberGroup &mg = mgroups[(size_t)((q0 + g) / VG_MEMBER_GROUP)];
                if ((rc = member->member_enqueue(c, member->ctx, mg.at, mg.nd, mg.total)) != VG_OK) break;
            }
            rc = launch_fused_multi(c, f, metric, fn, NQ, s, (const uint8_t *)c->d_bq + (size_t)g * c->stride,
                                     reinterpret_cast<const uint64_t *>((const uint8_t *)c->d_bq + fl_off) + g,
                                     reinterpret_cast<const uint32_t *>((const uint8_t *)c->d_bq + lb_off) + g, k, c->d_cand,
                                     c->d_bkeys + (size_t)(q0 + g) * kpitch, (q0 + g) % VG_MEMBER_GROUP);
        }
    }
    if (rc != VG_OK) { hipStreamSynchronize(c->stream); return rc; }      // (hq must outlive what was enqueued)
    std::vector<uint64_t> keys((size_t)nq * kpitch);
    hipError_t e = hipMemcpyAsync(keys.data(), c->d_bkeys, (size_t)nq * kpitch * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess)
        return vg_fail(VG_ERR_HIP, "%s: %s", f.who, hipGetErrorString(e != hipSuccess ? e : e2));
    vg_collect_timing(c);
    for (int i = 0; i < nq; ++i) {
        int cnt = 0;
        for (int j = 0; j < k; ++j) {
            const uint64_t key = keys[(size_t)i * kpitch + j];
            if (key == VG_KEY_EMPTY) break;
            out_keys[(size_t)i * k + cnt] = key;
            if (grouped) out_labels[(size_t)i * k + cnt] = reinterpret_cast<const uint32_t *>(&keys[(size_t)i * kpitch + 64])[j];
            ++cnt;
        }
        out_counts[i] = cnt;
    }
    return VG_OK;
}

// packed keys (distance image << 32 | position local to this corpus), ascending, nq x k: the form a multi-shard caller merges.
// Slots behind out_counts[i] are not written.  `floors`: a key per query, read by an after form only.  `out_labels` (nq x k): the
// winners' labels, filled by a grouped form only.
int vg_fused_batch_run(vg_corpus *c, const VgFusedBatchForm &f, int metric, const void *queries, int nq, int k, const uint64_t *floors,
                       uint64_t *out_keys, int *out_counts, const uint32_t *qlabels, uint32_t *out_labels, const VgMemberForm *member) {
    const bool grouped = f.single.result.with_labels();
    if (!c || !queries || !out_counts || (f.single.after && !floors) || (f.rows == VG_QROWS_LABEL && !qlabels) ||
        (f.rows == VG_QROWS_MEMBER && !member)) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", f.who);
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", f.who);
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    if (k < 1) return vg_fail(VG_ERR_INVALID, "%s: k must be at least 1", f.who);
    if (k > VG_MAX_FUSED_K) return vg_fail(VG_ERR_UNSUPPORTED, "%s: k must be in 1..%d (%s scans use the fused list only)", f.who, VG_MAX_FUSED_K, f.single.noun);
    if (!out_keys || (grouped && !out_labels)) return vg_fail(VG_ERR_INVALID, "%s: NULL output", f.who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (f.rows == VG_QROWS_MASK && c->mask_count < 0) return vg_fail(VG_ERR_INVALID, "%s: no row mask set", f.who);
    if (f.single.needs_values && !c->has_values) return vg_fail(VG_ERR_INVALID, "%s: no values set", f.who);
    if (f.single.needs_labels && !c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", f.who);
    for (int i = 0; i < nq && f.rows == VG_QROWS_LABEL; ++i)
        if (qlabels[i] == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: query %d: VG_LABEL_NONE names no row", f.who, i);
    if (int rcm = vg_metric_check(c->vtype, metric, f.who)) return rcm;
    if ((f.rows == VG_QROWS_MASK && c->mask_count == 0) || c->n_rows == 0) return VG_OK;      // an empty mask: no launch
    HIP_TRY(hipSetDevice(c->device));
    VgShape s{};
    scan_fn_t fn = nullptr;
    const int NQ = fused_multi_plan(c, metric, &s, &fn, f.pick);
    if (NQ == 0) {                                               // no multi-query form: the single scans of the form, one by one
        const size_t row_bytes = (size_t)c->dim * c->es;
        for (int i = 0; i < nq; ++i) {
            // (a labeled form: the bitmap of a label is built once and serves the run of queries that share it)
            if (f.rows == VG_QROWS_LABEL && (i == 0 || qlabels[i] != qlabels[i - 1])) {
                int rcb = vg_pred_bits_enqueue(c, vg_pred_label(qlabels[i]));
                if (rcb != VG_OK) return rcb;
            }
            // (a membership form: the same per run of equal conditions; a condition that allows no row at all - no launch, count 0)
            if (f.rows == VG_QROWS_MEMBER) {
                bool skip = false;
                int rcb = member->bits_enqueue(c, member->ctx, i, &skip);
                if (rcb != VG_OK) return rcb;
                if (skip) continue;
            }
            int rc = vg_fused_run(c, f.single, metric, (const uint8_t *)queries + (size_t)i * row_bytes, k, floors ? floors[i] : 0ull,
                                  out_keys + (size_t)i * k, &out_counts[i], grouped ? out_labels + (size_t)i * k : nullptr);
            if (rc != VG_OK) return rc;
        }
        return VG_OK;
    }
    return fused_batch_multi(c, f, metric, fn, NQ, s, queries, nq, floors, qlabels, k, out_keys, out_counts, out_labels, member);
}

extern "C" int vg_scan_topk_batch_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, uint64_t *out_keys,
                                              int *out_counts) {
    const VgFusedBatchForm form = {"vg_scan_topk_batch_masked", vg_pick_multi<MultiFamily<VG_MQ_MASKED>>, VG_QROWS_MASK,
                                   vg_fused_form("vg_scan_topk_masked", "masked", vg_pick_scan_masked, VG_ROWS_MASK)};
    return vg_fused_batch_run(c, form, metric, queries, nq, k, nullptr, out_keys, out_counts);
}

extern "C" int vg_scan_topk_batch_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, int64_t *out_rowids,
                                         double *out_dist, int *out_counts) {
    return vg_batch_rows_from_keys(c, "vg_scan_topk_batch_masked", !c || !queries || !out_counts, nq, k, k >= 1 && k <= VG_MAX_FUSED_K, false,
                                   out_rowids, out_dist, nullptr, out_counts, [&](uint64_t *keys, uint32_t *) {
        return vg_scan_topk_batch_masked_keys(c, metric, queries, nq, k, keys, out_counts);
    });
}
