// vg_multi_within.hip - batch range scans: every row within a radius, for many queries with a radius each (vg_scan_within_batch,
// include/vectorgpu.h).
//
// Host side of the range form of the multi-query scan (vg_scan_multi.h, VG_MQ_WITHIN): kernel table, launch, the overflow protocol and the entry points.
// The plan is the multi-query scan's (vg_multi_plan: 4 queries per pass with up to 3 chunks per lane, 2 with 4 or 6; f32 / uint8 /
// int8 rows that fit the register-resident shapes).  Shapes without a multi-query form (f16 / bf16, long rows) are answered by nq
// single range scans (vg_scan_within.hip): same contract, no sharing.
//
// Queries go up in slices; a slice's staging area holds, per pass, [NQ queries | NQ descriptors], and its key regions - [count | cap
// keys] per query, one pitch - share one fixed budget of keys, so neither grows with nq.  All passes of a slice are enqueued back to
// back; the counts are gathered by one small kernel and come back in one copy behind one wait.  A count past its capacity IS the size
// needed: that pass - and only that pass - runs once more as a whole into regions of the counted sizes; a partial answer is never
// returned.  From the counted keys of a query on - sorted, cut to `limit`, held, read - the result path is the single range scan's
// (vg_scan_within.hip: vg_within_collect / _finish / _held_*); the batch's held results stay apart from the single scan's on a handle.
//
// The masked batch (vg_scan_within_batch_masked) is the same host code: its kernels are the VG_MQ_WITHIN | VG_MQ_MASKED instances, held by
// vg_multi_within_masked.hip, its launches set ScanArgs.mask, its fallback is nq single MASKED range scans - nothing else differs, and
// it leaves its held results where the unmasked batch leaves its own.
//
// The labeled batch (vg_scan_within_batch_labeled: each query its own label and its own radius) is the same host code once more: its
// kernels are the VG_MQ_LABELED | VG_MQ_WITHIN instances, held by vg_multi_within_labeled.hip, its launches set ScanArgs.labels and
// every query's label travels in its descriptor, its fallback is nq single labeled range scans (vg_rowpred.hip).  What is
// its own is the entry point's: the queries are ordered by label (stable) before they are cut into passes, as in vg_multi_labeled.hip
// - a pass' queries then share as few distinct labels as possible, which is what lets a pass skip the batches of rows that carry none
// of them - and the held results are put back at the caller's indices.
#include "vg_internal.h"

#include "vg_scan_multi.h"
#include "vg_pick.h"

// what differs between the unmasked, the masked and the labeled batch: whose name errors carry, and whether the launches read the
// handle's mask or its labels (then every query names one).  No membership form
struct WbForm { const char *who; VgBatchRows rows; };

// (queries per pass, launch shape, kernel) of the multi-query range scan, unmasked, masked or labeled; 0 queries per pass: the fallback
// serves the shape.  Every instance of the three tables compiles without scratch or spills: the masked and
// the labeled plan are the unmasked one.
static int mw_plan(const vg_corpus *c, int metric, const WbForm &form, VgShape *s, scan_fn_t *fn) {
    const int NQ = vg_multi_plan(c, metric, s);
    if (NQ == 0) return 0;
    const int acc = vg_metric_to_acc(metric);
    scan_fn_t f = form.rows == VG_QROWS_LABEL  ? vg_pick_multi_within_labeled(c->vtype, acc, s->U, NQ)
                  : form.rows == VG_QROWS_MASK ? vg_pick_multi_within_masked(c->vtype, acc, s->U, NQ)
                                               : vg_pick_multi<MultiFamily<VG_MQ_WITHIN>>(c->vtype, acc, s->U, NQ);
    if (fn) *fn = f;
    return f ? NQ : 0;
}

static int within_batch_plan(const vg_corpus *c, int metric, const WbForm &form, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    if (int rcm = vg_metric_check(c->vtype, metric, form.who)) return rcm;
    VgShape s{};
    const int NQ = mw_plan(c, metric, form, &s, nullptr);
    if (NQ == 0) vg_plain_scan_shape(c, metric, &s);          // the fallback's shape: the single range scan's
    if (out_queries_per_pass) *out_queries_per_pass = NQ;
    if (out_lpr) *out_lpr = s.long_rows ? VG_WAVE : (1 << s.lpr_log2);
    if (out_u) *out_u = s.long_rows ? 0 : s.U;
    return VG_OK;
}
extern "C" int vg_within_batch_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return within_batch_plan(c, metric, WbForm{"vg_within_batch_plan", VG_QROWS_ALL}, out_queries_per_pass, out_lpr, out_u);
}
extern "C" int vg_within_batch_masked_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return within_batch_plan(c, metric, WbForm{"vg_within_batch_masked_plan", VG_QROWS_MASK}, out_queries_per_pass, out_lpr, out_u);
}
extern "C" int vg_within_batch_labeled_plan(const vg_corpus *c, int metric, int *out_queries_per_pass, int *out_lpr, int *out_u) {
    return within_batch_plan(c, metric, WbForm{"vg_within_batch_labeled_plan", VG_QROWS_LABEL}, out_queries_per_pass, out_lpr, out_u);
}

// queries go up in slices of this many (a multiple of every queries-per-pass): staging and key regions do not grow with the batch
#define VG_WB_SLICE 256
#define VG_WB_MIN_CAP 1024            // the floor of a query's share of VG_WITHIN_INITIAL_CAP keys

// the first word of n regions `pitch` words apart: zeroed (dst == nullptr) or gathered into dst
__global__ void vg_wb_counts_kernel(unsigned long long *regions, long long pitch, int n, unsigned long long *dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dst) dst[i] = regions[(long long)i * pitch];
    else regions[(long long)i * pitch] = 0ull;
}

// one pass: NQ queries + their descriptors at dev_block.  Asynchronous on the corpus stream.
static int launch_multi_within(vg_corpus *c, const WbForm &f, int metric, scan_fn_t fn, int NQ, const VgShape &s, const uint8_t *dev_block) {
    const long long blocks = vg_percu_scan_blocks(c, c->n_rows, s);      // the multi-query scan's launch shape
    ScanArgs a = vg_scan_args(c, metric, vg_metric_to_acc(metric), s, dev_block, 0);
    if (f.rows == VG_QROWS_MASK) a.mask = c->d_mask;
    if (f.rows == VG_QROWS_LABEL) a.labels = c->d_labels;                     // (the queries' labels are in their descriptors)
    a.store_lds_off = (int)(((size_t)NQ * c->nch * 16 + 255) / 256 * 256);     // the key queues behind the staged queries
    const size_t smem = (size_t)a.store_lds_off + (size_t)NQ * VG_WITHIN_LDS_BYTES;
    hipEvent_t *evs = vg_prof_slot(c, 0);                      // one slot of the profiling ring per pass
    if (evs) hipEventRecord(evs[0], c->stream);
    int rc = vg_launch_scan_kernel(fn, blocks, smem, c->stream, a);
    if (rc != VG_OK) return rc;
    if (evs) { hipEventRecord(evs[2], c->stream); hipEventRecord(evs[3], c->stream); }
    HIP_TRY(hipGetLastError());
    ++c->wb_launches;
    return VG_OK;
}

// `count` keys at dev_keys -> the held keys of query qi (vg_within_collect; the caller waits once for the small results of a slice)
static int collect_keys(vg_corpus *c, int qi, const unsigned long long *dev_keys, int64_t count, int64_t limit, bool *pending) {
    c->wb_matches[(size_t)qi] = count;
    return vg_within_collect(c, dev_keys, count, limit, &c->wb_keys[(size_t)qi], pending);
}

// nq queries, NQ per pass; qlabels: a label per query (the labeled form, nullptr otherwise)
static int batch_within_multi(vg_corpus *c, const WbForm &f, int metric, scan_fn_t fn, int NQ, const VgShape &s, const void *queries, int nq,
                              const double *radii, const uint32_t *qlabels, int64_t limit) {
    const int ngroups = (nq + NQ - 1) / NQ, nq_pad = ngroups * NQ;
    const int slice = std::min(nq_pad, VG_WB_SLICE);
    const size_t block_bytes = (size_t)NQ * c->stride + (size_t)NQ * sizeof(VgWithinQuery);      // one pass: [NQ queries | NQ descriptors]
    const size_t qbytes = (size_t)(slice / NQ) * block_bytes;
    VG_TRY(vg_dev_reserve(&c->d_bq, &c->bq_bytes, qbytes));
    if (!c->d_wb_counts) HIP_TRY(hipMalloc(&c->d_wb_counts, (size_t)VG_WB_SLICE * sizeof(unsigned long long)));
    if (!c->h_wb) HIP_TRY(hipHostMalloc(&c->h_wb, (size_t)(VG_WB_SLICE + 8) * sizeof(unsigned long long)));
    // zero-padded rows of the corpus stride; a pad query is zero with no capacity, a radius nothing is below and no label.  The whole batch stays
    // on the host until the last wait: a slice's copy is ordered behind the passes of the slice in front of it by the stream
    std::vector<uint8_t> hq((size_t)ngroups * block_bytes, 0);
    const size_t row_bytes = (size_t)c->dim * c->es;
    auto block_of = [&](int q) { return hq.data() + (size_t)(q / NQ) * block_bytes; };
    auto desc_of = [&](int q) { return reinterpret_cast<VgWithinQuery *>(block_of(q) + (size_t)NQ * c->stride) + (q % NQ); };
    for (int i = 0; i < nq; ++i) memcpy(block_of(i) + (size_t)(i % NQ) * c->stride, (const uint8_t *)queries + (size_t)i * row_bytes, row_bytes);
    uint8_t *d_stage = (uint8_t *)c->d_bq;

    for (int q0 = 0; q0 < nq_pad; q0 += slice) {
        const int nqs = std::min(slice, nq_pad - q0);
        // a query's share of the one key budget, never more than the rows there are
        int64_t cap = c->wb_cap_init > 0 ? c->wb_cap_init : std::max<int64_t>(VG_WB_MIN_CAP, (int64_t)VG_WITHIN_INITIAL_CAP / nqs);
        cap = std::max<int64_t>(1, std::min<int64_t>(cap, c->n_rows));
        const long long pitch = (long long)cap + 1;
        int rc = vg_dev_reserve(&c->d_wb, &c->wb_bytes, (size_t)nqs * (size_t)pitch * sizeof(unsigned long long));
        if (rc != VG_OK) return rc;
        for (int j = 0; j < nqs; ++j) {
            VgWithinQuery *d = desc_of(q0 + j);
            const bool real = q0 + j < nq;
            d->out = c->d_wb + (long long)j * pitch;
            d->cap = real ? (unsigned long long)cap : 0ull;
            d->r = real ? vg_within_radius(radii[q0 + j]) : -INFINITY;
            d->label = (real && f.rows == VG_QROWS_LABEL) ? qlabels[q0 + j] : VG_LABEL_NONE;
        }
        HIP_TRY(hipMemcpyAsync(d_stage, block_of(q0), (size_t)(nqs / NQ) * block_bytes, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(vg_wb_counts_kernel, dim3(1), dim3(VG_WB_SLICE), 0, c->stream, c->d_wb, pitch, nqs, (unsigned long long *)nullptr);
        for (int g = 0; g < nqs; g += NQ)
            if ((rc = launch_multi_within(c, f, metric, fn, NQ, s, d_stage + (size_t)(g / NQ) * block_bytes)) != VG_OK) { hipStreamSynchronize(c->stream); return rc; }
        hipLaunchKernelGGL(vg_wb_counts_kernel, dim3(1), dim3(VG_WB_SLICE), 0, c->stream, c->d_wb, pitch, nqs, c->d_wb_counts);
        hipError_t e = hipMemcpyAsync(c->h_wb, c->d_wb_counts, (size_t)nqs * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return vg_fail(VG_ERR_HIP, "%s: %s", f.who, hipGetErrorString(e != hipSuccess ? e : e2));
        std::vector<int64_t> counts((size_t)nqs);
        for (int j = 0; j < nqs; ++j) counts[(size_t)j] = (q0 + j < nq) ? (int64_t)c->h_wb[j] : 0;

        // the passes that fit: their keys leave first (nothing below touches d_wb)
        bool pending = false;
        for (int g = 0; g < nqs; g += NQ) {
            bool over = false;
            for (int n = 0; n < NQ; ++n) over = over || counts[(size_t)(g + n)] > cap;
            if (over) continue;
            for (int n = 0; n < NQ && q0 + g + n < nq; ++n)
                if ((rc = collect_keys(c, q0 + g + n, c->d_wb + (long long)(g + n) * pitch + 1, counts[(size_t)(g + n)], limit, &pending)) != VG_OK) return rc;
        }
        if (pending) HIP_TRY(hipStreamSynchronize(c->stream));
        // a pass with a query past its capacity: once more as a whole, counts reset, every region at its counted size
        for (int g = 0; g < nqs; g += NQ) {
            bool over = false;
            for (int n = 0; n < NQ; ++n) over = over || counts[(size_t)(g + n)] > cap;
            if (!over) continue;
            size_t words = 0;
            for (int n = 0; n < NQ; ++n) words += (size_t)counts[(size_t)(g + n)] + 1;
            if ((rc = vg_dev_reserve(&c->d_wb_grow, &c->wb_grow_bytes, words * sizeof(unsigned long long))) != VG_OK) return rc;
            size_t at = 0;
            for (int n = 0; n < NQ; ++n) {
                VgWithinQuery *d = desc_of(q0 + g + n);
                d->out = c->d_wb_grow + at;
                d->cap = (unsigned long long)counts[(size_t)(g + n)];
                HIP_TRY(hipMemsetAsync(d->out, 0, sizeof(unsigned long long), c->stream));
                at += (size_t)counts[(size_t)(g + n)] + 1;
            }
            uint8_t *d_block = d_stage + (size_t)(g / NQ) * block_bytes;
            HIP_TRY(hipMemcpyAsync(d_block + (size_t)NQ * c->stride, desc_of(q0 + g), (size_t)NQ * sizeof(VgWithinQuery), hipMemcpyHostToDevice, c->stream));
            if ((rc = launch_multi_within(c, f, metric, fn, NQ, s, d_block)) != VG_OK) { hipStreamSynchronize(c->stream); return rc; }
            for (int n = 0; n < NQ; ++n)
                HIP_TRY(hipMemcpyAsync(c->h_wb + VG_WB_SLICE + n, desc_of(q0 + g + n)->out, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            for (int n = 0; n < NQ && q0 + g + n < nq; ++n)
                if ((int64_t)c->h_wb[VG_WB_SLICE + n] != counts[(size_t)(g + n)])
                    return vg_fail(VG_ERR_HIP, "%s: two launches counted %lld and %lld rows for query %d", f.who, (long long)counts[(size_t)(g + n)],
                                   (long long)c->h_wb[VG_WB_SLICE + n], q0 + g + n);
            pending = false;
            for (int n = 0; n < NQ && q0 + g + n < nq; ++n)
                if ((rc = collect_keys(c, q0 + g + n, desc_of(q0 + g + n)->out + 1, counts[(size_t)(g + n)], limit, &pending)) != VG_OK) return rc;
            if (pending) HIP_TRY(hipStreamSynchronize(c->stream));          // (d_wb_grow serves the next such pass)
        }
        for (int j = 0; j < nqs && q0 + j < nq; ++j) vg_within_finish(&c->wb_keys[(size_t)(q0 + j)], c->wb_matches[(size_t)(q0 + j)], limit);
    }
    vg_collect_timing(c);
    return VG_OK;
}

static int within_batch(vg_corpus *c, const WbForm &f, int metric, const void *queries, int nq, const double *radii, const uint32_t *qlabels,
                        int64_t limit, int64_t *out_matches, int64_t *out_held) {
    for (int i = 0; i < nq; ++i) { if (out_matches) out_matches[i] = 0; if (out_held) out_held[i] = 0; }      // (every error leaves the counts zeroed)
    const bool masked = f.rows == VG_QROWS_MASK, labeled = f.rows == VG_QROWS_LABEL;
    if (!c || !queries || !radii || (labeled && !qlabels)) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", f.who);
    c->wb_keys.clear();
    c->wb_matches.clear();
    c->wb_launches = 0;
    if (nq < 1) return vg_fail(VG_ERR_INVALID, "%s: nq must be at least 1", f.who);
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    for (int i = 0; i < nq; ++i)
        if (radii[i] != radii[i]) return vg_fail(VG_ERR_INVALID, "%s: radius %d is NaN", f.who, i);
    if (masked && c->mask_count < 0) return vg_fail(VG_ERR_INVALID, "%s: no row mask set", f.who);
    if (labeled) {
        if (!c->has_labels) return vg_fail(VG_ERR_INVALID, "%s: no labels set", f.who);
        for (int i = 0; i < nq; ++i)
            if (qlabels[i] == VG_LABEL_NONE) return vg_fail(VG_ERR_INVALID, "%s: a query's label is VG_LABEL_NONE, which names no row", f.who);
    }
    if (int rcm = vg_metric_check(c->vtype, metric, f.who)) return rcm;
    c->wb_keys.resize((size_t)nq);
    c->wb_matches.assign((size_t)nq, 0);
    if (c->n_rows == 0 || (masked && c->mask_count == 0)) return VG_OK;      // nothing can match: no launch
    HIP_TRY(hipSetDevice(c->device));
    VgShape s{};
    scan_fn_t fn = nullptr;
    const int NQ = mw_plan(c, metric, f, &s, &fn);
    int rc = VG_OK;
    if (NQ == 0) {                                               // no multi-query form: the single range scans of the same form, one by one
        const size_t row_bytes = (size_t)c->dim * c->es;
        // (the single range scan keeps its own result apart: what the handle held for it is put back behind the loop)
        std::vector<uint64_t> single_keys;
        single_keys.swap(c->within_keys);
        const int64_t single_matches = c->within_matches;
        const int single_launches = c->within_launches;
        for (int i = 0; i < nq && rc == VG_OK; ++i) {
            int64_t m = 0, h = 0;
            const void *q = (const uint8_t *)queries + (size_t)i * row_bytes;
            rc = labeled  ? vg_scan_within_labeled(c, metric, q, radii[i], limit, qlabels[i], &m, &h)
                 : masked ? vg_scan_within_masked(c, metric, q, radii[i], limit, &m, &h)
                          : vg_scan_within(c, metric, q, radii[i], limit, &m, &h);
            if (rc != VG_OK) break;
            c->wb_keys[(size_t)i] = c->within_keys;
            c->wb_matches[(size_t)i] = m;
            c->wb_launches += c->within_launches;
        }
        c->within_keys.swap(single_keys);
        c->within_matches = single_matches;
        c->within_launches = single_launches;
    } else {
        rc = batch_within_multi(c, f, metric, fn, NQ, s, queries, nq, radii, qlabels, limit);
    }
    if (rc != VG_OK) { c->wb_keys.clear(); c->wb_matches.clear(); return rc; }
    for (int i = 0; i < nq; ++i) {
        if (out_matches) out_matches[i] = c->wb_matches[(size_t)i];
        if (out_held) out_held[i] = (int64_t)c->wb_keys[(size_t)i].size();
    }
    return VG_OK;
}

extern "C" int vg_scan_within_batch(vg_corpus *c, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                    int64_t *out_matches, int64_t *out_held) {
    return within_batch(c, WbForm{"vg_scan_within_batch", VG_QROWS_ALL}, metric, queries, nq, radii, nullptr, limit, out_matches, out_held);
}

extern "C" int vg_scan_within_batch_masked(vg_corpus *c, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                           int64_t *out_matches, int64_t *out_held) {
    return within_batch(c, WbForm{"vg_scan_within_batch_masked", VG_QROWS_MASK}, metric, queries, nq, radii, nullptr, limit, out_matches, out_held);
}

extern "C" int vg_scan_within_batch_labeled(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels,
                                            const double *radii, int64_t limit, int64_t *out_matches, int64_t *out_held) {
    const WbForm form = {"vg_scan_within_batch_labeled", VG_QROWS_LABEL};
    if (nq < 1 || !c || !queries || !radii || !query_labels)           // (nothing to order: the shared routine zeroes the counts and refuses)
        return within_batch(c, form, metric, queries, nq, radii, query_labels, limit, out_matches, out_held);
    // queries in label order (stable: equal labels keep caller order), their radii with them; everything else - argument checks
    // included - is the shared routine's
    const std::vector<int> order = vg_stable_order(nq, [&](int x, int y) { return query_labels[x] < query_labels[y]; });
    const std::vector<uint8_t> sq = vg_permute_queries(c, queries, order);
    std::vector<uint32_t> sl((size_t)nq);
    std::vector<double> sr((size_t)nq);
    for (int i = 0; i < nq; ++i) {
        const size_t src = (size_t)order[(size_t)i];
        sl[(size_t)i] = query_labels[src];
        sr[(size_t)i] = radii[src];
    }
    for (int i = 0; i < nq; ++i) { if (out_matches) out_matches[i] = 0; if (out_held) out_held[i] = 0; }
    int rc = within_batch(c, form, metric, sq.data(), nq, sr.data(), sl.data(), limit, nullptr, nullptr);
    if (rc != VG_OK) return rc;
    // held results and counts back at the caller's indices
    std::vector<std::vector<uint64_t>> keys((size_t)nq);
    std::vector<int64_t> matches((size_t)nq, 0);
    for (int i = 0; i < nq; ++i) {
        const size_t dst = (size_t)order[(size_t)i];
        keys[dst].swap(c->wb_keys[(size_t)i]);
        matches[dst] = c->wb_matches[(size_t)i];
    }
    c->wb_keys.swap(keys);
    c->wb_matches.swap(matches);
    for (int i = 0; i < nq; ++i) {
        if (out_matches) out_matches[i] = c->wb_matches[(size_t)i];
        if (out_held) out_held[i] = (int64_t)c->wb_keys[(size_t)i].size();
    }
    return VG_OK;
}

// the held keys of `query`, or nullptr (with the error set) when there is no such query
static const std::vector<uint64_t> *held_of(const vg_corpus *c, const char *who, int query) {
    if (query >= 0 && (size_t)query < c->wb_keys.size()) return &c->wb_keys[(size_t)query];
    vg_fail(VG_ERR_INVALID, "%s: query %d of %lld held", who, query, (long long)c->wb_keys.size());
    return nullptr;
}

extern "C" int vg_scan_within_batch_keys(const vg_corpus *c, int query, int64_t first, int64_t n, uint64_t *out_keys) {
    if (!c || (n > 0 && !out_keys)) return vg_fail(VG_ERR_INVALID, "vg_scan_within_batch_keys: NULL argument");
    const std::vector<uint64_t> *keys = held_of(c, "vg_scan_within_batch_keys", query);
    return keys ? vg_within_held_keys("vg_scan_within_batch_keys", *keys, first, n, out_keys) : VG_ERR_INVALID;
}

extern "C" int vg_scan_within_batch_fetch(const vg_corpus *c, int query, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist) {
    if (!c) return vg_fail(VG_ERR_INVALID, "vg_scan_within_batch_fetch: NULL argument");
    const std::vector<uint64_t> *keys = held_of(c, "vg_scan_within_batch_fetch", query);
    return keys ? vg_within_held_rows(c, "vg_scan_within_batch_fetch", *keys, first, n, out_rowids, out_dist) : VG_ERR_INVALID;
}

extern "C" int vg_within_batch_set_initial_capacity(vg_corpus *c, int64_t keys_per_query) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    c->wb_cap_init = keys_per_query > 0 ? keys_per_query : 0;
    return VG_OK;
}

extern "C" int vg_within_batch_last_launches(const vg_corpus *c) { return c ? c->wb_launches : 0; }
