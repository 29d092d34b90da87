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
// it leaves its held results where the unmasked batch leaves its own.  (Bit vectors of up to 128 bytes, 128 queries or more: the
// gathering matrix-core form below instead, within_bits_masked_eligible.)
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
#include "vg_batch_units.h"          // vg_batch_bits_within_launch, vg_batch_bits_within_masked_launch, vg_batch_bitsl_within_launch

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

// ---- packed bit vectors (uint8 corpora, Hamming / Jaccard), unmasked and unlabeled batches of VG_BATCH_BITS_MIN_QUERIES queries or more: the
// range forms of the matrix-core batch kernels.  Rows of 16 .. 128 bytes (vg_batch_bits_within.hip): a launch is one workgroup's 256
// queries against every row - the corpus is read once per 256 queries, not once per 4 - and a slice is one launch, so the staging
// area, the gathered counts and the overflow protocol above keep their sizes and their shape at the granularity of a launch.  Rows of
// 129 .. 512 bytes (vg_batch_bitsl_within.hip): a workgroup holds 128 (<= 256 bytes) or 64 queries; a slice is still 256 queries and one
// launch, of as many query groups as hold a real query - 1 to 2 of 128, 1 to 4 of 64.
#define VG_WITHIN_BITS_MIN_QUERIES_DEFAULT 256    // (0: never.  Measured, tools/bits_within_bench.py / DESIGN.md 3.27: at 64 queries the multi-query range scan still wins or ties cells)
// rows beyond 128 bytes, by K-split (0: never; measured).  Whatever the threshold - the switch included -, such a batch
// needs one full workgroup of real queries: a launch below that floor is more than half padding
#define VG_WITHIN_BITS_MIN_QUERIES_LONG2_DEFAULT 256   // strides 144 .. 256, 128 queries per workgroup: at 128 queries one (result-bound) cell stayed inside the spreads
#define VG_WITHIN_BITS_MIN_QUERIES_LONG4_DEFAULT 64    // strides 272 .. 512, 64 queries per workgroup: the floor wins every measured cell
static bool within_bits_eligible(const vg_corpus *c, int metric, int nq) {
    if (vg_sw(SW_VG_BATCH_MFMA, 1) == 0 || c->vtype != VG_TYPE_U8 || !vg_metric_is_bits(metric)) return false;
    if (c->stride <= 128) {
        const int min_q = vg_sw(SW_VG_BATCH_BITS_MIN_QUERIES, VG_WITHIN_BITS_MIN_QUERIES_DEFAULT);
        if (min_q <= 0 || nq < min_q) return false;
        return vg_batch_bits_within_lds_bytes(c->stride) != 0;
    }
    if (vg_batch_bitsl_within_lds_bytes(c->stride) == 0) return false;
    const int qpb = vg_batch_bitsl_within_queries_per_block(c->stride);
    const int min_q = vg_sw(SW_VG_BATCH_BITS_MIN_QUERIES, qpb == 128 ? VG_WITHIN_BITS_MIN_QUERIES_LONG2_DEFAULT : VG_WITHIN_BITS_MIN_QUERIES_LONG4_DEFAULT);
    return min_q > 0 && nq >= std::max(min_q, qpb);
}
// MASKED batches (vg_scan_within_batch_masked) over rows of up to 128 bytes: the gathering form of vg_batch_bits_within.hip,
// which walks the list of the mask's allowed positions (vg_ensure_mask_positions) and never reads an excluded row.  Whatever the
// threshold - the switch included -, such a batch needs half a workgroup of real queries: a launch is one workgroup of 256 query slots
// and below 128 of them it is mostly padding.  Rows beyond 128 bytes keep the masked multi-query range scan.
#define VG_WITHIN_BITS_MASKED_MIN_QUERIES_DEFAULT 128   // (0: never.  Measured, tools/bits_within_masked_bench.py / DESIGN.md 3.31: at 128 queries - the floor - the matrix cores win all 16 cells by more than both spreads, the closest a contiguous 10 % mask over 32-byte Hamming rows, 2.32 against 3.35 ms)
#define VG_WITHIN_BITS_MASKED_FLOOR 128
static bool within_bits_masked_eligible(const vg_corpus *c, int metric, int nq) {
    if (vg_sw(SW_VG_BATCH_MFMA, 1) == 0 || c->vtype != VG_TYPE_U8 || !vg_metric_is_bits(metric)) return false;
    if (c->mask_count <= 0 || c->stride > 128) return false;
    const int min_q = vg_sw(SW_VG_BATCH_BITS_MIN_QUERIES, VG_WITHIN_BITS_MASKED_MIN_QUERIES_DEFAULT);
    if (min_q <= 0 || nq < std::max(min_q, VG_WITHIN_BITS_MASKED_FLOOR)) return false;
    return vg_batch_bits_within_masked_lds_bytes(c->stride) != 0;
}

// the count word of n descriptors' regions: zeroed (dst == nullptr) or gathered into dst
__global__ void vg_wb_desc_counts_kernel(const VgWithinQuery *desc, int n, unsigned long long *dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dst) dst[i] = desc[i].out[0];
    else desc[i].out[0] = 0ull;
}

// masked: the batch of vg_scan_within_batch_masked over rows of up to 128 bytes - tiles and partitions count the mask's position list
static int batch_within_bits(vg_corpus *c, const char *who, int metric, const void *queries, int nq, const double *radii, int64_t limit, bool masked) {
    constexpr int QPB = VG_WB_SLICE;                                  // a slice = a launch; rows of up to 128 bytes: = the workgroup's queries
    const int lqpb = c->stride > 128 ? vg_batch_bitsl_within_queries_per_block(c->stride) : 0;      // the long rows' queries per workgroup
    const int nslices = (nq + QPB - 1) / QPB;
    const size_t qbytes = (size_t)QPB * c->stride, block_bytes = qbytes + (size_t)QPB * sizeof(VgWithinQuery);      // [256 queries | 256 descriptors]
    VG_TRY(vg_dev_reserve(&c->d_bq, &c->bq_bytes, block_bytes));
    if (!c->d_wb_counts) HIP_TRY(hipMalloc(&c->d_wb_counts, (size_t)VG_WB_SLICE * sizeof(unsigned long long)));
    if (!c->h_wb) HIP_TRY(hipHostMalloc(&c->h_wb, (size_t)(VG_WB_SLICE + 8) * sizeof(unsigned long long)));
    // partitions of a launch of G query groups: one workgroup per CU (VG_BATCH_BPC overrides the workgroups per CU) over the groups, a
    // multiple of 8 (one per XCD), a tile at least
    auto parts = [&](int G) {
        int npart = std::max(1, c->cu_count * std::max(1, vg_sw(SW_VG_BATCH_BPC, 1)) / G);
        if (npart >= 8) npart = (npart / 8) * 8;
        return (int)std::min<long long>(npart, ((masked ? c->mask_count : c->n_rows) + 31) / 32);
    };
    if (masked) VG_TRY(vg_ensure_mask_positions(c));
    // zero-padded rows of the corpus stride; a pad query is zero with no capacity and a radius nothing is below
    std::vector<uint8_t> hq((size_t)nslices * block_bytes, 0);
    const size_t row_bytes = (size_t)c->dim * c->es;
    for (int i = 0; i < nq; ++i)
        memcpy(hq.data() + (size_t)(i / QPB) * block_bytes + (size_t)(i % QPB) * c->stride, (const uint8_t *)queries + (size_t)i * row_bytes, row_bytes);
    uint8_t *d_stage = (uint8_t *)c->d_bq;
    const VgWithinQuery *d_desc = reinterpret_cast<const VgWithinQuery *>(d_stage + qbytes);
    const int jaccard = metric == VG_DIST_JACCARD ? 1 : 0;

    // descriptors up, counts zeroed, the launch, counts back into h_wb[0, nqs): one wait
    auto run = [&](uint8_t *block, VgWithinQuery *desc, int nqs) -> int {
        HIP_TRY(hipMemcpyAsync(d_stage, block, block_bytes, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(vg_wb_desc_counts_kernel, dim3(1), dim3(VG_WB_SLICE), 0, c->stream, d_desc, nqs, (unsigned long long *)nullptr);
        hipEvent_t *evs = vg_prof_slot(c, 0);
        if (evs) hipEventRecord(evs[0], c->stream);
        // (long rows: the query groups that hold a real query; the descriptors behind them are padding up to the slice)
        const int nq_pad = lqpb ? (nqs + lqpb - 1) / lqpb * lqpb : QPB;
        const int rc = masked ? vg_batch_bits_within_masked_launch(c->d_rows, c->n_rows, c->stride, c->d_mask_pos, c->mask_count, d_stage, d_desc, QPB, jaccard,
                                                                   parts(1), c->stream)
                       : lqpb ? vg_batch_bitsl_within_launch(c->d_rows, c->n_rows, c->stride, d_stage, d_desc, nq_pad, jaccard, parts(nq_pad / lqpb), c->stream)
                              : vg_batch_bits_within_launch(c->d_rows, c->n_rows, c->stride, d_stage, d_desc, QPB, jaccard, parts(1), c->stream);
        if (evs) { hipEventRecord(evs[2], c->stream); hipEventRecord(evs[3], c->stream); }
        if (rc != 0) {
            hipStreamSynchronize(c->stream);
            return vg_fail(VG_ERR_HIP, "%s: range batch launch (bit vectors) failed: %s", who, rc == -1 ? "shape not served" : hipGetErrorString((hipError_t)rc));
        }
        ++c->wb_launches;
        hipLaunchKernelGGL(vg_wb_desc_counts_kernel, dim3(1), dim3(VG_WB_SLICE), 0, c->stream, d_desc, nqs, c->d_wb_counts);
        hipError_t e = hipMemcpyAsync(c->h_wb, c->d_wb_counts, (size_t)nqs * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
        hipError_t e2 = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || e2 != hipSuccess) return vg_fail(VG_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
        return VG_OK;
    };

    for (int s = 0; s < nslices; ++s) {
        const int q0 = s * QPB, nqs = std::min(QPB, nq - q0);         // (real queries: the pad queries own no region)
        uint8_t *block = hq.data() + (size_t)s * block_bytes;
        VgWithinQuery *desc = reinterpret_cast<VgWithinQuery *>(block + qbytes);
        // a query's share of the one key budget, never more than the rows there are
        int64_t cap = c->wb_cap_init > 0 ? c->wb_cap_init : std::max<int64_t>(VG_WB_MIN_CAP, (int64_t)VG_WITHIN_INITIAL_CAP / nqs);
        cap = std::max<int64_t>(1, std::min<int64_t>(cap, c->n_rows));
        const long long pitch = (long long)cap + 1;
        VG_TRY(vg_dev_reserve(&c->d_wb, &c->wb_bytes, (size_t)nqs * (size_t)pitch * sizeof(unsigned long long)));
        for (int j = 0; j < QPB; ++j) {
            const bool real = j < nqs;
            desc[j].out = real ? c->d_wb + (long long)j * pitch : c->d_wb;      // (a pad query never matches: its region is never touched)
            desc[j].cap = real ? (unsigned long long)cap : 0ull;
            desc[j].r = real ? vg_within_radius(radii[q0 + j]) : -INFINITY;
            desc[j].label = VG_LABEL_NONE;
        }
        VG_TRY(run(block, desc, nqs));
        std::vector<int64_t> counts((size_t)nqs);
        bool over = false;
        for (int j = 0; j < nqs; ++j) { counts[(size_t)j] = (int64_t)c->h_wb[j]; over = over || counts[(size_t)j] > cap; }
        // the queries that fit: their keys leave first (nothing below touches d_wb)
        bool pending = false;
        for (int j = 0; j < nqs; ++j)
            if (counts[(size_t)j] <= cap) VG_TRY(collect_keys(c, q0 + j, c->d_wb + (long long)j * pitch + 1, counts[(size_t)j], limit, &pending));
        if (pending) HIP_TRY(hipStreamSynchronize(c->stream));
        if (over) {
            // a launch with a query past its capacity: once more as a whole, counts reset, every region at its counted size
            size_t words = 0;
            for (int j = 0; j < nqs; ++j) words += (size_t)std::max<int64_t>(counts[(size_t)j], 1) + 1;
            VG_TRY(vg_dev_reserve(&c->d_wb_grow, &c->wb_grow_bytes, words * sizeof(unsigned long long)));
            size_t at = 0;
            for (int j = 0; j < QPB; ++j) {
                desc[j].out = c->d_wb_grow + (j < nqs ? at : 0);
                if (j < nqs) { desc[j].cap = (unsigned long long)std::max<int64_t>(counts[(size_t)j], 1); at += (size_t)desc[j].cap + 1; }
            }
            VG_TRY(run(block, desc, nqs));
            for (int j = 0; j < nqs; ++j)
                if ((int64_t)c->h_wb[j] != counts[(size_t)j])
                    return vg_fail(VG_ERR_HIP, "%s: two launches counted %lld and %lld rows for query %d", who, (long long)counts[(size_t)j],
                                   (long long)c->h_wb[j], q0 + j);
            pending = false;
            for (int j = 0; j < nqs; ++j)
                if (counts[(size_t)j] > cap) VG_TRY(collect_keys(c, q0 + j, desc[j].out + 1, counts[(size_t)j], limit, &pending));
            if (pending) HIP_TRY(hipStreamSynchronize(c->stream));          // (d_wb_grow serves the next such launch)
        }
        for (int j = 0; j < nqs; ++j) vg_within_finish(&c->wb_keys[(size_t)(q0 + j)], c->wb_matches[(size_t)(q0 + j)], limit);
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
    c->wb_last_path = 0;
    if (f.rows == VG_QROWS_ALL && within_bits_eligible(c, metric, nq)) {      // bit vectors, enough queries: the integer matrix cores
        rc = batch_within_bits(c, f.who, metric, queries, nq, radii, limit, false);
        c->wb_last_path = 8;
    } else if (masked && within_bits_masked_eligible(c, metric, nq)) {        // ... under a mask: their gathering form (rows of up to 128 bytes)
        rc = batch_within_bits(c, f.who, metric, queries, nq, radii, limit, true);
        c->wb_last_path = 8;
    } else if (NQ == 0) {                                        // no multi-query form: the single range scans of the same form, one by one
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
        c->wb_last_path = 6;
    } else {
        rc = batch_within_multi(c, f, metric, fn, NQ, s, queries, nq, radii, qlabels, limit);
        c->wb_last_path = 5;
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
extern "C" int vg_within_batch_last_path(const vg_corpus *c) { return c ? c->wb_last_path : 0; }
