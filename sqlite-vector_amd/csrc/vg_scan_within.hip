// vg_scan_within.hip - range scans: every row within a distance of the query (vg_scan_within, include/vectorgpu.h).
//
// The kernels are the WITHIN = true instantiations of vg_scan_kernel / vg_scan_long_kernel (vg_scan.h): the plain scan's loads,
// arithmetic and summation order with a fixed threshold in place of the converging k-th best - compare, ballot, and only for the rare
// batch with a match a key parked in the wavefront's LDS queue, flushed in bursts (vg_within_offer / vg_within_flush).  A translation
// unit of their own, like vg_scan_ex.hip: the plain kernels keep their register budget.  One load policy (non-temporal).
//
// Host side: [count | capacity keys] in device memory; the count keeps counting past the capacity, so ONE more launch into a buffer of
// the counted size answers an overflow - a partial answer is never returned.  The unsigned order of the keys is the contract order
// (distance, scan position): up to VG_WITHIN_HOST_SORT keys are sorted on the host behind the copy, more by a device radix sort
// (vg_select.hip) so that a `limit` below the match count brings only `limit` keys across the host link.
#include "vg_internal.h"

#include "vg_scan.h"

typedef void (*scan_fn_t)(ScanArgs);

template <int VT, int ACC>
static scan_fn_t pick_u(int U) {
    switch (U) {
        case 1: return vg_scan_kernel<VT, ACC, 1, true, false, true>;
        case 2: return vg_scan_kernel<VT, ACC, 2, true, false, true>;
        case 3: return vg_scan_kernel<VT, ACC, 3, true, false, true>;
        case 4: return vg_scan_kernel<VT, ACC, 4, true, false, true>;
        case 6: return vg_scan_kernel<VT, ACC, 6, true, false, true>;
        case 8: return vg_scan_kernel<VT, ACC, 8, true, false, true>;
    }
    return nullptr;
}

template <int VT>
static scan_fn_t pick_acc(int acc, int U, bool long_rows) {
    if (long_rows) {
        switch (acc) {
            case A_L2: return vg_scan_long_kernel<VT, A_L2, true, true>;
            case A_COS: return vg_scan_long_kernel<VT, A_COS, true, true>;
            case A_DOT: return vg_scan_long_kernel<VT, A_DOT, true, true>;
            case A_L1: return vg_scan_long_kernel<VT, A_L1, true, true>;
        }
        return nullptr;
    }
    switch (acc) {
        case A_L2: return pick_u<VT, A_L2>(U);
        case A_COS: return pick_u<VT, A_COS>(U);
        case A_DOT: return pick_u<VT, A_DOT>(U);
        case A_L1: return pick_u<VT, A_L1>(U);
        case A_COSN:
            if constexpr (VT == T_F16 || VT == T_BF16) return pick_u<VT, A_COSN>(U);
            return nullptr;
    }
    return nullptr;
}

static scan_fn_t pick_within_kernel(int vtype, int acc, const VgShape &s) {
    switch (vtype) {
        case VG_TYPE_F32: return pick_acc<T_F32>(acc, s.U, s.long_rows);
        case VG_TYPE_U8: return pick_acc<T_U8>(acc, s.U, s.long_rows);
        case VG_TYPE_I8: return pick_acc<T_I8>(acc, s.U, s.long_rows);
        case VG_TYPE_F16: return pick_acc<T_F16>(acc, s.U, s.long_rows);
        case VG_TYPE_BF16: return pick_acc<T_BF16>(acc, s.U, s.long_rows);
    }
    return nullptr;
}

extern "C" int vg_select_temp_bytes(long long n, size_t *bytes);                                                  // vg_select.hip
extern "C" int vg_select_sort_keys(const uint64_t *keys, long long n, uint64_t *keys_sorted, void *temp, size_t temp_bytes, hipStream_t stream);

// the largest float not above the radius: the device then compares floats and `d <= r` decides what (double)d <= radius decides
static float radius_to_float(double radius) {
    float r = (float)radius;
    if ((double)r > radius) r = std::nextafterf(r, -INFINITY);
    return r;
}

// one launch of the within kernel into c->d_within ([count | cap keys]); the count lands in the pinned c->h_keys[0] behind it
static int launch_within(vg_corpus *c, int metric, float r, int64_t cap) {
    int acc = vg_metric_to_acc(metric);
    VgShape s;
    vg_plain_scan_shape(c, metric, &s);
    if (acc == A_COS && (c->vtype == VG_TYPE_F16 || c->vtype == VG_TYPE_BF16) && !s.long_rows && vg_sw(SW_VG_HALF_COSN, 1)) {
        int rcn = vg_ensure_row_norms(c);                    // the plain scan's cached-norm cosine: the same floats
        if (rcn != VG_OK) return rcn;
        acc = A_COSN;
    }
    scan_fn_t fn = pick_within_kernel(c->vtype, acc, s);
    if (!fn) return vg_fail(VG_ERR_UNSUPPORTED, "vg_scan_within: no kernel for this type / metric");

    // the launch shape of the plain top-k scan (vg_api.hip: launch_scan)
    const int rpb = VG_WAVE >> s.lpr_log2;
    const long long nbatch = (c->n_rows + rpb - 1) / rpb;
    const int bpc = std::max(1, std::min(8, vg_sw(SW_VG_BLOCKS_PER_CU, 1)));
    long long blocks = (nbatch + VG_WAVES_PER_BLOCK - 1) / VG_WAVES_PER_BLOCK;
    blocks = std::max<long long>(1, std::min<long long>(blocks, (long long)c->cu_count * bpc));

    ScanArgs a{};
    a.rows = c->d_rows;
    a.query = c->d_query;
    a.n_rows = c->n_rows;
    a.stride = c->stride;
    a.nch = c->nch;
    a.lpr_log2 = s.lpr_log2;
    a.k = 0;
    a.root = (metric == VG_DIST_L2) ? 1 : 0;
    a.dim = c->dim;
    a.row_nn = (acc == A_COSN) ? c->d_xnorm : nullptr;
    a.emit = c->d_within;
    a.within_r = r;
    a.within_cap = (unsigned long long)cap;
    size_t qbytes = (size_t)c->nch * 16;
    if (s.long_rows) {
        const size_t slice = (size_t)VG_WAVE * VG_LONG_U;
        qbytes = ((c->nch + slice - 1) / slice) * slice * 16;
    }
    a.store_lds_off = (int)((qbytes + 255) / 256 * 256);     // the wavefronts' key queues behind the query
    const size_t smem = (size_t)a.store_lds_off + VG_WITHIN_LDS_BYTES;

    HIP_TRY(hipMemsetAsync(c->d_within, 0, sizeof(unsigned long long), c->stream));
    hipEvent_t *evs = vg_prof_slot(c, 0);
    if (evs) hipEventRecord(evs[0], c->stream);
    if (smem > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(VG_BLOCK), smem, c->stream, a);
    if (evs) { hipEventRecord(evs[2], c->stream); hipEventRecord(evs[3], c->stream); }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_keys, c->d_within, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->within_launches;
    return VG_OK;
}

static int ensure_within_buffer(vg_corpus *c, int64_t cap) {
    if (c->within_cap >= cap) return VG_OK;
    if (c->d_within) { hipFree(c->d_within); c->d_within = nullptr; c->within_cap = 0; }
    HIP_TRY(hipMalloc(&c->d_within, ((size_t)cap + 1) * sizeof(unsigned long long)));
    c->within_cap = cap;
    return VG_OK;
}

static int ensure_within_sort(vg_corpus *c, int64_t n) {
    if (c->within_sort_cap >= n) return VG_OK;
    if (c->d_within_sorted) hipFree(c->d_within_sorted);
    if (c->d_within_temp) hipFree(c->d_within_temp);
    c->d_within_sorted = nullptr; c->d_within_temp = nullptr; c->within_sort_cap = 0;
    if (vg_select_temp_bytes(n, &c->within_temp_bytes) != 0) return vg_fail(VG_ERR_HIP, "radix sort temp-size query failed");
    HIP_TRY(hipMalloc(&c->d_within_sorted, (size_t)n * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(&c->d_within_temp, c->within_temp_bytes ? c->within_temp_bytes : 16));
    c->within_sort_cap = n;
    return VG_OK;
}

extern "C" int vg_scan_within(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                              int64_t *out_held) {
    if (!c || !query) return vg_fail(VG_ERR_INVALID, "vg_scan_within: NULL argument");
    if (out_matches) *out_matches = 0;
    if (out_held) *out_held = 0;
    c->within_keys.clear();
    c->within_matches = 0;
    c->within_launches = 0;
    if (vg_metric_to_acc(metric) < 0) return vg_fail(VG_ERR_INVALID, "unknown distance metric %d", metric);
    if (radius != radius) return vg_fail(VG_ERR_INVALID, "vg_scan_within: the radius is NaN");
    if (c->n_rows == 0) return VG_OK;
    HIP_TRY(hipSetDevice(c->device));
    c->enqueued = false;                                     // (the pinned key buffer is this scan's landing zone now)
    const float r = radius_to_float(radius);
    int64_t cap = c->within_cap_init > 0 ? c->within_cap_init : (int64_t)VG_WITHIN_INITIAL_CAP;
    cap = std::max<int64_t>(std::min<int64_t>(cap, c->n_rows), c->within_cap);      // (a buffer an earlier scan grew is kept)
    int rc = ensure_within_buffer(c, cap);
    if (rc != VG_OK) return rc;
    memset(c->h_query, 0, (size_t)c->stride);
    memcpy(c->h_query, query, (size_t)c->dim * c->es);
    HIP_TRY(hipMemcpyAsync(c->d_query, c->h_query, (size_t)c->stride, hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_within(c, metric, r, cap)) != VG_OK) return rc;
    int64_t count = (int64_t)c->h_keys[0];
    if (count > cap) {                                       // overflow: the count IS the size needed - grow, launch once more
        cap = count;
        if ((rc = ensure_within_buffer(c, cap)) != VG_OK) return rc;
        if ((rc = launch_within(c, metric, r, cap)) != VG_OK) return rc;
        if ((int64_t)c->h_keys[0] != count) return vg_fail(VG_ERR_HIP, "vg_scan_within: two launches counted %lld and %lld rows", (long long)count, (long long)c->h_keys[0]);
    }
    vg_collect_timing(c);
    const int64_t held = (limit > 0) ? std::min<int64_t>(limit, count) : count;
    c->within_keys.resize((size_t)held);
    if (count > 0 && count <= VG_WITHIN_HOST_SORT) {
        std::vector<uint64_t> all((size_t)count);
        HIP_TRY(hipMemcpy(all.data(), c->d_within + 1, (size_t)count * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::sort(all.begin(), all.end());
        std::copy(all.begin(), all.begin() + held, c->within_keys.begin());
    } else if (count > 0) {
        if ((rc = ensure_within_sort(c, count)) != VG_OK) return rc;
        if (vg_select_sort_keys(reinterpret_cast<const uint64_t *>(c->d_within + 1), count, c->d_within_sorted, c->d_within_temp, c->within_temp_bytes, c->stream) != 0)
            return vg_fail(VG_ERR_HIP, "device key sort failed: %s", hipGetErrorString(hipGetLastError()));
        HIP_TRY(hipMemcpyAsync(c->within_keys.data(), c->d_within_sorted, (size_t)held * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->within_matches = count;
    if (out_matches) *out_matches = count;
    if (out_held) *out_held = held;
    return VG_OK;
}

extern "C" int vg_scan_within_keys(const vg_corpus *c, int64_t first, int64_t n, uint64_t *out_keys) {
    if (!c || (n > 0 && !out_keys)) return vg_fail(VG_ERR_INVALID, "vg_scan_within_keys: NULL argument");
    if (n <= 0) return VG_OK;
    if (first < 0 || first + n > (int64_t)c->within_keys.size())
        return vg_fail(VG_ERR_INVALID, "vg_scan_within_keys: rows %lld..%lld of %lld held", (long long)first, (long long)(first + n), (long long)c->within_keys.size());
    memcpy(out_keys, c->within_keys.data() + first, (size_t)n * sizeof(uint64_t));
    return VG_OK;
}

extern "C" int vg_scan_within_fetch(const vg_corpus *c, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist) {
    if (!c) return vg_fail(VG_ERR_INVALID, "vg_scan_within_fetch: NULL argument");
    if (n <= 0) return VG_OK;
    if (first < 0 || first + n > (int64_t)c->within_keys.size())
        return vg_fail(VG_ERR_INVALID, "vg_scan_within_fetch: rows %lld..%lld of %lld held", (long long)first, (long long)(first + n), (long long)c->within_keys.size());
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = c->within_keys[(size_t)(first + i)];
        if (out_rowids) out_rowids[i] = vg_corpus_rowid_at(c, (int64_t)vg_key_position(key));
        if (out_dist) out_dist[i] = (double)vg_key_distance(key);
    }
    return VG_OK;
}

extern "C" int vg_within_set_initial_capacity(vg_corpus *c, int64_t keys) {
    if (!c) return vg_fail(VG_ERR_INVALID, "corpus is NULL");
    c->within_cap_init = keys > 0 ? keys : 0;
    if (c->d_within) { hipSetDevice(c->device); hipFree(c->d_within); c->d_within = nullptr; c->within_cap = 0; }   // (the next scan starts from that size)
    return VG_OK;
}

extern "C" int vg_within_last_launches(const vg_corpus *c) { return c ? c->within_launches : 0; }
