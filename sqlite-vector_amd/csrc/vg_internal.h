// vg_internal.h - what the host-side translation units of libvectorgpu.so share: the corpus object, the error
// helpers and the few internal entry points that cross files.  Not part of the C-ABI (include/vectorgpu.h is).
//   vg_corpus.hip     corpus lifetime + staging, key / quantizer / instrumentation helpers
//   vg_api.hip        kernel selection, the scan launches (needs the kernel templates of vg_scan.h)
//   vg_batch_api.hip  batched queries: planning, cached row statistics, launches of vg_batch*.hip
#pragma once

#include "../../include/vectorgpu.h"
#include "../../include/vectorgpu_diag.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define VG_PROF_RING 1024
#define VG_PROF_EVS 4             // events per recorded launch: start | after the pre-pass | after the scan kernel | after the merge
#define VG_EVF_MERGE 1            // ev_flags bits: the launch had a merge kernel / a pre-pass of its own
#define VG_EVF_PREPASS 2
#define VG_WAVE_HOST 64
#define VG_KEYS_BYTES (VG_WAVE_HOST * (sizeof(uint64_t) + sizeof(uint32_t)))   // d_keys / h_keys: 64 keys, then (grouped scans) their 64 labels

int vg_fail(int code, const char *fmt, ...);         // sets the thread-local message, returns code (vg_corpus.hip)

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess)                                                                            \
            return vg_fail(e__ == hipErrorOutOfMemory ? VG_ERR_NOMEM : VG_ERR_HIP, "%s failed: %s (%s:%d)", \
                           #expr, hipGetErrorString(e__), __FILE__, __LINE__);                            \
    } while (0)


static inline int vg_elem_size(int vtype) {
    switch (vtype) {
        case VG_TYPE_F32: return 4;
        case VG_TYPE_F16: case VG_TYPE_BF16: return 2;
        case VG_TYPE_U8: case VG_TYPE_I8: return 1;
    }
    return 0;
}

struct vg_corpus {
    int device = 0;
    int vtype = 0;
    int dim = 0;
    int es = 0;
    int nch = 0;               // 16-byte chunks per stored row
    int64_t stride = 0;        // bytes per stored row (nch * 16)
    int64_t n_rows = 0;
    int64_t cap_rows = 0;
    uint8_t *d_rows = nullptr;
    std::vector<int64_t> rowids;   // empty => implicit rowid_base + position
    bool rowids_ascending = true;  // every appended rowid was larger than the one before it (a rowid table in key order)
    int64_t rowid_base = 1;

    hipStream_t stream = nullptr;
    uint8_t *d_query = nullptr;    // nch*16 bytes
    uint8_t *h_query = nullptr;    // pinned
    uint64_t *d_cand = nullptr;    // max_blocks * 64 keys
    uint64_t *d_cand_pre = nullptr; // the same size: a filter scan's pre-pass lists, read unmerged by the filter kernel
    uint64_t *d_keys = nullptr;    // 64 keys (+ 64 labels behind them: VG_KEYS_BYTES)
    uint64_t *h_keys = nullptr;    // pinned, the same
    float *d_dist = nullptr;       // lazily sized to n_rows (stream scans / large k / tie_order = reference)
    int64_t d_dist_cap = 0;
    int64_t dist_valid_rows = 0;   // rows of d_dist the last vg_scan_distances_resident filled (0: none)
    unsigned long long *d_below = nullptr;   // vg_reforder.hip: [count | VG_BELOW_CAP (position, distance) pairs]
    uint8_t *h_ref = nullptr;      // pinned landing zone of its small device-to-host copies (a pageable destination costs ~100 us each)
    size_t h_ref_bytes = 0;
    std::vector<uint64_t> ref_pairs;   // its candidate pairs on the host (kept between scans: no 1 MB clear per query)
    int tie_order = 0;             // VG_TIE_POSITION / VG_TIE_REFERENCE (vg_corpus_set_tie_order)
    // tie_order = reference, the fused form (vg_reforder.hip): a top-k scan with one more list slot; only when its k+1 best distances
    // hold a tie does the host replay the reference's slots - over the prefix pass' distances + the candidate stream the scan emitted
    float *d_ref_prefix = nullptr; // distances of the first ref_prefix_rows rows (written by the prefix pass: top-k + store)
    int64_t ref_prefix_cap = 0;
    int64_t ref_prefix_rows = -1;  // rows the LAST emitting launch stored (-1: that launch could not emit - long rows / a small corpus)
    int ref_hot = 0;               // > 0: ties were seen recently - plain-kernel scans pay the prefix pass up front instead of a second scan
    unsigned long long ref_stats[4] = {0, 0, 0, 0};   // reference-order scans | with a tie among the k+1 best | answered by the fused replay | by the store-mode replay
    uint64_t *d_sel_keys = nullptr, *d_sel_sorted = nullptr;   // k > 64 path: N keys, unsorted / sorted
    void *d_sel_temp = nullptr;
    uint32_t *d_sel_state = nullptr;   // radix-select state + histogram (vg_select.hip)
    size_t sel_temp_bytes = 0;
    int64_t sel_cap = 0;
    uint8_t *pin[2] = {nullptr, nullptr};      // staging pipeline: pinned bounce buffers + their completion events
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    int pin_idx = 0;
    uint8_t *d_stage = nullptr;                // device-side landing zone for rows that need de-interleaving
    hipEvent_t append_ev = nullptr;            // recorded behind the last enqueued host append (other streams wait on it)
    bool append_pending = false;
    bool enqueued = false;                     // a vg_scan_topk_enqueue is in flight (vg_scan_topk_collect pending)
    float *d_xnorm = nullptr;                  // lazily: row norms for rows [0, xnorm_rows) (see ensure_row_norms)
    int64_t xnorm_rows = 0, xnorm_cap = 0;
    hipEvent_t norm_ev = nullptr;
    // quantized batches (vg_batch_i8.hip): per-row sum x / sum x^2 and, for uint8, the XOR-0x80 copy the matrix core reads
    uint32_t *d_sx = nullptr;                     // per row: (sum x, sum x^2)
    uint8_t *d_rows_s8 = nullptr;
    uint8_t *d_rows_tm = nullptr;                 // f16 / bf16 corpora: the tile-major copy the batched matrix-core kernel streams
    int64_t tm_rows = 0, tm_cap = 0;
    bool tm_disabled = false;                     // (it did not fit: the kernel gathers from the row-major corpus)
    uint8_t *d_rows_bf = nullptr;                 // f32 corpora: bf16 shadow copy for the matrix-core filter (vg_batch_h.hip)
    int64_t bf_rows = 0, bf_cap = 0;
    uint8_t *d_rows_q8 = nullptr;                 // f32 corpora: int8 shadow copy for the single-query filter scan (vg_filter.hip) ...
    void *d_q8stat = nullptr;                     // ... and per row (scale, residual norm) as float2
    int64_t q8_rows = 0, q8_cap = 0;
    uint8_t *d_rows_q8tm = nullptr;               // f32 corpora: the TILE-MAJOR copy of that int8 shadow, what the int8 batch filter streams (vg_batch_q8.hip) ...
    void *d_q8tm_stat = nullptr;                  // ... and per row (scale | -1, residual norm, ||x||, 0) as float4, two tiles of slack behind the last row
    int64_t q8tm_rows = 0, q8tm_cap = 0;
    bool q8tm_disabled = false;                   // (it did not fit: batches keep the bf16 filter / the f32 matrix-core kernel)
    int bq8_cooldown = 0;                         // > 0: a batch overflowed a pair region - that many batches take the other paths
    int bq8_status = 0;                           // the last int8-filter batch: 0 answered, 1 no room for the copies, 2 shape not served, 3 a pair region overflowed (vg_batch_q8_status)
    uint8_t *d_rows_n4 = nullptr;                 // uint8 / int8 corpora: high-nibble shadow copy for the filter scan (vg_scan_filter_n4.h) ...
    void *d_n4stat = nullptr;                     // ... and per row (sum x^2, sum of low nibbles, their centred norm), 16 bytes
    int64_t n4_rows = 0, n4_cap = 0;
    bool n4_disabled = false;
    int n4_probe = 0;                             // 0 = not probed yet, 1 = selective on this data (filter on), 2 = not selective (plain kernel)
    int64_t n4_probe_rows = 0;                    // n_rows at that probe (an unselective corpus is probed again once it has doubled)
    bool q8_disabled = false;                     // (it did not fit next to an f16 / bf16 corpus: the filter scans read the rows themselves)
    bool filter_disabled = false;                 // the shadow copy / norms did not fit HBM: single queries keep the plain f32 scan
    int scan_filter_mode = -1;                    // vg_corpus_set_scan_filter: -1 = default (env VG_SCAN_FILTER, else on), 0 = off, 1 = on
    unsigned long long *d_filter_evals = nullptr; // filter scan: exact evaluations so far (device counter, one atomic per workgroup) ...
    unsigned long long *h_filter_evals = nullptr; // ... and its pinned host mirror, refreshed by an 8-byte copy behind every filter launch: the
                                                  //   host can look at it without a wait (system-scope atomics straight into host memory were
                                                  //   tried: 256 of them per launch serialise on the host link, +160 us per scan)
    unsigned long long filter_evals_read = 0;     // its value at the last vg_filter_exact_evals read-out
    unsigned long long filter_evals_seen = 0;     // ... and when the selectivity guard last looked
    long long filter_launches_seen = 0, filter_launches = 0;
    int filter_cooldown = 0;                      // > 0: the bound is not selective on this data - that many scans take the plain kernel
    int filter_prepass_div = 128;                 // the filter scan's pre-pass covers 1 / this of the rows (16 .. 128, follows the candidate rate)
    // f32 batches through the bf16 filter (vg_batch_api.hip): counter [1] of d_filter_evals, the same kind of guard
    unsigned long long bfilter_evals_seen = 0, bfilter_evals_read = 0;
    long long bfilter_pairs = 0;                  // (query, row) pairs of the filtered batches since the guard last looked
    int bfilter_cooldown = 0;                     // > 0: that many batches take the f32 matrix-core kernel
    int64_t i8_rows = 0, i8_cap = 0;              // orders a caller-stream scan behind a norm pass on the corpus stream
    uint8_t *h_bq = nullptr;       // long-row batches: the pinned buffer the padded queries go up through (+ their norms coming back)
    size_t h_bq_bytes = 0;
    void *d_bq = nullptr;          // batched path: padded queries, per-(query, partition) candidates, final keys
    uint64_t *d_bcand = nullptr, *d_bkeys = nullptr;
    size_t bq_bytes = 0, bcand_bytes = 0, bkeys_bytes = 0;
    uint64_t *d_bpairs = nullptr;  // half-precision batches, split form (vg_batch_h.hip): candidate pairs per filter wavefront ...
    uint32_t *d_bpcounts = nullptr; // ... and their counts + overflow flag
    size_t bpairs_bytes = 0, bpcount_bytes = 0;
    bool bsplit_off = false;       // a batch overflowed a pair region: this corpus keeps the fused kernel
    int last_batch_path = 0;       // vg_batch_last_path (vectorgpu_diag.h)
    bool last_batch_half = false;  // (the last matrix-core batch went through vg_batch_h.hip)
    int blong_cooldown = 0;        // ... of the long-row kernel (vg_batch_hl.hip): the next batches over this corpus take the multi-query scan
    // range scans (vg_scan_within.hip): the device buffer the kernel appends to, the sort's buffers, and the last result - kept on the host
    unsigned long long *d_within = nullptr;   // [count | within_cap keys]
    int64_t within_cap = 0;
    int64_t within_cap_init = 0;              // vg_within_set_initial_capacity (0: VG_WITHIN_INITIAL_CAP)
    uint64_t *d_within_sorted = nullptr;
    void *d_within_temp = nullptr;
    size_t within_temp_bytes = 0;
    int64_t within_sort_cap = 0;
    std::vector<uint64_t> within_keys;        // the held keys of the last vg_scan_within, ascending = (distance, scan position)
    int64_t within_matches = 0;
    int within_launches = 0;                  // kernel launches the last vg_scan_within took (2: the buffer overflowed once)
    // batch range scans (vg_multi_within.hip): the key regions of one slice of queries, [count | cap keys] each at one pitch; the
    // regions of a pass that overflowed and ran once more; the slice's counts gathered (device, then pinned host); the last result
    unsigned long long *d_wb = nullptr, *d_wb_grow = nullptr, *d_wb_counts = nullptr, *h_wb = nullptr;
    size_t wb_bytes = 0, wb_grow_bytes = 0;
    int64_t wb_cap_init = 0;                  // vg_within_batch_set_initial_capacity: keys per query (0: a share of VG_WITHIN_INITIAL_CAP)
    int wb_launches = 0;                      // scan kernel launches of the last vg_scan_within_batch
    std::vector<std::vector<uint64_t>> wb_keys;   // per query: the held keys, ascending = (distance, scan position)
    std::vector<int64_t> wb_matches;
    // masked scans (vg_scan_masked.hip): the row mask - bit (p & 63) of word (p >> 6) = the row at scan position p may be returned.  Read
    // by the masked scans only (vectorgpu.h lists them); dropped (vg_drop_mask) by every call that changes the number of rows or which row sits where
    uint64_t *d_mask = nullptr;               // ceil(n_rows / 64) words while a mask is set (mask_cap_words allocated)
    int64_t mask_cap_words = 0;
    std::vector<uint64_t> mask_host;          // the same words on the host (vg_corpus_clone copies them)
    int64_t mask_count = -1;                  // rows allowed; -1: no mask
    // labeled scans (vg_rowpred.hip, vg_multi_labeled.hip): a uint32 per scan position in device memory (VG_LABEL_NONE: the row
    // matches no query).  Read by the labeled scans only; lifetime rule for rule the mask's (vg_drop_labels).  d_label_bits: the bitmap
    // "rows the query may see" a row predicate's scan builds for itself (vg_pred_bits_enqueue) - scratch, never the user's mask
    uint32_t *d_labels = nullptr;             // n_rows dwords while labels are set (labels_cap allocated)
    int64_t labels_cap = 0;
    bool has_labels = false;
    uint64_t *d_label_bits = nullptr;         // ceil(n_rows / 64) words (label_bits_cap_words allocated)
    int64_t label_bits_cap_words = 0;
    // label-set scans (vg_rowpred.hip, vg_multi_labelset.hip): scratch the handle owns.  d_lset: the sorted, de-duplicated
    // set(s) of the call in flight (single forms: one set; the batch: every membership group's sets, offsets and query masks);
    // lset_host: what the single forms upload from - it must not move before the upload ran, and every call ends in a wait.
    // d_member: the batch form's membership dword per row, refilled for every group of up to 32 queries in stream order
    uint32_t *d_lset = nullptr;
    size_t lset_bytes = 0;
    std::vector<uint32_t> lset_host;
    uint32_t *d_member = nullptr;
    int64_t member_cap = 0;
    // value-range scans (vg_rowpred.hip, vg_multi_valued.hip): an int64 per scan position in device memory - any int64 is a value.
    // Read by the valued scans only; lifetime rule for rule the labels' (vg_drop_values).  Their bitmap and membership dwords go into
    // the label-set scans' scratch (d_label_bits, d_lset, d_member)
    int64_t *d_values = nullptr;              // n_rows values while values are set (values_cap allocated)
    int64_t values_cap = 0;
    bool has_values = false;
    int max_blocks = 0;
    int cu_count = 0;

    // instrumentation: a ring of event quadruples (start | after the pre-pass | after the scan kernel | after the merge),
    // recorded on the stream each launch runs on, read back only when asked - no host synchronisation inside a timed region
    bool profiling = false;
    std::vector<hipEvent_t> ev;            // VG_PROF_EVS * VG_PROF_RING events, created on first enable
    std::vector<uint8_t> ev_flags;         // VG_EVF_* per slot
    long long prof_launches = 0;           // launches recorded since profiling was (re)enabled
    float last_scan_ms = 0.f, last_merge_ms = 0.f, last_prepass_ms = 0.f;
    char kernel_name[64] = {0};
    // kernel milliseconds / rows of the last minmax [0], quantize [1] and int8-shadow [2] pass (HIP events on the corpus stream;
    // the first two always, the shadow pass while profiling is on) - bench.py --workload stage prices them against the HBM peak
    float pass_ms[3] = {0.f, 0.f, 0.f};
    long long pass_rows[3] = {0, 0, 0};
};

#define VG_TRY(expr) do { const int rc__ = (expr); if (rc__ != VG_OK) return rc__; } while (0)   // a VG_* code other than VG_OK: return it

// ---- the handle's grow-only work buffers (d_bq, d_bcand, d_bkeys, d_bpairs, d_bpcounts, d_wb ...): *p holds at least `need` bytes
// and *have says how many.  Large enough: nothing to do; else the old buffer is freed - what it held is NOT carried over - and one of
// `need` bytes allocated.  After a failed allocation *p is null and *have 0
template <class T> static inline hipError_t vg_dev_regrow(T **p, size_t *have, size_t need) {
    if (*have >= need) return hipSuccess;
    if (*p) hipFree(*p);
    *p = nullptr; *have = 0;
    const hipError_t e = hipMalloc(p, need);
    if (e == hipSuccess) *have = need;
    else *p = nullptr;
    return e;
}
// ... where the caller cannot go on without the buffer: VG_OK, or VG_ERR_NOMEM / VG_ERR_HIP with the message set
template <class T> static inline int vg_dev_reserve(T **p, size_t *have, size_t need) {
    HIP_TRY(vg_dev_regrow(p, have, need));
    return VG_OK;
}
// ... where it can (a form of the kernel that needs no such buffer): false - not available, the HIP error cleared, nothing reported
template <class T> static inline bool vg_dev_reserve_optional(T **p, size_t *have, size_t need) {
    if (vg_dev_regrow(p, have, need) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
// h_bq, the pinned buffer the batch drivers stage their queries in (small results come back through its tail): the same rule
static inline int vg_reserve_h_bq(vg_corpus *c, size_t need) {
    if (c->h_bq_bytes >= need) return VG_OK;
    if (c->h_bq) hipHostFree(c->h_bq);
    c->h_bq = nullptr; c->h_bq_bytes = 0;
    HIP_TRY(hipHostMalloc(&c->h_bq, need));
    c->h_bq_bytes = need;
    return VG_OK;
}
// nq queries of row_bytes each, back to back -> dst as nq_pad rows of `stride` bytes, the layout every batch kernel reads at d_bq:
// a row zero-padded to the stride, rows [nq, nq_pad) zero
static inline void vg_stage_queries(uint8_t *dst, const void *queries, int nq, int nq_pad, size_t stride, size_t row_bytes) {
    if (row_bytes == stride) memcpy(dst, queries, (size_t)nq * row_bytes);
    else
        for (int i = 0; i < nq; ++i) {
            memcpy(dst + (size_t)i * stride, (const uint8_t *)queries + (size_t)i * row_bytes, row_bytes);
            memset(dst + (size_t)i * stride + row_bytes, 0, stride - row_bytes);
        }
    if (nq_pad > nq) memset(dst + (size_t)nq * stride, 0, (size_t)(nq_pad - nq) * stride);
}

#include "vg_switches.h"           // the environment switches: vg_sw(SW_..., default)

// What one scan launch covers.  n_rows < 0: the whole corpus; a prefix otherwise (the filter scan's plain pre-pass).
struct ScanPlan {
    int64_t n_rows = -1;
    bool allow_filter = true;      // false: the plain kernel of vg_scan.h whatever the corpus / the switches say
    bool record = true;            // false: no entry in the profiling ring (a pre-pass is recorded by its parent launch)
    // tie_order = reference (vg_reforder.hip).  ref_emit: a whole-corpus top-k scan that also leaves behind what a host replay of the
    // reference's slot algorithm needs - the distances of the first c->ref_prefix_rows rows (c->d_ref_prefix, written by a prefix pass
    // that runs in front: top-k + store) and every later row that can enter the slots (c->d_below, emitted by the lists).
    bool ref_emit = false;
    float *store_prefix = nullptr;            // (the prefix pass itself) top-k mode that also stores every row's distance here ...
    unsigned long long *emit_reset = nullptr; // ... and zeroes the candidate counter of the pass behind it
    // a pre-pass whose per-CU lists are consumed UNMERGED by the kernel behind it (vg_kth_head): lists go to lists_out, no merge launch
    uint64_t *lists_out = nullptr;
    int *n_lists_out = nullptr;
    // where the LAST merge of the launch leaves the k winners, if not in dev_out_keys: the corpus' pinned, device-mapped h_keys -
    // the one workgroup of the merge writes its 512 bytes straight across the host link and the copy command behind it goes away
    // (anything in front that reads dev_out_keys on the device - a pre-pass' threshold keys - still finds them in device memory)
    uint64_t *final_out = nullptr;
};
#define VG_WITHIN_INITIAL_CAP (1 << 20) // keys the within scans' device buffer starts with (8 MB); more matches: one more launch into a buffer of the counted size
#define VG_WITHIN_HOST_SORT 4096      // up to this many matches are sorted on the host behind the copy, more by the device radix sort
#define VG_BELOW_CAP (1 << 17)        // candidate pairs the device buffer holds (more: the store-mode replay takes over)
#define VG_REF_EMIT_MIN_ROWS (1 << 17) // below this a reference-order scan with a tie simply replays a store-mode scan (cheap at that size)
#define VG_REF_PREFIX_MAX (1 << 20)   // rows of the prefix pass whose distances travel to the host on a tie (4 MB of pinned memory)
#define VG_REF_PINNED_BYTES (((size_t)VG_REF_PREFIX_MAX * 4) + ((size_t)VG_BELOW_CAP + 1) * 8)
static inline int64_t vg_ref_prefix_for(int64_t n_rows) {
    int64_t p = n_rows / 128;
    if (p < 16384) p = 16384;
    if (p > VG_REF_PREFIX_MAX) p = VG_REF_PREFIX_MAX;
    return p;
}
int vg_ensure_ref_buffers(vg_corpus *c, int64_t prefix_rows);       // vg_reforder.hip: d_ref_prefix / d_below / h_ref
#define VG_REF_FIRST_PAIRS 8191       // candidate pairs that travel with the counter in the first copy (nearly always all of them)
// vg_reforder.hip: what the last emitting launch of a corpus left behind, brought to the host (enqueue the copies, then wait)
int vg_ref_emitted_enqueue(vg_corpus *c);
int vg_ref_emitted_wait(vg_corpus *c, const float **prefix, int64_t *prefix_rows, unsigned long long **pairs, unsigned long long *count,
                        bool *overflow);
struct VgRefSlots;
void vg_ref_offer_run(VgRefSlots &slots, const float *d, int64_t n, int64_t g0);   // a run of consecutive rows offered to the slots
int vg_ref_replay_slab(vg_corpus *c, int metric, const void *query, int k, VgRefSlots &slots, int64_t gbase, bool fresh);   // vg_reforder.hip

// a (position << 32 | float bits) pair of the candidate streams (ScanArgs.emit, vg_resident_distances_below)
static inline float vg_pair_distance(unsigned long long pair) {
    const uint32_t bits = (uint32_t)pair;
    float d;
    memcpy(&d, &bits, 4);
    return d;
}
static inline int64_t vg_pair_position(unsigned long long pair) { return (int64_t)(pair >> 32); }

static inline void vg_drop_within_results(vg_corpus *c) {           // (held range-scan results name positions of the rows as they were)
    c->within_keys.clear(); c->within_matches = 0; c->wb_keys.clear(); c->wb_matches.clear();
}
static inline void vg_drop_mask(vg_corpus *c) { c->mask_count = -1; c->mask_host.clear(); }   // (the device words stay allocated for the next mask)
int vg_mask_upload(vg_corpus *c);             // vg_scan_masked.hip: mask_host -> d_mask
static inline void vg_drop_labels(vg_corpus *c) { c->has_labels = false; }   // (the device dwords stay allocated for the next labels)
static inline void vg_drop_values(vg_corpus *c) { c->has_values = false; }   // (the same: the device values stay allocated)
// ---- row predicates (vg_rowpred.hip): "which rows a query may see", as a condition over the handle's labels / values.  The single
// and the range forms of the labeled, the label-set and the valued scans turn theirs into the scratch bitmap d_label_bits and run the
// masked kernel tables over it (VG_ROWS_BITMAP below).  A fourth predicate: a kind, a constructor, a device functor, a case each in
// vg_pred_refusal / vg_pred_allows_nothing / vg_pred_bits_enqueue, and its extern "C" entry points
enum VgPredKind { VG_PRED_LABEL, VG_PRED_LABELSET, VG_PRED_VALUE };
struct VgRowPred {
    VgPredKind kind;
    const char *noun;                          // "labeled" / "label-set" / "valued": what messages call the scans
    uint32_t label; bool use_label;            // LABEL: the label.  VALUE: use_label - the row must also carry `label`
    const uint32_t *set; int64_t n_set; int exclude;   // LABELSET: the caller's labels, any order, on the host
    int64_t lo, hi;                            // VALUE: the closed interval
};
static inline VgRowPred vg_pred_label(uint32_t label) { return VgRowPred{VG_PRED_LABEL, "labeled", label, true, nullptr, 0, 0, 0, 0}; }
static inline VgRowPred vg_pred_labelset(const uint32_t *labels, int64_t n, int exclude) {
    return VgRowPred{VG_PRED_LABELSET, "label-set", 0u, false, labels, n, exclude ? 1 : 0, 0, 0};
}
static inline VgRowPred vg_pred_value(int64_t lo, int64_t hi) { return VgRowPred{VG_PRED_VALUE, "valued", 0u, false, nullptr, 0, 0, lo, hi}; }
static inline VgRowPred vg_pred_value_labeled(int64_t lo, int64_t hi, uint32_t label) {
    return VgRowPred{VG_PRED_VALUE, "valued", label, true, nullptr, 0, 0, lo, hi};
}
// what depends on the condition, in the order every form refuses: the column it reads is set (values first, then labels - also
// required where the result is grouped by label), then the condition itself (VG_LABEL_NONE, a bad set pointer / count).  VG_OK: go on
int vg_pred_refusal(const vg_corpus *c, const char *who, const VgRowPred &pred, bool needs_labels_for_grouping);
bool vg_pred_allows_nothing(const VgRowPred &pred);   // lo > hi, an empty set without `exclude`: count 0 without a launch
// d_label_bits <- "the row at p passes" for every row (bits behind n_rows clear), enqueued on the corpus stream, no wait.  A set is
// sorted and de-duplicated into lset_host and uploaded into d_lset from there: it does not move before the scan behind this call has
// waited for the stream
int vg_pred_bits_enqueue(vg_corpus *c, const VgRowPred &pred);
int vg_lset_reserve(vg_corpus *c, size_t bytes);      // vg_rowpred.hip: d_lset holds at least `bytes`
// `n` labels of a caller's set -> ascending and distinct in *out; false (and the message set in `who`'s name): a bad pointer / count
// or VG_LABEL_NONE in the set
bool vg_labelset_normalise(const char *who, const uint32_t *labels, int64_t n, std::vector<uint32_t> *out);
// the label-set batch (vg_multi_labelset.hip): what vg_fused_batch_run needs next to a VG_QROWS_MEMBER form - the
// queries' normalised sets in CSR form over the queries AS HANDED OVER (ordered by set: equal sets are neighbours), all on the host
struct VgLabelsetBatch { const uint32_t *flat; const int64_t *offsets; int exclude; };
// What a membership form (VG_QROWS_MEMBER) plugs into vg_fused_batch_run: where the allowed rows of its queries come from.  The
// routine owns groups, slices, passes and the fallback's loop; the form owns the three steps that know its conditions.  `ctx`: the
// form's conditions over the queries AS HANDED OVER (equal conditions are neighbours), on the host until the routine returns.
//   pack_group     appends the table of queries [g0, g1) - one membership group - to *data (dwords of d_lset) and says what
//                  member_enqueue needs to find it again (nd, total); a refusal in `who`'s name
//   member_enqueue the group's pre-pass on the corpus stream: d_member[row] bit j <- query g0 + j may see the row; the group's table
//                  sits at dword `at` of d_lset
//   bits_enqueue   the fallback, query i: d_label_bits <- its allowed rows, enqueued only where the condition differs from query
//                  i - 1's; *skip <- true where the condition allows no row at all (no launch, count 0)
struct VgMemberForm {
    const void *ctx;
    int (*pack_group)(const void *ctx, const char *who, int g0, int g1, std::vector<uint32_t> *data, int *nd, size_t *total);
    int (*member_enqueue)(vg_corpus *c, const void *ctx, size_t at, int nd, size_t total);
    int (*bits_enqueue)(vg_corpus *c, const void *ctx, int i, bool *skip);
};
// vg_multi_valued.hip: the membership pre-pass of one group of the valued batch - `nd` conditions of VG_VALUE_COND_DWORDS dwords
// each behind one count dword, at dword `at` of d_lset
int vg_value_member_enqueue(vg_corpus *c, size_t at, int nd, int any_label);

// next slot of the profiling ring (nullptr when profiling is off)
static inline hipEvent_t *vg_prof_slot(vg_corpus *c, uint8_t flags) {
    if (!c->profiling) return nullptr;
    const int slot = (int)(c->prof_launches % VG_PROF_RING);
    c->ev_flags[(size_t)slot] = flags;
    ++c->prof_launches;
    return &c->ev[(size_t)slot * VG_PROF_EVS];
}

// ---- internal entry points that cross translation units
int vg_metric_to_acc(int metric);                                  // vg_api.hip; -1 for an unknown metric
bool vg_metric_is_bits(int metric);                                // vg_api.hip: a distance over packed bit vectors (Hamming, Jaccard)
// vg_api.hip: VG_OK, or the refusal every entry point gives for its metric - unknown: VG_ERR_INVALID; Hamming or Jaccard distance
// over an element type other than uint8: VG_ERR_UNSUPPORTED, the message in `who`'s name
int vg_metric_check(int vtype, int metric, const char *who);
int vg_metric_check_tie(int vtype, int metric, int tie_order, const char *who);   // ... and either under tie_order = reference: VG_ERR_UNSUPPORTED
void vg_collect_timing(vg_corpus *c);                              // vg_api.hip: event times of the last launch
int vg_ensure_row_norms(vg_corpus *c);                             // vg_api.hip (uses the f16 / bf16 norm kernel of vg_scan.h)
struct VgShape { int lpr_log2; int U; bool long_rows; };           // launch shape of a scan: lanes per row, chunks per lane
bool vg_choose_shape(int nch, int vtype, int acc, VgShape *out, int u_cap);   // vg_api.hip
int vg_launch_merge(const uint64_t *dev_cand, int nlists, int k, uint64_t *dev_out_keys, int nq, hipStream_t stream);   // vg_api.hip
// vg_api.hip <-> vg_filter.hip (the filter scans of vg_scan_filter.h are a translation unit of their own)
int vg_launch_plain_scan(vg_corpus *c, int metric, const uint8_t *dev_query, int k, uint64_t *dev_out_keys, hipStream_t stream,
                         const ScanPlan &plan);                    // vg_api.hip: the plain scan + merge (the filter's pre-pass)
// vg_api.hip; mirror_*: three counter words the merge's workgroup copies on its way (the filter scans' pinned counter mirror)
int vg_launch_merge_one(const uint64_t *dev_cand, int nlists, int k, uint64_t *dev_out_keys, hipStream_t stream,
                        const unsigned long long *mirror_src = nullptr, unsigned long long *mirror_dst = nullptr);
int vg_plain_scan_shape(const vg_corpus *c, int metric, VgShape *out);   // vg_api.hip: launch shape of the plain kernel
// ---- what the launchers of the scan variants share (vg_api.hip; the kernel tables are vg_pick.h)
struct ScanArgs;                                                    // vg_device.h
typedef void (*scan_fn_t)(ScanArgs);
// workgroups of a launch over n_rows rows: the three formulas, side by side in vg_api.hip
long long vg_plain_scan_blocks(const vg_corpus *c, int64_t n_rows, const VgShape &s);    // top-k scans that end in the one-workgroup merge
long long vg_within_scan_blocks(const vg_corpus *c, int64_t n_rows, const VgShape &s);   // the single range scan: no lists, no merge
long long vg_percu_scan_blocks(const vg_corpus *c, int64_t n_rows, const VgShape &s);    // multi-query and filter scans: one per CU
// *acc = A_COSN where the plain scan reads cached row norms (f16 / bf16 cosine), the norms made sure of on the corpus stream
int vg_half_cosine_acc(vg_corpus *c, const VgShape &s, int *acc);
// the fields every scan kernel reads, everything else zero; n_rows < 0: the whole corpus
ScanArgs vg_scan_args(const vg_corpus *c, int metric, int acc, const VgShape &s, const uint8_t *dev_query, int k, int64_t n_rows = -1);
size_t vg_query_lds_bytes(const vg_corpus *c, const VgShape &s);   // the staged query in LDS (long rows: padded to whole slices)
// the launch itself (VG_BLOCK threads), behind the dynamic-LDS attribute step a window above 64 KiB needs; enqueue only
int vg_launch_scan_kernel(scan_fn_t fn, long long blocks, size_t smem, hipStream_t stream, const ScanArgs &a);
// ---- what the form descriptors below are made of
typedef scan_fn_t (*vg_pick_scan_fn_t)(int vtype, int acc, int U, bool long_rows);
// where ScanArgs.mask of a single or a range scan comes from: nowhere, the user's mask (then required), or the scratch bitmap
// d_label_bits a row predicate built on this stream in front of the scan (vg_pred_bits_enqueue)
enum VgRows { VG_ROWS_ALL, VG_ROWS_MASK, VG_ROWS_BITMAP };
// the same for a batch: the user's mask, a label per query (ScanArgs.labels / .qlabels; the caller hands the queries over ordered by
// label), or the membership dwords of the pass' group (ScanArgs.labels = d_member, the pass' bit offset in ScanArgs.within_cap)
enum VgBatchRows { VG_QROWS_ALL, VG_QROWS_MASK, VG_QROWS_LABEL, VG_QROWS_MEMBER };
// the result: the k nearest rows; the k nearest labels by their best row (ScanArgs.labels, the label-deduping merge, labels in the
// result); or the k nearest rows with at most per_label of one label (the grouped path with the cap, clamped to k, in
// ScanArgs.within_cap and the capped merge)
enum VgResultKind { VG_RESULT_PLAIN, VG_RESULT_GROUPED, VG_RESULT_CAPPED };
struct VgResult {
    VgResultKind kind; int per_label;
    bool with_labels() const { return kind != VG_RESULT_PLAIN; }
};
static inline VgResult vg_result_plain() { return VgResult{VG_RESULT_PLAIN, 0}; }
static inline VgResult vg_result_grouped() { return VgResult{VG_RESULT_GROUPED, 0}; }
static inline VgResult vg_result_capped(int per_label) { return VgResult{VG_RESULT_CAPPED, per_label}; }
// ---- the single range scan (vg_scan_within.hip: vg_within_run), shared by every range form: whose name errors carry, the kernel
// table (vg_pick_scan<Family> of the unit that holds the kernels), the allowed rows, and the columns the handle must hold
struct VgWithinForm { const char *who; vg_pick_scan_fn_t pick; VgRows rows; bool needs_labels; bool needs_values; };
static inline VgWithinForm vg_within_form(const char *who, vg_pick_scan_fn_t pick, VgRows rows) { return VgWithinForm{who, pick, rows, false, false}; }
// what every single range scan answers first, whatever its form: the counts zeroed, NULL arguments, the held result and the launch
// count of the scan in front dropped, then the metric and the radius.  VG_OK: go on
int vg_within_begin(vg_corpus *c, const char *who, int metric, const void *query, double radius, int64_t *out_matches, int64_t *out_held);
int vg_within_run(vg_corpus *c, const VgWithinForm &f, int metric, const void *query, double radius, int64_t limit, int64_t *out_matches,
                  int64_t *out_held);
scan_fn_t vg_pick_scan_within_masked(int vtype, int acc, int U, bool long_rows);   // vg_scan_within_masked.hip: the masked single range scan's kernel table
scan_fn_t vg_pick_multi_within_masked(int vtype, int acc, int U, int NQ);   // vg_multi_within_masked.hip: the masked batch range scan's kernel table
scan_fn_t vg_pick_multi_within_labeled(int vtype, int acc, int U, int NQ);  // vg_multi_within_labeled.hip: the labeled batch range scan's kernel table
// ---- the fused top-k scan of a variant (k <= 64, ascending (distance, scan position) order): whose name errors carry and what they
// call the scans (`noun`), the kernel table, the allowed rows, the columns the handle must hold, the result, and `after` - ScanArgs.floor
// is set (the paged scans).  vg_fused_run (vg_scan_masked.hip): one query; `floor` = the smallest key admitted (after forms).
// vg_fused_batch_run (vg_multi_masked.hip): nq queries, `floors` = a key each (after forms, nullptr otherwise); the fallback of a
// shape without a multi-query form is nq calls of vg_fused_run with the single form.
typedef scan_fn_t (*vg_pick_multi_fn_t)(int vtype, int acc, int U, int NQ);
scan_fn_t vg_pick_scan_masked(int vtype, int acc, int U, bool long_rows);   // vg_scan_masked.hip: the masked single scan's kernel table
scan_fn_t vg_pick_scan_after(int vtype, int acc, int U, bool long_rows);    // vg_scan_after.hip: the paged single scans' tables,
scan_fn_t vg_pick_scan_after_masked(int vtype, int acc, int U, bool long_rows);   // ... all rows / the allowed rows
struct VgFusedForm {
    const char *who; const char *noun; vg_pick_scan_fn_t pick;
    VgRows rows; bool needs_labels; bool needs_values; VgResult result; bool after;
};
// a form over all rows or the user's mask; a result by label requires labels.  Anything else: set the field by name
static inline VgFusedForm vg_fused_form(const char *who, const char *noun, vg_pick_scan_fn_t pick, VgRows rows, VgResult result = vg_result_plain()) {
    return VgFusedForm{who, noun, pick, rows, result.with_labels(), false, result, false};
}
struct VgFusedBatchForm { const char *who; vg_pick_multi_fn_t pick; VgBatchRows rows; VgFusedForm single; };
int vg_fused_run(vg_corpus *c, const VgFusedForm &f, int metric, const void *query, int k, uint64_t floor, uint64_t *out_keys, int *out_count,
                 uint32_t *out_labels = nullptr);
// vg_scan_grouped.hip: the label-deduping final merge of `nlists` <= 256 per-workgroup lists (keys only; a key's label is
// labels[position]) on `stream`: dev_out receives 64 keys (VG_EMPTY_KEY padded) followed by their 64 labels - VG_KEYS_BYTES in all
int vg_launch_merge_grouped(const uint64_t *dev_cand, int nlists, int k, const uint32_t *dev_labels, uint64_t *dev_out, hipStream_t stream);
// vg_scan_capped.hip: the same for the capped scans - at most `per_label` (1 .. k) keys of one label among the k
int vg_launch_merge_capped(const uint64_t *dev_cand, int nlists, int k, int per_label, const uint32_t *dev_labels, uint64_t *dev_out, hipStream_t stream);
int vg_fused_batch_run(vg_corpus *c, const VgFusedBatchForm &f, int metric, const void *queries, int nq, int k, const uint64_t *floors,
                       uint64_t *out_keys, int *out_counts, const uint32_t *qlabels = nullptr, uint32_t *out_labels = nullptr,
                       const VgMemberForm *member = nullptr);
// vg_scan_masked.hip: the winners' keys as rows - query i's counts[i] keys at keys + i * k become (rowid, distance[, label]) at
// out_* + i * k.  labels / out_labels: both or neither; a single scan is nq = 1
void vg_keys_to_rows(const vg_corpus *c, const uint64_t *keys, const uint32_t *labels, int nq, int k, const int *counts, int64_t *out_rowids,
                     double *out_dist, uint32_t *out_labels);
// ---- the single and the range form of every row predicate (vg_rowpred.hip): argument checks, vg_pred_refusal, the answer without a
// launch, the bitmap, then vg_fused_run / vg_within_run with a VG_ROWS_BITMAP form over the masked table of the result.  out_labels:
// required by a result with labels, ignored otherwise
int vg_pred_topk_keys(vg_corpus *c, const char *who, VgResult result, const VgRowPred &pred, int metric, const void *query, int k,
                      uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int vg_pred_topk_rows(vg_corpus *c, const char *who, VgResult result, const VgRowPred &pred, int metric, const void *query, int k,
                      int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int vg_pred_within(vg_corpus *c, const char *who, const VgRowPred &pred, int metric, const void *query, double radius, int64_t limit,
                   int64_t *out_matches, int64_t *out_held);
VgFusedForm vg_pred_form(const char *who, const VgRowPred &pred, VgResult result);   // ... that form (the fallback of the batches names it)
// ---- a batch that runs its queries in an order of its own (by label, by set, by condition: equal ones become neighbours)
// the stable order of nq queries under `less(x, y)` over caller indices
template <class Less> static inline std::vector<int> vg_stable_order(int nq, Less less) {
    std::vector<int> order((size_t)nq);
    for (int i = 0; i < nq; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), less);
    return order;
}
// the query block in that order: slot i holds the caller's query order[i]
static inline std::vector<uint8_t> vg_permute_queries(const vg_corpus *c, const void *queries, const std::vector<int> &order) {
    const size_t row_bytes = (size_t)c->dim * c->es;
    std::vector<uint8_t> sq(order.size() * row_bytes);
    for (size_t i = 0; i < order.size(); ++i) memcpy(sq.data() + i * row_bytes, (const uint8_t *)queries + (size_t)order[i] * row_bytes, row_bytes);
    return sq;
}
// run(ordered queries, keys, counts) over buffers in that order - keys: nq x k, nullptr where the caller's out_keys is; counts: zeroed -
// then, when it answered VG_OK, keys and counts back at the caller's indices.  out_counts is not touched before `run` returns
template <class Run> static inline int vg_ordered_batch(const vg_corpus *c, const void *queries, int nq, int k, const std::vector<int> &order,
                                                        uint64_t *out_keys, int *out_counts, Run run) {
    const std::vector<uint8_t> sq = vg_permute_queries(c, queries, order);
    std::vector<uint64_t> skeys((k >= 1 && k <= VG_WAVE_HOST) ? (size_t)nq * k : 1);
    std::vector<int> scounts((size_t)nq, 0);
    int rc = run((const void *)sq.data(), out_keys ? skeys.data() : nullptr, scounts.data());
    if (rc != VG_OK) return rc;
    for (int i = 0; i < nq; ++i) {
        const int dst = order[(size_t)i];
        out_counts[dst] = scounts[(size_t)i];
        memcpy(out_keys + (size_t)dst * k, skeys.data() + (size_t)i * k, (size_t)scounts[(size_t)i] * sizeof(uint64_t));
    }
    return VG_OK;
}
// the rows form of a batch over its keys form: NULL arguments (args_null: the caller's own test of them, the corpus included), the
// counts zeroed, the outputs checked where nq and k (k_ok) size them, then run(keys, labels) into buffers of nq x k - labels only
// for with_labels - and the keys as rows
template <class Run> static inline int vg_batch_rows_from_keys(const vg_corpus *c, const char *who, bool args_null, int nq, int k, bool k_ok,
                                                               bool with_labels, int64_t *out_rowids, double *out_dist, uint32_t *out_labels,
                                                               int *out_counts, Run run) {
    if (args_null) return vg_fail(VG_ERR_INVALID, "%s: NULL argument", who);
    for (int i = 0; i < nq; ++i) out_counts[i] = 0;
    const bool sized = nq >= 1 && k_ok;
    if (sized && (!out_rowids || !out_dist || (with_labels && !out_labels))) return vg_fail(VG_ERR_INVALID, "%s: NULL output", who);
    std::vector<uint64_t> keys(sized ? (size_t)nq * k : 1);
    std::vector<uint32_t> labels(!with_labels ? 0 : sized ? (size_t)nq * k : 1);
    uint32_t *labs = with_labels ? labels.data() : nullptr;
    int rc = run(keys.data(), labs);
    if (rc != VG_OK) return rc;
    vg_keys_to_rows(c, keys.data(), labs, nq, k, out_counts, out_rowids, out_dist, out_labels);
    return VG_OK;
}
// vg_multi_masked.hip: what every vg_batch_*_plan answers - `pick`: the form's multi-query kernel table; queries per pass (0: the
// table has no instance for the shape, the single scans serve it) and the launch shape of whichever runs.  Refuses a NULL corpus and
// an unknown metric
int vg_batch_plan_report(const vg_corpus *c, int metric, vg_pick_multi_fn_t pick, int *out_queries_per_pass, int *out_lpr, int *out_u);
// vg_scan_grouped.hip: the host merge of several corpora's labeled lists behind vg_merge_keys_grouped (cap 1) and
// vg_merge_keys_capped (cap per_label), whose argument checks stay their own; `who` names the caller in the core's one refusal
int vg_merge_keys_by_label(const char *who, const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets,
                           int k, int cap, uint64_t *out_keys, uint32_t *out_labels, int *out_count);
// vg_multi_labelset.hip: the membership pre-pass of one group - d_member[row] bit j <- query j of the group may see the row.  The
// group's data sits in d_lset at dword offset `at`: [nd offsets + 1 | nd query masks | the nd distinct sets back to back]
int vg_labelset_member_enqueue(vg_corpus *c, size_t at, int nd, size_t total, int exclude);
scan_fn_t vg_pick_multi_labelset(int vtype, int acc, int U, int NQ);   // vg_multi_labelset.hip: the label-set batch's kernel table
int vg_member_reserve(vg_corpus *c);                  // vg_multi_labelset.hip: d_member holds a dword per row
// the batch launch of that merge (vg_multi_grouped.hip): workgroup n merges query n's `nlists` lists ([nq][nlists][64] keys at dev_cand) and writes its 64
// keys and 64 labels at dev_out + n * VG_KEYS_BYTES.  A VgFusedBatchForm with a grouped result (vg_multi_grouped.hip) ends in it:
// vg_fused_batch_run then sets ScanArgs.labels, requires labels, sizes a slice's key buffer for the labels and fills out_labels (nq x k)
int vg_launch_merge_grouped_batch(const uint64_t *dev_cand, int nlists, int k, const uint32_t *dev_labels, uint64_t *dev_out, int nq, hipStream_t stream);
scan_fn_t vg_pick_scan_grouped(int vtype, int acc, int U, bool long_rows);          // vg_scan_grouped.hip: the grouped single scans' tables,
scan_fn_t vg_pick_scan_grouped_masked(int vtype, int acc, int U, bool long_rows);   // ... all rows / the allowed rows
scan_fn_t vg_pick_multi_grouped_masked(int vtype, int acc, int U, int NQ);          // vg_multi_grouped_masked.hip: the masked grouped batch's table
// the capped batch (vg_multi_capped.hip): a VgFusedBatchForm with a capped result - vg_fused_batch_run then puts the
// cap, clamped to k, into ScanArgs.within_cap and ends every pass in this merge in place of the grouped batch's; the rest is that path
int vg_launch_merge_capped_batch(const uint64_t *dev_cand, int nlists, int k, int per_label, const uint32_t *dev_labels, uint64_t *dev_out, int nq,
                                 hipStream_t stream);
scan_fn_t vg_pick_scan_capped(int vtype, int acc, int U, bool long_rows);           // vg_scan_capped.hip: the capped single scans' tables,
scan_fn_t vg_pick_scan_capped_masked(int vtype, int acc, int U, bool long_rows);    // ... all rows / the allowed rows
scan_fn_t vg_pick_multi_capped_masked(int vtype, int acc, int U, int NQ);           // vg_multi_capped_masked.hip: the masked capped batch's table
// ---- paged scans (vg_scan_after.hip, vg_multi_after.hip): the floor-key forms behind the C ABI, what the shards call per shard.
// Floors are keys over positions LOCAL to the corpus; a floor of VG_KEY_EMPTY admits nothing (no launch in the single form).
int vg_after_floor_run(vg_corpus *c, bool masked, int metric, const void *query, int k, uint64_t floor, uint64_t *out_keys, int *out_count);
int vg_after_floor_batch_run(vg_corpus *c, bool masked, int metric, const void *queries, int nq, int k, const uint64_t *floors,
                             uint64_t *out_keys, int *out_counts);
int64_t vg_corpus_rows_upto_rowid(const vg_corpus *c, int64_t rowid);   // vg_scan_after.hip: rows held with rowid <= `rowid`; -2: rowids not ascending
// ---- range-scan results (vg_scan_within.hip), shared by the single and the batch form
float vg_within_radius(double radius);                              // the largest float not above the radius
// `count` keys at dev_keys -> *dst, ascending and cut to `limit`.  Up to VG_WITHIN_HOST_SORT keys: the copy is only enqueued and
// *pending set - the caller waits for the corpus stream once, then calls vg_within_finish; more: sorted on the device, waits itself
int vg_within_collect(vg_corpus *c, const unsigned long long *dev_keys, int64_t count, int64_t limit, std::vector<uint64_t> *dst, bool *pending);
void vg_within_finish(std::vector<uint64_t> *dst, int64_t count, int64_t limit);
// keys / rows [first, first + n) of a held result; outside it: VG_ERR_INVALID in `who`'s name
int vg_within_held_keys(const char *who, const std::vector<uint64_t> &held, int64_t first, int64_t n, uint64_t *out_keys);
int vg_within_held_rows(const vg_corpus *c, const char *who, const std::vector<uint64_t> &held, int64_t first, int64_t n, int64_t *out_rowids,
                        double *out_dist);
int vg_launch_scan_filter(vg_corpus *c, int metric, const uint8_t *dev_query, int k, uint64_t *dev_out_keys, hipStream_t stream,
                          bool ref_emit = false, uint64_t *final_out = nullptr);   // vg_filter.hip; -1: not served
int vg_scan_topk_enqueue_plan(vg_corpus *c, int metric, const void *query, int k, bool ref_emit);   // vg_api.hip: vg_scan_topk_enqueue with the reference-order extras
bool vg_scan_filter_would_serve(const vg_corpus *c, int metric, int k);   // vg_filter.hip: a single scan would take a filter scan right now
bool vg_scan_filter_policy(const vg_corpus *c);      // vg_filter.hip: filter switched on for this corpus and the corpus large enough for the shadow copy to pay
int vg_ensure_filter_counters(vg_corpus *c);         // vg_filter.hip: d_filter_evals[2] + pinned mirror
bool vg_scan_filter_name(vg_corpus *c, int metric, char *out, size_t out_len);   // vg_filter.hip: kernel name when the filter serves the scan
bool vg_batch_keys_are_scan_exact(const vg_corpus *c, int metric, int k);   // vg_batch_api.hip: a batch's floats are the single scan's
long long vg_bf16_shadow_stride(const vg_corpus *c);               // vg_batch_api.hip: row stride of the bf16 shadow copy of an f32 corpus
int vg_ensure_bf16_shadow(vg_corpus *c);                           // vg_batch_api.hip: build / extend it (corpus stream)
int vg_ensure_q8_shadow(vg_corpus *c);                             // vg_filter.hip: the int8 shadow copy + per-row (scale, residual norm)
int vg_multi_queries_per_pass(const vg_corpus *c, int metric);     // vg_multi.hip: queries per pass of the multi-query scan, 0 = none
int vg_launch_scan_multi(vg_corpus *c, int metric, const uint8_t *dev_queries, int k, uint64_t *dev_cand,
                         uint64_t *dev_out_keys, hipStream_t stream);   // vg_multi.hip; -1: no multi-query kernel for this shape
int vg_multi_plan(const vg_corpus *c, int metric, VgShape *s);     // vg_multi.hip: queries per pass + the launch shape they run with
