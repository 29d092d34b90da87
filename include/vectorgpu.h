/*
 * vectorgpu.h - C-ABI of the MI355X (gfx950) brute-force distance-scan + top-k engine.
 *
 * This is the drop-in boundary for sqlite-vector's hot path.  The SQLite extension host
 * (sqlite-vector_amd/ext/vector_ext.c, plain C) keeps the reference's SQL surface and calls only the
 * functions below; everything behind them is HIP.  Plain pointers and sizes, opaque handles, int return
 * codes (0 = VG_OK); no C++/torch/SQLite types.  Citations are file:line under /root/reference/src/.
 *
 * What each entry point replaces in the reference:
 *   vg_backend_name         distance_backend_name               distance-cpu.c:20, vector_backend() sqlite-vector.c:2549
 *   vg_corpus_*             the per-query "SELECT pk, col FROM tbl" row stream      sqlite-vector.c:2077-2096
 *                           and t_ctx->preloaded / precounter (quantized preload)   sqlite-vector.c:138-139, 1338-1404
 *   vg_scan_topk            vcursor_run_callback + vcursor_sort_callback            sqlite-vector.c:183-184
 *                           = vFullScanRun / vQuantRunMemory + vFullScanSortSlots   sqlite-vector.c:2071-2157, 2051-2069
 *                           incl. dispatch_distance_table[metric][type]             distance-cpu.c:21, distance-cpu.h:60
 *                           and the nearly_zero_float32 clamp                       sqlite-vector.c:994-996, 2099
 *   vg_scan_distances       the per-row body of the *_stream cursors                sqlite-vector.c:1901-1998
 *   vg_scan_topk_batch      (no reference entry point: Q independent vector_full_scan calls)
 *   vg_quantize_query       quantize_float32/16/b16/u8/i8 on the query              sqlite-vector.c:2166-2177, 495-757
 *
 * Result contract (differs from the reference only where the reference is history-dependent):
 *   - distances are the reference's float values (int8/uint8: bit-exact with distance-avx2.c; f32: <= 1e-5 rel);
 *   - order is ascending (distance, scan position); NaN and +Inf distances never enter (strict '<' vs INFINITY
 *     slots, sqlite-vector.c:1809,2102); fewer than k rows come back when fewer qualify (:1816-1817).
 */
#ifndef VECTORGPU_H
#define VECTORGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* same numbering as the reference's enums, distance-cpu.h:36-58 */
enum { VG_TYPE_F32 = 1, VG_TYPE_F16 = 2, VG_TYPE_BF16 = 3, VG_TYPE_U8 = 4, VG_TYPE_I8 = 5 };
enum { VG_DIST_L2 = 1, VG_DIST_SQUARED_L2 = 2, VG_DIST_COSINE = 3, VG_DIST_DOT = 4, VG_DIST_L1 = 5,
       VG_DIST_HAMMING = 6 /* not a metric of the reference: see below */,
       VG_DIST_JACCARD = 7 /* Jaccard / Tanimoto distance, not a metric of the reference either: see below */ };
/* Hamming distance (VG_DIST_HAMMING): rows are bit vectors packed 8 dimensions to a byte, served for VG_TYPE_U8 corpora only - a row
 * of `dim` bytes is 8 * dim bits and the query is `dim` bytes like every uint8 query.  The distance of a row is popcount(q XOR x)
 * over its `dim` bytes, returned as a float: exact (8 * dim < 2^24 for every supported row length) and always finite; the zero
 * padding of both sides contributes nothing.  Every entry point that takes a metric serves it - plain, masked, range (the radius
 * compares against this float), paged, labeled, label-set, valued, grouped and capped scans, single and batch, one corpus or shards -
 * with the order, counts, VG_KEY_EMPTY padding and rowid mapping of every other metric.  Over any other element type the call is
 * refused with VG_ERR_UNSUPPORTED ("<entry point>: Hamming distance needs a uint8 corpus") behind the argument checks that return
 * VG_ERR_INVALID and in front of any launch, counts and outputs zeroed as for the entry point's other refusals.  tie_order =
 * reference (corpus, shard set, vg_slab_scan_begin) together with it is VG_ERR_UNSUPPORTED: the reference has no such metric and so
 * no history-dependent order to reproduce.  The batch never takes the matrix cores and the single scan never the nibble filter:
 * vg_batch_last_path() reports 5 (multi-query scan) or 6 (single scans). */
/* Jaccard / Tanimoto distance (VG_DIST_JACCARD): the distance of sparse bit sets of varying weight (fingerprints, tag and shingle
 * sets), over the same rows as Hamming distance - VG_TYPE_U8 corpora only, `dim` bytes = 8 * dim bits a row, the query `dim` bytes.
 * With i = popcount(q AND x) and u = popcount(q OR x) over the row's `dim` bytes the distance is the float (float)(u - i) / (float)u:
 * two exact int-to-float conversions (u <= 8 * dim < 2^24) and ONE correctly rounded IEEE single division - not 1.0f - i / u, which
 * rounds twice - and 0.0f where u == 0 (query and row both empty).  It is always finite and lies in [0, 1]; the zero padding of
 * either side contributes nothing to i or u; equal rationals give equal floats (1/2, 2/4, 64/128), so ties are ordered as everywhere:
 * (distance, scan position).  (Rows of 2^17 bytes and more: a non-zero distance of at most 8 * 2^-23 comes back as 0.0f, the
 * engine's near-zero rule of every metric; no shorter row can have one.)  Every entry point that takes a metric serves it - plain,
 * masked, range (the radius compares against this float), paged, labeled, label-set, valued, grouped and capped scans, single and
 * batch, one corpus or shards, k > 64 - with the order, counts, VG_KEY_EMPTY padding and rowid mapping of every other metric.  The
 * refusals are Hamming's two in the same positions: over any other element type VG_ERR_UNSUPPORTED ("<entry point>: Jaccard
 * distance needs a uint8 corpus") behind the argument checks that return VG_ERR_INVALID and in front of any launch, counts and
 * outputs zeroed; with tie_order = reference (corpus, shard set, vg_slab_scan_begin) VG_ERR_UNSUPPORTED.  The batch never takes the
 * matrix cores and the single scan never the nibble filter: vg_batch_last_path() reports 5 or 6. */
enum { VG_QUANT_AUTO = 0, VG_QUANT_U8 = 1, VG_QUANT_S8 = 2 };

enum {
    VG_OK = 0,
    VG_ERR_INVALID = 1,      /* bad argument */
    VG_ERR_NO_DEVICE = 2,    /* no usable gfx950 device / HIP runtime failure at init */
    VG_ERR_NOMEM = 3,        /* device or host allocation failed */
    VG_ERR_HIP = 4,          /* any other HIP runtime error (see vg_last_error) */
    VG_ERR_UNSUPPORTED = 5   /* valid request the engine does not implement (see vg_last_error) */
};

typedef struct vg_corpus vg_corpus;    /* one HBM-resident N x D matrix + host rowid map, on one device */
/* Threading: different handles may be used from different threads at the same time (each owns its stream and
 * buffers; vg_last_error is thread-local).  ONE handle must not be used by two threads at once - the extension
 * keeps one set of handles per connection, like the reference keeps one context per connection. */

/* ---- process / device ---- */
int         vg_device_count(void);                 /* number of visible HIP devices (0 if none) */
const char *vg_backend_name(void);                 /* "HIP gfx950" style string, static storage */
const char *vg_last_error(void);                   /* thread-local message of the last failing call */

/* ---- corpus staging ("stage once into HBM") ----
 * Rows are stored row-major with a 16-byte-multiple stride (zero padded), base 256-byte aligned, in scan order.
 * rowids == NULL means rowid = 1-based scan position (+ vg_corpus_set_rowid_base). */
int     vg_corpus_create(int device, int vtype, int dim, int64_t capacity_rows_hint, vg_corpus **out);
void    vg_corpus_destroy(vg_corpus *c);
int     vg_corpus_clear(vg_corpus *c);
int     vg_corpus_reserve(vg_corpus *c, int64_t capacity_rows);   /* grow HBM to hold that many rows (no-op if it does) */
int     vg_corpus_trim(vg_corpus *c);                              /* give back a reservation more than 25 % above the rows held */
int     vg_corpus_clone(const vg_corpus *src, vg_corpus **out);    /* the same rows, rowids and switches again (device-to-device copy): copy-on-write */
int64_t vg_corpus_rows(const vg_corpus *c);
int     vg_corpus_dim(const vg_corpus *c);
int     vg_corpus_type(const vg_corpus *c);
int     vg_corpus_device(const vg_corpus *c);
int64_t vg_corpus_hbm_bytes(const vg_corpus *c);   /* bytes of HBM held by the row matrix */
int     vg_corpus_set_rowid_base(vg_corpus *c, int64_t base);   /* implicit rowid = base + position (default 1) */

/* host rows, any byte stride >= dim*elem_size (NULL rows in the SQL table are simply not appended, :2093).
 * The rows are copied into a pinned bounce buffer before the call returns (the caller may reuse host_rows at once);
 * the H2D transfer itself is only enqueued, so staging overlaps with the caller producing the next block. */
int vg_corpus_append(vg_corpus *c, const void *host_rows, int64_t n_rows, int64_t row_stride_bytes,
                     const int64_t *rowids);
/* the reference's persisted/preloaded quantized format: n records of [int64 LE rowid][dim bytes], stride 8+dim
 * (sqlite-vector.c:1296-1309, 2127-2147).  Corpus type must be U8 or I8.  De-interleaved on the GPU. */
int vg_corpus_append_records(vg_corpus *c, const void *host_records, int64_t n_records);
/* Row maintenance - what keeps a resident corpus equal to the table after UPDATE / DELETE without re-reading the table (the
 * reference re-reads it for every scan, sqlite-vector.c:2077-2107).  vg_corpus_find_rowid: scan position of a rowid (-1: not
 * held; -2: the rowids were not appended in ascending order, no lookup).  vg_corpus_patch_rows: overwrite the rows at
 * `positions` with host_rows[i].  vg_corpus_delete_rows: take the rows at `positions` (strictly ascending) out and close the
 * gaps on the device - scan order, hence every tie-break, stays that of a fresh staging.  Per-row derived data (norms, shadow
 * copies) is re-made from the first touched row on by the next scan that needs it. */
int64_t vg_corpus_find_rowid(const vg_corpus *c, int64_t rowid);
int     vg_corpus_patch_rows(vg_corpus *c, const int64_t *positions, int64_t n, const void *host_rows, int64_t row_stride_bytes);
int     vg_corpus_delete_rows(vg_corpus *c, const int64_t *positions, int64_t n);
/* rows already in device memory (same device), e.g. produced by another kernel / a torch tensor */
int vg_corpus_append_device(vg_corpus *c, const void *dev_rows, int64_t n_rows, int64_t row_stride_bytes,
                            const int64_t *host_rowids);

/* ---- the hot path ---- */
/* One query (dim elements of the corpus type, host memory) -> the k best rows.
 * out_rowids[k], out_dist[k] (float values widened to double, like vFullScanCursor.distance), *out_count <= k.
 * Large f32 / f16 / bf16 corpora, k <= 64 (L2 / SQUARED_L2 / DOT / COSINE; f16 / bf16 also L1): the scan goes through a
 * provable LOWER BOUND of every row's distance and evaluates only the candidates exactly, with the plain kernel's own
 * arithmetic - the same rowids and distance bits as the plain scan.  From 2^20 rows and 512 MB it streams an int8 shadow copy
 * (per row: int8 elements + scale + residual norm; built on the first such scan after rows were appended or patched; + 26 %
 * device memory for f32, + 52 % for f16 / bf16; a quarter resp. half of the bytes per query); L1 (f16 / bf16) streams the rows
 * themselves (the bound replaces the reference's f64 chain for non-candidates).  VG_SCAN_FILTER_SHADOW=bf16: f32 corpora
 * (>= 3 GB) through a bf16 shadow copy (+ 50 %), f16 / bf16 (>= 1 GB) through their own rows.  vg_corpus_set_scan_filter(c, 0)
 * / VG_SCAN_FILTER=0 turn it off; a corpus whose shadow copy does not fit device memory, or whose rows the bound cannot tell
 * apart (it evaluates more than 1/8 of them), keeps the plain scan by itself.  uint8 / int8 corpora (2^20 rows, 768 MB): a
 * high-nibble shadow copy (+ 52 %, half the bytes), used only if a probe over a 2M-row prefix finds the data selective under it
 * (vg_corpus_set_scan_filter(c, 1): without the probe). */
int vg_scan_topk(vg_corpus *c, int metric, const void *query, int k,
                 int64_t *out_rowids, double *out_dist, int *out_count);

/* Same scan, but the k candidates stay on the device as packed 64-bit keys
 * (hi 32 = order-preserving image of the float distance, lo 32 = scan position), ascending, padded with
 * VG_KEY_EMPTY.  dev_query / dev_out_keys are device pointers (dev_query: the dim elements followed by ZERO bytes up
 * to the next 16-byte multiple; dev_out_keys: 64 keys); stream is a hipStream_t (NULL = the corpus' own stream).
 * No host synchronisation: this is what one rank of a row-sharded multi-GPU scan runs before the candidate
 * gather (RCCL) and what bench.py times. */
int vg_scan_topk_device(vg_corpus *c, int metric, const void *dev_query, int k,
                        uint64_t *dev_out_keys, void *stream);
#define VG_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull
/* decode / merge helpers for gathered keys (host side, tiny): */
float   vg_key_distance(uint64_t key);
uint32_t vg_key_position(uint64_t key);
/* k-way merge of n_lists key lists (each list_len long, ascending, VG_KEY_EMPTY padded), list i's positions are
 * offset by pos_offsets[i] (NULL = 0) to form global scan positions; ties broken by (list index, position) which
 * equals global scan position order for row-range shards.  Returns count written (<= k). */
int vg_merge_keys(const uint64_t *keys, int n_lists, int list_len, const int64_t *pos_offsets, int k,
                  int64_t *out_global_pos, double *out_dist);

/* the same merge for nq queries at once: keys[list][query][list_len] (an all_gather of every shard's
 * vg_scan_topk_batch_keys output), out_global_pos / out_dist are nq x k, out_counts nq.  Returns 0, -1 on bad arguments. */
int vg_merge_keys_batch(const uint64_t *keys, int n_lists, int nq, int list_len, const int64_t *pos_offsets, int k,
                        int64_t *out_global_pos, double *out_dist, int *out_counts);

/* The host-side scan again, but returning the packed keys (positions, not rowids) - the form a multi-shard caller
 * merges.  vg_scan_topk_keys: any k, out_keys[min(k, rows)], synchronous.  enqueue / collect: the fused path
 * (k <= 64) split in two, so that several corpora (one per device) are all in flight before the first wait;
 * collect fills 64 keys (VG_KEY_EMPTY padded; all empty for an empty corpus). */
int vg_scan_topk_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, int *out_count);
int vg_scan_topk_enqueue(vg_corpus *c, int metric, const void *query, int k);
int vg_scan_topk_collect(vg_corpus *c, uint64_t *out_keys64);

/* All N distances in scan order (clamp applied), for the *_stream table-valued functions. */
int vg_scan_distances(vg_corpus *c, int metric, const void *query, float *out_dist_host);
int vg_scan_distances_device(vg_corpus *c, int metric, const void *dev_query, float *dev_out_dist, void *stream);
/* rowid of a scan position (host map) */
int64_t vg_corpus_rowid_at(const vg_corpus *c, int64_t position);

/* ---- range scans: every row within a distance of the query (no reference entry point; the reference's form is
 * "SELECT ... FROM vector_full_scan_stream(...) WHERE distance <= r": N rows stepped to keep a handful) ----
 * A row matches when its distance d - the float vg_scan_distances reports for it, bit for bit - satisfies (double)d <= radius.
 * NaN and +Inf distances never match, whatever the radius (the top-k contract: they never enter a list); radius = +Inf means
 * "every row with a finite distance"; a NaN radius is VG_ERR_INVALID.  The host turns the radius into the largest float not above
 * it, so the device compares floats and decides what SQLite's comparison of the stream function's output would decide.
 * Order: ascending (distance, scan position), whatever the handle's tie_order (membership does not depend on history).
 * limit > 0: the first `limit` matches in that order are held, *out_matches still counts all of them; limit <= 0: all are held.
 * The compare-and-compact runs inside the streaming scan kernel (nothing is written for a row that does not match); the caller
 * never guesses a buffer size and the corpus is never scanned twice to learn one - only a result larger than the device buffer
 * (2^20 keys to start with) costs ONE more launch into a buffer of the counted size.
 * The result stays on the handle, in host memory, until the next call that scans or changes the handle; vg_scan_within_fetch copies
 * rows [first, first + n) of it as (rowid, distance widened to double), vg_scan_within_keys as packed keys with positions local to
 * this corpus - the form a multi-shard caller merges.  out_rowids / out_dist may be NULL (not wanted).  vg_scan_within_masked (below)
 * leaves its result in the same place: either call overwrites what the other one held.  The handle's row mask is not read. */
int vg_scan_within(vg_corpus *c, int metric, const void *query, double radius, int64_t limit,
                   int64_t *out_matches, int64_t *out_held);
int vg_scan_within_fetch(const vg_corpus *c, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist);
int vg_scan_within_keys(const vg_corpus *c, int64_t first, int64_t n, uint64_t *out_keys);

/* ---- batch range scans: nq queries (row-major nq x dim, host), a radius each - "for each of these vectors, every row within r":
 * near-duplicate detection, similarity joins, neighbourhood queries.  out_matches / out_held are nq (either may be NULL).
 * Query i's answer is what vg_scan_within(c, metric, q_i, radii[i], limit, ..) is contracted to return: the rows with
 * (double)d <= radii[i]; NaN / +Inf distances never match, whatever the radius; radii[i] = +Inf means every row with a finite
 * distance; each radius is turned into the largest float not above it; ascending (distance, scan position) whatever the handle's
 * tie_order; limit > 0 holds the first `limit` matches PER QUERY while out_matches[i] still counts all of them.
 * f32 / uint8 / int8 rows of a register-resident shape: 4 queries (2 where a lane holds 4 or 6 chunks of the row) share every row
 * load of a pass (vg_scan_multi.h, range form; the plan: vg_within_batch_plan, vectorgpu_diag.h), nq queries cost ceil(nq / 4) - or
 * ceil(nq / 2) - such passes.  Queries go up in slices; the passes of a slice are enqueued back to back with one copy of the counts
 * and one wait behind them.  A query's device region starts as a share of one fixed budget of keys (2^20 over the queries of a
 * slice); a pass in which a query counted past its region runs ONCE more as a whole into regions of the counted sizes - passes that
 * fit are not launched again, and a partial answer is never returned.
 * uint8 / int8: rowids, order, distance bits and counts identical to nq vg_scan_within calls.  f32: the single scan's arithmetic per
 * (query, row) pair, possibly under another lane decomposition (the multi-query scans' launch shape) - the single range scan's
 * result bit for bit where the two shapes agree; elsewhere its distances up to the summation order, so a row whose distance lies
 * within that difference of the radius may fall on either side.  f16 / bf16, long rows and every other shape without a multi-query
 * form: nq single vg_scan_within calls whose results are copied into the per-query storage - same contract, no sharing.  Timings
 * not measured yet.
 * nq < 1 or a NULL c / queries / radii: VG_ERR_INVALID; any NaN radius: VG_ERR_INVALID before any launch; unknown metric:
 * VG_ERR_INVALID - each with the counts zeroed first.  An empty corpus: every count 0 without a launch.
 * The result stays on the handle, in host memory, per query, until the next call that scans or changes the handle (the single
 * vg_scan_within keeps its own result apart); vg_scan_within_batch_fetch / _keys copy rows [first, first + n) of query `query` as
 * (rowid, distance widened to double) / packed keys with positions local to this corpus; a query index or a row range outside what
 * is held: VG_ERR_INVALID.  vg_scan_within_batch_masked (below) leaves its result in the same place: either call overwrites what the
 * other one held.  The handle's row mask is not read. */
int vg_scan_within_batch(vg_corpus *c, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                         int64_t *out_matches, int64_t *out_held);
int vg_scan_within_batch_fetch(const vg_corpus *c, int query, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist);
int vg_scan_within_batch_keys(const vg_corpus *c, int query, int64_t first, int64_t n, uint64_t *out_keys);

/* ---- masked scans: the k nearest rows among an allowed set ("... of this tenant / this category"; no reference entry point) ----
 * A row mask is a bitmap over scan positions kept on the handle, in device memory (rows / 8 bytes): bit (p & 63) of 64-bit word
 * (p >> 6) set = the row at scan position p may be returned.  Setting it and scanning are two calls: one filter serves many queries.
 * vg_corpus_set_mask_bits: n_bits <= rows, the rows behind n_bits are not allowed.  vg_corpus_set_mask_rowids: the rowids are
 * mapped to positions on the host (implicit rowids: rowid - base; an ascending map: the search behind vg_corpus_find_rowid; a map
 * that is not ascending: VG_ERR_UNSUPPORTED); rowids the corpus does not hold are ignored, duplicates are harmless, *out_set (may
 * be NULL) = rows allowed.  vg_corpus_mask_count: rows allowed, -1 without a mask.
 * ONLY the masked scans (vg_scan_topk_masked[_keys], vg_scan_topk_batch_masked[_keys], vg_scan_within_masked, vg_scan_within_batch_masked) read the mask: every other call behaves the same with and without one.  The row mask and the
 * labels (labeled scans, below) are independent: the labeled scans do not read the mask, the masked scans do not read the labels.  A call that changes the
 * number of rows or which row sits at which position (append*, delete_rows, clear) drops the mask; patch_rows, reserve and trim
 * keep it; vg_corpus_clone copies it.
 * vg_scan_topk_masked: the contract of vg_scan_topk restricted to the allowed rows - NaN / +Inf never enter, fewer than k rows
 * when fewer allowed rows qualify, every distance the float vg_scan_distances reports for that row, bit for bit - in ascending
 * (distance, scan position) order whatever the handle's tie_order.  The plain streaming kernel with one scalar load of mask bits
 * per batch of rows: a batch without an allowed row is not read (by construction; timings not measured yet).  1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below);
 * no mask set: VG_ERR_INVALID; an empty mask: *out_count = 0 without a launch.  vg_scan_topk_masked_keys: the same as packed keys
 * with positions local to this corpus (out_keys[k]) - the form a multi-shard caller merges. */
int     vg_corpus_set_mask_bits(vg_corpus *c, const uint64_t *words, int64_t n_bits);
int     vg_corpus_set_mask_rowids(vg_corpus *c, const int64_t *rowids, int64_t n, int64_t *out_set);
int     vg_corpus_clear_mask(vg_corpus *c);
int64_t vg_corpus_mask_count(const vg_corpus *c);
int     vg_scan_topk_masked(vg_corpus *c, int metric, const void *query, int k,
                            int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, int *out_count);

/* ---- masked batch scans: one row mask, nq queries (row-major nq x dim, host) - "the k nearest rows of this tenant, for these 50
 * queries".  The mask is the one vg_corpus_set_mask_* left on the handle; these calls, vg_scan_topk_masked[_keys] and the masked range
 * scans (vg_scan_within_masked, vg_scan_within_batch_masked) are the only ones that read it - vg_scan_topk_batch still ignores it.  out_rowids / out_dist are nq x k, out_counts nq; the slots of
 * query i behind out_counts[i] are NOT written.
 * Query i's answer is what vg_scan_topk_masked is contracted to return for it: only allowed rows, ascending (distance, scan
 * position) whatever the handle's tie_order, NaN / +Inf never enter, fewer than k rows when fewer allowed rows qualify.
 * f32 / uint8 / int8 rows of a register-resident shape: 4 queries (2 where a lane holds 4 or 6 chunks of the row) share every row
 * load of a pass, and a pass reads only the batches of rows that hold an allowed row (vg_scan_multi.h, masked form; the plan:
 * vg_batch_masked_plan, vectorgpu_diag.h); nq queries cost ceil(nq / 4) - or ceil(nq / 2) - such passes, enqueued back to back with
 * one wait at the end.  uint8 / int8: rowids, order and distance bits identical to nq vg_scan_topk_masked calls.  f32: the single
 * scan's arithmetic per (query, row) pair, possibly under another lane decomposition (the multi-query scans' launch shape) - the
 * single masked scan's bits where the two shapes agree, its floats up to the summation order elsewhere.  f16 / bf16, long rows and
 * every other shape without a multi-query form: nq single masked scans - same contract, no sharing.  Timings not measured yet
 * (DESIGN.md 3.9).
 * 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below); nq < 1 or a NULL argument: VG_ERR_INVALID; no mask set:
 * VG_ERR_INVALID; an empty mask or an empty corpus: every count 0 without a launch.  vg_scan_topk_batch_masked_keys: the same as
 * packed keys with positions local to this corpus (out_keys nq x k) - the form a multi-shard caller merges. */
int     vg_scan_topk_batch_masked(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                  int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                       uint64_t *out_keys, int *out_counts);

/* ---- labeled scans: a label per row, each query its own label - the equality filter on a metadata column ("the k nearest rows of
 * tenant T", and in a batch a different T per query; no reference entry point) ----
 * A label is a uint32_t per scan position kept on the handle, in device memory (4 bytes per row).  vg_corpus_set_labels: n must equal
 * vg_corpus_rows(c) (VG_ERR_INVALID otherwise); VG_LABEL_NONE is the "no label" value - such a row matches no query.
 * vg_corpus_has_labels: 1 while labels are set.  Lifetime: the mask's, rule for rule - append*, delete_rows and clear drop the
 * labels; patch_rows, reserve and trim keep them; vg_corpus_clone copies them.
 * ONLY the labeled scans (vg_scan_topk_labeled[_keys], vg_scan_topk_batch_labeled[_keys]) read the labels: every other call behaves
 * the same with and without them.  Labels and row mask are independent: the labeled scans do not read the mask (and leave it as it
 * is), the masked scans do not read the labels.
 * vg_scan_topk_labeled: the contract of vg_scan_topk_masked with "allowed" meaning labels[p] == label - ascending (distance, scan
 * position) whatever the handle's tie_order, NaN / +Inf never enter, every distance the float vg_scan_distances reports for that
 * row, bit for bit.  A small kernel turns (labels, label) into a bitmap in a scratch buffer of the handle, then the single masked
 * kernels run over it: two launches on the corpus stream, one wait.  1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below);
 * no labels set: VG_ERR_INVALID; label == VG_LABEL_NONE: VG_ERR_INVALID; an empty corpus or a label no row carries: *out_count = 0.
 * vg_scan_topk_labeled_keys: the same as packed keys with positions local to this corpus (out_keys[k]).
 * vg_scan_topk_batch_labeled: nq queries (row-major nq x dim, host), query i's answer is what vg_scan_topk_labeled(c, metric, q_i,
 * k, query_labels[i], ..) is contracted to return; out_rowids / out_dist are nq x k, the slots of query i behind out_counts[i] are
 * NOT written.  f32 / uint8 / int8 rows of a register-resident shape: the queries are ordered by label, then 4 (or 2) of them share
 * every row load of a pass; a row is computed once with its batch and offered only to the queries whose label it carries, and a
 * batch of rows that carries none of the pass' labels is not read (vg_scan_multi.h, labeled form; the plan: vg_batch_labeled_plan,
 * vectorgpu_diag.h).  uint8 / int8: identical to nq vg_scan_topk_labeled calls; f32: the floats of vg_scan_topk_batch_masked under
 * the same launch shape.  f16 / bf16, long rows and every other shape without a multi-query form: one single labeled scan per query,
 * one bitmap per distinct label of the batch.  Any query_labels[i] == VG_LABEL_NONE, nq < 1 or a NULL argument: VG_ERR_INVALID, with
 * the counts zeroed first.  Timings not measured yet. */
#define VG_LABEL_NONE 0xFFFFFFFFu
int     vg_corpus_set_labels(vg_corpus *c, const uint32_t *labels, int64_t n);
int     vg_corpus_clear_labels(vg_corpus *c);
int     vg_corpus_has_labels(const vg_corpus *c);
int     vg_scan_topk_labeled(vg_corpus *c, int metric, const void *query, int k, uint32_t label,
                             int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_labeled_keys(vg_corpus *c, int metric, const void *query, int k, uint32_t label, uint64_t *out_keys, int *out_count);
int     vg_scan_topk_batch_labeled(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                   int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_labeled_keys(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                        uint64_t *out_keys, int *out_counts);

/* ---- grouped scans: the k nearest LABELS, each represented by its best row - rows are chunks, the label is the document (product,
 * user) a chunk belongs to, the caller wants the k nearest documents (no reference entry point).  The labels are those of the labeled
 * scans (vg_corpus_set_labels).  Contract:
 *   take every row with a finite distance and a label other than VG_LABEL_NONE (the masked forms: whose mask bit is set as well);
 *   1. order them by the 64-bit scan key, i.e. by (distance, scan position), whatever the handle's tie_order;
 *   2. walk that order and keep the first row of each label;
 *   3. return the first k rows kept - (rowid, distance, label), ascending by key.
 * Fewer than k labels present: fewer results.  Every distance is the float vg_scan_distances reports for that row, bit for bit; NaN /
 * +Inf rows never enter; a row without a label is never returned.  One pass over the rows: the label (4 bytes per row) rides with the
 * row prefetch and the candidate lists stay distinct by label in the kernel, the workgroup merge and the final merge (all on the
 * device, corpus stream); one copy brings back k keys and k labels.  A top-k with a host-side dedupe is NOT this: one label owning
 * the 64 nearest rows hides every other label from it.
 * 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below); no labels set: VG_ERR_INVALID; the masked forms without a mask:
 * VG_ERR_INVALID; NULL arguments: VG_ERR_INVALID; an empty corpus or an empty mask: *out_count = 0, nothing is launched.
 * Not served: f16 corpora with rows of 2049 .. 3072 elements under the cosine and dot metrics (VG_ERR_UNSUPPORTED: the kernels of that
 * shape do not fit the register file with a label per lane; L2 and L1 are served).
 * The _keys forms return packed keys with positions local to this corpus (out_keys[k], out_labels[k]).
 * vg_merge_keys_grouped (host): the label-deduping twin of vg_merge_keys for lists of several corpora, because one label can live on
 * several of them - keys / labels are n_lists x list_len (ascending lists, VG_KEY_EMPTY padded), list i's positions are offset by
 * pos_offsets[i] (NULL = 0); the three steps above over the union, by (distance, global position); out_keys carry the GLOBAL position
 * (which must fit 32 bits: VG_ERR_UNSUPPORTED otherwise).  n_lists, list_len or k < 1, or a NULL argument: VG_ERR_INVALID. */
int     vg_scan_topk_grouped(vg_corpus *c, int metric, const void *query, int k,
                             int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_grouped_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_grouped_masked(vg_corpus *c, int metric, const void *query, int k,
                                    int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_grouped_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t *out_keys, uint32_t *out_labels,
                                         int *out_count);
int     vg_merge_keys_grouped(const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets, int k,
                              uint64_t *out_keys, uint32_t *out_labels, int *out_count);

/* ---- grouped batch scans: the k nearest labels for each of nq queries (row-major nq x dim, host) - "the k nearest documents, for
 * these 64 requests".  Query i's answer is exactly what vg_scan_topk_grouped (the _masked forms: vg_scan_topk_grouped_masked) is
 * contracted to return for query i alone.  out_rowids / out_dist / out_labels are nq x k, out_counts nq; the slots of query i behind
 * out_counts[i] are NOT written.
 * f32 / uint8 / int8 rows of a register-resident shape: 4 queries (2 where a lane holds 4 or 6 chunks of the row) share every row
 * load - and every label load - of a pass (vg_scan_multi.h, grouped form; the plan: vg_batch_grouped_plan, vectorgpu_diag.h); each
 * query keeps its own list, distinct by label, and the lists of a query merge on the device; nq queries cost ceil(nq / 4) - or
 * ceil(nq / 2) - passes, enqueued back to back, one copy of keys and labels, one wait.  uint8 / int8: rowids, labels, order and
 * distance bits identical to nq vg_scan_topk_grouped calls; f32: the floats of vg_scan_topk_batch_masked under the same launch
 * shape.  f16 / bf16, long rows and every other shape without a multi-query form (the masked forms only: also rows of 193 .. 384
 * 16-byte chunks under cosine, and under L2 for f32 - DESIGN.md 3.16): one single grouped scan per query - a shape that
 * scan refuses (f16 cosine / dot over rows of 2049 .. 3072 elements) is VG_ERR_UNSUPPORTED here too.
 * 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below); nq < 1 or a NULL argument: VG_ERR_INVALID, with the counts zeroed
 * first where there are counts; no labels set: VG_ERR_INVALID; the masked forms without a mask: VG_ERR_INVALID; an empty corpus or an
 * empty mask: every count 0, nothing is launched.  The _keys forms return packed keys with positions local to this corpus (out_keys
 * and out_labels nq x k) - the form a multi-shard caller merges per query with vg_merge_keys_grouped. */
int     vg_scan_topk_batch_grouped(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                   int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_grouped_keys(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                        uint64_t *out_keys, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_grouped_masked(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_grouped_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k,
                                               uint64_t *out_keys, uint32_t *out_labels, int *out_counts);

/* ---- capped scans: the k nearest ROWS, at most per_label of one label - rows are chunks, the label is the document (product, brand) a
 * chunk belongs to, the caller wants "the 20 nearest chunks, but no more than 3 of any document" (group_size / max hits per group
 * elsewhere; no reference entry point).  The labels are those of the labeled scans (vg_corpus_set_labels).  Contract, m = per_label:
 *   1. take every row with a finite distance and a label other than VG_LABEL_NONE (the masked forms: whose mask bit is set as well);
 *   2. order them by the 64-bit scan key, i.e. by (distance, scan position), whatever the handle's tie_order;
 *   3. walk that order and keep a row iff fewer than m rows of its label have been kept;
 *   4. return the first k rows kept - (rowid, distance, label), ascending by key.
 * m = 1 is vg_scan_topk_grouped's contract and returns its answer bit for bit; m above k behaves as k.  Every distance is the float
 * vg_scan_distances reports for that row; NaN / +Inf rows never enter; a row without a label is never returned.  One pass over the
 * rows: the grouped scans' kernels with a list that holds up to m rows of a label (a new row of a full label replaces the label's
 * worst kept row), the same merges on the device, one copy of k keys and k labels.  A top-k with a host-side cap is NOT this: one label
 * owning the 64 nearest rows hides every other row from it.
 * 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below); per_label < 1: VG_ERR_INVALID; no labels set: VG_ERR_INVALID; the
 * masked forms without a mask: VG_ERR_INVALID; NULL arguments: VG_ERR_INVALID; an empty corpus or an empty mask: *out_count = 0,
 * nothing is launched.  Not served, like the grouped scans: f16 corpora with rows of 2049 .. 3072 elements under the cosine and dot
 * metrics (VG_ERR_UNSUPPORTED; L2 and L1 are served).  The batch form: vg_scan_topk_batch_capped, below; no SQL function yet.
 * The _keys forms return packed keys with positions local to this corpus (out_keys[k], out_labels[k]).
 * vg_merge_keys_capped (host): vg_merge_keys_grouped with the cap, for lists of several corpora that are each a capped answer with
 * the same k and per_label - the four steps over the union, by (distance, global position); same layout, offsets and errors, and
 * per_label < 1: VG_ERR_INVALID. */
int     vg_scan_topk_capped(vg_corpus *c, int metric, const void *query, int k, int per_label,
                            int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_keys(vg_corpus *c, int metric, const void *query, int k, int per_label,
                                 uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_masked(vg_corpus *c, int metric, const void *query, int k, int per_label,
                                   int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_masked_keys(vg_corpus *c, int metric, const void *query, int k, int per_label,
                                        uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_merge_keys_capped(const uint64_t *keys, const uint32_t *labels, int n_lists, int list_len, const int64_t *pos_offsets, int k,
                             int per_label, uint64_t *out_keys, uint32_t *out_labels, int *out_count);

/* ---- capped batch scans: the k nearest rows, at most per_label of one label, for each of nq queries (row-major nq x dim, host) -
 * "the 20 nearest chunks, no more than 3 of any document, for these 64 requests".  Query i's answer is exactly what
 * vg_scan_topk_capped (the _masked forms: vg_scan_topk_capped_masked) is contracted to return for query i alone - the four steps
 * above; one per_label = m covers the whole batch, m above k behaves as k, and m = 1 returns what vg_scan_topk_batch_grouped returns,
 * bit for bit.  out_rowids / out_dist / out_labels are nq x k, out_counts nq; the slots of query i behind out_counts[i] are NOT
 * written.
 * f32 / uint8 / int8 rows of a register-resident shape: the grouped batch's passes - 4 queries (2 where a lane holds 4 or 6 chunks
 * of the row) share every row load and every label load (vg_scan_multi.h, capped form; the plan: vg_batch_capped_plan,
 * vectorgpu_diag.h) - each query keeps its own capped list, and the lists of a query merge on the device; one copy of keys and
 * labels, one wait.  uint8 / int8: rowids, labels, order and distance bits identical to nq vg_scan_topk_capped calls; f32: the floats
 * of vg_scan_topk_batch_masked under the same launch shape.  f16 / bf16, long rows and every other shape without a multi-query form
 * (the masked forms only: also rows of 193 .. 384 16-byte chunks under cosine, and under L2 for f32 - DESIGN.md 3.18): one single
 * capped scan per query - a shape that scan refuses (f16 cosine / dot over rows of 2049 .. 3072 elements) is VG_ERR_UNSUPPORTED here
 * too.
 * nq < 1 or a NULL argument: VG_ERR_INVALID, answered before the handle is read; k < 1 or per_label < 1: VG_ERR_INVALID, k > 64:
 * VG_ERR_UNSUPPORTED, with the counts zeroed first; no labels set: VG_ERR_INVALID; the masked forms without a mask: VG_ERR_INVALID; an
 * empty corpus or an empty mask: every count 0, nothing is launched.  No cap per query and no SQL function.  The _keys forms return
 * packed keys with positions local to this corpus (out_keys and out_labels nq x k) - the form a multi-shard caller merges per query
 * with vg_merge_keys_capped. */
int     vg_scan_topk_batch_capped(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label,
                                  int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_capped_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label,
                                       uint64_t *out_keys, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_capped_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label,
                                         int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_scan_topk_batch_capped_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, int per_label,
                                              uint64_t *out_keys, uint32_t *out_labels, int *out_counts);

/* ---- label-set scans: the labeled, grouped and capped scans over the rows whose label is in a SET of labels, or - exclude != 0 - is
 * not in it: access control ("the documents of the groups this user belongs to"), facets ("category IN (...)"), exclusion ("not the
 * documents already shown" - and with it exact paging through grouped results, which stop at 64 labels per call; no reference entry
 * point).  The labels are those of the labeled scans (vg_corpus_set_labels).
 * A label set is n_labels >= 0 labels (labels may be NULL when n_labels == 0): order does not matter, duplicates are allowed and mean
 * nothing, VG_LABEL_NONE in a set is VG_ERR_INVALID.  exclude == 0: a row is ALLOWED iff it carries a label and that label is in the
 * set; exclude != 0: iff it carries a label and that label is NOT in the set.  A row without a label (VG_LABEL_NONE) is never
 * allowed.  An empty set with exclude == 0 allows no row: count 0, not an error; an empty set with exclude != 0 allows every labeled
 * row.  The handle's row mask is neither read nor written by any of these calls.
 * vg_scan_topk_labelset: the contract of vg_scan_topk_masked over the allowed rows - rows with a finite distance, ascending (distance,
 * scan position) whatever the handle's tie_order, the first k, every distance the float vg_scan_distances reports for that row, bit
 * for bit.  The host sorts the set and uploads it into scratch the handle owns; a small kernel (one binary search per row) turns
 * (labels, set, exclude) into a bitmap in the scratch buffer the labeled scans use, then the single masked kernels run over it.
 * vg_scan_topk_grouped_labelset / vg_scan_topk_capped_labelset: what vg_scan_topk_grouped_masked / vg_scan_topk_capped_masked are
 * contracted to return under a mask holding exactly the allowed rows - the same bitmap in front of the masked grouped / capped
 * kernels, so the shapes those leave out stay VG_ERR_UNSUPPORTED (f16 cosine and dot over rows of 2049 .. 3072 halves).
 * Paging grouped results: call with exclude = 1 and the labels returned so far; the pages, concatenated, are the grouped order.
 * All forms: 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below, the count(s) zeroed first); no labels set: VG_ERR_INVALID;
 * an empty corpus: VG_OK with count 0; per_label < 1: VG_ERR_INVALID.  The _keys forms: packed keys, positions local to this corpus.
 * vg_scan_topk_batch_labelset: nq queries (row-major nq x dim, host), each its OWN set - query i's is set_labels[set_offsets[i] ..
 * set_offsets[i + 1]) (CSR: nq + 1 offsets that do not decrease, VG_ERR_INVALID otherwise), one `exclude` for the whole batch.  Query
 * i's answer is what vg_scan_topk_labelset(c, metric, q_i, k, its set, exclude, ..) is contracted to return, in caller order;
 * out_rowids / out_dist are nq x k, the slots of query i behind out_counts[i] are NOT written; nq < 1: VG_ERR_INVALID.  f32 / uint8 /
 * int8 rows of a register-resident shape: the queries are ordered by their sets, a pre-pass per 32 queries reads the labels once and
 * writes one membership dword per row (n_rows dwords of scratch whatever nq), then 4 (or 2) queries share every row load of a pass;
 * a row is offered only to the queries that may see it and a batch of rows none of them may see is not read (vg_scan_multi.h,
 * label-set form; the plan: vg_batch_labelset_plan, vectorgpu_diag.h).  uint8 / int8: identical to nq single calls; f32: the floats
 * of vg_scan_topk_batch_masked under the same launch shape.  Every other shape: one single label-set scan per query, the bitmap
 * rebuilt only where the set changes.  Timings NOT measured. */
int     vg_scan_topk_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                              int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                                   uint64_t *out_keys, int *out_count);
int     vg_scan_topk_grouped_labelset(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                                      int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_grouped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                           int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_labelset(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                     int64_t n_labels, int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_labelset_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                          int64_t n_labels, int exclude, uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_batch_labelset(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                    const int64_t *set_offsets, int exclude, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_labelset_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                         const int64_t *set_offsets, int exclude, uint64_t *out_keys, int *out_counts);

/* ---- masked range scans: every ALLOWED row within a distance of the query - "every row of this tenant within r", near-duplicate
 * detection inside one category (no reference entry point; the reference's form is "SELECT ... FROM vector_full_scan_stream(...)
 * WHERE id IN (...) AND distance <= r": N rows stepped).  The contract is the conjunction of vg_scan_within's and vg_scan_topk_masked's.
 * The mask is the one vg_corpus_set_mask_* left on the handle.  A row matches when its bit is set AND its distance d - the float
 * vg_scan_distances reports for it, bit for bit - satisfies (double)d <= radius.  NaN and +Inf distances never match, whatever the
 * radius; radius = +Inf means "every allowed row with a finite distance"; the radius is turned into the largest float not above it.
 * Order: ascending (distance, scan position), whatever the handle's tie_order.  limit > 0: the first `limit` matches in that order
 * are held (per query), *out_matches still counts all of them; limit <= 0: all are held.
 * The kernels are the masked scans' loops with the range scans' compare-and-compact: a batch of rows without an allowed row is not
 * read, nothing is written for a row that does not match, and only ALLOWED matches take room in the device buffer - a result larger
 * than it costs ONE more launch into a buffer of the counted size, as in vg_scan_within (timings not measured yet).
 * vg_scan_within_masked leaves its result where vg_scan_within leaves its own and overwrites it (and the reverse): read it with
 * vg_scan_within_fetch / _keys.  vg_scan_within_batch_masked: nq queries (row-major nq x dim, host), a radius each, out_matches /
 * out_held nq (either may be NULL); it leaves its results where vg_scan_within_batch leaves its own and overwrites them (and the
 * reverse): read them with vg_scan_within_batch_fetch / _keys.  The single and the batch form keep their results apart.
 * Batch precision: f32 / uint8 / int8 rows of a register-resident shape share every row load of a pass among 4 (or 2) queries
 * (vg_scan_multi.h, masked range form; the plan: vg_within_batch_masked_plan, vectorgpu_diag.h), slices, key budget and the "a pass that
 * overflowed runs once more as a whole" rule as in vg_scan_within_batch.  uint8 / int8: rowids, order, distance bits and counts
 * identical to nq vg_scan_within_masked calls.  f32: the single scan's arithmetic per (query, row) pair under the multi-query launch
 * shape - bit for bit the single masked range scan where the two shapes agree, and as in vg_scan_within_batch elsewhere (for an
 * allowed row, vg_scan_within_batch's float, bit for bit).  f16 / bf16, long rows and every other shape without a multi-query form:
 * nq single vg_scan_within_masked calls whose results are copied into the per-query storage.
 * No mask set: VG_ERR_INVALID; a NaN radius: VG_ERR_INVALID before any launch; an unknown metric, a NULL c / query / queries / radii
 * or nq < 1: VG_ERR_INVALID - each with the counts zeroed first.  An empty mask or an empty corpus: every count 0 without a launch. */
int     vg_scan_within_masked(vg_corpus *c, int metric, const void *query, double radius, int64_t limit,
                              int64_t *out_matches, int64_t *out_held);
int     vg_scan_within_batch_masked(vg_corpus *c, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                    int64_t *out_matches, int64_t *out_held);

/* ---- labeled range scans: every row of a label within a distance of the query - "every row of this tenant within r" for a caller
 * who keeps tenants as labels: no bitmap per tenant, no upload per request, and in a batch a different tenant per query (no
 * reference entry point).  The labels are those of the labeled scans (vg_corpus_set_labels).  The contract is the conjunction of
 * vg_scan_within's and the labeled scans': a row matches when it carries an ALLOWED label AND its distance d - the float
 * vg_scan_distances reports for it, bit for bit - satisfies (double)d <= radius; NaN and +Inf distances never match, whatever the
 * radius; a row without a label (VG_LABEL_NONE) never matches; the radius is turned into the largest float not above it.  Order:
 * ascending (distance, scan position), whatever the handle's tie_order.  limit > 0: the first `limit` matches in that order are held
 * (per query), *out_matches still counts all of them; limit <= 0: all are held.  The row mask is neither read nor written.
 * vg_scan_within_labeled: allowed = labels[p] == label.  vg_scan_within_labelset: the set semantics of vg_scan_topk_labelset - order
 * and duplicates mean nothing, VG_LABEL_NONE in the set is VG_ERR_INVALID, exclude == 0: allowed iff the row's label is in the set
 * (an empty set allows nothing: counts 0, no launch), exclude != 0: iff the row carries a label that is NOT in the set (an empty set:
 * every labeled row).  Both: a small kernel turns (labels, label or set) into a bitmap in the scratch buffer the labeled scans use,
 * then the single masked range kernels run over it (no scan kernels of their own: the distances are vg_scan_within_masked's, bit for
 * bit, where both see the row) - two launches on the corpus stream, the scan once more when the result outgrew the device buffer.
 * They leave their result where vg_scan_within leaves its own and overwrite it (and the reverse): read it with vg_scan_within_fetch
 * / _keys.
 * vg_scan_within_batch_labeled: nq queries (row-major nq x dim, host), query i's answer is what vg_scan_within_labeled(c, metric,
 * q_i, radii[i], limit, query_labels[i], ..) is contracted to return, at the caller's index i; out_matches / out_held nq (either may
 * be NULL).  A query whose label is VG_LABEL_NONE: the rule of vg_scan_topk_batch_labeled - the whole call is VG_ERR_INVALID, with
 * every count zeroed first and nothing launched.  f32 / uint8 / int8 rows of a register-resident shape: the queries are ordered by
 * label, then 4 (or 2) of them share every row load of a pass; a row is computed once with its batch and compared only against the
 * radii of the queries whose label it carries, and a batch of rows that carries none of the pass' labels is not read (vg_scan_multi.h,
 * labeled range form; the plan: vg_within_batch_labeled_plan, vectorgpu_diag.h); slices, key budget and the "a pass that overflowed
 * runs once more as a whole" rule as in vg_scan_within_batch.  uint8 / int8: rowids, order, distance bits and counts identical to nq
 * vg_scan_within_labeled calls.  f32: the single scan's arithmetic per (query, row) pair under the multi-query launch shape - for a
 * row of the query's label, vg_scan_within_batch's float, bit for bit.  f16 / bf16, long rows and every other shape without a
 * multi-query form: nq single vg_scan_within_labeled calls whose results are copied into the per-query storage.  It leaves its
 * results where vg_scan_within_batch leaves its own and overwrites them (and the reverse): read them with vg_scan_within_batch_fetch
 * / _keys.  The single and the batch form keep their results apart.  Timings not measured yet.
 * No labels set: VG_ERR_INVALID; label == VG_LABEL_NONE: VG_ERR_INVALID; a NaN radius: VG_ERR_INVALID before any launch; an unknown
 * metric, a NULL c / query / queries / query_labels / radii or nq < 1: VG_ERR_INVALID - each with the counts zeroed first.  An empty
 * corpus or a label no row carries: every count 0 (the empty corpus without a launch). */
int     vg_scan_within_labeled(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, uint32_t label,
                               int64_t *out_matches, int64_t *out_held);
int     vg_scan_within_labelset(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, const uint32_t *labels,
                                int64_t n_labels, int exclude, int64_t *out_matches, int64_t *out_held);
int     vg_scan_within_batch_labeled(vg_corpus *c, int metric, const void *queries, int nq, const uint32_t *query_labels,
                                     const double *radii, int64_t limit, int64_t *out_matches, int64_t *out_held);

/* ---- value-range scans: an int64 per row, the k nearest rows whose value lies in [lo, hi] - "the 20 nearest chunks newer than T",
 * "priced between a and b", "of tenant 7 and from the last 30 days", "the nearest documents among the rows of this week" (no
 * reference entry point).
 * A value is an int64_t per scan position kept on the handle, in device memory (8 bytes per row); any int64 is a value, there is no
 * "none".  vg_corpus_set_values: n must equal vg_corpus_rows(c) (VG_ERR_INVALID otherwise); vg_corpus_has_values: 1 while values are
 * set.  Lifetime: the labels', rule for rule - append*, delete_rows and clear drop the values; patch_rows, reserve and trim keep
 * them; vg_corpus_clone copies them.  Values, labels and row mask are independent: only the calls below read the values, and they
 * neither read nor write the row mask.
 * A row is ALLOWED iff lo <= values[p] <= hi: a signed 64-bit comparison, the interval closed at both ends, INT64_MIN / INT64_MAX the
 * open ends.  lo > hi is the empty interval: VG_OK, count 0, nothing launched.
 * vg_scan_topk_valued: the contract of vg_scan_topk_masked over the allowed rows - rows with a finite distance, ascending (distance,
 * scan position) whatever the handle's tie_order, the first k, every distance the float vg_scan_distances reports for that row, bit
 * for bit.  A small kernel (one comparison per row, one ballot per 64 rows) turns (values, lo, hi) into a bitmap in the scratch buffer
 * the labeled scans use, then the single masked kernels run over it.  vg_scan_topk_valued_labeled: allowed additionally requires
 * labels[p] == label (the labels of vg_corpus_set_labels; none set, or label == VG_LABEL_NONE: VG_ERR_INVALID).
 * vg_scan_topk_grouped_valued / vg_scan_topk_capped_valued: filter by value, group by label - what vg_scan_topk_grouped_masked /
 * vg_scan_topk_capped_masked are contracted to return under a mask holding exactly the allowed rows; they need labels and values,
 * and the shapes those tables leave out stay VG_ERR_UNSUPPORTED.  per_label < 1: VG_ERR_INVALID; per_label = 1 is the grouped form.
 * vg_scan_within_valued: the contract of vg_scan_within_masked under that bitmap; it leaves its result where vg_scan_within leaves
 * its own: read it with vg_scan_within_fetch / _keys.
 * All top-k forms: 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below, the count(s) zeroed first); no values set:
 * VG_ERR_INVALID; an empty corpus: VG_OK with count 0.  The _keys forms: packed keys, positions local to this corpus.
 * vg_scan_topk_batch_valued: nq queries (row-major nq x dim, host), query i under its OWN interval [los[i], his[i]]; query_labels is
 * NULL or a label per query for the conjunction (then labels must be set; VG_LABEL_NONE in it: VG_ERR_INVALID with the counts zeroed
 * first).  Query i's answer is what the single form is contracted to return for it, in caller order; out_rowids / out_dist are nq x
 * k, the slots of query i behind out_counts[i] are NOT written; a query with lo > hi gets count 0; nq < 1: VG_ERR_INVALID.  f32 /
 * uint8 / int8 rows of a register-resident shape: the queries are ordered by (label, lo, hi), a pre-pass per 32 queries reads the
 * values (and labels) once and writes one membership dword per row, then the label-set multi-query instances run over it, 4 (or 2)
 * queries a pass (the plan: vg_batch_valued_plan, vectorgpu_diag.h).  Every other shape: one single valued scan per query, the
 * bitmap rebuilt only where the condition changes. */
int     vg_corpus_set_values(vg_corpus *c, const int64_t *values, int64_t n);
int     vg_corpus_clear_values(vg_corpus *c);
int     vg_corpus_has_values(const vg_corpus *c);
int     vg_scan_topk_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi,
                            int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                 uint64_t *out_keys, int *out_count);
int     vg_scan_topk_valued_labeled(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                    int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_valued_labeled_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                         uint64_t *out_keys, int *out_count);
int     vg_scan_topk_grouped_valued(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                    int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_grouped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                         uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_valued(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                   int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_scan_topk_capped_valued_keys(vg_corpus *c, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                        uint64_t *out_keys, uint32_t *out_labels, int *out_count);
int     vg_scan_within_valued(vg_corpus *c, int metric, const void *query, double radius, int64_t limit, int64_t lo, int64_t hi,
                              int64_t *out_matches, int64_t *out_held);
int     vg_scan_topk_batch_valued(vg_corpus *c, int metric, const void *queries, int nq, int k, const int64_t *los, const int64_t *his,
                                  const uint32_t *query_labels, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_valued_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const int64_t *los, const int64_t *his,
                                       const uint32_t *query_labels, uint64_t *out_keys, int *out_counts);

/* ---- paged scans: the next k rows behind a (distance, rowid) cursor ("search after"; the reference's surface has LIMIT k OFFSET m,
 * a top-(m + k) scan) ----
 * A cursor is (after_dist, after_rowid): the distance and rowid of the last row of the previous page.  The row at scan position p
 * with distance d - the float vg_scan_distances reports for it, bit for bit - is BEHIND the cursor iff d < +Inf (NaN / +Inf never
 * enter, -Inf is a legal distance) and ((double)d > after_dist, or (double)d == after_dist and rowid(p) > after_rowid).  Returned:
 * the first k such rows in ascending (distance, scan position) order whatever the handle's tie_order, fewer when fewer qualify.
 * 1 <= k <= 64 (VG_ERR_UNSUPPORTED above, VG_ERR_INVALID below).  Pages are exact when the cut falls inside a run of equal distances.
 * (-INFINITY, INT64_MIN) is "from the start"; a NaN distance: VG_ERR_INVALID; +Inf or a distance above FLT_MAX: *out_count = 0 without
 * a launch; -0.0 is 0.0; after_dist need not be a float (a midpoint between two held distances is valid).  The rowid form needs
 * ascending rowids (implicit ones are), as vg_corpus_set_mask_rowids does: VG_ERR_UNSUPPORTED otherwise.  rowid(p) > after_rowid is
 * then p >= P, P = rows held with rowid <= after_rowid (a lower bound, not a find): the cursor's row need not exist any more, a page
 * taken after it was deleted continues where it should.
 * How: every kernel ranks rows by the key sortable(distance) << 32 | scan position; the host turns the cursor into the smallest key
 * behind it (vg_after_floor, vectorgpu_diag.h) and the kernel admits a key iff key >= floor - one 64-bit compare in the offer of the
 * plain (or the masked) streaming kernel.  Timings not measured yet.
 * The _keys forms take the cursor as after_key, the LAST key of the previous page (floor = after_key + 1), and return packed keys with
 * positions local to this corpus; they work for any rowid layout; after_key = VG_KEY_EMPTY: VG_ERR_INVALID; 0 starts in front of every row.
 * The _masked forms read the handle's row mask (vg_corpus_set_mask_*): the same contract restricted to the allowed rows (the
 * cursor's row need not be allowed); no mask set: VG_ERR_INVALID; an empty mask: count 0 without a launch.
 * The batch forms answer nq queries (row-major nq x dim, host), a cursor each (after_dists / after_rowids / after_keys hold nq
 * values); out_rowids / out_dist / out_keys are nq x k, out_counts nq, the slots of query i behind out_counts[i] are NOT written.
 * Query i's answer is the single form's for its query and cursor, bit for bit, for every element type - a cursor taken from a
 * single page or from vg_scan_distances is valid in the batch form and the reverse.  uint8 / int8 rows of a register-resident shape,
 * and f32 rows whose multi-query launch shape is the plain scan's (the same summation order), share every row load of a pass among 4
 * (or 2) queries (vg_scan_multi.h, floor forms - the multi-query scan, not the matrix-core filters, whose thresholds assume an unrestricted
 * top-k); every other f32 shape, f16 / bf16 and long rows take one single paged scan per query. */
int     vg_scan_topk_after(vg_corpus *c, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                           int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_after_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t after_key,
                                uint64_t *out_keys, int *out_count);
int     vg_scan_topk_after_masked(vg_corpus *c, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                  int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_scan_topk_after_masked_keys(vg_corpus *c, int metric, const void *query, int k, uint64_t after_key,
                                       uint64_t *out_keys, int *out_count);
int     vg_scan_topk_batch_after(vg_corpus *c, int metric, const void *queries, int nq, int k, const double *after_dists,
                                 const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_after_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                      uint64_t *out_keys, int *out_counts);
int     vg_scan_topk_batch_after_masked(vg_corpus *c, int metric, const void *queries, int nq, int k, const double *after_dists,
                                        const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_scan_topk_batch_after_masked_keys(vg_corpus *c, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                             uint64_t *out_keys, int *out_counts);

/* nq queries at once (row-major nq x dim, host).  out_rowids / out_dist are nq x k, out_counts nq.
 * f32 corpora, k <= 32, rows <= 512 floats, metric DOT / COSINE / L2 / SQUARED_L2: one pass over the corpus on the
 * matrix cores (Q x C^T tiles feed per-query candidate lists; L2 survivors are re-evaluated with the direct formula);
 * rows of 513 .. 1024 floats: a bf16 shadow copy of the corpus feeds the matrix cores as a filter, every candidate is
 * re-evaluated on the f32 rows with the single scan's arithmetic - and so do shorter rows of a corpus the filter scan serves
 * (switched on, >= 3 GB: the shadow copy those scans make; the GEMM at the bf16 rate over half the bytes, the distances are
 * the single scans' distances; a selectivity guard falls back to the f32 matrix-core kernel on data the bound does not
 * separate; environment VG_F32_FILTER=0 / 1 forces it off / on).
 * uint8 / int8 corpora, k <= 32, rows <= 2048 bytes, same metrics: the integer matrix cores, results identical to
 * nq vg_scan_topk calls.  f16 / bf16 corpora, k <= 32, rows <= 1024 elements, same metrics: the matrix cores filter,
 * every candidate is re-evaluated with the single scan's f64 arithmetic.  Other shapes on f32 / uint8 / int8 corpora
 * with k <= 64: 4 (long rows: 2) queries share each pass of the scan kernel.  Everything else: nq single-query
 * scans.  Same result contract as vg_scan_topk (float batches: tolerance 1e-5, quantized batches bit-exact). */
int vg_scan_topk_batch(vg_corpus *c, int metric, const void *queries, int nq, int k,
                       int64_t *out_rowids, double *out_dist, int *out_counts);

/* same, as keys: out_keys nq x k (positions local to this corpus) */
int vg_scan_topk_batch_keys(vg_corpus *c, int metric, const void *queries, int nq, int k,
                            uint64_t *out_keys, int *out_counts);

/* ---- query-side quantizer (host, bit-exact with sqlite-vector.c:495-757) ---- */
int vg_quantize_query(int src_type, const void *src, int dim, float scale, float offset, int qtype, void *dst);

/* ---- vector_quantize on the staged corpus (sqlite-vector.c:1147-1336 moved to the GPU) ----
 * pass 1: global min / max / any-negative over every element, widened to float like :1228-1254;
 * pass 2: rows [row0, row0+n) quantized with (scale, offset, qtype) into n x dim tightly packed bytes on the host,
 *         bit-exact with quantize_* (:495-757).  The caller interleaves rowids into the persisted record format. */
int vg_corpus_minmax(vg_corpus *c, float *out_min, float *out_max, int *out_any_negative);
int vg_corpus_quantize_rows(vg_corpus *c, float scale, float offset, int qtype, int64_t row0, int64_t n_rows,
                            uint8_t *out_host);

/* ---- one logical corpus over several devices of ONE process (vg_shards.hip) ----
 * What the SQLite extension holds per (table, column): a connection lives in one process, so its multi-GPU form
 * is S per-device corpora driven from one host thread, not S processes.  Rows are dealt out
 * block-cyclically in scan order (block_rows rows per block, 0 = 65536); every call below is the vg_corpus_* /
 * vg_scan_* call of the same name with results merged by (distance, GLOBAL scan position): bit-identical to a
 * single corpus holding all rows.  devices == NULL means devices 0..n-1; the same device may be listed more than
 * once (logical shards - how the tests exercise this on a 1-GPU box).  With n_devices == 1 every call forwards. */
typedef struct vg_shards vg_shards;
int     vg_shards_create(const int *devices, int n_devices, int vtype, int dim, int64_t block_rows, vg_shards **out);
void    vg_shards_destroy(vg_shards *s);
int     vg_shards_clear(vg_shards *s);
int     vg_shards_count(const vg_shards *s);
int64_t vg_shards_rows(const vg_shards *s);
vg_corpus *vg_shards_shard(const vg_shards *s, int i);          /* borrow shard i (profiling, introspection) */
int     vg_shards_reserve(vg_shards *s, int64_t total_rows);
int     vg_shards_trim(vg_shards *s);                                                      /* vg_corpus_trim on every shard */
int     vg_shards_clone(const vg_shards *src, vg_shards **out);                            /* vg_corpus_clone of every shard */
int     vg_shards_set_rowid_base(vg_shards *s, int64_t base);
int     vg_shards_append(vg_shards *s, const void *host_rows, int64_t n_rows, int64_t row_stride_bytes, const int64_t *rowids);
int     vg_shards_append_records(vg_shards *s, const void *host_records, int64_t n_records);
int64_t vg_shards_rowid_at(const vg_shards *s, int64_t position);
int     vg_shards_rowids(const vg_shards *s, int64_t pos0, int64_t n, int64_t *out);   /* rowids of positions [pos0, pos0 + n) */
int64_t vg_shards_find_rowid(const vg_shards *s, int64_t rowid);                       /* single-shard handles only (else -2 / VG_ERR_UNSUPPORTED): */
int     vg_shards_patch_rows(vg_shards *s, const int64_t *positions, int64_t n, const void *host_rows, int64_t row_stride_bytes);
int     vg_shards_delete_rows(vg_shards *s, const int64_t *positions, int64_t n);
int     vg_shards_set_scan_filter(vg_shards *s, int mode);                             /* vg_corpus_set_scan_filter on every shard */
/* How the S x 64 candidate keys of a top-k scan reach the host: 0 = every shard copies its own 64 keys back (default), 1 = ONE grouped
 * ncclAllGather over RCCL / xGMI on the scan streams + one copy from the first device (librccl.so is dlopen'ed on first use; devices
 * must be distinct; any failure falls back to 0 for the handle).  Default from VECTORGPU_SHARD_GATHER=host|rccl.  Same keys, same
 * merge, same result either way (vg_shards_gather_stats, vectorgpu_diag.h, counts which form served). */
int     vg_shards_set_gather(vg_shards *s, int mode);
int     vg_shards_scan_topk(vg_shards *s, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_scan_topk_batch(vg_shards *s, int metric, const void *queries, int nq, int k,
                                  int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_shards_scan_distances(vg_shards *s, int metric, const void *query, float *out_dist_host);
/* vg_scan_within over every shard, merged by (distance, GLOBAL scan position): the rows, order and distance bits of one corpus holding
 * all rows.  Same contract; the merged result stays on the shards handle until its next scan. */
int     vg_shards_scan_within(vg_shards *s, int metric, const void *query, double radius, int64_t limit,
                              int64_t *out_matches, int64_t *out_held);
int     vg_shards_scan_within_fetch(const vg_shards *s, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist);
/* vg_scan_within_batch over every shard (each answers all nq queries over its own rows, same radii, same limit), merged per query by
 * (distance, GLOBAL scan position) and cut to `limit`: the answer of one corpus holding all rows.  Same contract; the merged result
 * stays on the shards handle until its next batch range scan. */
int     vg_shards_scan_within_batch(vg_shards *s, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                    int64_t *out_matches, int64_t *out_held);
int     vg_shards_scan_within_batch_fetch(const vg_shards *s, int query, int64_t first, int64_t n, int64_t *out_rowids, double *out_dist);
/* the row mask over GLOBAL scan positions (vg_corpus_set_mask_*): the bits are dealt out to the shards by the block-cyclic map of the
 * rows; vg_shards_scan_topk_masked = vg_scan_topk_masked of one corpus holding all rows (rowids, order and distance bits). */
int     vg_shards_set_mask_bits(vg_shards *s, const uint64_t *words, int64_t n_bits);
int     vg_shards_set_mask_rowids(vg_shards *s, const int64_t *rowids, int64_t n, int64_t *out_set);
int     vg_shards_clear_mask(vg_shards *s);
int64_t vg_shards_mask_count(const vg_shards *s);
int     vg_shards_scan_topk_masked(vg_shards *s, int metric, const void *query, int k,
                                   int64_t *out_rowids, double *out_dist, int *out_count);
/* vg_scan_topk_batch_masked over every shard (each answers all nq queries over its own bits), merged per query by (distance,
 * GLOBAL scan position): the answer of one corpus holding all rows.  Same contract. */
int     vg_shards_scan_topk_batch_masked(vg_shards *s, int metric, const void *queries, int nq, int k,
                                         int64_t *out_rowids, double *out_dist, int *out_counts);
/* the labels over GLOBAL scan positions (vg_corpus_set_labels: n must equal vg_shards_rows), dealt out to the shards by the
 * block-cyclic map of the rows; vg_shards_has_labels: 1 while every shard holds labels.  The labeled scans over every shard: each
 * shard answers over its own rows, merged per query by (distance, GLOBAL scan position) = one corpus holding all rows (rowids,
 * order and distance bits). */
int     vg_shards_set_labels(vg_shards *s, const uint32_t *labels, int64_t n);
int     vg_shards_clear_labels(vg_shards *s);
int     vg_shards_has_labels(const vg_shards *s);
int     vg_shards_scan_topk_labeled(vg_shards *s, int metric, const void *query, int k, uint32_t label,
                                    int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_scan_topk_batch_labeled(vg_shards *s, int metric, const void *queries, int nq, const uint32_t *query_labels, int k,
                                          int64_t *out_rowids, double *out_dist, int *out_counts);
/* the grouped scans over every shard: each shard answers over its own rows (its k nearest labels), the lists merge through
 * vg_merge_keys_grouped by (distance, GLOBAL scan position) - a label's rows may sit on several shards: the rowids, labels, order and
 * distance bits of one corpus holding all rows.  Same contract; at most 2^32 - 1 rows over all shards. */
int     vg_shards_scan_topk_grouped(vg_shards *s, int metric, const void *query, int k,
                                    int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_shards_scan_topk_grouped_masked(vg_shards *s, int metric, const void *query, int k,
                                           int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
/* vg_scan_topk_batch_grouped[_masked] over every shard: each shard answers all nq queries over its own rows, then every query's
 * lists merge through vg_merge_keys_grouped as above.  Same contract and errors. */
int     vg_shards_scan_topk_batch_grouped(vg_shards *s, int metric, const void *queries, int nq, int k,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_shards_scan_topk_batch_grouped_masked(vg_shards *s, int metric, const void *queries, int nq, int k,
                                                 int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
/* the capped scans over every shard: each shard answers over its own rows (its k nearest rows under the cap), the lists merge
 * through vg_merge_keys_capped by (distance, GLOBAL scan position): the rowids, labels, order and distance bits of one corpus holding
 * all rows.  Same contract; at most 2^32 - 1 rows over all shards. */
int     vg_shards_scan_topk_capped(vg_shards *s, int metric, const void *query, int k, int per_label,
                                   int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_shards_scan_topk_capped_masked(vg_shards *s, int metric, const void *query, int k, int per_label,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
/* vg_scan_topk_batch_capped[_masked] over every shard: each shard answers all nq queries over its own rows, then every query's
 * lists merge through vg_merge_keys_capped as above.  Same contract and errors. */
int     vg_shards_scan_topk_batch_capped(vg_shards *s, int metric, const void *queries, int nq, int k, int per_label,
                                         int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
int     vg_shards_scan_topk_batch_capped_masked(vg_shards *s, int metric, const void *queries, int nq, int k, int per_label,
                                                int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_counts);
/* label-set scans (see above): the sets name labels, which mean the same on every shard - every shard answers over its own rows and
 * the lists merge like the labeled / grouped / capped scans' */
int     vg_shards_scan_topk_labelset(vg_shards *s, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels, int exclude,
                                     int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_scan_topk_batch_labelset(vg_shards *s, int metric, const void *queries, int nq, int k, const uint32_t *set_labels,
                                           const int64_t *set_offsets, int exclude, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_shards_scan_topk_grouped_labelset(vg_shards *s, int metric, const void *query, int k, const uint32_t *labels, int64_t n_labels,
                                             int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_shards_scan_topk_capped_labelset(vg_shards *s, int metric, const void *query, int k, int per_label, const uint32_t *labels,
                                            int64_t n_labels, int exclude, int64_t *out_rowids, double *out_dist, uint32_t *out_labels,
                                            int *out_count);
/* value-range scans (see above): the values over GLOBAL scan positions (n must equal vg_shards_rows), dealt out to the shards as
 * the labels are; vg_shards_has_values: 1 while every shard holds values.  An interval means the same on every shard: every shard
 * answers over its own rows and the lists merge like the labeled / grouped / capped scans'; the range form is read with
 * vg_shards_scan_within_fetch.  The five top-k forms are named vg_shards_valued_scan_topk[_labeled | _batch | _grouped | _capped]
 * after the vg_scan_topk_valued, _valued_labeled, _batch_valued, _grouped_valued and _capped_valued they fan out to. */
int     vg_shards_set_values(vg_shards *s, const int64_t *values, int64_t n);
int     vg_shards_clear_values(vg_shards *s);
int     vg_shards_has_values(const vg_shards *s);
int     vg_shards_valued_scan_topk(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                   int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_valued_scan_topk_labeled(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi, uint32_t label,
                                           int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_valued_scan_topk_batch(vg_shards *s, int metric, const void *queries, int nq, int k, const int64_t *los,
                                         const int64_t *his, const uint32_t *query_labels, int64_t *out_rowids, double *out_dist,
                                         int *out_counts);
int     vg_shards_valued_scan_topk_grouped(vg_shards *s, int metric, const void *query, int k, int64_t lo, int64_t hi,
                                           int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_shards_valued_scan_topk_capped(vg_shards *s, int metric, const void *query, int k, int per_label, int64_t lo, int64_t hi,
                                          int64_t *out_rowids, double *out_dist, uint32_t *out_labels, int *out_count);
int     vg_shards_scan_within_valued(vg_shards *s, int metric, const void *query, double radius, int64_t limit, int64_t lo, int64_t hi,
                                     int64_t *out_matches, int64_t *out_held);
/* the masked range scans over every shard: each shard answers over its own bits (a shard whose share of the mask is empty launches
 * nothing and contributes nothing), merged like vg_shards_scan_within[_batch]: the rowids, order and distance bits of one corpus
 * holding all rows.  Same contract; the results are read with vg_shards_scan_within_fetch / vg_shards_scan_within_batch_fetch and
 * overwrite what the unmasked forms held there (and the reverse). */
int     vg_shards_scan_within_masked(vg_shards *s, int metric, const void *query, double radius, int64_t limit,
                                     int64_t *out_matches, int64_t *out_held);
int     vg_shards_scan_within_batch_masked(vg_shards *s, int metric, const void *queries, int nq, const double *radii, int64_t limit,
                                           int64_t *out_matches, int64_t *out_held);
/* the labeled range scans over every shard: labels mean the same on every shard - each shard answers over its own rows, merged like
 * vg_shards_scan_within[_batch]: the rowids, order and distance bits of one corpus holding all rows.  Same contract; the results are
 * read with vg_shards_scan_within_fetch / vg_shards_scan_within_batch_fetch and overwrite what the other range forms held there (and
 * the reverse). */
int     vg_shards_scan_within_labeled(vg_shards *s, int metric, const void *query, double radius, int64_t limit, uint32_t label,
                                      int64_t *out_matches, int64_t *out_held);
int     vg_shards_scan_within_labelset(vg_shards *s, int metric, const void *query, double radius, int64_t limit, const uint32_t *labels,
                                       int64_t n_labels, int exclude, int64_t *out_matches, int64_t *out_held);
int     vg_shards_scan_within_batch_labeled(vg_shards *s, int metric, const void *queries, int nq, const uint32_t *query_labels,
                                            const double *radii, int64_t limit, int64_t *out_matches, int64_t *out_held);
/* the paged scans over every shard: the cursor is one over GLOBAL scan order - each shard gets the floor over its own positions
 * ("local rows of this shard in front of global position P", by the block-cyclic map) and the lists merge by (distance, GLOBAL scan
 * position): the rowids, order and distance bits of one corpus holding all rows.  Same contracts.  The _keys forms take and return keys
 * over GLOBAL positions (sortable(distance) << 32 | global position): VG_ERR_UNSUPPORTED for 2^32 rows or more. */
int     vg_shards_scan_topk_after(vg_shards *s, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                  int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_scan_topk_after_keys(vg_shards *s, int metric, const void *query, int k, uint64_t after_key,
                                       uint64_t *out_keys, int *out_count);
int     vg_shards_scan_topk_after_masked(vg_shards *s, int metric, const void *query, int k, double after_dist, int64_t after_rowid,
                                         int64_t *out_rowids, double *out_dist, int *out_count);
int     vg_shards_scan_topk_after_masked_keys(vg_shards *s, int metric, const void *query, int k, uint64_t after_key,
                                              uint64_t *out_keys, int *out_count);
int     vg_shards_scan_topk_batch_after(vg_shards *s, int metric, const void *queries, int nq, int k, const double *after_dists,
                                        const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_shards_scan_topk_batch_after_keys(vg_shards *s, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                             uint64_t *out_keys, int *out_counts);
int     vg_shards_scan_topk_batch_after_masked(vg_shards *s, int metric, const void *queries, int nq, int k, const double *after_dists,
                                               const int64_t *after_rowids, int64_t *out_rowids, double *out_dist, int *out_counts);
int     vg_shards_scan_topk_batch_after_masked_keys(vg_shards *s, int metric, const void *queries, int nq, int k, const uint64_t *after_keys,
                                                    uint64_t *out_keys, int *out_counts);
int     vg_shards_minmax(vg_shards *s, float *out_min, float *out_max, int *out_any_negative);
int     vg_shards_quantize_rows(vg_shards *s, float scale, float offset, int qtype, int64_t row0, int64_t n_rows, uint8_t *out_host);

/* Diagnostics - profiling switches, kernel timings, launch plans, counters and the building blocks the tests compose - are declared
 * in vectorgpu_diag.h: exported by the same library, not part of the surface a binding has to keep stable. */

/* ---- tie order ----
 * VG_TIE_POSITION (default): results ordered by (distance, scan position) - deterministic, shard-invariant.
 * VG_TIE_REFERENCE: the reference's own result among EQUAL distances, rowid for rowid: its k unsorted slots, strict '<'
 * insertion into the FIRST slot holding the maximum and the final exchange sort (sqlite-vector.c:2022-2069, 2102-2106,
 * 2138-2146) are replayed on the host over the rows that can enter at all - the first P rows, then only the rows the
 * device finds below the bound reached so far (vg_reforder.hip).  Same distances either way; this mode makes
 * int8 / uint8 scans (where ties are routine) identical to the reference in rowids and order too.  With the mode set,
 * vg_scan_topk / vg_shards_scan_topk answer through vg_scan_topk_reference (k <= 64: the ordinary scan with one more list slot, a
 * host replay over what the scan left behind only when the k + 1 best hold a tie - no second scan, on any number of shards); the
 * batch calls run with one more slot too and answer only the queries with a tie again. */
enum { VG_TIE_POSITION = 0, VG_TIE_REFERENCE = 1 };
int vg_corpus_set_tie_order(vg_corpus *c, int mode);
int vg_corpus_tie_order(const vg_corpus *c);
int vg_shards_set_tie_order(vg_shards *s, int mode);
int vg_scan_topk_reference(vg_corpus *c, int metric, const void *query, int k, int64_t *out_rowids, double *out_dist, int *out_count);
/* ---- out-of-core scans: a table that does not fit device memory ----
 * The reference scans a table of ANY size: vFullScanRun walks the statement's rows one by one (sqlite-vector.c:2071-2113) and keeps k
 * slots.  Its form here: the caller hands the rows over in scan order, the device holds TWO slabs of slab_rows rows each - one being
 * filled through the pinned bounce buffers, the other one being scanned on a host thread of its own - and what is carried from slab to
 * slab is what the reference carries from row to row: the k best so far (tie_order = position: merged by (distance, scan position);
 * tie_order = reference: the slot state itself, offered the rows of each later slab that lie below the bound reached, vg_refslots.h).
 * Results are those of vg_scan_topk over one corpus holding all rows, bit for bit.  k = 0: every row's distance and rowid instead
 * (the *_stream functions), fetched with vg_slab_scan_all.  rowid_base: implicit rowid of scan position p = rowid_base + p where the
 * caller passes rowids = NULL.  The handle serves one query; the extension makes one per scan of a table it cannot keep resident
 * (VECTORGPU_HBM_LIMIT or the device's free memory: INTEGRATION.md). */
/* Pinned host memory for a HOST-RESIDENT copy of a table that does not fit the device (round 6): the tier between "staged in HBM" and the
 * reference's own cost model of reading the table for every query (sqlite-vector.c:2077-2107).  Rows handed to vg_slab_scan_rows /
 * vg_corpus_append from such a block are read by the DMA engine where they lie (no bounce copy): a scan of the copy runs at the host
 * link's rate.  VG_ERR_NOMEM when the runtime refuses to pin that much. */
int  vg_host_alloc(size_t bytes, void **out);
void vg_host_free(void *p);

typedef struct vg_slab_scan vg_slab_scan;
int  vg_slab_scan_begin(int device, int vtype, int dim, int metric, const void *query, int k, int tie_order, int64_t slab_rows,
                        int64_t rowid_base, vg_slab_scan **out);
int  vg_slab_scan_rows(vg_slab_scan *s, const void *host_rows, int64_t n_rows, int64_t row_stride_bytes, const int64_t *rowids);
int  vg_slab_scan_records(vg_slab_scan *s, const void *host_records, int64_t n_records);   /* [int64 LE rowid | dim bytes] records (uint8 / int8) */
int  vg_slab_scan_finish(vg_slab_scan *s, int64_t *out_rowids, double *out_dist, int *out_count);
int  vg_slab_scan_all(vg_slab_scan *s, int64_t *out_rows, const float **out_dist, const int64_t **out_rowids);   /* k = 0, after finish; valid until destroy */
void vg_slab_scan_destroy(vg_slab_scan *s);
int  vg_device_memory(int device, long long *out_free_bytes, long long *out_total_bytes);

/* ---- per-corpus switches ---- */
/* The lower-bound filter scans of single top-k queries (see vg_scan_topk): 0 = off (plain scans, no shadow copy is built),
 * -1 = default (environment VG_SCAN_FILTER, else on): f32 / f16 / bf16 corpora from 2^20 rows and 512 MB through an int8 shadow
 * copy (+ 26 % / + 52 % device memory), uint8 / int8 corpora through a high-nibble copy (+ 52 %) only after a probe of a 2M-row
 * prefix found the data selective under it; 1 = on where it serves WITHOUT that probe (uint8 / int8: the + 52 % is spent at
 * once).  The extension maps vector_init's scan_filter= option here - for the raw-vector corpus and the quantized one alike. */
int vg_corpus_set_scan_filter(vg_corpus *c, int mode);

#ifdef __cplusplus
}
#endif
#endif
