// vg_scan.h - the brute-force scan kernel (single query): HBM-bound streaming read of the N x D corpus with a
// fused wavefront-level top-k.  One template, instantiated per (element type, accumulation kind, U, load policy, FORM).
//
// FORM is a set of flags (VG_SQ_*); each changes which rows are read or what happens to a distance, none how it is computed:
//   (none)           top-k, k <= 64: one candidate list per wavefront, one published list per workgroup, vg_merge_kernel behind it.
//                    Store mode (ScanArgs.out_dist set) is this form too - a runtime branch: every distance to HBM, no lists.
//   VG_SQ_EX         what tie_order = reference needs (vg_reforder.hip) on top of the plain form: a start threshold from a pass
//                    over the rows in front (init_keys), the candidate stream (emit) and "top-k + store" (out_dist != nullptr with
//                    k > 0: the replay's prefix pass).  Instances of their own (vg_scan_ex.hip) because the plain kernels sit AT the
//                    128-VGPR / 106-SGPR limit of 16 wavefronts per CU: the few registers the extras take spilled f32 U = 8 and
//                    f16 U = 6, shapes the plain scans use.  Not combined with another flag; no long-row kernel.
//   VG_SQ_WITHIN     range scan in place of the candidate list (vg_scan_within.hip): a row matches when d <= ScanArgs.within_r and d
//                    is finite.  The keys of the matches are parked in a per-wavefront LDS queue and leave in bursts
//                    (vg_within_offer / vg_within_flush below); the tail flushes the queue - no list, no publish.
//   VG_SQ_MASKED     only the rows whose bit is set in ScanArgs.mask (vg_scan_masked.hip):
//                      * the bits of a batch (vg_mask_bits: wave-uniform, one scalar load) are fetched ONE loop step ahead of the row
//                        prefetch whose addresses they decide - `mnext` is asked for one step before the batch it describes is
//                        prefetched and has a whole step (the current batch's arithmetic) to arrive;
//                      * a batch without an allowed row points its U loads at vg_zero_chunk (one cache line, always a hit) and does
//                        no arithmetic: a scalar branch around `process`;
//                      * a row whose bit is clear was computed with its batch and is simply not offered.
//                    In the ring form the row prefetch is NB - 1 batches ahead of the arithmetic, the mask fetch therefore NB: still
//                    one scalar load in flight per wavefront, NB + 1 words of bits held (scalar registers).  Without the flag
//                    every statement of the pipeline is discarded (if constexpr): nothing of it reaches the generated code.  With
//                    VG_SQ_WITHIN: the masked range scan (vg_scan_within_masked.hip).
//   VG_SQ_AFTER      paged scans (vg_scan_after.hip, with and without VG_SQ_MASKED): a row is offered only when its key is >=
//                    ScanArgs.floor[0], the key just behind the caller's cursor.  One wave-uniform 64-bit value loaded before the
//                    loop and one compare in the offer.  Not combined with VG_SQ_WITHIN: a range scan has no cursor.
//   VG_SQ_GROUPED    grouped scans (vg_scan_grouped.hip, with and without VG_SQ_MASKED): the k nearest LABELS, each by its best row.  The
//                    row's label (ScanArgs.labels, one dword) rides with the batch prefetch exactly like A_COSN's row norm - issued with
//                    the row's chunk loads, unconditional, nothing loaded between batches - and the candidate list stays distinct by
//                    label (vg_list_offer_grouped, vg_device.h: one more register per lane).  A row without a label is never offered.
//                    The workgroup's lists merge through the same routine (vg_block_publish_grouped) and leave as keys only: a key's
//                    label is labels[position], gathered again by the final merge (vg_merge_grouped_kernel).  Not combined with
//                    EX, WITHIN or AFTER; no store mode.
//   VG_SQ_CAPPED     capped scans (vg_scan_capped.hip; set together with VG_SQ_GROUPED, with and without VG_SQ_MASKED): the k nearest
//                    rows, at most m = ScanArgs.within_cap of one label (a field that is dead here, like within_r: ScanArgs keeps its
//                    size).  Every statement of the grouped form stands - the label load, the scheduling barrier, row 0 standing in -
//                    except the two that touch the list: the offer is vg_list_offer_capped and the workgroup merge
//                    vg_block_publish_capped; the final merge is vg_merge_capped_kernel.
// The streaming loop was four hand-copied loops and the offer a ladder of seven branches; the code generated for every instance of
// the two templates was checked identical to that of the copies it replaced (instruction text, registers, spills, scratch, LDS:
// DESIGN.md 3.6) at the commit that folded them.
//
// Work decomposition (CDNA4):
//   * a row is `nch` 16-byte chunks; LPR = 2^lpr_log2 lanes share a row, lane `sub` owns chunks sub + u*LPR
//     (u < U), so one wave-wide global_load_dwordx4 reads 64/LPR rows x (LPR*16 B) contiguous bytes per row:
//     full 128-byte lines, every byte of the corpus fetched exactly once;
//   * a wavefront processes "batches" of 64/LPR rows in a grid-stride loop and keeps the next batch's U loads in
//     flight while it reduces the current one (loads straight to VGPRs, no LDS round trip: nothing is reused);
//   * the query lives in VGPRs (U x uint4 per lane), staged through LDS once per workgroup;
//   * per batch: U chunk folds -> butterfly over the lane group -> scalar epilogue -> clamp -> 64-bit key ->
//     ballot against the wave's current k-th best; only the rare survivors touch the sorted list;
//   * at the end the 16 wave lists of a workgroup merge through LDS (binary tree) and ONE list per workgroup -
//     i.e. per CU - goes to HBM (grid x 64 keys); vg_merge_kernel reduces those to the final k.
#pragma once

#include "vg_accum.h"
#include "vg_lists.h"

// LDS needed at the end of a scan workgroup: 16 wave lists + the selection scratch
#define VG_PUBLISH_LDS_BYTES (VG_WAVES_PER_BLOCK * VG_WAVE * 8 + VG_SEL_SCRATCH_BYTES)

// every wavefront deposits its sorted list in LDS, then the whole workgroup selects the k best into `dst` (global)
__device__ inline void vg_block_publish(uint8_t *smem, uint64_t mine, int k, uint64_t *dst) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    lists[wave * VG_WAVE + lane] = (lane < k) ? mine : VG_EMPTY_KEY;
    __syncthreads();
    vg_select_lists(lists, VG_WAVES_PER_BLOCK, k, dst, smem + VG_WAVES_PER_BLOCK * VG_WAVE * 8);
}

// The grouped counterpart (VG_SQ_GROUPED): a rank-select over keys would return two rows of one label, so wavefront 0 offers the
// other wavefronts' first k entries, one list of 64 at a time from LDS, to its own list (vg_list_offer_grouped: sorted lists are offered
// in ascending order, so once thr has tightened a list costs one ballot) and writes the k keys to `dst` (global; labels to
// `dst_labels` when asked for).  Every wavefront of the workgroup calls; the keys and labels take VG_WAVES * 64 * 12 bytes of smem
// - within the VG_PUBLISH_LDS_BYTES every fused launch asks for (launch_fused, vg_scan_masked.hip).  `nwaves` <= VG_WAVES_PER_BLOCK:
// wavefronts of the workgroup that hold a list.
static_assert(VG_WAVES_PER_BLOCK * VG_WAVE * 12 <= VG_PUBLISH_LDS_BYTES, "the grouped publish parks keys and labels in the plain publish's LDS");
__device__ inline void vg_block_publish_grouped(uint8_t *smem, uint64_t mine, uint32_t mlab, int k, int nwaves, uint64_t *dst, uint32_t *dst_labels) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    uint32_t *labs = reinterpret_cast<uint32_t *>(smem + (size_t)nwaves * VG_WAVE * 8);
    lists[wave * VG_WAVE + lane] = (lane < k) ? mine : VG_EMPTY_KEY;
    labs[wave * VG_WAVE + lane] = mlab;
    __syncthreads();
    if (wave != 0) return;
    uint64_t thr = vg_readlane64(mine, k - 1);
    for (int w = 1; w < nwaves; ++w) {
        const uint64_t key = lists[w * VG_WAVE + lane];
        vg_list_offer_grouped(key, labs[w * VG_WAVE + lane], key != VG_EMPTY_KEY, mine, mlab, thr, lane, k);
    }
    dst[lane] = (lane < k) ? mine : VG_EMPTY_KEY;
    if (dst_labels) dst_labels[lane] = (lane < k) ? mlab : 0xFFFFFFFFu;
}

// The capped counterpart (VG_SQ_CAPPED): the same statements with the cap m handed to the offer - wavefront 0 re-offers the other
// wavefronts' first k entries through vg_list_offer_capped.  A routine of its own: the grouped one, and every kernel that calls
// it, keeps its code.
__device__ inline void vg_block_publish_capped(uint8_t *smem, uint64_t mine, uint32_t mlab, int k, int m, int nwaves, uint64_t *dst, uint32_t *dst_labels) {
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    uint32_t *labs = reinterpret_cast<uint32_t *>(smem + (size_t)nwaves * VG_WAVE * 8);
    lists[wave * VG_WAVE + lane] = (lane < k) ? mine : VG_EMPTY_KEY;
    labs[wave * VG_WAVE + lane] = mlab;
    __syncthreads();
    if (wave != 0) return;
    uint64_t thr = vg_readlane64(mine, k - 1);
    for (int w = 1; w < nwaves; ++w) {
        const uint64_t key = lists[w * VG_WAVE + lane];
        vg_list_offer_capped(key, labs[w * VG_WAVE + lane], key != VG_EMPTY_KEY, mine, mlab, thr, lane, k, m);
    }
    dst[lane] = (lane < k) ? mine : VG_EMPTY_KEY;
    if (dst_labels) dst_labels[lane] = (lane < k) ? mlab : 0xFFFFFFFFu;
}

typedef uint32_t vg_u32x4 __attribute__((ext_vector_type(4)));

// NT = true streams the corpus with non-temporal loads (global_load_dwordx4 ... nt): every byte is read exactly
// once per query, so keeping it out of L2 / Infinity Cache is worth +11% on a 15 GB corpus (6.1 -> 6.8 TB/s
// measured).  NT = false is used when the whole corpus fits the 256 MiB Infinity Cache and repeated queries hit it.
template <bool NT>
__device__ inline uint4 vg_load16(const uint8_t *p) {
    if (NT) {
        vg_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const vg_u32x4 *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const uint4 *>(p);
}

// 16 zero bytes in device memory: where a lane that has nothing to load (a row behind the last one, a chunk behind the row's last
// one) points its load.  The loads of a batch are UNCONDITIONAL - only the address is selected: a load under `if (valid)` becomes a
// branch around the instruction, the compiler's wait-count bookkeeping must then assume that none of the prefetch loads were
// issued, and the wait in front of the CURRENT batch's arithmetic turns into vmcnt(0) - the wavefront sat out the full latency
// of the prefetch it had just issued before touching data that had long arrived (f16 U = 6, bf16 / uint8 U = 3: every shape
// whose loop the compiler unrolls into two register sets).  VG_LOAD_PREDICATED=1: the earlier form, for A/B runs.
#ifndef VG_LOAD_PREDICATED
#define VG_LOAD_PREDICATED 0
#endif
static __device__ __attribute__((aligned(16))) uint32_t vg_zero_chunk[4] = {0u, 0u, 0u, 0u};      // (not const: a constant-address-space pointer would turn the selected loads into flat loads)

template <int U, bool NT>
__device__ inline void vg_load_batch(uint4 (&dst)[U], const uint8_t *rows, long long row, long long n_rows,
                                     long long stride, int sub, int lpr, int nch) {
    const uint8_t *p = rows + row * stride + (long long)sub * 16;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = sub + u * lpr;
        if (VG_LOAD_PREDICATED) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < n_rows && c < nch) v = vg_load16<NT>(p + (long long)u * lpr * 16);
            dst[u] = v;
        } else {
            const uint8_t *src = (row < n_rows && c < nch) ? p + (long long)u * lpr * 16 : reinterpret_cast<const uint8_t *>(vg_zero_chunk);
            dst[u] = vg_load16<NT>(src);
        }
    }
}

#ifndef VG_HALF_LAUNDER
#define VG_HALF_LAUNDER 1
#endif
#ifndef VG_BF16_HOIST_Q
#define VG_BF16_HOIST_Q 1
#endif
#define VG_STORE_FLOATS 1024          // store mode: distances parked in LDS per wavefront between bursts of stores

// the forms of vg_scan_kernel / vg_scan_long_kernel (the head of this file); the first three have the values of VG_MQ_*
enum : int { VG_SQ_MASKED = 1, VG_SQ_AFTER = 2, VG_SQ_WITHIN = 4, VG_SQ_EX = 8, VG_SQ_GROUPED = 16, VG_SQ_CAPPED = 32 };

// ---- VG_SQ_WITHIN: the keys of the rows within the radius are parked in a per-wavefront LDS queue and leave in bursts - one atomicAdd of the burst size by one lane, then coalesced 8-byte-per-lane stores.
// A store (and the atomic's return) shares vmcnt with the batch prefetch, see the store-mode note in vg_scan_kernel: a burst of 64+
// keys makes that drain rare, and a batch without a match - nearly every batch - costs one ballot.
#define VG_WITHIN_QUEUE 128           // keys per wavefront: flushed once a further batch (<= 64 rows) might not fit
#define VG_WITHIN_LDS_BYTES (VG_WAVES_PER_BLOCK * VG_WITHIN_QUEUE * 8)
__device__ inline void vg_within_flush(const uint64_t *queue, int &queued, unsigned long long *out, unsigned long long cap, int lane) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(out, (unsigned long long)queued);      // keeps counting past cap: the host learns the size it needs
    base = vg_readlane64(base, 0);
    for (int i = lane; i < queued; i += VG_WAVE)
        if (base + (unsigned long long)i < cap) out[1 + base + i] = queue[i];
    queued = 0;
}
// `queued` is wave-uniform; lanes of one wavefront write and read the queue in program order (LDS operations of a wavefront are ordered)
__device__ inline void vg_within_offer(uint64_t key, bool match, uint64_t *queue, int &queued, unsigned long long *out,
                                       unsigned long long cap, int lane) {
    const unsigned long long m = __ballot(match);
    if (m == 0ull) return;
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (match) queue[queued + rank] = key;
    queued += __popcll(m);
    if (queued > VG_WITHIN_QUEUE - VG_WAVE) vg_within_flush(queue, queued, out, cap, lane);
}

// ---- VG_SQ_MASKED: the bits of the `n` rows from `row0` on (n a power of two <= 64 and row0 a multiple of it: adjacent bits of ONE word),
// bit i = row0 + i, zero when the rows are out of range.  Every lane of the wavefront asks for the same rows, but the compiler cannot
// know that of a value derived from threadIdx: the start row goes through readfirstlane (0xFFFFFFFF = out of range: a shard holds at
// most 2^32 - 1 rows), and from there on index, word, shift and result are wave-uniform - one scalar load (s_load_dwordx2) per call on
// the scalar cache's counter (lgkmcnt), nothing on the vector memory path the row prefetch lives on, and `bits != 0` is a scalar branch.
__device__ inline uint64_t vg_mask_bits(const uint64_t *mask, long long row0, int n, bool in_range) {
    const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(in_range ? (uint32_t)row0 : 0xFFFFFFFFu));
    const bool ok = r != 0xFFFFFFFFu;
    const uint64_t bits = mask[ok ? (r >> 6) : 0u] >> (r & 63u);
    const uint64_t keep = (n >= VG_WAVE) ? ~0ull : ((1ull << (n & 63)) - 1ull);
    return ok ? (bits & keep) : 0ull;
}

template <int VT, int ACC, int U, bool NT, int FORM = 0>      // FORM: VG_SQ_* flags
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_kernel(ScanArgs a) {
    constexpr bool EX = (FORM & VG_SQ_EX) != 0, WITHIN = (FORM & VG_SQ_WITHIN) != 0, MASKED = (FORM & VG_SQ_MASKED) != 0;
    constexpr bool AFTER = (FORM & VG_SQ_AFTER) != 0, GROUPED = (FORM & VG_SQ_GROUPED) != 0, CAPPED = (FORM & VG_SQ_CAPPED) != 0;
    static_assert(!EX || FORM == VG_SQ_EX, "the reference-order extras are not combined with the range, masked or paged forms");
    static_assert(!(WITHIN && AFTER), "a range scan has no cursor");
    static_assert(!GROUPED || !(EX || WITHIN || AFTER), "a grouped scan is combined with the mask only");
    static_assert(!CAPPED || (GROUPED && !(EX || WITHIN || AFTER)), "a capped scan is the grouped form with a cap, combined with the mask only");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ VgListExtras ex;
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int lpr_log2 = a.lpr_log2;
    const int lpr = 1 << lpr_log2;
    const int rpb = VG_WAVE >> lpr_log2;          // rows per batch
    const int sub = lane & (lpr - 1);
    const int rib = lane >> lpr_log2;             // row in batch

    // ---- query: global -> LDS (once per workgroup) -> VGPRs
    uint4 *qs = reinterpret_cast<uint4 *>(smem);
    for (int c = threadIdx.x; c < a.nch; c += VG_BLOCK) qs[c] = reinterpret_cast<const uint4 *>(a.query)[c];
    // ---- candidate list (top-k mode).  tie_order = reference (vg_reforder.hip): a start threshold from the pass over the rows in
    // front and the candidate stream - kept in LDS (`ex`), published by the same barrier as the query
    const int k = a.k;
    uint64_t mine = VG_EMPTY_KEY;
    uint64_t thr = VG_EMPTY_KEY;
    if constexpr (EX) {
        if (k > 0) thr = vg_list_extras_init(&ex, a.init_keys, k, a.emit, a.emit_cap);
        if (a.emit_reset && blockIdx.x == 0 && threadIdx.x == 0) *a.emit_reset = 0ull;
    }
    // after mode, f16 / bf16: these kernels sit AT the 106-SGPR limit and two more live scalar registers spilled into VGPR lanes; the
    // floor stays in LDS instead (as VgListExtras does), published by the same barrier as the query, read back in the offer
    constexpr bool AFTER_LDS = AFTER && (VT == T_F16 || VT == T_BF16);
    const uint64_t *floor_lds = nullptr;
    if constexpr (AFTER_LDS) {
        __shared__ uint64_t floor_slot;
        if (threadIdx.x == 0) floor_slot = a.floor[0];
        floor_lds = &floor_slot;
    }
    __syncthreads();
    uint4 q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = sub + u * lpr;
        q[u] = (c < a.nch) ? qs[c] : make_uint4(0u, 0u, 0u, 0u);
    }
    const typename Accum<VT, ACC>::QStat qstat = Accum<VT, ACC>::template query_stat<U>(q, lpr_log2);
    const bool store_mode = (WITHIN || MASKED || AFTER || GROUPED) ? false : EX ? ((a.out_dist != nullptr) && k == 0) : (a.out_dist != nullptr);
    uint32_t mlab = 0xFFFFFFFFu;                                      // grouped mode only: the label of the key in `mine`
    uint64_t floor_key = 0ull;                                        // after mode only: wave-uniform, scalar registers (f32 / uint8 / int8)
    if constexpr (AFTER && !AFTER_LDS) floor_key = vg_uniform64(a.floor[0]);
    const bool store_too = EX && (a.out_dist != nullptr) && k != 0; // the reference replay's prefix pass: top-k + every distance

    // ---- loop over row batches, one batch prefetched.  Top-k mode: grid-stride (batch b, b + W, ...).  Store mode:
    // each wavefront owns a CONTIGUOUS run of batches, parks VG_STORE_FLOATS distances in LDS and writes them out in
    // one burst of 16-byte-per-lane stores.  Stores share the load counter (vmcnt) and retire out of order with
    // loads, so the wait for the prefetched batch that follows a store drains EVERYTHING, prefetch included: with a
    // store every batch - or even every 16 batches - the kernel ran 10% slower than the top-k mode.  One burst per
    // 1024 rows makes that drain rare (measured: 2.46 -> 2.27 ms at 10M x 384; top-k mode 2.24).
    const long long nbatch = (a.n_rows + rpb - 1) / rpb;
    const long long nwaves = (long long)gridDim.x * VG_WAVES_PER_BLOCK;
    const long long gw = (long long)blockIdx.x * VG_WAVES_PER_BLOCK + wave;
    const int flush_every = VG_STORE_FLOATS / rpb;                    // iterations that fill the staging area
    long long per_wave = (nbatch + nwaves - 1) / nwaves;
    per_wave = ((per_wave + flush_every - 1) / flush_every) * flush_every;
    long long wstride = store_mode ? 1 : nwaves;
    long long b = store_mode ? gw * per_wave : gw;
    long long b_end = store_mode ? ((gw + 1) * per_wave < nbatch ? (gw + 1) * per_wave : nbatch) : nbatch;
    if (a.order == 1 && !store_mode) {                                // block-contiguous order (ScanArgs.order)
        const long long per_block = (nbatch + gridDim.x - 1) / gridDim.x;
        wstride = VG_WAVES_PER_BLOCK;
        b = (long long)blockIdx.x * per_block + wave;
        b_end = ((long long)blockIdx.x + 1) * per_block < nbatch ? ((long long)blockIdx.x + 1) * per_block : nbatch;
    }
    float *line = reinterpret_cast<float *>(smem + a.store_lds_off) + wave * VG_STORE_FLOATS;    // store mode only
    int in_line = 0;
    long long line_row0 = b * rpb;                                    // a multiple of VG_STORE_FLOATS: 16-byte aligned
    uint64_t *wqueue = reinterpret_cast<uint64_t *>(smem + a.store_lds_off) + wave * VG_WITHIN_QUEUE;   // within mode only
    int wqueued = 0;
    // Short uint8 / int8 rows (U <= 2) use a prefetch ring: NB buffers of U chunks, the loop unrolled NB times so that
    // every buffer keeps its registers (no copies); while buffer j is reduced the NB-1 others are in flight.  With
    // plain double buffering such rows have 1-2 KB per wavefront in flight and sit in s_waitcnt (dim-64 uint8 rows:
    // 4.0 -> 4.9 TB/s for L2, 4.8 -> 6.2 for dot).  Measured slower for f32 short rows and for U >= 3, which keep the
    // double buffer.
#ifndef VG_RING_F32
#define VG_RING_F32 0                 // > 0: f32 rows with 3 chunks per lane (the C2 / C4 shape, 40 VGPRs) run the ring with that many buffers
#endif
    constexpr bool RING_F32 = (VG_RING_F32 > 0) && VT == T_F32 && U == 3 && !EX;
    constexpr bool RING = ((U <= 2) && (VT == T_U8 || VT == T_I8)) || RING_F32;
    constexpr int NB = !RING ? 2 : RING_F32 ? (VG_RING_F32 > 2 ? VG_RING_F32 : 3) : (U == 2) ? 4 : 6;
    uint4 buf[NB][U];
    float nn[NB];
    uint32_t lab[NB];                                                 // grouped mode only
#pragma unroll
    for (int j = 0; j < NB; ++j) { nn[j] = 0.0f; lab[j] = 0xFFFFFFFFu; }
    // (masked mode: `live` = the batch has an allowed row; a batch without one points every load at vg_zero_chunk - no row is read)
    auto load = [&](uint4 (&dst)[U], float &nn_dst, uint32_t &lab_dst, long long batch, bool live) {
        vg_load_batch<U, NT>(dst, a.rows, batch * rpb + rib, (batch < b_end && live) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
        // A_COSN: the row's squared norm rides along with the batch prefetch (one dword per row from the cached vector)
        // (unconditional for the same reason as the chunk loads: row 0's norm stands in, the row's result is never used)
        if constexpr (ACC == A_COSN) { const long long r0 = batch * rpb + rib; nn_dst = a.row_nn[(batch < b_end && live && r0 < a.n_rows) ? r0 : 0]; }
        // GROUPED: so does the row's label (row 0's stands in for a row that is not read: its result is never offered)
        if constexpr (GROUPED) { const long long r0 = batch * rpb + rib; lab_dst = a.labels[(batch < b_end && live && r0 < a.n_rows) ? r0 : 0]; }
    };
    // MASKED: the mask bits of a batch (wave-uniform; 0 behind the wavefront's last batch)
    auto mask_of = [&](long long batch) -> uint64_t { return vg_mask_bits(a.mask, batch * rpb, rpb, batch < b_end); };
    auto process = [&](uint4 (&cur)[U], float nn_cur, uint32_t lab_cur, long long bcur, uint64_t mbits) {
        Accum<VT, ACC> acc;
        acc.init();
        if constexpr (VT == T_F16 || VT == T_BF16) {
            // keep the query as RAW halves in registers: without this the compiler hoists the widened (f32 / f64)
            // copies out of the loop - up to 48 more VGPRs per lane, which is what capped U (bytes in flight)
            // (bf16 with U <= 3 - its dot / cosine shapes - has the registers: there the hoisted f32 copies of the query save two
            // unpack operations per element pair, VG_BF16_HOIST_Q)
            if (VG_HALF_LAUNDER && !(VG_BF16_HOIST_Q && VT == T_BF16 && U <= 3)) {
#pragma unroll
                for (int u = 0; u < U; ++u) asm volatile("" : "+v"(q[u].x), "+v"(q[u].y), "+v"(q[u].z), "+v"(q[u].w));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc.chunk(q[u], cur[u]);
        const long long row = bcur * rpb + rib;
        const bool owner = (sub == 0) && (row < a.n_rows);
        float d;
        if constexpr (ACC == A_COSN) d = acc.finish_cached_norm(qstat, lpr_log2, nn_cur);
        else d = acc.finish(qstat, lpr_log2, a.root);
        if constexpr (VT == T_F16 || VT == T_BF16) {
            // rows (or a query) holding Inf/NaN: the owning lane replays the reference algorithm exactly (vg_half.h)
            if (acc.special(qstat, lpr_log2) && owner)
                d = vg_slow_distance<VT, (ACC == A_COSN ? A_COS : ACC)>(reinterpret_cast<const uint16_t *>(qs),
                                              reinterpret_cast<const uint16_t *>(a.rows + row * a.stride), a.dim, a.root);
        }
        d = vg_clamp(d);
        if constexpr (!WITHIN) {                                  // (a range scan has no store mode)
            if (store_mode) {                                     // (stores share vmcnt with the prefetch: the note above the loop)
                if (sub == 0) line[in_line * rpb + rib] = d;          // rows of consecutive batches are consecutive
                if (++in_line == flush_every) {
                    // same wavefront wrote the lines: LDS ops are ordered, no barrier needed
                    if (line_row0 + VG_STORE_FLOATS <= a.n_rows) {
#pragma unroll
                        for (int j = 0; j < VG_STORE_FLOATS / (4 * VG_WAVE); ++j)
                            reinterpret_cast<float4 *>(a.out_dist + line_row0)[j * VG_WAVE + lane] = reinterpret_cast<const float4 *>(line)[j * VG_WAVE + lane];
                    } else {
                        for (int j = lane; j < VG_STORE_FLOATS && line_row0 + j < a.n_rows; j += VG_WAVE) a.out_dist[line_row0 + j] = line[j];
                    }
                    in_line = 0;
                    line_row0 = (bcur + wstride) * rpb;
                }
                return;
            }
        }
        // One key, one predicate, one offer.  NaN and +Inf never enter (strict '<' against INFINITY-initialised slots,
        // sqlite-vector.c:1809,2102); WITHIN: d <= r is false for NaN, and +Inf never matches, whatever the radius (the top-k
        // contract: such rows never enter a list); MASKED: a row whose bit is clear was computed with its batch and is simply
        // not offered; AFTER: only keys from the floor on.
        // (Two spellings of the chain, so that its LAST operand is a real term in every form: behind a compile-time `true` in that
        //  place the compiler and-ed the same terms in another order than the copies had.)
        if constexpr (EX) { if (store_too && owner) a.out_dist[row] = d; }
        const uint64_t key = vg_make_key(d, (uint32_t)row);
        if constexpr (AFTER_LDS) floor_key = *reinterpret_cast<const volatile uint64_t *>(floor_lds);
        bool ok;
        if constexpr (AFTER) ok = owner && (!MASKED || ((mbits >> rib) & 1ull)) && (d < INFINITY) && (key >= floor_key);
        else ok = owner && (!MASKED || ((mbits >> rib) & 1ull)) && (!WITHIN || d <= a.within_r) && (d < INFINITY);
        if constexpr (WITHIN) vg_within_offer(key, ok, wqueue, wqueued, a.emit, a.within_cap, lane);
        else if constexpr (EX) vg_list_offer_ex(key, ok, mine, thr, lane, k, &ex);
        else if constexpr (CAPPED) vg_list_offer_capped(key, lab_cur, ok && (lab_cur != 0xFFFFFFFFu), mine, mlab, thr, lane, k, (int)a.within_cap);
        else if constexpr (GROUPED) vg_list_offer_grouped(key, lab_cur, ok && (lab_cur != 0xFFFFFFFFu), mine, mlab, thr, lane, k);
        else vg_list_offer(key, ok, mine, thr, lane, k);
    };
    // One ring loop and one double-buffer loop for every form.  mb[j] = the mask bits of the batch in buffer j, `mnext` those of the
    // batch that is prefetched next (MASKED, see the head of this file).  Without the flag every batch is live and neither is ever
    // written or read: the pipeline's statements are discarded, `!MASKED || ...` / `MASKED ? ... : ...` are constants to the front end.
    // (They are spelled out at every use on purpose.  Routing them through a helper lambda, or evaluating mask_of()'s argument for a
    // constant result, leaves the same instructions but in another order in some instances - DESIGN.md 3.6.)
    uint64_t mb[NB], mnext;
    if constexpr (RING) {
#pragma unroll
        for (int j = 0; j < NB - 1; ++j) {
            if constexpr (MASKED) mb[j] = mask_of(b + j * wstride);
            load(buf[j], nn[j], lab[j], b + j * wstride, !MASKED || mb[j] != 0ull);
        }
        if constexpr (MASKED) mnext = mask_of(b + (NB - 1) * wstride);
        while (b < b_end) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const long long bj = b + j * wstride;             // the batch in buffer j
                if constexpr (MASKED) { mb[(j + NB - 1) % NB] = mnext; mnext = mask_of(bj + NB * wstride); }
                load(buf[(j + NB - 1) % NB], nn[(j + NB - 1) % NB], lab[(j + NB - 1) % NB], bj + (NB - 1) * wstride, !MASKED || mb[(j + NB - 1) % NB] != 0ull);
                if (MASKED ? mb[j] != 0ull : bj < b_end) process(buf[j], nn[j], lab[j], bj, MASKED ? mb[j] : 0ull);       // (the bits are 0 behind b_end)
            }
            b += NB * wstride;
        }
    } else {
        if constexpr (MASKED) { mb[0] = mask_of(b); mnext = mask_of(b + wstride); }
        load(buf[0], nn[0], lab[0], b, !MASKED || mb[0] != 0ull);
        while (b < b_end) {
            const long long bn = b + wstride;
            if constexpr (MASKED) { mb[1] = mnext; mnext = mask_of(bn + wstride); }
            load(buf[1], nn[1], lab[1], bn, !MASKED || mb[1] != 0ull);
            // GROUPED: the whole prefetch is issued before the arithmetic starts.  Left to itself the scheduler spreads the label's
            // address arithmetic and load over `process`, which holds three more registers live through it: bf16 L2 at U = 6 spilled
            // query registers into scratch and reloaded them - a vmcnt(0) - behind every prefetch (128 VGPRs, 28 bytes; 112 and none now).
            if constexpr (GROUPED) __builtin_amdgcn_sched_barrier(0);
            if (!MASKED || mb[0] != 0ull) process(buf[0], nn[0], lab[0], b, MASKED ? mb[0] : 0ull);
#pragma unroll
            for (int u = 0; u < U; ++u) buf[0][u] = buf[1][u];
            nn[0] = nn[1];
            if constexpr (GROUPED) lab[0] = lab[1];
            if constexpr (MASKED) mb[0] = mb[1];
            b = bn;
        }
    }
    if constexpr (WITHIN) {
        if (wqueued > 0) vg_within_flush(wqueue, wqueued, a.emit, a.within_cap, lane);
        return;
    }
    if (store_mode) {
        // the run's last, partly filled staging area
        for (int j = lane; j < in_line * rpb && line_row0 + j < a.n_rows; j += VG_WAVE) a.out_dist[line_row0 + j] = line[j];
        return;
    }

    // ---- the workgroup's 16 wave lists -> ONE list per CU in HBM (parallel rank-select, vg_lists.h)
    __syncthreads();                                   // everyone is done with the query staging area
    if constexpr (CAPPED) vg_block_publish_capped(smem, mine, mlab, k, (int)a.within_cap, VG_WAVES_PER_BLOCK, a.cand + (long long)blockIdx.x * VG_WAVE, nullptr);
    else if constexpr (GROUPED) vg_block_publish_grouped(smem, mine, mlab, k, VG_WAVES_PER_BLOCK, a.cand + (long long)blockIdx.x * VG_WAVE, nullptr);
    else vg_block_publish(smem, mine, k, a.cand + (long long)blockIdx.x * VG_WAVE);
}

// Long rows (more 16-byte chunks than 64 lanes x the largest register-resident U): one row per wavefront per step,
// the row is consumed in `S` slices of 64 x VG_LONG_U chunks with the accumulator carried across slices and the
// query slice read from LDS (ds_read_b128) instead of living in VGPRs.  Same epilogue / top-k tail as above.
#define VG_LONG_U 2
template <int VT, int ACC, bool NT, int FORM = 0>             // FORM: VG_SQ_* flags, without VG_SQ_EX
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_long_kernel(ScanArgs a) {
    constexpr bool WITHIN = (FORM & VG_SQ_WITHIN) != 0, MASKED = (FORM & VG_SQ_MASKED) != 0, AFTER = (FORM & VG_SQ_AFTER) != 0;
    constexpr bool GROUPED = (FORM & VG_SQ_GROUPED) != 0, CAPPED = (FORM & VG_SQ_CAPPED) != 0;
    static_assert(!(FORM & VG_SQ_EX), "a long-row scan neither emits nor stores a prefix");
    static_assert(!(WITHIN && AFTER), "a range scan has no cursor");
    static_assert(!GROUPED || !(WITHIN || AFTER), "a grouped scan is combined with the mask only");
    static_assert(!CAPPED || (GROUPED && !(WITHIN || AFTER)), "a capped scan is the grouped form with a cap, combined with the mask only");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
    constexpr int U = VG_LONG_U;
    const int slice = VG_WAVE * U;                                  // chunks per slice
    const int S = (a.nch + slice - 1) / slice;
    const int nch_pad = S * slice;

    // ---- query: global -> LDS, zero padded to whole slices; the candidate lists reuse the space at the end
    uint4 *qs = reinterpret_cast<uint4 *>(smem);
    for (int c = threadIdx.x; c < nch_pad; c += VG_BLOCK)
        qs[c] = (c < a.nch) ? reinterpret_cast<const uint4 *>(a.query)[c] : make_uint4(0u, 0u, 0u, 0u);
    constexpr bool AFTER_LDS = AFTER && (VT == T_F16 || VT == T_BF16);      // (see vg_scan_kernel: the floor in LDS for the half types)
    const uint64_t *floor_lds = nullptr;
    if constexpr (AFTER_LDS) {
        __shared__ uint64_t floor_slot;
        if (threadIdx.x == 0) floor_slot = a.floor[0];
        floor_lds = &floor_slot;
    }
    __syncthreads();

    // query statistics over the whole query (norm / special flags), folded slice by slice
    typename Accum<VT, ACC>::QStat qstat;
    {
        uint4 q0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) q0[u] = qs[u * VG_WAVE + lane];
        qstat = Accum<VT, ACC>::template query_stat<U>(q0, 6);
        for (int s = 1; s < S; ++s) {
#pragma unroll
            for (int u = 0; u < U; ++u) q0[u] = qs[s * slice + u * VG_WAVE + lane];
            Accum<VT, ACC>::merge_qstat(qstat, Accum<VT, ACC>::template query_stat<U>(q0, 6));
        }
    }

    uint64_t mine = VG_EMPTY_KEY, thr = VG_EMPTY_KEY;
    const int k = a.k;
    const bool store_mode = (WITHIN || MASKED || AFTER || GROUPED) ? false : (a.out_dist != nullptr);
    uint32_t mlab = 0xFFFFFFFFu;                                    // grouped mode only: the label of the key in `mine`
    uint64_t floor_key = 0ull;                                      // after mode only (see vg_scan_kernel)
    if constexpr (AFTER && !AFTER_LDS) floor_key = vg_uniform64(a.floor[0]);
    uint64_t *wqueue = reinterpret_cast<uint64_t *>(smem + a.store_lds_off) + wave * VG_WITHIN_QUEUE;   // within mode only (vg_within_offer)
    int wqueued = 0;
    const long long wstride = (long long)gridDim.x * VG_WAVES_PER_BLOCK;
    const long long gw = (long long)blockIdx.x * VG_WAVES_PER_BLOCK + wave;

    // flattened (row, slice) stream per wavefront, one slice prefetched
    // (masked mode: `live` = the row's bit is set; a row whose bit is clear issues no slice loads - the same address selection)
    // (grouped mode: the row's label comes with EVERY slice of the row - one dword, the same address for all lanes and for all slices
    //  of a row, unconditional like the chunk loads - so that nothing is loaded outside the prefetch)
    auto load_slice = [&](uint4 (&dst)[U], uint32_t &lab_dst, long long row, int s, bool live = true) {
        if constexpr (GROUPED) lab_dst = a.labels[(row < a.n_rows && live) ? row : 0];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = s * slice + u * VG_WAVE + lane;
            if (VG_LOAD_PREDICATED) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (row < a.n_rows && live && c < a.nch) v = vg_load16<NT>(a.rows + row * a.stride + (long long)c * 16);
                dst[u] = v;
            } else {                                                // (unconditional, address selected: see vg_load_batch)
                dst[u] = vg_load16<NT>((row < a.n_rows && live && c < a.nch) ? a.rows + row * a.stride + (long long)c * 16
                                                                             : reinterpret_cast<const uint8_t *>(vg_zero_chunk));
            }
        }
    };
    uint4 cur[U], nxt[U];
    uint32_t lab_cur = 0xFFFFFFFFu, lab_nxt = 0xFFFFFFFFu;          // grouped mode only
    long long row = gw;
    // masked mode: the bit of the current row and of the wavefront's next one (wave-uniform, vg_mask_bits).  The next row's first slice is
    // prefetched during the current row's last step, so its bit is fetched when the current row STARTS: one step ahead of that prefetch
    // at least.  A row whose bit is clear takes one step (no loads, no arithmetic) instead of S.
    bool m_cur = true, m_nxt = true;
    if constexpr (MASKED) {
        m_cur = vg_mask_bits(a.mask, row, 1, row < a.n_rows) != 0ull;
        m_nxt = vg_mask_bits(a.mask, row + wstride, 1, row + wstride < a.n_rows) != 0ull;
    }
    load_slice(cur, lab_cur, row, 0, m_cur);
    Accum<VT, ACC> acc;
    acc.init();
    int s = 0;
    while (row < a.n_rows) {
        long long nrow = row;
        int ns = s + 1;
        bool m_load = m_cur;
        if (ns == S || (MASKED && !m_cur)) { ns = 0; nrow = row + wstride; m_load = m_nxt; }
        load_slice(nxt, lab_nxt, nrow, ns, m_load);
        if (!MASKED || m_cur) {
#pragma unroll
            for (int u = 0; u < U; ++u) acc.chunk(qs[s * slice + u * VG_WAVE + lane], cur[u]);
        }
        if (ns == 0 && (!MASKED || m_cur)) {                        // row complete (masked mode: nothing to finish for a row that was not read)
            float d = acc.finish(qstat, 6, a.root);
            if constexpr (VT == T_F16 || VT == T_BF16) {
                if (acc.special(qstat, 6) && lane == 0)
                    d = vg_slow_distance<VT, ACC>(reinterpret_cast<const uint16_t *>(qs),
                                                  reinterpret_cast<const uint16_t *>(a.rows + row * a.stride), a.dim, a.root);
            }
            d = vg_clamp(d);
            if (store_mode) {
                if (lane == 0) a.out_dist[row] = d;
            } else {
                // the predicate of vg_scan_kernel's offer (MASKED: a row whose bit is clear never gets here)
                const uint64_t key = vg_make_key(d, (uint32_t)row);
                if constexpr (AFTER_LDS) floor_key = *reinterpret_cast<const volatile uint64_t *>(floor_lds);
                bool ok;
                if constexpr (AFTER) ok = (lane == 0) && (d < INFINITY) && (key >= floor_key);
                else ok = (lane == 0) && (!WITHIN || d <= a.within_r) && (d < INFINITY);
                if constexpr (WITHIN) vg_within_offer(key, ok, wqueue, wqueued, a.emit, a.within_cap, lane);
                else if constexpr (CAPPED) vg_list_offer_capped(key, lab_cur, ok && (lab_cur != 0xFFFFFFFFu), mine, mlab, thr, lane, k, (int)a.within_cap);
                else if constexpr (GROUPED) vg_list_offer_grouped(key, lab_cur, ok && (lab_cur != 0xFFFFFFFFu), mine, mlab, thr, lane, k);
                else vg_list_offer(key, ok, mine, thr, lane, k);
            }
            acc.init();
        }
        if constexpr (MASKED) {
            if (ns == 0) { m_cur = m_nxt; m_nxt = vg_mask_bits(a.mask, nrow + wstride, 1, nrow + wstride < a.n_rows) != 0ull; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        if constexpr (GROUPED) lab_cur = lab_nxt;
        row = nrow;
        s = ns;
    }
    if constexpr (WITHIN) {
        if (wqueued > 0) vg_within_flush(wqueue, wqueued, a.emit, a.within_cap, lane);
        return;
    }
    if (store_mode) return;

    __syncthreads();                                   // everyone is done with the query staging area
    if constexpr (CAPPED) vg_block_publish_capped(smem, mine, mlab, k, (int)a.within_cap, VG_WAVES_PER_BLOCK, a.cand + (long long)blockIdx.x * VG_WAVE, nullptr);
    else if constexpr (GROUPED) vg_block_publish_grouped(smem, mine, mlab, k, VG_WAVES_PER_BLOCK, a.cand + (long long)blockIdx.x * VG_WAVE, nullptr);
    else vg_block_publish(smem, mine, k, a.cand + (long long)blockIdx.x * VG_WAVE);
}


// (float) sum x^2 per row of an f16 / bf16 corpus, accumulated exactly like AccumHalf<.., A_COS> does it during a scan
// (f32 squares - exact for halves - widened to f64, f64 sums, one rounding to float at the end): the cosine scan then
// only has to accumulate the dot product (A_COSN).  16 lanes per row.  Rows holding Inf/NaN get whatever comes out:
// the scan sends them to the exact slow path anyway.
template <int VT>
__global__ __launch_bounds__(256) void vg_half_rownorm_kernel(const uint8_t *rows, long long row0, long long n, long long stride,
                                                              int nch, float *out) {
    const int sub = threadIdx.x & 15;
    const long long group = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const long long ngroups = ((long long)gridDim.x * blockDim.x) >> 4;
    for (long long r = group; r < n; r += ngroups) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rows + (row0 + r) * stride);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int c = sub; c < nch; c += 16) {
            const uint4 v = p[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float lo, hi;
                vg_unpack2<VT>(w[j], lo, hi);
                if (j & 1) { s2 += (double)(lo * lo); s3 += (double)(hi * hi); }
                else { s0 += (double)(lo * lo); s1 += (double)(hi * hi); }
            }
        }
        const double s = vg_group_sum((s0 + s1) + (s2 + s3), 4);
        // (a sum that is not zero must not READ as zero: the filters judge a row of zeros - and only that - by its norm being exactly 0;
        //  bf16 elements below ~1e-23 square to less than the smallest float: such a row keeps the smallest one and stays unjudged)
        if (sub == 0) { const float f = (float)s; out[row0 + r] = (s > 0.0 && f == 0.0f) ? 1.401298464324817e-45f : f; }
    }
}
