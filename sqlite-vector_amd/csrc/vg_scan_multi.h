// vg_scan_multi.h - several queries per pass over the corpus: ONE kernel, its forms are compile-time flags.
//
// The batched entry points' path for every shape the matrix-core kernels (vg_batch.hip / vg_batch_i8.hip) do not serve on f32 /
// uint8 / int8 corpora: L1, rows > 512 floats / 1024 bytes, 32 < k <= 64 - and the path of the masked, paged and range batches.  NQ
// queries, staged through LDS into registers, share every row load of the HBM-bound scan
// (f16 / bf16 scans are bound by their f64 arithmetic and gain nothing - vg_multi.hip).  The arithmetic of each (query, row) pair is
// the single-query kernel's (same Accum<VT, ACC> chunk order, same finish / vg_clamp epilogue) in EVERY form, so int8 / uint8 results
// are bit-identical to the single scans and f32 results differ at most by the summation order of another launch shape.
// Double-buffered only: no prefetch ring for short uint8 / int8 rows.
//
// FORM is a set of flags; each changes what happens to a distance, none how it is computed:
//   (none)           top-k, k <= 64: one candidate list per query (`mine`, `thr`), NQ publishes at the end, merged per query by
//                    vg_merge_kernel (grid NQ).
//   VG_MQ_MASKED     only the rows the handle's mask allows, threaded through the way the MASKED branch of vg_scan_kernel does it
//                    (vg_scan.h):
//                      * the bits of a batch (vg_mask_bits: wave-uniform, one scalar load) are fetched ONE loop step ahead of the row
//                        prefetch whose addresses they decide - `mnext` is asked for while the batch in front of it is reduced;
//                      * a batch without an allowed row points its U loads at the zero chunk (one cache line, always a hit) and does
//                        nothing else: a scalar branch around all NQ reductions;
//                      * a row whose bit is clear is computed with its batch and offered to no query (the bit is folded into `owner`).
//                    So a pass reads the batches that hold an allowed row, once, for NQ queries.  Without the flag mask_of() is the
//                    constant ~0 and the compiler folds the whole pipeline away.
//   VG_MQ_AFTER      top-k behind a cursor per query (the paged scans): a row is offered to query n's list only when its key is
//                    >= a.floor[n] (the key just behind that query's cursor; VG_EMPTY_KEY in the pad slot of a ragged pass admits
//                    nothing).  The NQ floors are loaded once before the loop, made wave-uniform (vg_uniform64) and live in scalar
//                    registers (2 per query); the compare is one 64-bit v_cmp folded into the offer's predicate.  This is the batch
//                    path of the paged scans, NOT the matrix-core filters: their candidate thresholds assume an unrestricted top-k - a
//                    floor moves the k-th best distance arbitrarily far from what their lower bounds were tuned against.
//   VG_MQ_WITHIN     range scan in place of the candidate lists: per query the compare against that query's radius and one ballot.
//                    Only a batch with a match does more: BEHIND the arithmetic of all NQ queries, where the current row chunks are
//                    dead (the queue / flush temporaries then do not add to the loop's peak register pressure), the keys are parked
//                    in the wavefront's LDS queue of their query and leave in bursts (vg_mw_offer / vg_mw_flush below).  Nothing is
//                    written for a row that matches no query: a batch without a match costs NQ ballots.  What a query keeps between
//                    batches - radius and queue fill - is wave-uniform and lives in scalar registers (`wave` goes through
//                    readfirstlane so that the queue addresses stay scalar); region and capacity are read from the descriptors when
//                    a burst leaves.  Not combined with VG_MQ_AFTER.
//   VG_MQ_LABELED    a label per row, each query its own label: a row is offered to query n only when labels[row] == qlabels[n].
//                    The masked form's pipeline with a per-lane dword in place of the wave-uniform mask word:
//                      * every lane loads the label of its own row (lanes of one row read the same dword; row 0 stands in for a row
//                        out of range, whose result is then unused, as for row_nn) ONE loop step ahead of the row prefetch whose
//                        addresses it decides, and inside a step BEFORE that prefetch: vector loads return in order, so waiting for
//                        a label leaves the row loads issued before it - the current batch - as the only ones that must have landed;
//                      * one ballot over "carries the label of any of the pass' NQ queries" is the batch's wave-uniform word: zero
//                        points the U loads at the zero chunk and skips all arithmetic with a scalar branch;
//                      * the NQ query labels are loaded once, made wave-uniform and live in scalar registers; `label == qlabel[n]`
//                        is folded into query n's offer predicate.  VG_LABEL_NONE (0xFFFFFFFF) matches nothing on either side: it
//                        is folded into `owner`, so a pad query of a ragged pass (label NONE) collects nothing.
//                    What the pipeline carries: three label dwords per lane (current, prefetched, in flight) and the current batch's
//                    ballot - per-stage ballots PER QUERY would be 2 * NQ scalar registers a stage.  Combined with
//                    WITHIN only (next), not with MASKED / AFTER.  Without the flag the label values are never defined and everything
//                    folds away.
//   VG_MQ_LABELED | VG_MQ_WITHIN   the labeled range scan, each query its own label AND its own radius (vg_scan_within_batch_labeled,
//                    vg_multi_within.hip): the LABELED pipeline, statement for statement, with WITHIN's compare-and-compact behind the
//                    arithmetic.  `lcur == qlabel[n]` is folded into query n's match predicate - in the ballot that decides whether a
//                    batch does more, and in vg_mw_offer.  The query's label travels in its VgWithinQuery descriptor (12 of its bytes
//                    were spare) and is read with the radius by a scalar load: a.qlabels is not read, ScanArgs keeps its size and every
//                    field its offset.  A pad query of a ragged pass: label NONE, capacity 0, radius -Inf.  The instances are
//                    vg_multi_within_labeled.hip's; DESIGN.md 3.21 has their registers and the ones left out.
//   VG_MQ_LABELSET   a SET of labels per query (allowed or excluded; vg_multi_labelset.hip): the LABELED pipeline, statement for
//                    statement, with other predicates.  The per-lane dword loaded one step ahead of the row prefetch is the row's
//                    MEMBERSHIP word - a.labels points at the membership buffer a pre-pass filled for a group of up to 32 queries
//                    (bit j: query j of the group may see the row; exclusion folded in, 0 for a row without a label) - shifted right
//                    by the pass' offset inside its group, so that bit n is query n of the pass.  The batch's wave-uniform word is
//                    one ballot over "any of the pass' NQ bits set": zero points the U loads at the zero chunk and skips all
//                    arithmetic.  Bit n is folded into query n's offer predicate in place of `lcur == qlabel[n]`; no query labels
//                    are loaded.  The shift (wave-uniform, 0 .. 32 - NQ) travels in a.within_cap, which no other top-k instance of
//                    this form reads: ScanArgs keeps its size and every field its offset.  A pad query of a ragged pass has no bit
//                    set in any word (the pre-pass sets bits of real queries only) and collects nothing.  Not combined with any
//                    other flag.
//   VG_MQ_GROUPED    the k nearest LABELS per query, each by its best row (the batch form of VG_SQ_GROUPED, vg_scan.h).  Combined with
//                    VG_MQ_MASKED only.  Every lane loads the label of its own row WITH the row prefetch of that batch (row 0 stands
//                    in for a row out of range or in a batch that is not read); the label decides no address, so - unlike LABELED -
//                    it does not run a step ahead: two label dwords per lane, current and prefetched.  Each query keeps one more
//                    register next to `mine` / `thr`: `mlab`, the label of the key in `mine`, and its list stays distinct by label
//                    (vg_list_offer_grouped).  A row without a label is offered to no query.  The pad queries of a ragged pass
//                    collect whatever they collect; their lists are never read.  Lists leave as keys only
//                    (vg_block_publish_grouped), merged per query by vg_merge_grouped_batch_kernel (vg_multi_grouped.hip, grid NQ).
//   VG_MQ_CAPPED     the k nearest ROWS per query, at most m = ScanArgs.within_cap of one label (the batch form of VG_SQ_CAPPED,
//                    vg_scan.h; vg_multi_capped.hip).  A modifier of VG_MQ_GROUPED: legal only together with it, alone or with
//                    VG_MQ_MASKED.  Every statement of the grouped form stands - the label load behind the row prefetch, the
//                    scheduling barrier, row 0 standing in, the mlab registers - except the two that touch a list: the offer is
//                    vg_list_offer_capped and the workgroup merge vg_block_publish_capped.  m is wave-uniform, clamped to k by the
//                    host and shared by the NQ queries of a pass; within_cap is read by no other top-k instance of this kernel, so
//                    ScanArgs keeps its size.  Lists merge per query in vg_merge_capped_batch_kernel (vg_multi_capped.hip, grid NQ).
// The forms were five hand-copied loops; the code generated for every instance of this template was checked identical to that of the
// copy it replaced (instruction text, registers, spills, scratch, LDS: DESIGN.md 3.6) at the commit that folded them.
//
//   a.query         : NQ zero-padded queries back to back (nch * 16 bytes each); WITHIN: and BEHIND them NQ VgWithinQuery descriptors
//   a.mask          : (MASKED) ceil(n_rows / 64) words, bits behind the last row clear
//   a.floor         : (AFTER) NQ keys
//   a.labels        : (LABELED, GROUPED) n_rows dwords;  a.qlabels : (LABELED without WITHIN) NQ dwords
//                     (LABELSET) n_rows membership dwords
//   a.within_cap    : (CAPPED) the cap m, 1 .. k;  (LABELSET) the pass' bit offset inside its membership group
//   a.cand          : (top-k forms) [NQ][gridDim.x][64] candidate keys
//   descriptor n    : (WITHIN) the [count | cap keys] region of query n, its capacity and its radius (a float: the host rounds down);
//                     (LABELED | WITHIN) and its label
//   a.store_lds_off : (WITHIN) byte offset in dynamic LDS of the key queues, [NQ][wavefront][VG_WITHIN_QUEUE]
// Register budget: NQ * U query chunks + 2 * U row chunks per lane -> NQ = 4 with U <= 3, NQ = 2 with U <= 6.  The mask lives in scalar
// registers (three words of bits: current, prefetched, in flight, and the mask pointer).  A range form does without the two 64-bit
// list words per query: it is at or below the VGPR figure of the top-k instance of the same <VT, ACC, U, NQ>.  DESIGN.md 3.9 - 3.13
// have the compiler's figures of every instance.
#pragma once

#include "vg_scan.h"

enum : int { VG_MQ_MASKED = 1, VG_MQ_AFTER = 2, VG_MQ_WITHIN = 4, VG_MQ_LABELED = 8, VG_MQ_GROUPED = 16, VG_MQ_CAPPED = 32, VG_MQ_LABELSET = 64 };
#define VG_MQ_LABEL_NONE 0xFFFFFFFFu      // (VG_LABEL_NONE of vectorgpu.h)

struct VgWithinQuery {                 // 32 bytes, read through wave-uniform addresses (scalar loads)
    unsigned long long *out;           // [count | cap keys]; the count keeps counting past cap
    unsigned long long cap;
    float r;                           // rows with d <= r and d finite match
    uint32_t label;                    // (LABELED | WITHIN) ... and this label; no other range form reads it
    uint32_t pad[2];
};

// Kernel-local forms of vg_within_offer / vg_within_flush (vg_scan.h, which the single range scan keeps as it is): the same protocol -
// keys parked in the wavefront's queue, one atomicAdd of the burst size, the count keeps counting past the capacity - with the burst's
// room worked out in scalar registers and the stores addressed by a 32-bit lane offset against a wave-uniform base, so that the rare
// path holds a handful of vector temporaries next to the NQ * U query chunks instead of 64-bit indices and addresses per lane.
__device__ inline void vg_mw_flush(const uint64_t *queue, int &queued, unsigned long long *out, unsigned long long cap, int lane) {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(out, (unsigned long long)queued);
    base = vg_readlane64(base, 0);
    const unsigned long long left = base < cap ? cap - base : 0ull;                    // keys that still fit (wave-uniform)
    const int room = left < (unsigned long long)queued ? (int)left : queued;
    unsigned long long *dst = out + 1 + base;                                          // wave-uniform
    for (int i = lane; i < room; i += VG_WAVE) dst[i] = queue[i];
    queued = 0;
}
__device__ inline void vg_mw_offer(uint64_t key, bool match, uint64_t *queue, int &queued, unsigned long long *out, unsigned long long cap, int lane) {
    const unsigned long long m = __ballot(match);
    if (m == 0ull) return;
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (match) queue[queued + rank] = key;
    queued += __popcll(m);
    if (queued > VG_WITHIN_QUEUE - VG_WAVE) vg_mw_flush(queue, queued, out, cap, lane);
}

template <int VT, int ACC, int U, int NQ, int FORM>          // VT: T_F32 / T_U8 / T_I8; FORM: VG_MQ_* flags
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_multi_kernel(ScanArgs a) {
    constexpr bool MASKED = (FORM & VG_MQ_MASKED) != 0, AFTER = (FORM & VG_MQ_AFTER) != 0, WITHIN = (FORM & VG_MQ_WITHIN) != 0;
    constexpr bool LABELED = (FORM & VG_MQ_LABELED) != 0, GROUPED = (FORM & VG_MQ_GROUPED) != 0, CAPPED = (FORM & VG_MQ_CAPPED) != 0;
    static_assert(!(AFTER && WITHIN), "a range scan has no cursor");
    static_assert(!LABELED || FORM == VG_MQ_LABELED || FORM == (VG_MQ_LABELED | VG_MQ_WITHIN), "the labeled form is combined with the range form only");
    static_assert(!GROUPED || (FORM & ~(VG_MQ_MASKED | VG_MQ_CAPPED)) == VG_MQ_GROUPED, "the grouped form is combined with the mask and the cap only");
    static_assert(!CAPPED || GROUPED, "a capped scan is the grouped form with a cap");
    constexpr bool LABELSET = (FORM & VG_MQ_LABELSET) != 0;
    static_assert(!LABELSET || FORM == VG_MQ_LABELSET, "the label-set form is not combined with any other form");
    constexpr bool LANEWORD = LABELED || LABELSET;                     // a per-lane dword runs one step ahead of the row prefetch
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    // (WITHIN: wave-uniform by construction; readfirstlane says so to the compiler, and the queue addresses stay scalar)
    const int wave = WITHIN ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    const int lpr_log2 = a.lpr_log2;
    const int lpr = 1 << lpr_log2;
    const int rpb = VG_WAVE >> lpr_log2;
    const int sub = lane & (lpr - 1);
    const int rib = lane >> lpr_log2;

    uint4 *qs = reinterpret_cast<uint4 *>(smem);                       // [NQ][nch]
    for (int c = threadIdx.x; c < NQ * a.nch; c += VG_BLOCK) qs[c] = reinterpret_cast<const uint4 *>(a.query)[c];
    __syncthreads();
    uint4 q[NQ][U];
    typename Accum<VT, ACC>::QStat qstat[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = sub + u * lpr;
            q[n][u] = (c < a.nch) ? qs[n * a.nch + c] : make_uint4(0u, 0u, 0u, 0u);
        }
        qstat[n] = Accum<VT, ACC>::template query_stat<U>(q[n], lpr_log2);
    }
    // what a query keeps between batches: its candidate list (and floor), or its radius and queue
    uint64_t mine[NQ], thr[NQ], floor_key[NQ];
    uint32_t mlab[NQ];                                                 // GROUPED: the label of the key in `mine`
    const int k = a.k;
    const VgWithinQuery *wq = reinterpret_cast<const VgWithinQuery *>(a.query + (long long)NQ * a.nch * 16);
    float r[NQ];
    uint64_t *queue[NQ];
    int queued[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        if constexpr (WITHIN) {
            r[n] = wq[n].r;
            queue[n] = reinterpret_cast<uint64_t *>(smem + a.store_lds_off) + (n * VG_WAVES_PER_BLOCK + wave) * VG_WITHIN_QUEUE;
            queued[n] = 0;
        } else {
            mine[n] = VG_EMPTY_KEY;
            thr[n] = VG_EMPTY_KEY;
            if constexpr (GROUPED) mlab[n] = VG_MQ_LABEL_NONE;
            if constexpr (AFTER) floor_key[n] = vg_uniform64(a.floor[n]);
        }
    }
    uint32_t qlabel[NQ];                                               // LABELED: wave-uniform, scalar registers
    if constexpr (LABELED && WITHIN) {                                 // (the label travels with the radius, in the query's descriptor)
#pragma unroll
        for (int n = 0; n < NQ; ++n) qlabel[n] = (uint32_t)__builtin_amdgcn_readfirstlane((int)wq[n].label);
    } else if constexpr (LABELED) {
#pragma unroll
        for (int n = 0; n < NQ; ++n) qlabel[n] = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.qlabels[n]);
    }

    // LABELSET: the pass' bit offset inside its membership group (wave-uniform, a scalar register)
    int mshift = 0;
    if constexpr (LABELSET) mshift = __builtin_amdgcn_readfirstlane((int)a.within_cap);

    const long long nbatch = (a.n_rows + rpb - 1) / rpb;
    const long long wstride = (long long)gridDim.x * VG_WAVES_PER_BLOCK;
    long long b = (long long)blockIdx.x * VG_WAVES_PER_BLOCK + wave;
    // MASKED: the mask bits of a batch (wave-uniform; 0 behind the last batch).  Otherwise every batch in range is live.
    auto mask_of = [&](long long batch) -> uint64_t {
        if constexpr (MASKED) return vg_mask_bits(a.mask, batch * rpb, rpb, batch < nbatch);
        else return ~0ull;
    };
    // LABELED: the label of this lane's row of a batch (unconditional load, only the address is selected: see vg_load_batch), and
    // the batch's word - which lanes hold a row that carries the label of any query of the pass (0 behind the last batch)
    auto label_of = [&](long long batch) -> uint32_t {
        const long long r0 = batch * rpb + rib;
        return a.labels[(batch < nbatch && r0 < a.n_rows) ? r0 : 0];
    };
    auto label_hits = [&](uint32_t lab, long long batch) -> uint64_t {
        bool hit = false;
#pragma unroll
        for (int n = 0; n < NQ; ++n) hit |= (lab == qlabel[n]);
        return __ballot(hit && lab != VG_MQ_LABEL_NONE && batch < nbatch && batch * rpb + rib < a.n_rows);
    };
    // LABELSET: the membership word of this lane's row with the pass' NQ bits at the bottom (the same unconditional load), and the
    // batch's word - which lanes hold a row that any query of the pass may see
    auto member_of = [&](long long batch) -> uint32_t {
        const long long r0 = batch * rpb + rib;
        return (a.labels[(batch < nbatch && r0 < a.n_rows) ? r0 : 0] >> mshift) & ((1u << NQ) - 1u);
    };
    auto member_hits = [&](uint32_t bits, long long batch) -> uint64_t {
        return __ballot(bits != 0u && batch < nbatch && batch * rpb + rib < a.n_rows);
    };
    // GROUPED: the label of this lane's row of a batch, loaded with the batch's rows (`live`: the batch is read at all)
    auto group_label_of = [&](long long batch, bool live) -> uint32_t {
        const long long r0 = batch * rpb + rib;
        return a.labels[(batch < nbatch && live && r0 < a.n_rows) ? r0 : 0];
    };
    uint4 cur[U], nxt[U];
    uint32_t lcur = 0u, lnext = 0u;
    if constexpr (LABELED) { lcur = label_of(b); lnext = label_of(b + wstride); }
    if constexpr (LABELSET) { lcur = member_of(b); lnext = member_of(b + wstride); }
    uint64_t mcur = LABELSET ? member_hits(lcur, b) : LABELED ? label_hits(lcur, b) : mask_of(b);
    uint64_t mnext = LANEWORD ? 0ull : mask_of(b + wstride);
    vg_load_batch<U, true>(cur, a.rows, b * rpb + rib, (b < nbatch && mcur != 0ull) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
    if constexpr (GROUPED) lcur = group_label_of(b, mcur != 0ull);
    while (b < nbatch) {
        const long long bn = b + wstride;
        uint64_t mnxt = mnext;                                         // the bits of batch bn: asked for one step ago
        const uint32_t lnxt = lnext;                                   // LABELED: and the labels of batch bn
        if constexpr (LABELED) {
            mnxt = label_hits(lnxt, bn);
            lnext = label_of(bn + wstride);                            // (issued in front of the row prefetch below)
        } else if constexpr (LABELSET) {
            mnxt = member_hits(lnxt, bn);
            lnext = member_of(bn + wstride);                           // (the same)
        } else {
            mnext = mask_of(bn + wstride);
        }
        vg_load_batch<U, true>(nxt, a.rows, bn * rpb + rib, (bn < nbatch && mnxt != 0ull) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
        if constexpr (GROUPED) {
            lnext = group_label_of(bn, mnxt != 0ull);
            // (the whole prefetch, label included, is issued before the arithmetic starts: see the grouped single form, vg_scan.h)
            __builtin_amdgcn_sched_barrier(0);
        }
        if (mcur != 0ull) {
            const long long row = b * rpb + rib;
            // the row's lane, and the row is allowed (LABELED: carries a label at all - which query's is the offer's business)
            // (LABELSET: in range - which query may see it is the offer's business; a row without a label has no bit set)
            const bool owner = LABELSET  ? (sub == 0) && (row < a.n_rows)
                               : LABELED ? (sub == 0) && (row < a.n_rows) && (lcur != VG_MQ_LABEL_NONE)
                                         : (sub == 0) && (row < a.n_rows) && ((mcur >> rib) & 1ull);
            // (WITHIN: every query's distance first, one ballot each; the rare batch with a match parks its keys BEHIND the arithmetic)
            float d[NQ];
            unsigned long long any = 0ull;
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                Accum<VT, ACC> acc;
                acc.init();
#pragma unroll
                for (int u = 0; u < U; ++u) acc.chunk(q[n][u], cur[u]);
                const float dn = vg_clamp(acc.finish(qstat[n], lpr_log2, a.root));
                if constexpr (WITHIN) {
                    d[n] = dn;
                    // d <= r is false for NaN; +Inf never matches, whatever the radius (the single range scan's rule)
                    // (LABELED: and the row carries query n's label.  A branch of its own: the other range forms keep their expression,
                    //  and with it the code the compiler made of it)
                    if constexpr (LABELED) any |= __ballot(owner && (d[n] <= r[n]) && (d[n] < INFINITY) && (lcur == qlabel[n]));
                    else any |= __ballot(owner && (d[n] <= r[n]) && (d[n] < INFINITY));
                } else {
                    // (a top-k form uses the distance at once, NOT through d[]: with it the ten f32 L1 floor instances came out with
                    //  another, equivalent, predicate sequence than the copies had)
                    const uint64_t key = vg_make_key(dn, (uint32_t)row);
                    if constexpr (CAPPED) vg_list_offer_capped(key, lcur, owner && (dn < INFINITY) && (lcur != VG_MQ_LABEL_NONE), mine[n], mlab[n], thr[n], lane, k, (int)a.within_cap);
                    else if constexpr (GROUPED) vg_list_offer_grouped(key, lcur, owner && (dn < INFINITY) && (lcur != VG_MQ_LABEL_NONE), mine[n], mlab[n], thr[n], lane, k);
                    else if constexpr (LABELED) vg_list_offer(key, owner && (dn < INFINITY) && (lcur == qlabel[n]), mine[n], thr[n], lane, k);
                    else if constexpr (LABELSET) vg_list_offer(key, owner && (dn < INFINITY) && ((lcur >> n) & 1u), mine[n], thr[n], lane, k);
                    else vg_list_offer(key, owner && (dn < INFINITY) && (!AFTER || key >= floor_key[n]), mine[n], thr[n], lane, k);
                }
            }
            if constexpr (WITHIN) if (any != 0ull) {
                // (the lane index goes through an opaque move: queue and store addresses derived from it are then worked out HERE, in the
                //  rare path, instead of being hoisted out of the loop into vector registers that stay live across the arithmetic)
                int ln = lane;
                asm volatile("" : "+v"(ln));
                // (region and capacity are read from the descriptors here, by scalar loads, rather than held in 4 scalar registers per query
                //  across the loop: with them the NQ = 4 instances ran out of scalar registers)
                const VgWithinQuery *w = wq;
                asm volatile("" : "+s"(w));
#pragma unroll
                for (int n = 0; n < NQ; ++n) {
                    if constexpr (LABELED)
                        vg_mw_offer(vg_make_key(d[n], (uint32_t)row), owner && (d[n] <= r[n]) && (d[n] < INFINITY) && (lcur == qlabel[n]), queue[n], queued[n], w[n].out, w[n].cap, ln);
                    else
                        vg_mw_offer(vg_make_key(d[n], (uint32_t)row), owner && (d[n] <= r[n]) && (d[n] < INFINITY), queue[n], queued[n], w[n].out, w[n].cap, ln);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        mcur = mnxt;
        if constexpr (LANEWORD) lcur = lnxt;
        if constexpr (GROUPED) lcur = lnext;
        b = bn;
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        if constexpr (WITHIN) {
            if (queued[n] > 0) vg_mw_flush(queue[n], queued[n], wq[n].out, wq[n].cap, lane);
        } else {
            __syncthreads();                               // query staging area / the previous publish is done with LDS
            if constexpr (CAPPED) vg_block_publish_capped(smem, mine[n], mlab[n], k, (int)a.within_cap, VG_WAVES_PER_BLOCK, a.cand + ((long long)n * gridDim.x + blockIdx.x) * VG_WAVE, nullptr);
            else if constexpr (GROUPED) vg_block_publish_grouped(smem, mine[n], mlab[n], k, VG_WAVES_PER_BLOCK, a.cand + ((long long)n * gridDim.x + blockIdx.x) * VG_WAVE, nullptr);
            else vg_block_publish(smem, mine[n], k, a.cand + ((long long)n * gridDim.x + blockIdx.x) * VG_WAVE);
        }
    }
}
