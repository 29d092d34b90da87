// vg_scan_multi_after.h - several queries per pass, each behind a cursor of its own (vg_scan_topk_batch_after[_masked]).
//
// vg_scan_multi_kernel's loop (vg_scan_multi.h) with one floor key per query: a row is offered to query n's list only when its key is
// >= a.floor[n] (the key just behind that query's cursor; VG_EMPTY_KEY in the pad slot of a ragged pass admits nothing).  The NQ
// floors are loaded once before the loop, wave-uniform, and live in scalar registers (2 per query); the compare is one 64-bit
// v_cmp folded into the offer's predicate.  MASKED = true threads the handle's row mask through exactly as
// vg_scan_multi_masked_kernel does (vg_scan_multi_masked.h): bits one step ahead of the row prefetch, the zero chunk and no
// arithmetic for a batch without an allowed row, a clear bit folded into `owner`.  Everything else - staging of the queries, Accum
// chunk order, finish / vg_clamp epilogue, one list per query, NQ publishes - is the parent loop's: the float of a (query, row) pair is
// bit for bit the one vg_scan_multi_kernel computes.  A copy of the loop, not a flag on it: the existing instances stay byte-identical.
//
// This is the batch path of the paged scans, NOT the matrix-core filters (vg_batch*.hip): their candidate thresholds assume an
// unrestricted top-k - a floor moves the k-th best distance arbitrarily far from what their lower bounds were tuned against.
//   a.query : NQ zero-padded queries back to back (nch * 16 bytes each)
//   a.floor : NQ keys
//   a.mask  : (MASKED) ceil(n_rows / 64) words, bits behind the last row clear
//   a.cand  : [NQ][gridDim.x][64] candidate keys, merged per query by vg_merge_kernel (grid NQ)
#pragma once

#include "vg_scan.h"

template <int VT, int ACC, int U, int NQ, bool NT, bool MASKED>          // VT: T_F32 / T_U8 / T_I8
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_multi_after_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = threadIdx.x >> 6;
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
    uint64_t mine[NQ], thr[NQ], floor_key[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) { mine[n] = VG_EMPTY_KEY; thr[n] = VG_EMPTY_KEY; floor_key[n] = vg_uniform64(a.floor[n]); }
    const int k = a.k;

    const long long nbatch = (a.n_rows + rpb - 1) / rpb;
    const long long wstride = (long long)gridDim.x * VG_WAVES_PER_BLOCK;
    long long b = (long long)blockIdx.x * VG_WAVES_PER_BLOCK + wave;
    // masked form: the mask bits of a batch (wave-uniform; 0 behind the last batch).  Unmasked: every batch in range is live.
    auto mask_of = [&](long long batch) -> uint64_t {
        if constexpr (MASKED) return vg_mask_bits(a.mask, batch * rpb, rpb, batch < nbatch);
        else return ~0ull;
    };
    uint4 cur[U], nxt[U];
    uint64_t mcur = mask_of(b);
    uint64_t mnext = mask_of(b + wstride);
    vg_load_batch<U, NT>(cur, a.rows, b * rpb + rib, (b < nbatch && mcur != 0ull) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
    while (b < nbatch) {
        const long long bn = b + wstride;
        const uint64_t mnxt = mnext;                                   // the bits of batch bn: asked for one step ago
        mnext = mask_of(bn + wstride);
        vg_load_batch<U, NT>(nxt, a.rows, bn * rpb + rib, (bn < nbatch && mnxt != 0ull) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
        if (mcur != 0ull) {
            const long long row = b * rpb + rib;
            const bool allowed = (sub == 0) && (row < a.n_rows) && ((mcur >> rib) & 1ull);
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                Accum<VT, ACC> acc;
                acc.init();
#pragma unroll
                for (int u = 0; u < U; ++u) acc.chunk(q[n][u], cur[u]);
                const float d = vg_clamp(acc.finish(qstat[n], lpr_log2, a.root));
                const uint64_t key = vg_make_key(d, (uint32_t)row);
                vg_list_offer(key, allowed && (d < INFINITY) && (key >= floor_key[n]), mine[n], thr[n], lane, k);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        mcur = mnxt;
        b = bn;
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        __syncthreads();                                   // query staging area / the previous publish is done with LDS
        vg_block_publish(smem, mine[n], k, a.cand + ((long long)n * gridDim.x + blockIdx.x) * VG_WAVE);
    }
}
