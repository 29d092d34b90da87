// vg_scan_multi_masked.h - several queries per pass over the ALLOWED rows of the corpus (vg_scan_topk_batch_masked).
//
// vg_scan_multi_kernel's loop (vg_scan_multi.h) with the row mask threaded through the way the MASKED branch of vg_scan_kernel does it
// (vg_scan.h): NQ queries staged through LDS into registers, every (query, row) pair through the same Accum<VT, ACC> chunk order and
// the same finish / vg_clamp epilogue as the single scans, one candidate list per query, NQ publishes at the end.  What the mask adds:
//   * the bits of a batch (vg_mask_bits: wave-uniform, one scalar load) are fetched ONE loop step ahead of the row prefetch whose
//     addresses they decide - `mnext` is asked for while the batch in front of it is reduced;
//   * a batch without an allowed row points its U loads at the zero chunk (one cache line, always a hit) and does no arithmetic for
//     any of the NQ queries: a scalar branch around the whole reduction;
//   * a row whose bit is clear is computed with its batch and not offered to any list.
// So a pass reads the batches that hold an allowed row, once, for NQ queries.  A copy of the loop, not a template flag on
// vg_scan_multi_kernel: the unmasked instances stay byte-identical, and both stay in step by hand (as the four loops of vg_scan_kernel do).
// Double-buffered only: no prefetch ring for short uint8 / int8 rows.
//   a.query : NQ zero-padded queries back to back (nch * 16 bytes each)
//   a.mask  : ceil(n_rows / 64) words, bits behind the last row clear
//   a.cand  : [NQ][gridDim.x][64] candidate keys, merged per query by vg_merge_kernel (grid NQ)
// Register budget: that of vg_scan_multi_kernel (NQ * U query chunks + 2 * U row chunks per lane); the mask lives in scalar registers
// (three words of bits: current, prefetched, in flight).
#pragma once

#include "vg_scan.h"

template <int VT, int ACC, int U, int NQ, bool NT>          // VT: T_F32 / T_U8 / T_I8
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_multi_masked_kernel(ScanArgs a) {
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
    uint64_t mine[NQ], thr[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) { mine[n] = VG_EMPTY_KEY; thr[n] = VG_EMPTY_KEY; }
    const int k = a.k;

    const long long nbatch = (a.n_rows + rpb - 1) / rpb;
    const long long wstride = (long long)gridDim.x * VG_WAVES_PER_BLOCK;
    long long b = (long long)blockIdx.x * VG_WAVES_PER_BLOCK + wave;
    // the mask bits of a batch (wave-uniform; 0 behind the last batch)
    auto mask_of = [&](long long batch) -> uint64_t { return vg_mask_bits(a.mask, batch * rpb, rpb, batch < nbatch); };
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
                vg_list_offer(vg_make_key(d, (uint32_t)row), allowed && (d < INFINITY), mine[n], thr[n], lane, k);
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
