// vg_scan_multi_within_masked.h - several queries per pass, every ALLOWED row within a radius of each (vg_scan_within_batch_masked).
//
// vg_scan_multi_within_kernel's loop (vg_scan_multi_within.h) with the row mask threaded through exactly as
// vg_scan_multi_masked_kernel does it (vg_scan_multi_masked.h):
//   * the bits of a batch (vg_mask_bits: wave-uniform, one scalar load) are fetched ONE loop step ahead of the row prefetch whose
//     addresses they decide - `mnext` is asked for while the batch in front of it is reduced;
//   * a batch without an allowed row points its U loads at the zero chunk and does nothing else: a scalar branch around all NQ
//     reductions and ballots;
//   * a row whose bit is clear is computed with its batch and matches no query (`allowed` folded into `owner`).
// Descriptors (VgWithinQuery), queues and the offer / flush protocol (vg_mw_offer / vg_mw_flush) are vg_scan_multi_within.h's, unchanged:
// the floats of an allowed row are those vg_scan_multi_within_kernel computes for it.  A copy of the loop, not a template flag: the
// unmasked instances stay byte-identical, and the copies stay in step by hand.
//   a.query         : NQ zero-padded queries back to back (nch * 16 bytes each), and BEHIND them NQ VgWithinQuery descriptors
//   a.mask          : ceil(n_rows / 64) words, bits behind the last row clear
//   a.store_lds_off : byte offset in dynamic LDS of the key queues, [NQ][wavefront][VG_WITHIN_QUEUE]
// Register budget: that of vg_scan_multi_within_kernel plus the mask in scalar registers (three words of bits: current, prefetched, in
// flight, and the mask pointer): DESIGN.md 3.12 has the compiler's figures of every instance.
#pragma once

#include "vg_scan_multi_within.h"

template <int VT, int ACC, int U, int NQ, bool NT>          // VT: T_F32 / T_U8 / T_I8
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_multi_within_masked_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & (VG_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // wave-uniform by construction: the queue addresses stay scalar
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
    const VgWithinQuery *wq = reinterpret_cast<const VgWithinQuery *>(a.query + (long long)NQ * a.nch * 16);
    float r[NQ];
    uint64_t *queue[NQ];
    int queued[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        r[n] = wq[n].r;
        queue[n] = reinterpret_cast<uint64_t *>(smem + a.store_lds_off) + (n * VG_WAVES_PER_BLOCK + wave) * VG_WITHIN_QUEUE;
        queued[n] = 0;
    }

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
            const bool owner = (sub == 0) && (row < a.n_rows) && ((mcur >> rib) & 1ull);      // the row's lane, and the row is allowed
            // every query's distance first, one ballot each; the rare batch with a match parks its keys BEHIND the arithmetic
            // (vg_scan_multi_within_kernel: the same order, the same reasons)
            float d[NQ];
            unsigned long long any = 0ull;
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                Accum<VT, ACC> acc;
                acc.init();
#pragma unroll
                for (int u = 0; u < U; ++u) acc.chunk(q[n][u], cur[u]);
                d[n] = vg_clamp(acc.finish(qstat[n], lpr_log2, a.root));
                any |= __ballot(owner && (d[n] <= r[n]) && (d[n] < INFINITY));
            }
            if (any != 0ull) {
                int ln = lane;
                asm volatile("" : "+v"(ln));
                const VgWithinQuery *w = wq;
                asm volatile("" : "+s"(w));
#pragma unroll
                for (int n = 0; n < NQ; ++n)
                    vg_mw_offer(vg_make_key(d[n], (uint32_t)row), owner && (d[n] <= r[n]) && (d[n] < INFINITY), queue[n], queued[n], w[n].out, w[n].cap, ln);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        mcur = mnxt;
        b = bn;
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n)
        if (queued[n] > 0) vg_mw_flush(queue[n], queued[n], wq[n].out, wq[n].cap, lane);
}
