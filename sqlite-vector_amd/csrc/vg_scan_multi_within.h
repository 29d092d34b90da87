// vg_scan_multi_within.h - several queries per pass, every row within a radius of each (vg_scan_within_batch).
//
// vg_scan_multi_kernel's loop (vg_scan_multi.h) with the range scan's tail in place of the candidate lists: NQ queries staged through
// LDS into registers, every (query, row) pair through the same Accum<VT, ACC> chunk order and the same finish / vg_clamp epilogue - the
// floats are those vg_scan_multi_kernel computes - and then, per query, the compare against that query's radius and one ballot.  Only
// a batch with a match does more: behind the arithmetic of all NQ queries, where the current row chunks are dead, the keys are parked
// in the wavefront's LDS queue of their query and leave in bursts (vg_mw_offer / vg_mw_flush below: the protocol of vg_within_offer /
// vg_within_flush of vg_scan.h, which the single range scan keeps unchanged).  Nothing is written for a row that matches no query: a
// batch without a match costs NQ ballots.  No per-lane candidate list (`mine`, `thr`): what a query keeps between batches - radius and
// queue fill - is wave-uniform and lives in scalar registers; region and capacity are read from the descriptors when a burst leaves.
// A copy of the loop, not a template flag on vg_scan_multi_kernel: the top-k instances stay byte-identical, and the copies stay in step
// by hand.
//   a.query         : NQ zero-padded queries back to back (nch * 16 bytes each), and BEHIND them NQ VgWithinQuery descriptors
//   descriptor n    : the [count | cap keys] region of query n, its capacity and its radius (a float: the host rounds down)
//   a.store_lds_off : byte offset in dynamic LDS of the key queues, [NQ][wavefront][VG_WITHIN_QUEUE]
// Register budget: NQ * U query chunks + 2 * U row chunks per lane, as in vg_scan_multi_kernel, less its two 64-bit list words per query:
// every instance is at or below the VGPR figure of the top-k instance of the same <VT, ACC, U, NQ>.
#pragma once

#include "vg_scan.h"

struct VgWithinQuery {                 // 32 bytes, read through wave-uniform addresses (scalar loads)
    unsigned long long *out;           // [count | cap keys]; the count keeps counting past cap
    unsigned long long cap;
    float r;                           // rows with d <= r and d finite match
    uint32_t pad[3];
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

template <int VT, int ACC, int U, int NQ, bool NT>          // VT: T_F32 / T_U8 / T_I8
__global__ __launch_bounds__(VG_BLOCK) void vg_scan_multi_within_kernel(ScanArgs a) {
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
    uint4 cur[U], nxt[U];
    vg_load_batch<U, NT>(cur, a.rows, b * rpb + rib, (b < nbatch) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
    while (b < nbatch) {
        const long long bn = b + wstride;
        vg_load_batch<U, NT>(nxt, a.rows, bn * rpb + rib, (bn < nbatch) ? a.n_rows : 0, a.stride, sub, lpr, a.nch);
        const long long row = b * rpb + rib;
        const bool owner = (sub == 0) && (row < a.n_rows);
        // every query's distance first, one ballot each; the rare batch with a match parks its keys BEHIND the arithmetic, where the
        // current row chunks are dead - the queue / flush temporaries then do not add to the loop's peak register pressure
        float d[NQ];
        unsigned long long any = 0ull;
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            Accum<VT, ACC> acc;
            acc.init();
#pragma unroll
            for (int u = 0; u < U; ++u) acc.chunk(q[n][u], cur[u]);
            d[n] = vg_clamp(acc.finish(qstat[n], lpr_log2, a.root));
            // d <= r is false for NaN; +Inf never matches, whatever the radius (the single range scan's rule)
            any |= __ballot(owner && (d[n] <= r[n]) && (d[n] < INFINITY));
        }
        if (any != 0ull) {
            // (the lane index goes through an opaque move: queue and store addresses derived from it are then worked out HERE, in the
            //  rare path, instead of being hoisted out of the loop into vector registers that stay live across the arithmetic)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // (region and capacity are read from the descriptors here, by scalar loads, rather than held in 4 scalar registers per query
            //  across the loop: with them the NQ = 4 instances ran out of scalar registers)
            const VgWithinQuery *w = wq;
            asm volatile("" : "+s"(w));
#pragma unroll
            for (int n = 0; n < NQ; ++n)
                vg_mw_offer(vg_make_key(d[n], (uint32_t)row), owner && (d[n] <= r[n]) && (d[n] < INFINITY), queue[n], queued[n], w[n].out, w[n].cap, ln);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        b = bn;
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n)
        if (queued[n] > 0) vg_mw_flush(queue[n], queued[n], wq[n].out, wq[n].cap, lane);
}
