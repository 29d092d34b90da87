// vg_batch_bits_within.hip - batch RANGE scans over PACKED BIT VECTORS (uint8 rows, VG_DIST_HAMMING / VG_DIST_JACCARD) on the integer
// matrix cores: every row within a radius, for many queries with a radius each.  The range form of vg_batch_bits.hip (rows of up to 128
// bytes): with i = popcount(q AND x) from the matrix product of the rows spread to 0 / 1 bytes,
//     Hamming = |q| + |x| - 2 i            Jaccard = (u - i) / u,  u = |q| + |x| - i,  0 when u == 0
// is the single scan's distance bit for bit (vg_accum.h, A_HAM / A_JAC), so a query's answer equals its single range scan's.
//
//   * work split, A operand (queries stationary in registers as 0 / 1 bytes), B operand (the corpus' own packed rows, 8 bytes per
//     thread, spread in registers into two LDS tile buffers in the i8 layout, |x| next to the tile), one ds_read_b128 per MFMA with
//     VGBB_BPIPE reads in flight, the barrier per tile, the NTB ladder: vg_batch_bits.hip's, statement for statement;
//   * what a range scan does NOT have: candidate lists, thresholds that move, a candidate buffer, a pre-pass, stages, a merge.  ONE launch
//     covers all tiles.  LDS holds the two tiles, |x|, and per query |q|, the radius and its region - read ONCE from the query's
//     VgWithinQuery descriptor (vg_scan_multi.h) when the kernel starts;
//   * the gate: a row matches iff d <= r <=> d < thr, thr = the next float above r (vg_batch_bits_defs.h) - the strict test of
//     vg_batch_bits.hip's gates, which serve as they are, computed once and never refreshed.  Hamming's is exact; Jaccard's cannot reject a
//     pair the float test accepts, its survivors are decided by fl((u - i) / u) <= r;
//   * emission (vgbb_within_emit): per accumulator register with a match the keys are compacted by ballot, ONE atomicAdd per (query, tile)
//     reserves their place in the query's region and vector stores write them while they fit; the count keeps counting past the capacity
//     - that is how the host learns the size it needs (vg_multi_within.hip).  Order inside a region is free: the host sorts;
//   * MASKED batches (GATHER; a unit of its own, -DVGBW_TU_GATHER): the tile loop of vg_batch_bits.hip's masked form - a
//     tile is 32 consecutive entries of the mask's position list (ascending scan positions, 0xFFFFFFFF behind the last), the entry fetched
//     two tiles ahead, the row at rows + position * stride one tile ahead.  Rows the mask excludes are never read; a tile's positions sit
//     in LDS next to its bit counts, under the same two-buffer scheme, and make the keys; a padding entry has a distance and never a key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vg_batch_bits_defs.h"
#include "vg_batch_common.h"
#include "vg_batch_units.h"
#include "vg_scan_multi.h"

#define VGBB_WAVES 8
#define VGBB_QPW 32
#define VGBB_QPB (VGBB_WAVES * VGBB_QPW)
#define VGBB_BPIPE 4                    // B-operand register quads in flight

// NTB = k-steps per row (32 bits = 4 packed bytes each): rows up to 4 * NTB bytes, shorter ones zero-padded in the k dimension
// JAC = Jaccard (else Hamming)
// GATHER = the masked form (BatchArgsBitsWithinGather, VGBB_NO_POS: vg_batch_bits_defs.h): tiles are runs of 32 entries of a.pos, not of 32 consecutive rows
template <int NTB, bool JAC, bool GATHER>
__global__ __launch_bounds__(64 * VGBB_WAVES, 1) void vg_batch_bits_within_kernel(std::conditional_t<GATHER, BatchArgsBitsWithinGather, BatchArgsBitsWithin> a) {
    constexpr int THREADS = 64 * VGBB_WAVES;
    constexpr int TILE_BYTES = NTB * 1024;                      // 32 rows x 32 NTB spread bytes
    constexpr int LPR = NTB <= 8 ? 4 : (NTB <= 16 ? 8 : 16);   // lanes that share a row of the packed tile, 8 bytes each
    constexpr int SPREADERS = VGBB_TILE * LPR;                  // threads that load and spread (whole wavefronts: 128 / 256 / 512)
    static_assert(NTB % 4 == 0 && NTB >= 2 * VGBB_BPIPE && NTB <= 32 && LPR * 8 >= NTB * 4, "row ladder");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *tile0 = smem;                                                               // 2 tile buffers
    uint32_t *xcnt_lds = reinterpret_cast<uint32_t *>(smem + 2 * TILE_BYTES);            // [2][32]: |x| of a buffer's rows
    uint32_t *xpos_lds = xcnt_lds + 2 * VGBB_TILE;                                       // GATHER only - [2][32]: the rows' scan positions
    uint32_t *qcnt_lds = xcnt_lds + (GATHER ? 4 : 2) * VGBB_TILE;                        // [waves][32]: |q|
    float *rad_lds = reinterpret_cast<float *>(qcnt_lds + VGBB_QPB);                     // [waves][32]: the radius (-Inf: matches nothing)
    unsigned long long *out_lds = reinterpret_cast<unsigned long long *>(rad_lds + VGBB_QPB);      // [waves][32]: the region [count | cap keys]
    unsigned long long *cap_lds = out_lds + VGBB_QPB;                                    // [waves][32]: its capacity

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = lane & 31, h = lane >> 5;

    const int G = a.nq_pad / VGBB_QPB;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int g = idx % G;
    const int part = (idx / G) * 8 + xcd;
    if (part >= a.npart) return;
    const int q0 = g * VGBB_QPB + wave * VGBB_QPW;

    // ---- A operand: the query's bits [32t + 16h, +16) = half h of its packed dword t, spread; |q| on the way
    vgb_i32x4 areg[NTB];
    uint32_t qc_part = 0;
    {
        const uint8_t *qrow = a.queries + (long long)(q0 + x) * a.stride;
        vgb_static_for<0, NTB / 4>([&](auto gc) {
            constexpr int g4 = decltype(gc)::value;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (16 * g4 < a.stride) v = *reinterpret_cast<const uint4 *>(qrow + 16 * g4);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            vgb_static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const uint32_t half = h ? (w[j] >> 16) : (w[j] & 0xFFFFu);
                qc_part += (uint32_t)__builtin_popcount(half);
                areg[4 * g4 + j] = vgbb_spread16(half);
            });
        });
    }
    uint32_t *qc_w = qcnt_lds + wave * VGBB_QPW;
    float *rad_w = rad_lds + wave * VGBB_QPW;
    unsigned long long *out_w = out_lds + wave * VGBB_QPW, *cap_w = cap_lds + wave * VGBB_QPW;
    {
        const uint32_t qc = qc_part + __shfl_xor(qc_part, 32);
        if (h == 0) {
            const VgWithinQuery d = reinterpret_cast<const VgWithinQuery *>(a.desc)[q0 + x];
            qc_w[x] = qc;
            // a query without capacity is padding; a radius below zero matches nothing either (vgbb_within_thr): both stand as -Inf
            rad_w[x] = (d.cap == 0ull || d.r < 0.0f) ? -INFINITY : d.r;
            out_w[x] = (unsigned long long)(uintptr_t)d.out;
            cap_w[x] = d.cap;
        }
    }
    // chunk columns past the row length are never written by the spreading: they read as 0 bits
    for (int s = tid; s < 2 * TILE_BYTES / 4; s += THREADS) reinterpret_cast<uint32_t *>(tile0)[s] = 0u;
    __syncthreads();

    // ---- the tile's producer side.  Thread (prow, pj) owns packed bytes [8 pj, +8) of row prow of a tile = chunk columns 4 pj .. 4 pj + 3
    const long long ntiles = [&]() __attribute__((always_inline)) -> long long {
        if constexpr (GATHER) return a.n_tiles;                     // tiles of the position list
        else return (a.n_rows + VGBB_TILE - 1) / VGBB_TILE;
    }();
    const long long tile_first = (long long)part * a.tiles_per_part;
    const long long tile_last = min(tile_first + a.tiles_per_part, ntiles);
    const bool spreader = tid < SPREADERS;                          // (wave-uniform)
    const int prow = tid / LPR, pj = tid % LPR;
    const bool pcols = spreader && 8 * pj < (int)a.stride;          // the row has such bytes
    const uint8_t *pbase = a.rows + (long long)prow * a.stride + 8 * pj;
    const unsigned long long tile_stride = (unsigned long long)a.stride * VGBB_TILE;
    uint8_t *pdst = tile0 + (pcols ? (4 * pj) * 512 + prow * 16 : 0);
    auto load_packed = [&](long long tile) __attribute__((always_inline)) -> uint2 {
        uint2 v = make_uint2(0u, 0u);
        if (pcols && tile * VGBB_TILE + prow < a.n_rows) v = *reinterpret_cast<const uint2 *>(pbase + (unsigned long long)tile * tile_stride);
        return v;
    };
    // GATHER: the thread's entry of a tile of the list (the LPR lanes of a row read the same dword; tile < ntiles: inside the list), and the
    // row behind an entry - a padding entry loads nothing and spreads as zeros
    auto load_pos = [&](long long tile) __attribute__((always_inline)) -> uint32_t {
        if constexpr (GATHER) return spreader ? a.pos[tile * VGBB_TILE + prow] : VGBB_NO_POS;
        else return 0u;
    };
    auto load_gathered = [&](uint32_t p) __attribute__((always_inline)) -> uint2 {
        uint2 v = make_uint2(0u, 0u);
        if (pcols && p != VGBB_NO_POS && (long long)p < a.n_rows)
            v = *reinterpret_cast<const uint2 *>(a.rows + (unsigned long long)p * (unsigned long long)a.stride + 8 * pj);
        return v;
    };
    // chunk c (0 .. 3) of the thread's 8 bytes into buffer `buf`
    auto spread_chunk = [&](auto cc, uint2 v, int buf) __attribute__((always_inline)) {
        constexpr int c = decltype(cc)::value;
        const uint32_t w = (c < 2) ? v.x : v.y;
        const vgb_i32x4 o = vgbb_spread16((c & 1) ? (w >> 16) : (w & 0xFFFFu));
        if (pcols) *reinterpret_cast<vgb_i32x4 *>(pdst + buf * TILE_BYTES + c * 512) = o;
    };
    auto store_count = [&](uint2 v, int buf, uint32_t p) __attribute__((always_inline)) {
        if (!spreader) return;
        uint32_t cnt = (uint32_t)__builtin_popcount(v.x) + (uint32_t)__builtin_popcount(v.y);
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) cnt += __shfl_xor(cnt, m);
        if (pj == 0) xcnt_lds[buf * VGBB_TILE + prow] = cnt;
        if constexpr (GATHER) { if (pj == 0) xpos_lds[buf * VGBB_TILE + prow] = p; }
    };

    // ---- the gate.  Register r of lane (x, h) belongs to query qi(r, h) = (r&3) + 8*(r>>2) + 4*h; i = acc[r].  Constants of the launch:
    // a query that matches nothing stands in the Jaccard gate with |q| = 4096 and gt = 0 and never passes
    vgb_i32x16 ng;                      // Hamming: the margin; Jaccard: |q|
    vgb_i32x16 gs;                      // Jaccard: gt
    vgb_static_for<0, 16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int qi = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float thr = vgbb_within_thr(rad_w[qi]);
        ng[r] = JAC ? (thr == -INFINITY ? 4096 : (int)qc_w[qi]) : vgbb_gate_ham(qc_w[qi], thr);
        gs[r] = JAC ? vgbb_gate_jac(thr) : 0;
    });
    auto passes = [&](int i, int ngr, int gsr, int xx) __attribute__((always_inline)) -> bool {
        if constexpr (JAC) { const int S = ngr + xx; return ((uint32_t)(S - 2 * i) << 18) <= __umul24((uint32_t)gsr, (uint32_t)(S - i)); }
        else return 2 * i + ngr - xx >= 0;
    };
    auto judge_any = [&](const vgb_i32x16 &acc, int xx) __attribute__((always_inline)) -> bool {
        if constexpr (JAC) {
            bool p = false;
            vgb_static_for<0, 16>([&](auto rc) { constexpr int r = decltype(rc)::value; p |= passes(acc[r], ng[r], gs[r], xx); });
            return __ballot(p) != 0;
        } else {
            int mm = -0x7FFFFFFF;
            vgb_static_for<0, 16>([&](auto rc) { constexpr int r = decltype(rc)::value; const int m = 2 * acc[r] + ng[r]; mm = mm > m ? mm : m; });
            return __ballot(mm - xx >= 0) != 0;
        }
    };
    // the slow path of a tile: which registers hold a passing pair, then - one copy of the code, looping over the pending registers by
    // run-time index - the exact distance, the exact test against the radius, the keys' way out
    auto judge_slow = [&](const vgb_i32x16 &acc, long long tile, int buf, int xx) __attribute__((always_inline)) {
        const long long row = GATHER ? (long long)xpos_lds[buf * VGBB_TILE + x] : tile * VGBB_TILE + x;
        unsigned pend = 0;
        vgb_static_for<0, 16>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            pend |= __ballot(passes(acc[r], ng[r], gs[r], xx)) ? (1u << r) : 0u;
        });
        while (pend) {
            const int r = __builtin_ctz(pend);
            pend &= pend - 1;
            const int qi = (r & 3) + 8 * (r >> 2) + 4 * h;
            const uint32_t qc = qc_w[qi];
            const uint32_t i = (uint32_t)acc[r];
            float d;
            if (JAC) {
                const uint32_t u = qc + (uint32_t)xx - i;
                d = u ? __fdiv_rn((float)(u - i), (float)u) : 0.0f;
            } else {
                d = (float)(qc + (uint32_t)xx - 2u * i);
            }
            d = vg_clamp(d);
            // (rows at or past n_rows - GATHER: padding entries - spread as zeros: they have a distance, and never a key.  -Inf in rad_w:
            // nothing is <= it)
            const bool pass = (GATHER ? row != (long long)VGBB_NO_POS : row < a.n_rows) && (d <= rad_w[qi]);
            vgbb_within_emit(pass, vg_make_key(d, (uint32_t)row), reinterpret_cast<unsigned long long *>((uintptr_t)out_w[qi]), cap_w[qi], lane);
        }
    };

    // ---- BARRIER PER TILE: the k loop of tile t with, in between its MFMAs, the load of tile t+1's packed bytes (top), their spreading
    // into the other buffer (second half, a chunk every NTB / 8 k-steps) and the rows' bit counts; test; barrier
    constexpr int BP = VGBB_BPIPE;
    vgb_i32x4 bq[BP];
    vgb_i32x16 acc;
    const uint32_t lds_tile0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)tile0;
    uint32_t pos_next = VGBB_NO_POS, pos_next2 = VGBB_NO_POS;          // GATHER: the thread's entries of tiles t + 1 and t + 2 (clamped like tile_next)
    if (tile_first < tile_last) {
        const uint32_t p0 = load_pos(tile_first);
        if constexpr (GATHER) pos_next = load_pos(min(tile_first + 1, tile_last - 1));
        const uint2 v0 = GATHER ? load_gathered(p0) : load_packed(tile_first);
        vgb_static_for<0, 4>([&](auto cc) { spread_chunk(cc, v0, 0); });
        store_count(v0, 0, p0);
    }
    __syncthreads();
    for (long long tile = tile_first; tile < tile_last; ++tile) {
        const int cur_buf = (int)((tile - tile_first) & 1), next_buf = cur_buf ^ 1;
        const long long tile_next = min(tile + 1, tile_last - 1);          // (the last iteration spreads its own tile again)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        const uint32_t baddr = lds_tile0 + (uint32_t)(cur_buf * TILE_BYTES + h * 512 + x * 16);
        uint2 pk = make_uint2(0u, 0u);
        vgb_static_for<0, BP>([&](auto tc) { vgb_lds_read128<1024 * decltype(tc)::value>(bq[decltype(tc)::value], baddr); });
        vgb_static_for<0, NTB>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            constexpr int in_flight_after = (NTB - 1 - t) < (BP - 1) ? (NTB - 1 - t) : (BP - 1);
            vgb_wait_lds<in_flight_after>(bq[t % BP]);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(areg[t], bq[t % BP], acc, 0, 0, 0);
            if constexpr (t + BP < NTB) vgb_lds_read128<1024 * (t + BP)>(bq[t % BP], baddr);
            if constexpr (t == 0) {
                if constexpr (GATHER) { pk = load_gathered(pos_next); pos_next2 = load_pos(min(tile + 2, tile_last - 1)); }
                else pk = load_packed(tile_next);
            }
            constexpr int S0 = NTB / 2, SD = NTB / 8;
            if constexpr (t >= S0 && (t - S0) % SD == 0 && (t - S0) / SD < 4)
                spread_chunk(std::integral_constant<int, (t - S0) / SD>{}, pk, next_buf);
            if constexpr (t == NTB - 1) store_count(pk, next_buf, pos_next);
            __builtin_amdgcn_sched_barrier(0);
        });
        const int xx = (int)xcnt_lds[cur_buf * VGBB_TILE + x];
        // (the judge reads cur_buf's counts and positions; this iteration's producers wrote next_buf's only, and write cur_buf's again
        // only behind the barrier below)
        if (judge_any(acc, xx)) judge_slow(acc, tile, cur_buf, xx);
        if constexpr (GATHER) pos_next = pos_next2;
        __syncthreads();
    }
}

// ---- host side
// the ladder of row lengths (vg_batch_bits.hip's): k-steps the kernels are instantiated for; 0: not served
static int vgbw_ntb(long long stride_bytes) {
    if (stride_bytes < 16 || stride_bytes > 128 || stride_bytes % 16 != 0) return 0;
    const long long ntb = stride_bytes / 4;
    return ntb <= 8 ? 8 : (ntb <= 16 ? 16 : (ntb <= 24 ? 24 : 32));
}

// The kernel instantiations are split over two translation units compiled from this file (build.py): the unmasked kernels and their
// entry points here, the masked form's kernels and entry points with -DVGBW_TU_GATHER.
template <int NTB, bool GATHER, typename Args>
static int launch_within(const Args &a, int jaccard, int blocks, size_t smem, hipStream_t stream) {
    return jaccard ? vgb_launch(vg_batch_bits_within_kernel<NTB, true, GATHER>, blocks, 64 * VGBB_WAVES, smem, stream, a)
                   : vgb_launch(vg_batch_bits_within_kernel<NTB, false, GATHER>, blocks, 64 * VGBB_WAVES, smem, stream, a);
}
template <bool GATHER, typename Args>
static int launch_within_ntb(const Args &a, int jaccard, int blocks, size_t smem, hipStream_t stream) {
    switch (vgbw_ntb(a.stride)) {
    case 8: return launch_within<8, GATHER>(a, jaccard, blocks, smem, stream);
    case 16: return launch_within<16, GATHER>(a, jaccard, blocks, smem, stream);
    case 24: return launch_within<24, GATHER>(a, jaccard, blocks, smem, stream);
    case 32: return launch_within<32, GATHER>(a, jaccard, blocks, smem, stream);
    }
    return -1;
}

#if defined(VGBW_TU_GATHER)
// the masked form's LDS: vg_batch_bits_within_lds_bytes + the two tiles' positions (128-byte rows: 72192)
extern "C" size_t vg_batch_bits_within_masked_lds_bytes(long long stride_bytes) {
    const size_t plain = vg_batch_bits_within_lds_bytes(stride_bytes);
    return plain ? plain + 2 * VGBB_TILE * 4 : 0;
}

// vg_batch_bits_within_launch over the n_pos rows of a position list (dev_pos: n_pos rounded up to 32 entries, vg_batch_bits_pos_launch's):
// tiles and partitions count tiles of the LIST.  The keys carry the rows' real scan positions.
extern "C" int vg_batch_bits_within_masked_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes, const uint32_t *dev_pos, long long n_pos,
                                                  const uint8_t *dev_queries, const void *dev_desc, int nq_pad, int jaccard, int npart, hipStream_t stream) {
    const size_t smem = vg_batch_bits_within_masked_lds_bytes(stride_bytes);
    const long long ntiles = (n_pos + VGBB_TILE - 1) / VGBB_TILE;
    if (!smem || nq_pad < VGBB_QPB || nq_pad % VGBB_QPB != 0 || npart < 1 || npart > ntiles || n_pos < 1 || n_pos > n_rows || !dev_pos) return -1;
    BatchArgsBitsWithinGather a;
    a.rows = dev_rows; a.queries = dev_queries; a.desc = dev_desc; a.pos = dev_pos;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.npart = npart; a.n_tiles = ntiles;
    a.tiles_per_part = (int)((ntiles + npart - 1) / npart);
    const int G = nq_pad / VGBB_QPB;
    return launch_within_ntb<true>(a, jaccard, G * ((npart + 7) / 8) * 8, smem, stream);
}
#else
// LDS bytes of one workgroup: two spread tiles, their rows' bit counts, per query |q|, radius, region, capacity
// (128-byte rows: 65536 + 256 + 1024 + 1024 + 2048 + 2048 = 71936).  0: rows it does not serve
extern "C" size_t vg_batch_bits_within_lds_bytes(long long stride_bytes) {
    const int NTB = vgbw_ntb(stride_bytes);
    if (!NTB) return 0;
    const size_t bytes = (size_t)2 * NTB * 1024 + 2 * VGBB_TILE * 4 + VGBB_QPB * 4 + VGBB_QPB * 4 + (size_t)VGBB_QPB * 8 * 2;
    return bytes <= VGBB_LDS_LIMIT ? bytes : 0;
}

// dev_rows: the corpus' row-major rows; dev_queries: nq_pad x stride packed bytes; dev_desc: nq_pad VgWithinQuery.  One launch over all
// rows.  Returns 0, -1 if the shape is not served, a hipError_t otherwise.
extern "C" int vg_batch_bits_within_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes,
                                           const uint8_t *dev_queries, const void *dev_desc, int nq_pad, int jaccard, int npart, hipStream_t stream) {
    const size_t smem = vg_batch_bits_within_lds_bytes(stride_bytes);
    if (!smem || nq_pad < VGBB_QPB || nq_pad % VGBB_QPB != 0 || npart < 1 || n_rows < 1) return -1;
    const long long ntiles = (n_rows + VGBB_TILE - 1) / VGBB_TILE;
    BatchArgsBitsWithin a;
    a.rows = dev_rows; a.queries = dev_queries; a.desc = dev_desc;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.npart = npart;
    a.tiles_per_part = (int)((ntiles + npart - 1) / npart);
    const int G = nq_pad / VGBB_QPB;
    return launch_within_ntb<false>(a, jaccard, G * ((npart + 7) / 8) * 8, smem, stream);
}
#endif
