// vg_batch_bitsl.hip - the LONG-ROW form of vg_batch_bits.hip: batched Hamming / Jaccard queries over packed bit vectors of 129 .. 512
// bytes (uint8 rows, stride 144 .. 512) on the integer matrix cores.  The identity, the exactness rule, the spreading of bits to 0 / 1
// bytes, the i8 tile layout, the gates and the slow path are that file's; what is new is the work split (3.26):
//
//   * a wavefront cannot hold 32 whole queries of more than 128 bytes (32 k-steps = 128 VGPRs), so the K dimension is split over the
//     wavefronts of a workgroup: 8 wavefronts = QG query groups x KS K-slices.  KS = 2: rows up to 256 bytes, 4 x 32 = 128 queries per
//     workgroup; KS = 4: rows up to 512 bytes, 2 x 32 = 64 queries.  Wavefront (qg, ks) keeps k-steps [ks NTBW, +NTBW) of its 32 queries
//     in registers (NTBW = 24 or 32) and runs the k loop over that slice of the tile: chunk columns 2 ks NTBW ... of the same layout;
//   * the partial accumulators are integers: the wavefronts ks > 0 hand their 16 registers through LDS to the lead (ks = 0) of their
//     query group, which adds them - exact in any order -, runs the gate and the slow path and owns the 32 lists.  The exchange lies in
//     the tile buffer just consumed (its first 16 / 24 KiB: chunk columns every row has, rewritten by the next spreading);
//   * every one of the 512 threads loads and spreads: thread (prow, pj) owns packed bytes [8 (pj + 16 u), +8) of row prow, u < UPT
//     (one global_load_dwordx2 each).  16 consecutive lanes hold 16 consecutive rows of one chunk column - a ds_write_b128 of a quarter
//     wavefront is 256 contiguous bytes - and 4 lanes x 16 rows share a load instruction (32 contiguous bytes per row).  |x| of a row
//     is summed over the lanes 16 and 32 apart; the four quarter sums per row (pj / 4) lie in LDS and the lead adds them;
//   * KS = 2 has two tile buffers (2 x 48 / 64 KiB): the next tile is spread between the MFMAs of the current one, as in the short form.
//     KS = 4 has ONE (96 / 128 KiB of the 160): the next tile's packed bytes are loaded at the top of the k loop, kept in registers (6 /
//     8 VGPRs) and spread after the exchange.  Barriers per tile: after the k loop, after the partials are written, after they are
//     read (the buffer is free again); the one-buffer form has a fourth behind its spreading;
//   * MASKED batches (GATHER): the tile loop runs over VIRTUAL tiles - 32 consecutive entries of the mask's position list
//     (vg_batch_bits.hip builds it).  Thread (prow, pj) fetches entry prow of the tile TWO ahead into a register and, one tile ahead, its
//     units of the row at rows + position * stride: 16 lanes read 128 contiguous bytes of one row.  A tile's positions lie in LDS next
//     to its bit counts; the lead takes both into registers before the tile's third barrier - past it the other wavefronts already
//     write the next tile's - and makes the keys from them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "vg_batch_bits_defs.h"
#include "vg_batch_common.h"
#include "vg_batch_units.h"

#define VGBL_WAVES 8
#define VGBL_BPIPE 4                    // B-operand register quads in flight

// KS = K-slices (wavefronts that share 32 queries), NTBW = k-steps (32 bits each) per slice: rows up to 4 KS NTBW bytes, shorter ones
// zero-padded in the k dimension; JAC = Jaccard (else Hamming); PRE = the pre-pass variant: only the smallest distance of a query in a
// tile enters; GATHER = the masked form: tiles are runs of 32 entries of a.pos, not of 32 consecutive rows
template <int KS, int NTBW, bool JAC, bool PRE, bool GATHER>
__global__ __launch_bounds__(64 * VGBL_WAVES, 1) void vg_batch_bitsl_kernel(std::conditional_t<GATHER, BatchArgsBitsGather, BatchArgsBits> a) {
    constexpr int THREADS = 64 * VGBL_WAVES;
    constexpr int QG = VGBL_WAVES / KS, QPB = QG * 32;
    constexpr int NTB = KS * NTBW;                              // k-steps of a whole row
    constexpr int TILE_BYTES = NTB * 1024;                      // 32 rows x 32 NTB spread bytes
    constexpr int NBUF = KS == 2 ? 2 : 1;                       // tile buffers
    constexpr int UPT = (NTB + 31) / 32;                        // 8-byte units a thread loads and spreads per tile
    constexpr int NCH = 4 * UPT;                                // ... = 16-byte chunks it writes
    static_assert((KS == 2 || KS == 4) && NTBW % 4 == 0 && NTBW >= 2 * VGBL_BPIPE && NTBW <= 32, "row ladder");
    static_assert((VGBL_WAVES - QG) * 4096 <= 144 / 2 * 512, "the exchange stays inside chunk columns every served row has");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *tile0 = smem;                                                               // NBUF tile buffers
    uint32_t *xcnt_lds = reinterpret_cast<uint32_t *>(smem + NBUF * TILE_BYTES);         // [NBUF][32][4]: |x| of a buffer's rows, by quarter
    uint32_t *xpos_lds = xcnt_lds + NBUF * VGBB_TILE * 4;                                // GATHER only - [NBUF][32]: the rows' scan positions
    uint32_t *qpart_lds = xpos_lds + (GATHER ? NBUF * VGBB_TILE : 0);                    // [waves][32]: |q| of a wavefront's slice
    uint32_t *qcnt_lds = qpart_lds + VGBL_WAVES * 32;                                    // [QG][32]: |q|
    float *thr_lds = reinterpret_cast<float *>(qcnt_lds + QPB);                          // [QG][32]: current k-th best distance
    uint64_t *lists = reinterpret_cast<uint64_t *>(thr_lds + QPB);                       // [QG][32][k]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qg = wave % QG, ks = wave / QG;                   // (the leads, ks == 0, are wavefronts 0 .. QG - 1: one per SIMD)
    const bool lead = ks == 0;
    const int x = lane & 31, h = lane >> 5;
    const int k = a.k;

    const int G = a.nq_pad / QPB;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int g = idx % G;
    const int part = (idx / G) * 8 + xcd;
    if (part >= a.npart) return;
    const int q0 = g * QPB + qg * 32;

    // ---- A operand: bits [32t + 16h, +16) of the slice = half h of packed dword ks NTBW + t of the query, spread; the slice's bits on the way
    vgb_i32x4 areg[NTBW];
    uint32_t qc_part = 0;
    {
        const uint8_t *qrow = a.queries + (long long)(q0 + x) * a.stride + ks * NTBW * 4;
        vgb_static_for<0, NTBW / 4>([&](auto gc) {
            constexpr int g4 = decltype(gc)::value;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (ks * NTBW * 4 + 16 * g4 < a.stride) v = *reinterpret_cast<const uint4 *>(qrow + 16 * g4);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            vgb_static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const uint32_t half = h ? (w[j] >> 16) : (w[j] & 0xFFFFu);
                qc_part += (uint32_t)__builtin_popcount(half);
                areg[4 * g4 + j] = vgbb_spread16(half);
            });
        });
    }
    uint32_t *qc_w = qcnt_lds + qg * 32;
    float *thr_w = thr_lds + qg * 32;
    uint64_t *wave_lists = lists + (size_t)qg * 32 * k;
    qc_part += __shfl_xor(qc_part, 32);
    if (h == 0) qpart_lds[wave * 32 + x] = qc_part;
    // chunk columns past the row length are never written by the spreading (and meet zero bytes of A)
    for (int s = tid; s < NBUF * TILE_BYTES / 4; s += THREADS) reinterpret_cast<uint32_t *>(tile0)[s] = 0u;
    __syncthreads();
    if (lead) {
        if (h == 0) {
            uint32_t qc = 0;
#pragma unroll
            for (int s = 0; s < KS; ++s) qc += qpart_lds[(s * QG + qg) * 32 + x];
            qc_w[x] = qc;
            // the pre-pass bound is the distance of an actual row, which the first real stage meets again: one ulp up, so that the
            // strict comparison of the slow path lets a row AT the bound in; padding queries never accept
            float t = a.init_keys ? nextafterf(vgb_kth_distance(a.init_keys[(long long)(q0 + x) * 64 + (k - 1)]), INFINITY) : INFINITY;
            if (q0 + x >= a.nq_real) t = -INFINITY;
            thr_w[x] = t;
        }
        const bool seeded = a.seed != 0 && part == 0;               // (keys of rows no later stage meets again)
        for (int s = lane; s < 32 * k; s += 64)
            wave_lists[s] = seeded ? a.init_keys[(long long)(q0 + s / k) * 64 + s % k] : VG_EMPTY_KEY;
    }
    __syncthreads();

    // ---- the tile's producer side.  Thread (prow, pj), unit u: packed bytes [8 (pj + 16 u), +8) of row prow = chunk columns 4 (pj + 16 u) ..
    const long long tile_first = a.tile_begin + (long long)part * a.tiles_per_part;
    const long long tile_last = min(tile_first + a.tiles_per_part, a.tile_end);
    const int prow = (wave & 1) * 16 + (lane & 15), pj = (wave >> 1) * 4 + (lane >> 4);
    const uint8_t *pbase = a.rows + (long long)prow * a.stride + 8 * pj;
    const unsigned long long tile_stride = (unsigned long long)a.stride * VGBB_TILE;
    uint8_t *pdst = tile0 + (4 * pj) * 512 + prow * 16;
    uint2 pk[UPT];
    auto load_packed = [&](long long tile) __attribute__((always_inline)) {
        const bool row_in = tile * VGBB_TILE + prow < a.n_rows;
        vgb_static_for<0, UPT>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            pk[u] = make_uint2(0u, 0u);
            if (row_in && 8 * (pj + 16 * u) < (int)a.stride)
                pk[u] = *reinterpret_cast<const uint2 *>(pbase + (unsigned long long)tile * tile_stride + 128 * u);
        });
    };
    // GATHER: the thread's entry of a virtual tile (16 consecutive lanes read 16 consecutive dwords; the 16 threads of a row the same
    // one), and the row behind an entry - a padding entry loads nothing and spreads zeros
    auto load_pos = [&](long long tile) __attribute__((always_inline)) -> uint32_t {
        if constexpr (GATHER) return a.pos[tile * VGBB_TILE + prow];
        else return 0u;
    };
    auto load_gathered = [&](uint32_t p) __attribute__((always_inline)) {
        const uint8_t *src = a.rows + (unsigned long long)p * (unsigned long long)a.stride + 8 * pj;
        vgb_static_for<0, UPT>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            pk[u] = make_uint2(0u, 0u);
            if (p != VGBB_NO_POS && 8 * (pj + 16 * u) < (int)a.stride) pk[u] = *reinterpret_cast<const uint2 *>(src + 128 * u);
        });
    };
    // chunk ci (0 .. NCH - 1: unit ci / 4, its 16 bits ci % 4) into buffer `buf`
    auto spread_chunk = [&](auto cc, int buf) __attribute__((always_inline)) {
        constexpr int u = decltype(cc)::value / 4, c = decltype(cc)::value % 4;
        const uint32_t w = (c < 2) ? pk[u].x : pk[u].y;
        const vgb_i32x4 o = vgbb_spread16((c & 1) ? (w >> 16) : (w & 0xFFFFu));
        if (8 * (pj + 16 * u) < (int)a.stride) *reinterpret_cast<vgb_i32x4 *>(pdst + buf * TILE_BYTES + (64 * u + c) * 512) = o;
    };
    auto store_count = [&](int buf, uint32_t p) __attribute__((always_inline)) {
        uint32_t cnt = 0;
        vgb_static_for<0, UPT>([&](auto uc) { constexpr int u = decltype(uc)::value; cnt += (uint32_t)__builtin_popcount(pk[u].x) + (uint32_t)__builtin_popcount(pk[u].y); });
        cnt += __shfl_xor(cnt, 16);
        cnt += __shfl_xor(cnt, 32);
        if (lane < 16) xcnt_lds[(buf * VGBB_TILE + prow) * 4 + (wave >> 1)] = cnt;
        if constexpr (GATHER) { if (pj == 0) xpos_lds[buf * VGBB_TILE + prow] = p; }
    };

    // ---- the gate (vg_batch_bits.hip's; the lead's).  Register r of lane (x, h) belongs to query qi(r, h) = (r&3) + 8*(r>>2) + 4*h; i = acc[r].
    //   Hamming  d = |q| + |x| - 2 i < thr  <=>  2 i + ng - |x| >= 0,  ng = ceil(thr) - 1 - |q|: integers, exact (d <= 8192)
    //   Jaccard  (S - 2 i) 2^18 <= gt (S - i),  S = |q| + |x| <= 8192,  gt = ceil(thr 2^18) <= 2^19: a real pair has S - i = u <= 4096, so
    //            the product stays below 2^32 and the shifted side below 2^31; implied by fl((u - i) / u) < thr.  A
    //            padding query (all zero: i = 0) stands in the gate with |q| = 4096 and gt = 0: S 2^18 <= 0 never holds, S 2^18 <= 2^31
    // The exact test - (float) distance < thr, the single scan's arithmetic - is the slow path's.
    vgb_i32x16 ng;                      // Hamming: the margin; Jaccard: |q|
    vgb_i32x16 gs;                      // Jaccard: gt
    auto gate_ham = [](uint32_t qc, float thr) __attribute__((always_inline)) -> int {
        if (thr == -INFINITY) return -(1 << 30);               // padding
        if (!(thr < 1.0e9f)) return 1 << 30;                   // list not full: everything passes
        return (int)ceilf(thr) - 1 - (int)qc;
    };
    auto gate_jac = [](float thr) __attribute__((always_inline)) -> int {
        if (thr == -INFINITY) return 0;                        // padding
        if (!(thr < 2.0f)) return 1 << 19;                     // list not full (a <= b always): everything passes
        return (int)ceilf(thr * 262144.0f);                    // (a power of two: exact, also for the denormal start threshold above 0)
    };
    if (lead)
        vgb_static_for<0, 16>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            const int qi = (r & 3) + 8 * (r >> 2) + 4 * h;
            ng[r] = JAC ? (thr_w[qi] == -INFINITY ? 4096 : (int)qc_w[qi]) : gate_ham(qc_w[qi], thr_w[qi]);
            gs[r] = JAC ? gate_jac(thr_w[qi]) : 0;
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
    // run-time index - the exact distance, the list inserts, the refreshed gate
    // (GATHER: the row's scan position xp comes in a register, like xx - the lead fetched both before the tile's third barrier, behind
    // which the other wavefronts write the next tile's counts and positions)
    auto judge_slow = [&](const vgb_i32x16 &acc, long long tile, int xx, uint32_t xp) __attribute__((always_inline)) {
        const long long row = GATHER ? (long long)xp : tile * VGBB_TILE + x;
        unsigned pend = 0;
        vgb_static_for<0, 16>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            pend |= __ballot(passes(acc[r], ng[r], gs[r], xx)) ? (1u << r) : 0u;
        });
        while (pend) {
            const int r = __builtin_ctz(pend);
            pend &= pend - 1;
            const int q_lo = (r & 3) + 8 * (r >> 2), qi = q_lo + 4 * h;
            const uint32_t qc = qc_w[qi];
            float thr_l = thr_w[qi];
            const uint32_t i = (uint32_t)acc[r];
            float d;
            if (JAC) {
                const uint32_t u = qc + (uint32_t)xx - i;
                d = u ? __fdiv_rn((float)(u - i), (float)u) : 0.0f;
            } else {
                d = (float)(qc + (uint32_t)xx - 2u * i);
            }
            d = vg_clamp(d);
            // strict: rows arrive in scan order, a row that only ties the k-th best has the larger position and loses
            const bool pass = (GATHER ? xp != VGBB_NO_POS : row < a.n_rows) && (d < thr_l);
            unsigned long long m = __ballot(pass);
            if (!m) continue;
            if constexpr (PRE) {
                uint64_t kmin = pass ? vg_make_key(d, (uint32_t)row) : VG_EMPTY_KEY;     // min over the 32 rows of each query
                kmin = vgb_min64(kmin, vgb_dpp64<VG_DPP_QUAD_PERM(1, 0, 3, 2)>(kmin));
                kmin = vgb_min64(kmin, vgb_dpp64<VG_DPP_QUAD_PERM(2, 3, 0, 1)>(kmin));
                kmin = vgb_min64(kmin, vgb_dpp64<VG_DPP_ROW_HALF_MIRROR>(kmin));
                kmin = vgb_min64(kmin, vgb_dpp64<VG_DPP_ROW_MIRROR>(kmin));
                kmin = vgb_min64(kmin, (uint64_t)__shfl_xor((unsigned long long)kmin, 16));
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const uint64_t c = vg_readlane64(kmin, 32 * hh);
                    if (c == VG_EMPTY_KEY) continue;
                    const float nt = vgb_kth_distance(vgb_list_insert(wave_lists + (q_lo + 4 * hh) * k, k, lane, c));
                    if (h == hh) thr_l = fminf(nt, thr_l);
                }
            } else {
                const uint64_t key = vg_make_key(d, (uint32_t)row);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int hh = src >> 5;
                    const uint64_t c = vg_readlane64(key, src);
                    const float nt = vgb_kth_distance(vgb_list_insert(wave_lists + (q_lo + 4 * hh) * k, k, lane, c));
                    if (h == hh) thr_l = fminf(nt, thr_l);
                }
            }
            if (x == 0) thr_w[qi] = thr_l;                                  // (the 32 lanes of a half hold the same value)
            if (JAC) gs[r] = gate_jac(thr_l);
            else ng[r] = gate_ham(qc, thr_l);
        }
    };

    // ---- per tile: the k loop over the wavefront's slice, with the load of tile t+1's packed bytes at its top and - two buffers - their
    // spreading into the other buffer between its later MFMAs; barrier; the partial sums to the lead; barrier; the lead adds them and
    // fetches |x|; barrier; the lead's test, next to - one buffer - everybody's spreading of tile t+1 and a last barrier
    constexpr int BP = VGBL_BPIPE;
    constexpr int SD = (3 * NTBW / 4) / NCH > 0 ? (3 * NTBW / 4) / NCH : 1, S0 = NTBW - NCH * SD;   // two buffers: chunk j behind k-step S0 + j SD
    static_assert(NBUF == 1 || S0 >= 1, "the spreading fits behind the load in the k loop");
    vgb_i32x4 bq[BP];
    vgb_i32x16 acc;
    const uint32_t lds_tile0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)tile0;
    uint32_t pos_next = VGBB_NO_POS, pos_next2 = VGBB_NO_POS;          // GATHER: the thread's entries of tiles t + 1 and t + 2 (clamped like tile_next)
    if (tile_first < tile_last) {
        const uint32_t p0 = load_pos(tile_first);
        if constexpr (GATHER) { pos_next = load_pos(min(tile_first + 1, tile_last - 1)); load_gathered(p0); }
        else load_packed(tile_first);
        vgb_static_for<0, NCH>([&](auto cc) { spread_chunk(cc, 0); });
        store_count(0, p0);
    }
    __syncthreads();
    for (long long tile = tile_first; tile < tile_last; ++tile) {
        const int cur_buf = NBUF == 2 ? (int)((tile - tile_first) & 1) : 0, next_buf = NBUF == 2 ? cur_buf ^ 1 : 0;
        const long long tile_next = min(tile + 1, tile_last - 1);          // (the last iteration spreads its own tile again)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0;
        const uint32_t baddr = lds_tile0 + (uint32_t)(cur_buf * TILE_BYTES + ks * (NTBW * 1024) + h * 512 + x * 16);
        vgb_static_for<0, BP>([&](auto tc) { vgb_lds_read128<1024 * decltype(tc)::value>(bq[decltype(tc)::value], baddr); });
        vgb_static_for<0, NTBW>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            constexpr int in_flight_after = (NTBW - 1 - t) < (BP - 1) ? (NTBW - 1 - t) : (BP - 1);
            vgb_wait_lds<in_flight_after>(bq[t % BP]);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(areg[t], bq[t % BP], acc, 0, 0, 0);
            if constexpr (t + BP < NTBW) vgb_lds_read128<1024 * (t + BP)>(bq[t % BP], baddr);
            if constexpr (t == 0) {
                if constexpr (GATHER) { load_gathered(pos_next); pos_next2 = load_pos(min(tile + 2, tile_last - 1)); }
                else load_packed(tile_next);
            }
            if constexpr (NBUF == 2 && t >= S0 && (t - S0) % SD == 0 && (t - S0) / SD < NCH)
                spread_chunk(std::integral_constant<int, (t - S0) / SD>{}, next_buf);
            if constexpr (NBUF == 2 && t == NTBW - 1) store_count(next_buf, pos_next);
            __builtin_amdgcn_sched_barrier(0);
        });
        __syncthreads();                                                    // the tile is consumed (two buffers: and the next one complete)
        vgb_i32x4 *xchg = reinterpret_cast<vgb_i32x4 *>(tile0 + cur_buf * TILE_BYTES) + qg * (KS - 1) * 256 + lane;
        if (!lead)
            vgb_static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                vgb_i32x4 v;
                v[0] = acc[4 * j]; v[1] = acc[4 * j + 1]; v[2] = acc[4 * j + 2]; v[3] = acc[4 * j + 3];
                xchg[(ks - 1) * 256 + j * 64] = v;
            });
        __syncthreads();
        int xx = 0;
        uint32_t xp = VGBB_NO_POS;
        if (lead) {
            vgb_static_for<0, 4 * (KS - 1)>([&](auto jc) {
                constexpr int s = decltype(jc)::value / 4, j = decltype(jc)::value % 4;
                const vgb_i32x4 v = xchg[s * 256 + j * 64];
                acc[4 * j] += v[0]; acc[4 * j + 1] += v[1]; acc[4 * j + 2] += v[2]; acc[4 * j + 3] += v[3];
            });
            const uint4 xc = reinterpret_cast<const uint4 *>(xcnt_lds)[cur_buf * VGBB_TILE + x];
            xx = (int)(xc.x + xc.y + xc.z + xc.w);
            if constexpr (GATHER) xp = xpos_lds[cur_buf * VGBB_TILE + x];
        }
        __syncthreads();                                                    // the exchange is read: the buffer may be spread into again
        if (lead && judge_any(acc, xx)) judge_slow(acc, tile, xx, xp);
        if constexpr (NBUF == 1) {
            vgb_static_for<0, NCH>([&](auto cc) { spread_chunk(cc, 0); });
            store_count(0, pos_next);
            __syncthreads();
        }
        if constexpr (GATHER) pos_next = pos_next2;
    }

    if (lead)
        for (int s = lane; s < 32 * 64; s += 64) {
            const int qi = s >> 6, slot = s & 63;
            a.cand[((long long)(q0 + qi) * a.npart_total + a.part_base + part) * 64 + slot] = (slot < k) ? wave_lists[qi * k + slot] : VG_EMPTY_KEY;
        }
}

// ---- host side
// Four translation units are compiled from this file (build.py): the real-pass kernels and the entry points here, the PRE kernels with
// -DVGBL_TU_PRE; the masked form's real-pass kernels and its entry points with -DVGBL_TU_GATHER, its PRE kernels with -DVGBL_TU_GATHER_PRE.
// the ladder of row lengths: rows of up to 192 / 256 bytes run as KS = 2 with 24 / 32 k-steps per slice, up to 384 / 512 as KS = 4;
// 64 KS + NTBW, 0: not served
static int vgbl_step(long long stride_bytes) {
    if (stride_bytes <= 128 || stride_bytes > 512 || stride_bytes % 16 != 0) return 0;
    return stride_bytes <= 192 ? 2 * 64 + 24 : (stride_bytes <= 256 ? 2 * 64 + 32 : (stride_bytes <= 384 ? 4 * 64 + 24 : 4 * 64 + 32));
}

template <int KS, int NTBW, bool JAC, bool PRE, bool GATHER, typename Args>
static int launch_bitsl(const Args &a, int blocks, size_t smem, hipStream_t stream) {
    return vgb_launch(vg_batch_bitsl_kernel<KS, NTBW, JAC, PRE, GATHER>, blocks, 64 * VGBL_WAVES, smem, stream, a);
}
template <bool PRE, bool GATHER, typename Args>
static int launch_bitsl_step(const Args &a, int step, int jaccard, int blocks, size_t smem, hipStream_t stream) {
    switch (step) {
    case 2 * 64 + 24: return jaccard ? launch_bitsl<2, 24, true, PRE, GATHER>(a, blocks, smem, stream) : launch_bitsl<2, 24, false, PRE, GATHER>(a, blocks, smem, stream);
    case 2 * 64 + 32: return jaccard ? launch_bitsl<2, 32, true, PRE, GATHER>(a, blocks, smem, stream) : launch_bitsl<2, 32, false, PRE, GATHER>(a, blocks, smem, stream);
    case 4 * 64 + 24: return jaccard ? launch_bitsl<4, 24, true, PRE, GATHER>(a, blocks, smem, stream) : launch_bitsl<4, 24, false, PRE, GATHER>(a, blocks, smem, stream);
    case 4 * 64 + 32: return jaccard ? launch_bitsl<4, 32, true, PRE, GATHER>(a, blocks, smem, stream) : launch_bitsl<4, 32, false, PRE, GATHER>(a, blocks, smem, stream);
    }
    return -1;
}
#if defined(VGBL_TU_PRE)
extern "C" int vgbl_launch_pre(const BatchArgsBits *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bitsl_step<true, false>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}
#elif defined(VGBL_TU_GATHER_PRE)
extern "C" int vgbl_launch_gather_pre(const BatchArgsBitsGather *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bitsl_step<true, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}
#elif defined(VGBL_TU_GATHER)
extern "C" int vgbl_launch_gather_real(const BatchArgsBitsGather *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bitsl_step<false, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}

// the masked form's LDS: vg_batch_bitsl_lds_bytes + the positions of each tile buffer's rows (NBUF x 128 bytes)
//   <= 192 bytes  134 400 at k = 32
//   <= 256       131 072 + 3 328 + 1024 k = 163 072 at k = 28: k = 29 .. 32 are handed on (the unmasked form fills the LDS exactly at 29)
//   <= 384       116 864 at k = 32
//   <= 512       149 632 at k = 32
extern "C" size_t vg_batch_bitsl_masked_lds_bytes(long long stride_bytes, int k) {
    const size_t plain = vg_batch_bitsl_lds_bytes(stride_bytes, k);
    if (!plain) return 0;
    const size_t bytes = plain + ((vgbl_step(stride_bytes) >> 6) == 2 ? 2 : 1) * VGBB_TILE * 4;
    return bytes <= VGBB_LDS_LIMIT ? bytes : 0;
}

// vg_batch_bits_masked_launch's arguments and answers (vg_batch_bits.hip hands rows beyond 128 bytes on to here): tiles, partitions,
// the pre-pass and the stages count VIRTUAL tiles of the position list; the keys carry the rows' real scan positions
extern "C" int vg_batch_bitsl_masked_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes, const uint32_t *dev_pos, long long n_pos,
                                            const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int jaccard,
                                            uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, hipStream_t stream) {
    const size_t smem = vg_batch_bitsl_masked_lds_bytes(stride_bytes, k);
    const int QPB = vg_batch_bitsl_queries_per_block(stride_bytes);
    const long long ntiles = (n_pos + VGBB_TILE - 1) / VGBB_TILE;
    if (!smem || nq_pad < QPB || nq_pad % QPB != 0 || npart < 1 || npart > VG_SEL_MAX_HEADS || npart > ntiles || n_pos < 1 || n_pos > n_rows) return -1;
    BatchArgsBitsGather a;
    a.rows = dev_rows; a.queries = dev_queries; a.cand = dev_cand; a.pos = dev_pos;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.nq_real = nq_real; a.npart = npart; a.k = k;
    const int variant = vgbl_step(stride_bytes) * 2 + (jaccard ? 1 : 0);
    const int G = nq_pad / QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    long long pre = 0;
    {
        const int denom = vg_sw(SW_VG_BATCH_PREPASS, VGB_PREPASS_DENOM_DEFAULT);
        if (denom > 0 && ntiles >= 65536) pre = ((ntiles / denom + npart - 1) / npart) * npart;
    }
    return vgb_run_staged(a, ntiles, pre, 400, dev_out_keys, stream,
                          [&](const BatchArgsBitsGather &b) { return vgbl_launch_gather_pre(&b, variant, blocks, smem, stream); },
                          [&](const BatchArgsBitsGather &b) { return vgbl_launch_gather_real(&b, variant, blocks, smem, stream); });
}
#else
extern "C" int vgbl_launch_real(const BatchArgsBits *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bitsl_step<false, false>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}

extern "C" int vg_batch_bitsl_queries_per_block(long long stride_bytes) {
    const int step = vgbl_step(stride_bytes);
    return step ? 32 * VGBL_WAVES / (step >> 6) : 0;
}

// LDS bytes of one workgroup: the tile buffers (two of KS = 2, one of KS = 4), their rows' bit counts by quarter, the slices' and the
// queries' bit counts, the thresholds, the lists; 0: rows / k it does not serve - lists that do not fit beside the tiles included
//   <= 192 bytes  98 304 + 1024 + 1024 + 1024 + 1024 k   = 134 144 at k = 32
//   <= 256       131 072 + 1024 + 1024 + 1024 + 1024 k   = 154 624 at k = 20, 163 840 at k = 29: k = 30 .. 32 are handed on
//   <= 384        98 304 +  512 + 1024 +  512 +  512 k   = 116 736 at k = 32
//   <= 512       131 072 +  512 + 1024 +  512 +  512 k   = 149 504 at k = 32
extern "C" size_t vg_batch_bitsl_lds_bytes(long long stride_bytes, int k) {
    const int step = vgbl_step(stride_bytes);
    if (!step || k < 1 || k > VGBB_MAX_K) return 0;
    const int KS = step >> 6, NTBW = step & 63, NBUF = KS == 2 ? 2 : 1, QPB = 32 * VGBL_WAVES / KS;
    const size_t bytes = (size_t)NBUF * KS * NTBW * 1024 + NBUF * VGBB_TILE * 16 + VGBL_WAVES * 32 * 4 + QPB * 4 + QPB * 4 + (size_t)QPB * k * 8;
    return bytes <= VGBB_LDS_LIMIT ? bytes : 0;
}

// vg_batch_bits_launch's arguments and answers (vg_batch_bits.hip hands rows beyond 128 bytes on to here)
extern "C" int vg_batch_bitsl_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes,
                                     const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int jaccard,
                                     uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, hipStream_t stream) {
    const size_t smem = vg_batch_bitsl_lds_bytes(stride_bytes, k);
    const int QPB = vg_batch_bitsl_queries_per_block(stride_bytes);
    if (!smem || nq_pad < QPB || nq_pad % QPB != 0 || npart < 1 || npart > VG_SEL_MAX_HEADS || n_rows < 1) return -1;
    BatchArgsBits a;
    a.rows = dev_rows; a.queries = dev_queries; a.cand = dev_cand;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.nq_real = nq_real; a.npart = npart; a.k = k;
    const int variant = vgbl_step(stride_bytes) * 2 + (jaccard ? 1 : 0);      // what the two units' launchers take
    const int G = nq_pad / QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    const long long ntiles = (n_rows + VGBB_TILE - 1) / VGBB_TILE;
    // large corpora: the pre-pass hands every query a start threshold, the real pass runs in stages from there (vg_batch_i8.hip)
    long long pre = 0;
    {
        const int denom = vg_sw(SW_VG_BATCH_PREPASS, VGB_PREPASS_DENOM_DEFAULT);
        if (denom > 0 && ntiles >= 65536) pre = ((ntiles / denom + npart - 1) / npart) * npart;
    }
    return vgb_run_staged(a, ntiles, pre, 400, dev_out_keys, stream,
                          [&](const BatchArgsBits &b) { return vgbl_launch_pre(&b, variant, blocks, smem, stream); },
                          [&](const BatchArgsBits &b) { return vgbl_launch_real(&b, variant, blocks, smem, stream); });
}
#endif
