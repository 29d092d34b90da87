// vg_batch_bitsl_within.hip - the LONG-ROW form of vg_batch_bits_within.hip: batch RANGE scans (every row within a radius, a radius per
// query) over packed bit vectors of 129 .. 512 bytes (uint8 rows, stride 144 .. 512, Hamming / Jaccard) on the integer matrix cores.
// The work split and the data movement are vg_batch_bitsl.hip's, the range semantics - radius to gate, exact test,
// emission - vg_batch_bits_within.hip's (3.27); what is new is who judges (3.28):
//
//   * 8 wavefronts = QG query groups x KS K-slices (KS = 2: rows up to 256 bytes, 128 queries per workgroup; KS = 4: up to 512, 64).
//     Wavefront (qg, ks) keeps k-steps [ks NTBW, +NTBW) of its 32 queries in registers as 0 / 1 bytes and runs the k loop over that
//     slice of the tile; all 512 threads load packed rows, 8 bytes each, and spread them into the i8 tile layout, |x| as quarter sums
//     next to the tile; two tile buffers at KS = 2 (the next tile is spread between the MFMAs), one at KS = 4 (its packed bytes wait in
//     registers and are spread after the exchange) - that file's, statement for statement;
//   * a range scan keeps no per-query state beyond constants of the launch - |q|, the radius, the region and its capacity, read ONCE
//     from the VgWithinQuery descriptors into LDS -, so there is no lead that owns lists: EVERY wavefront judges.  Accumulator quad
//     j = r >> 2 holds queries [8j, +8) of the group; wavefront ks owns quads [ks 4 / KS, +4 / KS), i.e. queries [16 ks, +16) at KS = 2
//     and [8 ks, +8) at KS = 4.  After the k loop it writes every quad it does not own into the owner's slot of the exchange area (one
//     vgb_i32x4 per quad and lane, in the first (8 - QG) x 4096 bytes of the tile buffer just consumed: the lead form's format, place
//     and volume), and after the barrier adds the KS - 1 partial quads of its own queries - integers, exact in any order -, reads
//     the rows' |x| and runs the gate and the slow path over its 16 / KS registers.  No wavefront idles while another judges, and the
//     atomics of a dense radius are spread over KS wavefronts;
//   * no lists, no thresholds that move, no candidate buffer, no pre-pass, no stages, no merge: ONE launch covers all tiles and all
//     query groups.  Barriers per tile: after the k loop, after the partials are written, after they are read (the buffer is free
//     again); the one-buffer form has a fourth behind its spreading.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vg_batch_bits_defs.h"
#include "vg_batch_common.h"
#include "vg_batch_units.h"
#include "vg_scan_multi.h"

#define VGBL_WAVES 8
#define VGBL_BPIPE 4                    // B-operand register quads in flight

typedef int vgblw_i32x8 __attribute__((ext_vector_type(8)));

// KS = K-slices (wavefronts that share 32 queries), NTBW = k-steps (32 bits each) per slice: rows up to 4 KS NTBW bytes, shorter ones
// zero-padded in the k dimension; JAC = Jaccard (else Hamming)
template <int KS, int NTBW, bool JAC>
__global__ __launch_bounds__(64 * VGBL_WAVES, 1) void vg_batch_bitsl_within_kernel(BatchArgsBitsWithin a) {
    constexpr int THREADS = 64 * VGBL_WAVES;
    constexpr int QG = VGBL_WAVES / KS, QPB = QG * 32;
    constexpr int NTB = KS * NTBW;                              // k-steps of a whole row
    constexpr int TILE_BYTES = NTB * 1024;                      // 32 rows x 32 NTB spread bytes
    constexpr int NBUF = KS == 2 ? 2 : 1;                       // tile buffers
    constexpr int UPT = (NTB + 31) / 32;                        // 8-byte units a thread loads and spreads per tile
    constexpr int NCH = 4 * UPT;                                // ... = 16-byte chunks it writes
    constexpr int QPO = 4 / KS;                                 // accumulator quads a wavefront owns (judges) ...
    constexpr int NR = 4 * QPO;                                 // ... = registers: 8 / 4
    using OwnV = std::conditional_t<KS == 2, vgblw_i32x8, vgb_i32x4>;
    static_assert((KS == 2 || KS == 4) && NTBW % 4 == 0 && NTBW >= 2 * VGBL_BPIPE && NTBW <= 32, "row ladder");
    static_assert((VGBL_WAVES - QG) * 4096 <= 144 / 2 * 512, "the exchange stays inside chunk columns every served row has");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *tile0 = smem;                                                               // NBUF tile buffers
    uint32_t *xcnt_lds = reinterpret_cast<uint32_t *>(smem + NBUF * TILE_BYTES);         // [NBUF][32][4]: |x| of a buffer's rows, by quarter
    uint32_t *qpart_lds = xcnt_lds + NBUF * VGBB_TILE * 4;                               // [waves][32]: |q| of a wavefront's slice
    uint32_t *qcnt_lds = qpart_lds + VGBL_WAVES * 32;                                    // [QG][32]: |q|
    float *rad_lds = reinterpret_cast<float *>(qcnt_lds + QPB);                          // [QG][32]: the radius (-Inf: matches nothing)
    unsigned long long *out_lds = reinterpret_cast<unsigned long long *>(rad_lds + QPB); // [QG][32]: the region [count | cap keys]
    unsigned long long *cap_lds = out_lds + QPB;                                         // [QG][32]: its capacity

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qg = wave % QG, ks = wave / QG;
    const int x = lane & 31, h = lane >> 5;

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
    float *rad_w = rad_lds + qg * 32;
    unsigned long long *out_w = out_lds + qg * 32, *cap_w = cap_lds + qg * 32;
    qc_part += __shfl_xor(qc_part, 32);
    if (h == 0) qpart_lds[wave * 32 + x] = qc_part;
    // chunk columns past the row length are never written by the spreading (and meet zero bytes of A)
    for (int s = tid; s < NBUF * TILE_BYTES / 4; s += THREADS) reinterpret_cast<uint32_t *>(tile0)[s] = 0u;
    __syncthreads();
    // the constants of the launch: one wavefront per query group adds the slices' bit counts and reads the 32 descriptors
    if (ks == 0 && h == 0) {
        uint32_t qc = 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) qc += qpart_lds[(s * QG + qg) * 32 + x];
        const VgWithinQuery d = reinterpret_cast<const VgWithinQuery *>(a.desc)[q0 + x];
        qc_w[x] = qc;
        // a query without capacity is padding; a radius below zero matches nothing either (vgbb_within_thr): both stand as -Inf
        rad_w[x] = (d.cap == 0ull || d.r < 0.0f) ? -INFINITY : d.r;
        out_w[x] = (unsigned long long)(uintptr_t)d.out;
        cap_w[x] = d.cap;
    }
    __syncthreads();

    // ---- the tile's producer side.  Thread (prow, pj), unit u: packed bytes [8 (pj + 16 u), +8) of row prow = chunk columns 4 (pj + 16 u) ..
    const long long ntiles = (a.n_rows + VGBB_TILE - 1) / VGBB_TILE;
    const long long tile_first = (long long)part * a.tiles_per_part;
    const long long tile_last = min(tile_first + a.tiles_per_part, ntiles);
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
    // chunk ci (0 .. NCH - 1: unit ci / 4, its 16 bits ci % 4) into buffer `buf`
    auto spread_chunk = [&](auto cc, int buf) __attribute__((always_inline)) {
        constexpr int u = decltype(cc)::value / 4, c = decltype(cc)::value % 4;
        const uint32_t w = (c < 2) ? pk[u].x : pk[u].y;
        const vgb_i32x4 o = vgbb_spread16((c & 1) ? (w >> 16) : (w & 0xFFFFu));
        if (8 * (pj + 16 * u) < (int)a.stride) *reinterpret_cast<vgb_i32x4 *>(pdst + buf * TILE_BYTES + (64 * u + c) * 512) = o;
    };
    auto store_count = [&](int buf) __attribute__((always_inline)) {
        uint32_t cnt = 0;
        vgb_static_for<0, UPT>([&](auto uc) { constexpr int u = decltype(uc)::value; cnt += (uint32_t)__builtin_popcount(pk[u].x) + (uint32_t)__builtin_popcount(pk[u].y); });
        cnt += __shfl_xor(cnt, 16);
        cnt += __shfl_xor(cnt, 32);
        if (lane < 16) xcnt_lds[(buf * VGBB_TILE + prow) * 4 + (wave >> 1)] = cnt;
    };

    // ---- the gate, over the registers the wavefront owns.  Accumulator register r of lane (x, h) belongs to query (r&3) + 8*(r>>2) + 4*h of the
    // group; owned register m is r = 4 (ks QPO) + m, so its query is qi(m, h) = (m&3) + 8*(ks QPO + (m>>2)) + 4*h.  Constants of the launch:
    //   Hamming  d = |q| + |x| - 2 i < thr  <=>  2 i + ng - |x| >= 0: integers, exact (d <= 4096)
    //   Jaccard  (S - 2 i) 2^18 <= gt (S - i),  S = |q| + |x| <= 8192, so the shifted side is at most 2^31; a real pair has S - i = u <= 4096
    //            and gt <= 2^19, so the product (both factors below 2^24) stays below 2^32.  A query that matches nothing stands in the gate
    //            with |q| = 4096 and gt = 0: S - 2 i >= 4096 - |x| >= 0 reaches 0 only for all 4096 bits set in the query and in the row - that
    //            pair passes the gate, and the exact test against -Inf rejects it
    const int jown = ks * QPO;                                  // the first quad the wavefront owns
    OwnV ng;                            // Hamming: the margin; Jaccard: |q|
    OwnV gs;                            // Jaccard: gt
    vgb_static_for<0, NR>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const int qi = (m & 3) + 8 * (jown + (m >> 2)) + 4 * h;
        const float thr = vgbb_within_thr(rad_w[qi]);
        ng[m] = JAC ? (thr == -INFINITY ? 4096 : (int)qc_w[qi]) : vgbb_gate_ham(qc_w[qi], thr);
        gs[m] = JAC ? vgbb_gate_jac(thr) : 0;
    });
    auto passes = [&](int i, int ngr, int gsr, int xx) __attribute__((always_inline)) -> bool {
        if constexpr (JAC) { const int S = ngr + xx; return ((uint32_t)(S - 2 * i) << 18) <= __umul24((uint32_t)gsr, (uint32_t)(S - i)); }
        else return 2 * i + ngr - xx >= 0;
    };
    auto judge_any = [&](const OwnV &own, int xx) __attribute__((always_inline)) -> bool {
        if constexpr (JAC) {
            bool p = false;
            vgb_static_for<0, NR>([&](auto mc) { constexpr int m = decltype(mc)::value; p |= passes(own[m], ng[m], gs[m], xx); });
            return __ballot(p) != 0;
        } else {
            int mm = -0x7FFFFFFF;
            vgb_static_for<0, NR>([&](auto mc) { constexpr int m = decltype(mc)::value; const int v = 2 * own[m] + ng[m]; mm = mm > v ? mm : v; });
            return __ballot(mm - xx >= 0) != 0;
        }
    };
    // the slow path of a tile: which registers hold a passing pair, then - one copy of the code, looping over the pending registers by
    // run-time index - the exact distance, the exact test against the radius, the keys' way out
    auto judge_slow = [&](const OwnV &own, long long tile, int xx) __attribute__((always_inline)) {
        const long long row = tile * VGBB_TILE + x;
        unsigned pend = 0;
        vgb_static_for<0, NR>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            pend |= __ballot(passes(own[m], ng[m], gs[m], xx)) ? (1u << m) : 0u;
        });
        while (pend) {
            const int m = __builtin_ctz(pend);
            pend &= pend - 1;
            const int qi = (m & 3) + 8 * (jown + (m >> 2)) + 4 * h;
            const uint32_t qc = qc_w[qi];
            const uint32_t i = (uint32_t)own[m];
            float d;
            if (JAC) {
                const uint32_t u = qc + (uint32_t)xx - i;
                d = u ? __fdiv_rn((float)(u - i), (float)u) : 0.0f;
            } else {
                d = (float)(qc + (uint32_t)xx - 2u * i);
            }
            d = vg_clamp(d);
            // (rows at or past n_rows spread as zeros: they have a distance, and never a key.  -Inf in rad_w: nothing is <= it)
            const bool pass = (row < a.n_rows) && (d <= rad_w[qi]);
            vgbb_within_emit(pass, vg_make_key(d, (uint32_t)row), reinterpret_cast<unsigned long long *>((uintptr_t)out_w[qi]), cap_w[qi], lane);
        }
    };

    // ---- per tile: the k loop over the wavefront's slice, with the load of tile t+1's packed bytes at its top and - two buffers - their
    // spreading into the other buffer between its later MFMAs; barrier; every quad the wavefront does not own to its owner; barrier; the
    // owner adds the KS - 1 partials of its quads and fetches |x|; barrier; everybody's test over the owned registers, next to - one
    // buffer - everybody's spreading of tile t+1 and a last barrier
    constexpr int BP = VGBL_BPIPE;
    constexpr int SD = (3 * NTBW / 4) / NCH > 0 ? (3 * NTBW / 4) / NCH : 1, S0 = NTBW - NCH * SD;   // two buffers: chunk j behind k-step S0 + j SD
    static_assert(NBUF == 1 || S0 >= 1, "the spreading fits behind the load in the k loop");
    vgb_i32x4 bq[BP];
    vgb_i32x16 acc;
    const uint32_t lds_tile0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)tile0;
    if (tile_first < tile_last) {
        load_packed(tile_first);
        vgb_static_for<0, NCH>([&](auto cc) { spread_chunk(cc, 0); });
        store_count(0);
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
            if constexpr (t == 0) load_packed(tile_next);
            if constexpr (NBUF == 2 && t >= S0 && (t - S0) % SD == 0 && (t - S0) / SD < NCH)
                spread_chunk(std::integral_constant<int, (t - S0) / SD>{}, next_buf);
            if constexpr (NBUF == 2 && t == NTBW - 1) store_count(next_buf);
            __builtin_amdgcn_sched_barrier(0);
        });
        __syncthreads();                                                    // the tile is consumed (two buffers: and the next one complete)
        // the exchange of a query group: [owner][sender, the owner left out][owned quad][lane], one vgb_i32x4 each
        vgb_i32x4 *xchg = reinterpret_cast<vgb_i32x4 *>(tile0 + cur_buf * TILE_BYTES) + qg * (KS - 1) * 256 + lane;
        vgb_static_for<0, 4>([&](auto jc) {
            constexpr int j = decltype(jc)::value, o = j / QPO, jj = j % QPO;
            if (ks != o) {
                vgb_i32x4 v;
                v[0] = acc[4 * j]; v[1] = acc[4 * j + 1]; v[2] = acc[4 * j + 2]; v[3] = acc[4 * j + 3];
                xchg[((o * (KS - 1) + (ks < o ? ks : ks - 1)) * QPO + jj) * 64] = v;
            }
        });
        __syncthreads();
        OwnV own;
        vgb_static_for<0, NR>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            if constexpr (KS == 2) own[m] = ks ? acc[8 + m] : acc[m];
            else own[m] = ks < 2 ? (ks == 0 ? acc[m] : acc[4 + m]) : (ks == 2 ? acc[8 + m] : acc[12 + m]);
        });
        vgb_static_for<0, (KS - 1) * QPO>([&](auto jc) {
            constexpr int s = decltype(jc)::value / QPO, jj = decltype(jc)::value % QPO;
            const vgb_i32x4 v = xchg[((ks * (KS - 1) + s) * QPO + jj) * 64];
            own[4 * jj] += v[0]; own[4 * jj + 1] += v[1]; own[4 * jj + 2] += v[2]; own[4 * jj + 3] += v[3];
        });
        const uint4 xc = reinterpret_cast<const uint4 *>(xcnt_lds)[cur_buf * VGBB_TILE + x];
        const int xx = (int)(xc.x + xc.y + xc.z + xc.w);
        __syncthreads();                                                    // the exchange is read: the buffer may be spread into again
        if (judge_any(own, xx)) judge_slow(own, tile, xx);
        if constexpr (NBUF == 1) {
            vgb_static_for<0, NCH>([&](auto cc) { spread_chunk(cc, 0); });
            store_count(0);
            __syncthreads();
        }
    }
}

// ---- host side
// the ladder of row lengths (vg_batch_bitsl.hip's): rows of up to 192 / 256 bytes run as KS = 2 with 24 / 32 k-steps per slice, up to
// 384 / 512 as KS = 4; 64 KS + NTBW, 0: not served
static int vgblw_step(long long stride_bytes) {
    if (stride_bytes <= 128 || stride_bytes > 512 || stride_bytes % 16 != 0) return 0;
    return stride_bytes <= 192 ? 2 * 64 + 24 : (stride_bytes <= 256 ? 2 * 64 + 32 : (stride_bytes <= 384 ? 4 * 64 + 24 : 4 * 64 + 32));
}

extern "C" int vg_batch_bitsl_within_queries_per_block(long long stride_bytes) {
    const int step = vgblw_step(stride_bytes);
    return step ? 32 * VGBL_WAVES / (step >> 6) : 0;
}

// LDS bytes of one workgroup: the tile buffers (two of KS = 2, one of KS = 4), their rows' bit counts by quarter, the slices' bit counts,
// per query |q|, radius, region, capacity (24 bytes); 0: rows it does not serve
//   <= 192 bytes  98 304 + 1024 + 1024 + 128 x 24 = 103 424
//   <= 256       131 072 + 1024 + 1024 + 128 x 24 = 136 192
//   <= 384        98 304 +  512 + 1024 +  64 x 24 = 101 376
//   <= 512       131 072 +  512 + 1024 +  64 x 24 = 134 144
extern "C" size_t vg_batch_bitsl_within_lds_bytes(long long stride_bytes) {
    const int step = vgblw_step(stride_bytes);
    if (!step) return 0;
    const int KS = step >> 6, NTBW = step & 63, NBUF = KS == 2 ? 2 : 1, QPB = 32 * VGBL_WAVES / KS;
    const size_t bytes = (size_t)NBUF * KS * NTBW * 1024 + NBUF * VGBB_TILE * 16 + VGBL_WAVES * 32 * 4 + (size_t)QPB * (4 + 4 + 8 + 8);
    return bytes <= VGBB_LDS_LIMIT ? bytes : 0;
}

template <int KS, int NTBW>
static int launch_within_long(const BatchArgsBitsWithin &a, int jaccard, int blocks, size_t smem, hipStream_t stream) {
    return jaccard ? vgb_launch(vg_batch_bitsl_within_kernel<KS, NTBW, true>, blocks, 64 * VGBL_WAVES, smem, stream, a)
                   : vgb_launch(vg_batch_bitsl_within_kernel<KS, NTBW, false>, blocks, 64 * VGBL_WAVES, smem, stream, a);
}

// vg_batch_bits_within_launch's arguments and answers; nq_pad: a multiple of the queries per workgroup - every query group of the launch
// meets every row.  Returns 0, -1 if the shape is not served, a hipError_t otherwise.
extern "C" int vg_batch_bitsl_within_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes,
                                            const uint8_t *dev_queries, const void *dev_desc, int nq_pad, int jaccard, int npart, hipStream_t stream) {
    const size_t smem = vg_batch_bitsl_within_lds_bytes(stride_bytes);
    const int QPB = vg_batch_bitsl_within_queries_per_block(stride_bytes);
    if (!smem || nq_pad < QPB || nq_pad % QPB != 0 || npart < 1 || n_rows < 1) return -1;
    const long long ntiles = (n_rows + VGBB_TILE - 1) / VGBB_TILE;
    BatchArgsBitsWithin a;
    a.rows = dev_rows; a.queries = dev_queries; a.desc = dev_desc;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.npart = npart;
    a.tiles_per_part = (int)((ntiles + npart - 1) / npart);
    const int G = nq_pad / QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    switch (vgblw_step(stride_bytes)) {
    case 2 * 64 + 24: return launch_within_long<2, 24>(a, jaccard, blocks, smem, stream);
    case 2 * 64 + 32: return launch_within_long<2, 32>(a, jaccard, blocks, smem, stream);
    case 4 * 64 + 24: return launch_within_long<4, 24>(a, jaccard, blocks, smem, stream);
    case 4 * 64 + 32: return launch_within_long<4, 32>(a, jaccard, blocks, smem, stream);
    }
    return -1;
}
