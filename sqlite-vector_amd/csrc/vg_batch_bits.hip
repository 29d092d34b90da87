// vg_batch_bits.hip - batched queries over PACKED BIT VECTORS (uint8 rows, VG_DIST_HAMMING / VG_DIST_JACCARD) on the integer matrix
// cores.  A bit count is a matrix product once the bits are spread to bytes: with i = popcount(q AND x) = the dot product of the two
// rows seen as 0 / 1 vectors,
//     Hamming = |q| + |x| - 2 i            Jaccard = (u - i) / u,  u = |q| + |x| - i,  0 when u == 0
// - exact integers up to the one division the single scan performs too (vg_accum.h, A_HAM / A_JAC), so every pair's distance is the
// single scan's bit for bit and the lists equal nq separate scans, ties included.  No filter, no re-evaluation stage.
//
//   * the work split is vg_batch_i8.hip's: a workgroup = 8 wavefronts x 32 queries = 256 queries x one partition of the corpus,
//     partitions interleaved over the 8 XCDs, tiles of 32 rows, lists of k <= 32 keys per query in LDS, the barrier-per-tile schedule;
//   * A (queries) is stationary in registers: a query row of `stride` packed bytes is spread ONCE to 8 * stride bytes of 0 / 1; lane
//     (x, h) keeps the 16 values of bits [32t + 16h, +16) of query x in areg[t]; NTB = stride / 4 k-steps <= 32 (128 VGPRs).  Signed
//     bytes 0 / 1: no sign flip, no correction term;
//   * B (rows) is read from the corpus ITSELF: 32 consecutive row-major rows are 32 * stride contiguous bytes.  No tile-major copy, no
//     shadow copy, no cached per-row statistic - nothing to patch when rows change.  LPR lanes share a row; each loads 8 packed bytes
//     of the NEXT tile (one global_load_dwordx2: 4 KB of HBM per tile at 128-byte rows), spreads each 16 bits to a 16-byte chunk -
//     per output dword: 4 bits out (v_bfe_u32), times 0x00204081 (v_mul_u32_u24: the four copies of the nibble do not overlap, bit j
//     lands on bit 8j), AND 0x01010101 - and stores it with ds_write_b128 into the other tile buffer, in the i8 kernel's layout
//     (transposed by 16-byte chunk: chunk column c of the 32 rows at c * 512 + row * 16; one ds_read_b128 feeds one MFMA).  The same
//     lanes count their bits (v_bcnt) and a butterfly over the LPR lanes leaves |x| of the 32 rows in LDS next to the tile;
//   * rows past n_rows are not loaded (they spread as zeros) and never offered to a list;
//   * the gate is an integer margin on the raw accumulator for Hamming (2 i + ng - |x| >= 0, exact) and an integer product test without
//     a division for Jaccard (it cannot reject a pair whose float distance is below the threshold); survivors get the
//     exact distance - the expressions of vg_accum.h - and go through vgb_list_insert;
//   * large corpora: the pre-pass and the staged real passes of vg_batch_common.h;
//   * rows of 129 .. 512 bytes: vg_batch_bitsl.hip, the K dimension split over the wavefronts of a workgroup - the host entry points at
//     the end of this file hand such strides on;
//   * MASKED batches (GATHER): the tile loop runs over VIRTUAL tiles - 32 consecutive entries of the mask's position list
//     (ascending scan positions, padded with 0xFFFFFFFF to whole tiles; built by vgbb_pos_* at the end of this file).  The producer lanes
//     already compute the address of every row they load: here it is rows + position * stride, the position fetched two tiles ahead, the
//     row one tile ahead.  Rows the mask excludes are never read; a tile's positions sit in LDS next to its bit counts and make the keys.
//   * LABELED batches: every query asks for the rows of ITS label.  All pairs are multiplied as before; the label of a
//     tile's rows travels with their bit counts (one dword per row, loaded one tile ahead by the row's first producer lane), the 16 query
//     labels of a lane sit in registers next to its gate values, and the equality test stands IN FRONT of the gate: a row of another
//     label never reaches the slow path, whatever its distance.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <type_traits>

#include "vg_batch_bits_defs.h"
#include "vg_batch_common.h"
#include "vg_batch_units.h"

#define VGBB_WAVES 8
#define VGBB_QPW 32
#define VGBB_QPB (VGBB_WAVES * VGBB_QPW)
#define VGBB_BPIPE 4                    // B-operand register quads in flight

// NTB = k-steps per row (32 bits = 4 packed bytes each): rows up to 4 * NTB bytes, shorter ones zero-padded in the k dimension
// JAC = Jaccard (else Hamming); PRE = the pre-pass variant (vg_batch_i8.hip): only the smallest distance of a query in a tile enters
// GATHER = the masked form (BatchArgsBitsGather, VGBB_NO_POS: vg_batch_bits_defs.h): tiles are runs of 32 entries of a.pos, not of 32 consecutive rows
// LABELED = the labeled form (BatchArgsBitsLabeled, VGBB_NO_LABEL): a pair counts only where the row carries the query's label
template <bool GATHER, bool LABELED>
using vgbb_args_t = std::conditional_t<LABELED, BatchArgsBitsLabeled, std::conditional_t<GATHER, BatchArgsBitsGather, BatchArgsBits>>;
template <int NTB, bool JAC, bool PRE, bool GATHER, bool LABELED = false>
__global__ __launch_bounds__(64 * VGBB_WAVES, 1) void vg_batch_bits_kernel(vgbb_args_t<GATHER, LABELED> a) {
    static_assert(!(GATHER && LABELED), "the labeled form walks consecutive rows: it is not combined with the gathering one");
    constexpr int THREADS = 64 * VGBB_WAVES;
    constexpr int TILE_BYTES = NTB * 1024;                      // 32 rows x 32 NTB spread bytes
    constexpr int LPR = NTB <= 8 ? 4 : (NTB <= 16 ? 8 : 16);   // lanes that share a row of the packed tile, 8 bytes each
    constexpr int SPREADERS = VGBB_TILE * LPR;                  // threads that load and spread (whole wavefronts: 128 / 256 / 512)
    static_assert(NTB % 4 == 0 && NTB >= 2 * VGBB_BPIPE && NTB <= 32 && LPR * 8 >= NTB * 4, "row ladder");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t *tile0 = smem;                                                               // 2 tile buffers
    uint32_t *xcnt_lds = reinterpret_cast<uint32_t *>(smem + 2 * TILE_BYTES);            // [2][32]: |x| of a buffer's rows
    uint32_t *xpos_lds = xcnt_lds + 2 * VGBB_TILE;                                       // GATHER only - [2][32]: the rows' scan positions
    uint32_t *xlab_lds = xcnt_lds + 2 * VGBB_TILE;                                       // LABELED only - [2][32]: the rows' labels (the same dwords)
    uint32_t *qcnt_lds = xcnt_lds + (GATHER || LABELED ? 4 : 2) * VGBB_TILE;             // [waves][32]: |q|
    float *thr_lds = reinterpret_cast<float *>(qcnt_lds + VGBB_QPB);                     // [waves][32]: current k-th best distance
    uint64_t *lists = reinterpret_cast<uint64_t *>(thr_lds + VGBB_QPB);                  // [waves][32][k]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x = lane & 31, h = lane >> 5;
    const int k = a.k;

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
    float *thr_w = thr_lds + wave * VGBB_QPW;
    uint64_t *wave_lists = lists + (size_t)wave * VGBB_QPW * k;
    {
        const uint32_t qc = qc_part + __shfl_xor(qc_part, 32);
        if (h == 0) {
            qc_w[x] = qc;
            // the pre-pass bound is the distance of an actual row, which the first real stage meets again: one ulp up, so that the
            // strict comparison of the slow path lets a row AT the bound in; padding queries never accept
            float t = a.init_keys ? nextafterf(vgb_kth_distance(a.init_keys[(long long)(q0 + x) * 64 + (k - 1)]), INFINITY) : INFINITY;
            if (q0 + x >= a.nq_real) t = -INFINITY;
            thr_w[x] = t;
        }
        const bool seeded = a.seed != 0 && part == 0;               // (keys of rows no later stage meets again)
        for (int s = lane; s < VGBB_QPW * k; s += 64)
            wave_lists[s] = seeded ? a.init_keys[(long long)(q0 + s / k) * 64 + s % k] : VG_EMPTY_KEY;
    }
    // chunk columns past the row length are never written by the spreading: they read as 0 bits
    for (int s = tid; s < 2 * TILE_BYTES / 4; s += THREADS) reinterpret_cast<uint32_t *>(tile0)[s] = 0u;
    __syncthreads();

    // ---- the tile's producer side.  Thread (prow, pj) owns packed bytes [8 pj, +8) of row prow of a tile = chunk columns 4 pj .. 4 pj + 3
    const long long tile_first = a.tile_begin + (long long)part * a.tiles_per_part;
    const long long tile_last = min(tile_first + a.tiles_per_part, a.tile_end);
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
    // GATHER: the thread's entry of a virtual tile (the LPR lanes of a row read the same dword), and the row behind an entry
    auto load_pos = [&](long long tile) __attribute__((always_inline)) -> uint32_t {
        if constexpr (GATHER) return spreader ? a.pos[tile * VGBB_TILE + prow] : VGBB_NO_POS;
        else return 0u;
    };
    auto load_gathered = [&](uint32_t p) __attribute__((always_inline)) -> uint2 {
        uint2 v = make_uint2(0u, 0u);
        if (pcols && p != VGBB_NO_POS) v = *reinterpret_cast<const uint2 *>(a.rows + (unsigned long long)p * (unsigned long long)a.stride + 8 * pj);
        return v;
    };
    // LABELED: the label of row prow of a tile, fetched by the row's first producer lane alone; a row at or past n_rows carries none
    auto load_label = [&](long long tile) __attribute__((always_inline)) -> uint32_t {
        if constexpr (LABELED) return (spreader && pj == 0 && tile * VGBB_TILE + prow < a.n_rows) ? a.labels[tile * VGBB_TILE + prow] : VGBB_NO_LABEL;
        else return 0u;
    };
    // chunk c (0 .. 3) of the thread's 8 bytes into buffer `buf`
    auto spread_chunk = [&](auto cc, uint2 v, int buf) __attribute__((always_inline)) {
        constexpr int c = decltype(cc)::value;
        const uint32_t w = (c < 2) ? v.x : v.y;
        const vgb_i32x4 o = vgbb_spread16((c & 1) ? (w >> 16) : (w & 0xFFFFu));
        if (pcols) *reinterpret_cast<vgb_i32x4 *>(pdst + buf * TILE_BYTES + c * 512) = o;
    };
    auto store_count = [&](uint2 v, int buf, uint32_t p, uint32_t lab) __attribute__((always_inline)) {
        if (!spreader) return;
        uint32_t cnt = (uint32_t)__builtin_popcount(v.x) + (uint32_t)__builtin_popcount(v.y);
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) cnt += __shfl_xor(cnt, m);
        if (pj == 0) xcnt_lds[buf * VGBB_TILE + prow] = cnt;
        if constexpr (GATHER) { if (pj == 0) xpos_lds[buf * VGBB_TILE + prow] = p; }
        if constexpr (LABELED) { if (pj == 0) xlab_lds[buf * VGBB_TILE + prow] = lab; }
    };

    // ---- the gate.  Register r of lane (x, h) belongs to query qi(r, h) = (r&3) + 8*(r>>2) + 4*h; i = acc[r].
    //   Hamming  d = |q| + |x| - 2 i < thr  <=>  2 i + ng - |x| >= 0,  ng = ceil(thr) - 1 - |q|: integers, exact
    //   Jaccard  (S - 2 i) 2^18 <= gt (S - i),  S = |q| + |x|,  gt = ceil(thr 2^18) <= 2^19: integers (v_mul_u32_u24), implied by
    //            fl((u - i) / u) < thr; a padding query stands in the gate with |q| = 4096 and gt = 0 and never passes
    // The exact test - (float) distance < thr, the single scan's arithmetic - is the slow path's.
    // LABELED: the pair stands in the gate only where ok_r = (qlab[r] == the row's label) and the row has one.  A list holds rows of its
    // query's label only, so its threshold is the k-th best among those: without the test in the gate every closer row of another tenant
    // would enter the slow path.  Hamming: a pair that is not ok takes the padding query's margin -(1 << 30) into the max (2 i + ng of an
    // ok pair of a real query lies above it, and the subtraction of |x| cannot wrap).  A padding query carries VGBB_NO_LABEL, a row
    // without a label too: the row's own test keeps the two apart, and the padding query's threshold (-Inf) passes nothing either way.
    vgb_i32x16 ng;                      // Hamming: the margin; Jaccard: |q|
    vgb_i32x16 gs;                      // Jaccard: gt
    uint32_t qlab[LABELED ? 16 : 1];    // LABELED: the label of query qi(r, h)
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
    vgb_static_for<0, 16>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int qi = (r & 3) + 8 * (r >> 2) + 4 * h;
        ng[r] = JAC ? (thr_w[qi] == -INFINITY ? 4096 : (int)qc_w[qi]) : gate_ham(qc_w[qi], thr_w[qi]);
        gs[r] = JAC ? gate_jac(thr_w[qi]) : 0;
        if constexpr (LABELED) qlab[r] = a.qlabels[q0 + qi];
    });
    auto passes = [&](int i, int ngr, int gsr, int xx) __attribute__((always_inline)) -> bool {
        if constexpr (JAC) { const int S = ngr + xx; return ((uint32_t)(S - 2 * i) << 18) <= __umul24((uint32_t)gsr, (uint32_t)(S - i)); }
        else return 2 * i + ngr - xx >= 0;
    };
    // LABELED, Jaccard: `passes` of a pair of equal labels; any other pair stands with the left side 2^32 - 1, above every right side
    // (gt (S - i) <= 2^19 * 5120) - a select on a value, like Hamming's, so that no comparison result has to outlive its statement
    auto passes_lab = [&](int i, int ngr, int gsr, int xx, uint32_t ql, uint32_t xlab) __attribute__((always_inline)) -> bool {
        const int S = ngr + xx;
        const uint32_t lhs = (ql == xlab) ? ((uint32_t)(S - 2 * i) << 18) : 0xFFFFFFFFu;
        return lhs <= __umul24((uint32_t)gsr, (uint32_t)(S - i));
    };
    auto judge_any = [&](const vgb_i32x16 &acc, int xx, uint32_t xlab) __attribute__((always_inline)) -> bool {
        if constexpr (LABELED) {
            const bool labeled_row = xlab != VGBB_NO_LABEL;
            if constexpr (JAC) {
                bool p = false;
                vgb_static_for<0, 16>([&](auto rc) { constexpr int r = decltype(rc)::value; p |= passes_lab(acc[r], ng[r], gs[r], xx, qlab[r], xlab); });
                return __ballot(p && labeled_row) != 0;
            } else {
                int mm = -(1 << 30);
                vgb_static_for<0, 16>([&](auto rc) {
                    constexpr int r = decltype(rc)::value;
                    const int m = (qlab[r] == xlab) ? 2 * acc[r] + ng[r] : -(1 << 30);
                    mm = mm > m ? mm : m;
                });
                return __ballot(labeled_row && mm - xx >= 0) != 0;
            }
        } else if constexpr (JAC) {
            bool p = false;
            vgb_static_for<0, 16>([&](auto rc) { constexpr int r = decltype(rc)::value; p |= passes(acc[r], ng[r], gs[r], xx); });
            return __ballot(p) != 0;
        } else {
            int mm = -0x7FFFFFFF;
            vgb_static_for<0, 16>([&](auto rc) { constexpr int r = decltype(rc)::value; const int m = 2 * acc[r] + ng[r]; mm = mm > m ? mm : m; });
            return __ballot(mm - xx >= 0) != 0;
        }
    };
    // the slow path of a tile (vg_batch_i8.hip's): which registers hold a passing pair, then - one copy of the code, looping over the
    // pending registers by run-time index - the exact distance, the list inserts, the refreshed gate
    // (LABELED: `mine`, bit r = the lane's row carries the label of the query of register r - the predicate of the gate, kept per lane
    //  for the exact test below, where r is a run-time index)
    auto judge_slow = [&](const vgb_i32x16 &acc, long long tile, int buf, int xx, uint32_t xlab) __attribute__((always_inline)) {
        const long long row = GATHER ? (long long)xpos_lds[buf * VGBB_TILE + x] : tile * VGBB_TILE + x;
        unsigned pend = 0, mine = 0;
        vgb_static_for<0, 16>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            if constexpr (LABELED) {
                const unsigned ok = (qlab[r] == xlab && xlab != VGBB_NO_LABEL) ? (1u << r) : 0u;
                mine |= ok;
                pend |= __ballot(ok != 0u && passes(acc[r], ng[r], gs[r], xx)) ? (1u << r) : 0u;
            } else {
                pend |= __ballot(passes(acc[r], ng[r], gs[r], xx)) ? (1u << r) : 0u;
            }
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
            const bool pass = (GATHER ? row != (long long)VGBB_NO_POS : row < a.n_rows) && (!LABELED || ((mine >> r) & 1u)) && (d < thr_l);
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

    // ---- BARRIER PER TILE: the k loop of tile t with, in between its MFMAs, the load of tile t+1's packed bytes (top), their spreading
    // into the other buffer (second half, a chunk every NTB / 8 k-steps) and the rows' bit counts; test; barrier
    constexpr int BP = VGBB_BPIPE;
    vgb_i32x4 bq[BP];
    vgb_i32x16 acc;
    const uint32_t lds_tile0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)tile0;
    uint32_t pos_next = VGBB_NO_POS, pos_next2 = VGBB_NO_POS;          // GATHER: the thread's entries of tiles t + 1 and t + 2 (clamped like tile_next)
    uint32_t lab_next = VGBB_NO_LABEL;                                  // LABELED: the label of the thread's row of tile t + 1
    if (tile_first < tile_last) {
        const uint32_t p0 = load_pos(tile_first);
        if constexpr (GATHER) pos_next = load_pos(min(tile_first + 1, tile_last - 1));
        const uint2 v0 = GATHER ? load_gathered(p0) : load_packed(tile_first);
        vgb_static_for<0, 4>([&](auto cc) { spread_chunk(cc, v0, 0); });
        store_count(v0, 0, p0, load_label(tile_first));
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
                if constexpr (LABELED) lab_next = load_label(tile_next);
            }
            constexpr int S0 = NTB / 2, SD = NTB / 8;
            if constexpr (t >= S0 && (t - S0) % SD == 0 && (t - S0) / SD < 4)
                spread_chunk(std::integral_constant<int, (t - S0) / SD>{}, pk, next_buf);
            if constexpr (t == NTB - 1) store_count(pk, next_buf, pos_next, lab_next);
            __builtin_amdgcn_sched_barrier(0);
        });
        const int xx = (int)xcnt_lds[cur_buf * VGBB_TILE + x];
        const uint32_t xlab = LABELED ? xlab_lds[cur_buf * VGBB_TILE + x] : 0u;
        if (judge_any(acc, xx, xlab)) judge_slow(acc, tile, cur_buf, xx, xlab);
        if constexpr (GATHER) pos_next = pos_next2;
        __syncthreads();
    }

    for (int s = lane; s < VGBB_QPW * 64; s += 64) {
        const int qi = s >> 6, slot = s & 63;
        a.cand[((long long)(q0 + qi) * a.npart_total + a.part_base + part) * 64 + slot] = (slot < k) ? wave_lists[qi * k + slot] : VG_EMPTY_KEY;
    }
}


// ---- host side
// The kernel instantiations are split over six translation units compiled from this file (build.py): the real-pass kernels and the
// entry points here, the PRE kernels with -DVGBB_TU_PRE; the masked form's real-pass kernels, its position-list kernels and its entry
// points with -DVGBB_TU_GATHER, its PRE kernels with -DVGBB_TU_GATHER_PRE; the labeled form's real-pass kernels and entry points with
// -DVGBB_TU_LABELED, its PRE kernels with -DVGBB_TU_LABELED_PRE.
// the ladder of row lengths: k-steps the kernels are instantiated for (rows of up to 32 / 64 / 96 / 128 bytes); 0: not served
static int vgbb_ntb(long long stride_bytes) {
    if (stride_bytes < 16 || stride_bytes % 16 != 0) return 0;
    const long long ntb = stride_bytes / 4;
    return ntb <= 8 ? 8 : (ntb <= 16 ? 16 : (ntb <= 24 ? 24 : (ntb <= 32 ? 32 : 0)));
}

template <int NTB, bool JAC, bool PRE, bool GATHER, bool LABELED, typename Args>
static int launch_bits(const Args &a, int blocks, size_t smem, hipStream_t stream) {
    return vgb_launch(vg_batch_bits_kernel<NTB, JAC, PRE, GATHER, LABELED>, blocks, 64 * VGBB_WAVES, smem, stream, a);
}
template <bool PRE, bool GATHER, bool LABELED = false, typename Args>
static int launch_bits_ntb(const Args &a, int ntb, int jaccard, int blocks, size_t smem, hipStream_t stream) {
    switch (ntb) {
    case 8: return jaccard ? launch_bits<8, true, PRE, GATHER, LABELED>(a, blocks, smem, stream) : launch_bits<8, false, PRE, GATHER, LABELED>(a, blocks, smem, stream);
    case 16: return jaccard ? launch_bits<16, true, PRE, GATHER, LABELED>(a, blocks, smem, stream) : launch_bits<16, false, PRE, GATHER, LABELED>(a, blocks, smem, stream);
    case 24: return jaccard ? launch_bits<24, true, PRE, GATHER, LABELED>(a, blocks, smem, stream) : launch_bits<24, false, PRE, GATHER, LABELED>(a, blocks, smem, stream);
    case 32: return jaccard ? launch_bits<32, true, PRE, GATHER, LABELED>(a, blocks, smem, stream) : launch_bits<32, false, PRE, GATHER, LABELED>(a, blocks, smem, stream);
    }
    return -1;
}
#if defined(VGBB_TU_LABELED_PRE)
extern "C" int vgbb_launch_labeled_pre(const BatchArgsBitsLabeled *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<true, false, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}
#elif defined(VGBB_TU_LABELED)
extern "C" int vgbb_launch_labeled_real(const BatchArgsBitsLabeled *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<false, false, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}

// the labeled form's LDS: vg_batch_bits_lds_bytes + the two tiles' labels (128-byte rows, k = 32: 133632).  Rows of up to 128 bytes only:
// longer ones have no labeled form (the multi-query scan answers)
extern "C" size_t vg_batch_bits_labeled_lds_bytes(long long stride_bytes, int k) {
    if (stride_bytes > 128) return 0;
    const size_t plain = vg_batch_bits_lds_bytes(stride_bytes, k);
    return plain ? plain + 2 * VGBB_TILE * 4 : 0;
}

// vg_batch_bits_launch with a label per row (dev_labels: n_rows dwords) and per query (dev_qlabels: nq_pad dwords, VGBB_NO_LABEL for the
// padding queries): tiles, partitions, the pre-pass and the stages are the plain form's
extern "C" int vg_batch_bits_labeled_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes, const uint32_t *dev_labels,
                                            const uint8_t *dev_queries, const uint32_t *dev_qlabels, int nq_pad, int nq_real, int k, int jaccard,
                                            uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, hipStream_t stream) {
    const size_t smem = vg_batch_bits_labeled_lds_bytes(stride_bytes, k);
    const long long ntiles = (n_rows + VGBB_TILE - 1) / VGBB_TILE;
    if (!smem || !dev_labels || !dev_qlabels || nq_pad < VGBB_QPB || nq_pad % VGBB_QPB != 0 || npart < 1 || npart > VG_SEL_MAX_HEADS ||
        npart > ntiles || n_rows < 1) return -1;
    BatchArgsBitsLabeled a;
    a.rows = dev_rows; a.queries = dev_queries; a.cand = dev_cand; a.labels = dev_labels; a.qlabels = dev_qlabels;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.nq_real = nq_real; a.npart = npart; a.k = k;
    const int variant = vgbb_ntb(stride_bytes) * 2 + (jaccard ? 1 : 0);
    const int G = nq_pad / VGBB_QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    long long pre = 0;
    {
        const int denom = vg_sw(SW_VG_BATCH_PREPASS, VGB_PREPASS_DENOM_DEFAULT);
        if (denom > 0 && ntiles >= 65536) pre = ((ntiles / denom + npart - 1) / npart) * npart;
    }
    return vgb_run_staged(a, ntiles, pre, 400, dev_out_keys, stream,
                          [&](const BatchArgsBitsLabeled &b) { return vgbb_launch_labeled_pre(&b, variant, blocks, smem, stream); },
                          [&](const BatchArgsBitsLabeled &b) { return vgbb_launch_labeled_real(&b, variant, blocks, smem, stream); });
}
#elif defined(VGBB_TU_PRE)
extern "C" int vgbb_launch_pre(const BatchArgsBits *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<true, false>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}
#elif defined(VGBB_TU_GATHER_PRE)
extern "C" int vgbb_launch_gather_pre(const BatchArgsBitsGather *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<true, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}
#elif defined(VGBB_TU_GATHER)
extern "C" int vgbb_launch_gather_real(const BatchArgsBitsGather *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<false, true>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}

// ---- the position list of a row mask (bit p & 63 of word p >> 6: the row at scan position p is allowed): the allowed positions,
// ascending, then VGBB_NO_POS up to a multiple of 32.  Two launches over blocks of VGBB_POS_WORDS mask words, a word per thread: the
// blocks' popcount sums; then every block adds up the sums in front of it, scans its own words and writes its positions.
#define VGBB_POS_WORDS 256
// word w of the mask with the bits from n_rows on cleared (what lies behind the last row is not relied on); words past the mask: 0
__device__ __forceinline__ uint64_t vgbb_mask_word(const uint64_t *mask, long long w, long long n_rows) {
    const long long left = n_rows - w * 64;
    if (left <= 0) return 0ull;
    const uint64_t m = mask[w];
    return left < 64 ? (m & ((1ull << left) - 1ull)) : m;
}
__device__ __forceinline__ uint32_t vgbb_wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__global__ __launch_bounds__(VGBB_POS_WORDS) void vgbb_pos_sums_kernel(const uint64_t *mask, long long n_rows, uint32_t *sums) {
    __shared__ uint32_t wsum[VGBB_POS_WORDS / 64];
    const int tid = threadIdx.x;
    const uint32_t c = vgbb_wave_sum((uint32_t)__popcll(vgbb_mask_word(mask, (long long)blockIdx.x * VGBB_POS_WORDS + tid, n_rows)));
    if ((tid & 63) == 0) wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// pos: `cap` entries = the mask's count rounded up to 32 (nothing is written at or past cap, whatever the mask holds)
__global__ __launch_bounds__(VGBB_POS_WORDS) void vgbb_pos_write_kernel(const uint64_t *mask, long long n_rows, const uint32_t *sums, uint32_t *pos,
                                                                        long long cap) {
    __shared__ uint32_t wfront[VGBB_POS_WORDS / 64], wown[VGBB_POS_WORDS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t front = 0;
    for (unsigned b = (unsigned)tid; b < blockIdx.x; b += VGBB_POS_WORDS) front += sums[b];
    front = vgbb_wave_sum(front);
    const long long w = (long long)blockIdx.x * VGBB_POS_WORDS + tid;
    uint64_t m = vgbb_mask_word(mask, w, n_rows);
    const uint32_t c = (uint32_t)__popcll(m);
    uint32_t inc = c;                                           // inclusive scan over the wavefront's words
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 0) wfront[wave] = front;
    if (lane == 63) wown[wave] = inc;
    __syncthreads();
    long long at = (long long)wfront[0] + wfront[1] + wfront[2] + wfront[3] + (inc - c);
    for (int i = 0; i < wave; ++i) at += wown[i];
    const uint32_t p0 = (uint32_t)(w * 64);
    while (m) {
        const int bit = __builtin_ctzll(m);
        m &= m - 1;
        if (at < cap) pos[at] = p0 + (uint32_t)bit;
        ++at;
    }
    if (blockIdx.x == gridDim.x - 1 && tid < 32) {              // the last virtual tile's padding
        const long long total = (long long)wfront[0] + wfront[1] + wfront[2] + wfront[3] + wown[0] + wown[1] + wown[2] + wown[3];
        if (total + tid < ((total + 31) & ~31ll) && total + tid < cap) pos[total + tid] = VGBB_NO_POS;
    }
}
// dwords of scratch (the blocks' sums) vg_batch_bits_pos_launch needs behind the list
extern "C" size_t vg_batch_bits_pos_scratch_dwords(long long n_rows) { return (size_t)(((n_rows + 63) / 64 + VGBB_POS_WORDS - 1) / VGBB_POS_WORDS); }
// dev_mask: ceil(n_rows / 64) words; dev_pos: `cap` entries (the mask's count rounded up to 32); 0 or a hipError_t
extern "C" int vg_batch_bits_pos_launch(const uint64_t *dev_mask, long long n_rows, uint32_t *dev_pos, long long cap, uint32_t *dev_sums, hipStream_t stream) {
    const unsigned blocks = (unsigned)vg_batch_bits_pos_scratch_dwords(n_rows);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(vgbb_pos_sums_kernel, dim3(blocks), dim3(VGBB_POS_WORDS), 0, stream, dev_mask, n_rows, dev_sums);
    hipLaunchKernelGGL(vgbb_pos_write_kernel, dim3(blocks), dim3(VGBB_POS_WORDS), 0, stream, dev_mask, n_rows, (const uint32_t *)dev_sums, dev_pos, cap);
    return (int)hipGetLastError();
}

// the masked form's LDS: vg_batch_bits_lds_bytes + the two tiles' positions (128-byte rows, k = 32: 133632); rows beyond 128 bytes: the
// long-row form's answer
extern "C" size_t vg_batch_bits_masked_lds_bytes(long long stride_bytes, int k) {
    if (stride_bytes > 128) return vg_batch_bitsl_masked_lds_bytes(stride_bytes, k);
    const size_t plain = vg_batch_bits_lds_bytes(stride_bytes, k);
    return plain ? plain + 2 * VGBB_TILE * 4 : 0;
}

// vg_batch_bits_launch over the n_pos rows of a position list (dev_pos: n_pos rounded up to 32 entries, vg_batch_bits_pos_launch's):
// tiles, partitions, the pre-pass and the stages count VIRTUAL tiles.  The keys carry the rows' real scan positions.
extern "C" int vg_batch_bits_masked_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes, const uint32_t *dev_pos, long long n_pos,
                                           const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int jaccard,
                                           uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, hipStream_t stream) {
    if (stride_bytes > 128)
        return vg_batch_bitsl_masked_launch(dev_rows, n_rows, stride_bytes, dev_pos, n_pos, dev_queries, nq_pad, nq_real, k, jaccard, dev_cand, npart,
                                            dev_out_keys, stream);
    const size_t smem = vg_batch_bits_masked_lds_bytes(stride_bytes, k);
    const long long ntiles = (n_pos + VGBB_TILE - 1) / VGBB_TILE;
    const int QPB = vg_batch_bits_queries_per_block(stride_bytes);
    if (!smem || nq_pad < QPB || nq_pad % QPB != 0 || npart < 1 || npart > VG_SEL_MAX_HEADS || npart > ntiles || n_pos < 1 || n_pos > n_rows) return -1;
    BatchArgsBitsGather a;
    a.rows = dev_rows; a.queries = dev_queries; a.cand = dev_cand; a.pos = dev_pos;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.nq_real = nq_real; a.npart = npart; a.k = k;
    const int variant = vgbb_ntb(stride_bytes) * 2 + (jaccard ? 1 : 0);
    const int G = nq_pad / VGBB_QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    long long pre = 0;
    {
        const int denom = vg_sw(SW_VG_BATCH_PREPASS, VGB_PREPASS_DENOM_DEFAULT);
        if (denom > 0 && ntiles >= 65536) pre = ((ntiles / denom + npart - 1) / npart) * npart;
    }
    return vgb_run_staged(a, ntiles, pre, 400, dev_out_keys, stream,
                          [&](const BatchArgsBitsGather &b) { return vgbb_launch_gather_pre(&b, variant, blocks, smem, stream); },
                          [&](const BatchArgsBitsGather &b) { return vgbb_launch_gather_real(&b, variant, blocks, smem, stream); });
}
#else
extern "C" int vgbb_launch_real(const BatchArgsBits *a, int variant, int blocks, size_t smem, hipStream_t stream) {
    return launch_bits_ntb<false, false>(*a, variant >> 1, variant & 1, blocks, smem, stream);
}

// queries a workgroup serves: 256, or the long-row form's 128 (rows of up to 256 bytes) / 64 (up to 512)
extern "C" int vg_batch_bits_queries_per_block(long long stride_bytes) {
    return stride_bytes > 128 ? vg_batch_bitsl_queries_per_block(stride_bytes) : VGBB_QPB;
}

// LDS bytes of one workgroup: two spread tiles, their rows' bit counts, the queries' bit counts and thresholds, the lists
// (128-byte rows, k = 32: 65536 + 256 + 1024 + 1024 + 65536 = 133376); rows beyond 128 bytes: the long-row form's answer.  0: not
// served - the ONE place that decides which rows and k take the matrix cores
extern "C" size_t vg_batch_bits_lds_bytes(long long stride_bytes, int k) {
    if (stride_bytes > 128) return vg_batch_bitsl_lds_bytes(stride_bytes, k);
    const int NTB = vgbb_ntb(stride_bytes);
    if (!NTB || k < 1 || k > VGBB_MAX_K) return 0;
    return (size_t)2 * NTB * 1024 + 2 * VGBB_TILE * 4 + VGBB_QPB * 4 + VGBB_QPB * 4 + (size_t)VGBB_QPB * k * 8;
}

// dev_rows: the corpus' row-major rows; dev_queries: nq_pad x stride packed bytes.  Returns 0, -1 if the shape is not served, a
// hipError_t otherwise.  dev_cand sized like the f32 kernel's.
extern "C" int vg_batch_bits_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes,
                                    const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int jaccard,
                                    uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, hipStream_t stream) {
    if (stride_bytes > 128)
        return vg_batch_bitsl_launch(dev_rows, n_rows, stride_bytes, dev_queries, nq_pad, nq_real, k, jaccard, dev_cand, npart, dev_out_keys, stream);
    const size_t smem = vg_batch_bits_lds_bytes(stride_bytes, k);
    if (!smem || nq_pad < VGBB_QPB || nq_pad % VGBB_QPB != 0 || npart < 1 || npart > VG_SEL_MAX_HEADS || n_rows < 1) return -1;
    BatchArgsBits a;
    a.rows = dev_rows; a.queries = dev_queries; a.cand = dev_cand;
    a.n_rows = n_rows; a.stride = stride_bytes; a.nq_pad = nq_pad; a.nq_real = nq_real; a.npart = npart; a.k = k;
    const int variant = vgbb_ntb(stride_bytes) * 2 + (jaccard ? 1 : 0);       // what the two units' launchers take
    const int G = nq_pad / VGBB_QPB;
    const int blocks = G * ((npart + 7) / 8) * 8;
    const long long ntiles = (n_rows + VGBB_TILE - 1) / VGBB_TILE;
    // large corpora: the pre-pass hands every query a start threshold, the real pass runs in stages from there (vg_batch_i8.hip)
    long long pre = 0;
    {
        const int denom = vg_sw(SW_VG_BATCH_PREPASS, VGB_PREPASS_DENOM_DEFAULT);
        if (denom > 0 && ntiles >= 65536) pre = ((ntiles / denom + npart - 1) / npart) * npart;
    }
    return vgb_run_staged(a, ntiles, pre, 400, dev_out_keys, stream,
                          [&](const BatchArgsBits &b) { return vgbb_launch_pre(&b, variant, blocks, smem, stream); },
                          [&](const BatchArgsBits &b) { return vgbb_launch_real(&b, variant, blocks, smem, stream); });
}
#endif
