// vg_batch_bits_defs.h - what the two forms of the bit-vector batch kernel share: vg_batch_bits.hip (rows of up to 128 bytes, a wavefront
// holds its 32 queries whole) and vg_batch_bitsl.hip (rows of 129 .. 512 bytes, the K dimension split over the wavefronts of a workgroup).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vg_batch_dma.h"

#define VGBB_TILE 32                    // rows per tile
#define VGBB_MAX_K 32
#define VGBB_LDS_LIMIT 163840           // bytes of LDS a workgroup can have (gfx950)

struct BatchArgsBits {
    const uint8_t *rows;      // the corpus' own row-major rows: `stride` packed bytes each
    const uint8_t *queries;   // nq_pad x stride packed bytes, zero padded
    uint64_t *cand;
    long long n_rows;
    long long stride;         // bytes per row (multiple of 16; <= 128: vg_batch_bits.hip, 144 .. 512: vg_batch_bitsl.hip)
    int nq_pad, nq_real, npart, k;   // queries [nq_real, nq_pad) are padding
    int tiles_per_part;
    long long tile_begin, tile_end;
    int part_base, npart_total;
    const uint64_t *init_keys;
    int seed;                 // staged real passes (vg_batch_common.h): partition 0 starts its lists from init_keys
};

// the masked (GATHER) forms of both units: tiles are runs of 32 entries of the mask's position list, not of 32 consecutive rows
#define VGBB_NO_POS 0xFFFFFFFFu          // a padding entry of the position list: no row
struct BatchArgsBitsGather : BatchArgsBits {
    const uint32_t *pos;      // GATHER: tile_end * 32 entries - the allowed scan positions, ascending, VGBB_NO_POS behind the last
};

// the labeled (LABELED) form of vg_batch_bits.hip: every query asks for the rows of ITS label only; tiles stay runs of
// 32 consecutive rows
#define VGBB_NO_LABEL 0xFFFFFFFFu        // = VG_LABEL_NONE (vectorgpu.h; vg_batch_api.hip asserts the value): a row no query matches, a padding query
struct BatchArgsBitsLabeled : BatchArgsBits {
    const uint32_t *labels;   // LABELED: n_rows dwords - the label of the row at each scan position
    const uint32_t *qlabels;  // LABELED: nq_pad dwords - the queries' labels, VGBB_NO_LABEL for the padding queries
};

// ---- the range forms (every row within a radius): vg_batch_bits_within.hip (rows of up to 128 bytes) and its K-split
// sibling vg_batch_bitsl_within.hip (129 .. 512 bytes; 3.28), which share the arguments, the gate and the emission below.
struct BatchArgsBitsWithin {
    const uint8_t *rows;      // as BatchArgsBits
    const uint8_t *queries;   // nq_pad x stride packed bytes, zero padded
    const void *desc;         // nq_pad VgWithinQuery (vg_scan_multi.h): region [count | cap keys], cap, radius; a padding query: cap 0, radius -Inf
    long long n_rows;
    long long stride;         // bytes per row, a multiple of 16: 16 .. 128 (vg_batch_bits_within.hip), 144 .. 512 (vg_batch_bitsl_within.hip)
    int nq_pad, npart;        // nq_pad: a multiple of the unit's queries per workgroup (256; the long rows' 128 / 64)
    int tiles_per_part;
};
// the masked (GATHER) range form of vg_batch_bits_within.hip: tiles are runs of 32 entries of the mask's position list;
// tiles_per_part and npart then count tiles of the LIST, n_rows stays the corpus' (no entry names a row at or past it)
struct BatchArgsBitsWithinGather : BatchArgsBitsWithin {
    const uint32_t *pos;      // n_tiles * 32 entries - the allowed scan positions, ascending, VGBB_NO_POS behind the last
    long long n_tiles;        // ceil(allowed rows / 32)
};

// A row matches iff d <= r.  Every distance here is finite and >= 0: a radius below zero (-0.0 is not) matches nothing and stands as
// -Inf, the padding query's; otherwise d <= r <=> d < thr with thr the next float above r (+Inf stays +Inf) - the strict test the
// top-k kernels' gates were derived for
__device__ __forceinline__ float vgbb_within_thr(float r) { return (r < 0.0f) ? -INFINITY : nextafterf(r, INFINITY); }
// the gates of vg_batch_bits.hip (its gate_ham / gate_jac, statement for statement; that kernel keeps its own copies and with them its code)
//   Hamming  d = |q| + |x| - 2 i < thr  <=>  2 i + ng - |x| >= 0,  ng = ceil(thr) - 1 - |q|
//   Jaccard  (S - 2 i) 2^18 <= gt (S - i),  S = |q| + |x|,  gt = ceil(thr 2^18) <= 2^19
__device__ __forceinline__ int vgbb_gate_ham(uint32_t qc, float thr) {
    if (thr == -INFINITY) return -(1 << 30);               // never matches
    if (!(thr < 1.0e9f)) return 1 << 30;                   // everything matches
    return (int)ceilf(thr) - 1 - (int)qc;
}
__device__ __forceinline__ int vgbb_gate_jac(float thr) {
    if (thr == -INFINITY) return 0;                        // never matches (with |q| = 4096 in the gate)
    if (!(thr < 2.0f)) return 1 << 19;                     // everything matches (a <= b always)
    return (int)ceilf(thr * 262144.0f);                    // (a power of two: exact, also for the denormal threshold of the radius 0)
}
// One accumulator register's matches leave: lanes 0 .. 31 hold rows 0 .. 31 of a tile against one query, lanes 32 .. 63 against another;
// out / cap are the lane's query's.  Per half: the keys compacted by ballot, ONE atomicAdd on the region's count, vector stores while
// they fit - the count keeps counting past cap (vg_within_flush's protocol).  All 64 lanes call it.
__device__ __forceinline__ void vgbb_within_emit(bool pass, uint64_t key, unsigned long long *out, unsigned long long cap, int lane) {
    const unsigned long long m = __ballot(pass);
    const uint32_t mh = (lane & 32) ? (uint32_t)(m >> 32) : (uint32_t)m;
    const uint32_t cnt = (uint32_t)__popc(mh), rank = (uint32_t)__popc(mh & ((1u << (lane & 31)) - 1u));
    unsigned long long base = 0ull;
    if ((lane & 31) == 0 && cnt) base = atomicAdd(out, (unsigned long long)cnt);
    base = __shfl(base, lane & 32);
    if (pass && base + rank < cap) out[1 + base + rank] = key;
}

// bits 0 .. 15 of v -> 16 bytes of 0 / 1, byte j of dword d = bit 4d + j
__device__ __forceinline__ vgb_i32x4 vgbb_spread16(uint32_t v) {
    vgb_i32x4 o;
    o[0] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 0, 4), 0x00204081u) & 0x01010101u);
    o[1] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 4, 4), 0x00204081u) & 0x01010101u);
    o[2] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 8, 4), 0x00204081u) & 0x01010101u);
    o[3] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 12, 4), 0x00204081u) & 0x01010101u);
    return o;
}
