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

// bits 0 .. 15 of v -> 16 bytes of 0 / 1, byte j of dword d = bit 4d + j
__device__ __forceinline__ vgb_i32x4 vgbb_spread16(uint32_t v) {
    vgb_i32x4 o;
    o[0] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 0, 4), 0x00204081u) & 0x01010101u);
    o[1] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 4, 4), 0x00204081u) & 0x01010101u);
    o[2] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 8, 4), 0x00204081u) & 0x01010101u);
    o[3] = (int)(__umul24(__builtin_amdgcn_ubfe(v, 12, 4), 0x00204081u) & 0x01010101u);
    return o;
}
