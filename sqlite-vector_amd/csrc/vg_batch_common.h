// vg_batch_common.h - what the matrix-core batch kernels share (vg_batch.hip: f32, vg_batch_h.hip / vg_batch_hl.hip: f16 / bf16 and f32
// behind a bf16 filter, vg_batch_i8.hip: uint8 / int8, vg_batch_q8.hip: f32 behind an int8 filter): the compile-time loop and the list
// insert of the kernels, the device-side primitives of vg_batch_dma.h, and the host side - row-length buckets, the kernel launch, the
// merge, the staged-pass driver.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vg_batch_dma.h"
#include "vg_batch_units.h"
#include "vg_lists.h"
#include "vg_switches.h"

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [I0, N)  (a plain "#pragma unroll" gives up on the
// kernels' k loops and demotes the register-resident operands to scratch)
template <int I, int N, typename F>
__device__ __forceinline__ void vgb_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        vgb_static_for<I + 1, N>(f);
    }
}

// One candidate key into a sorted per-query list of k keys in LDS (lane i of the wavefront owns slot i, k <= 64), one
// LDS round trip: a key that does not beat the tail changes nothing.  `c` is wave-uniform.  Returns the new k-th key.
__device__ __forceinline__ uint64_t vgb_list_insert(uint64_t *list, int k, int lane, uint64_t c) {
    uint64_t mine = (lane < k) ? list[lane] : 0ull;
    const uint64_t prev = vg_wave_shr1(mine);
    mine = (mine > c) ? ((prev > c) ? prev : c) : mine;
    if (lane < k) list[lane] = mine;
    return vg_readlane64(mine, k - 1);
}

// the distance a list's k-th key stands for; a list that is not full yet accepts everything
__device__ __forceinline__ float vgb_kth_distance(uint64_t kth) {
    return (kth == VG_EMPTY_KEY) ? INFINITY : vg_sortable_f32((uint32_t)(kth >> 32));
}

// ---- STAGED REAL PASSES (host side).  A two-pass launch starts every list of the real pass at the query's k-th best of a
// pre-pass over 1/32 of the rows: ~k * 32 rows per query still beat that threshold in the real pass (655k slow-path entries
// for 1024 queries x 10M rows), and each of them holds its workgroup at a tile barrier.  The real pass therefore runs in
// STAGES over growing row ranges [0, 2P), [2P, 4P), [4P, 8P) ... (P = the pre-pass rows): the lists are merged after every
// stage and the next one starts from the query's k-th best over ALL rows scanned so far - a stage that doubles the scanned
// range lets ~k rows per query through, ~6k per query in all instead of 32k.  From the second stage on, partition 0 of a
// query group seeds its lists with the merged keys (they stand for rows of EARLIER stages, which no later stage meets again),
// so every stage writes - and every merge reads - the same npart lists per query.
// bounds[0 .. n]: stage i scans tiles [bounds[i], bounds[i+1]); returns n.  growth_pct: VG_BATCH_STAGES (200 = doubling,
// 0 = one real pass over everything), else the caller's default.
// Round 3 re-measured both knobs on the kernels as they are now (tile-major copies, tile-minimum pre-pass, staged passes;
// tools/batch_knob_sweep.py, profiles/r4h_batch_knob_sweeps.jsonl): the pre-pass wants to be SMALL - 1/512 of the rows instead of
// 1/32 - because the staged passes do the warming-up more cheaply than a longer pre-pass does: 1024 x 10M, f32 through the bf16
// filter 10.54 -> 8.95 ms, f16 dot 9.92 -> 8.68, bf16 cosine 10.03 -> 8.43, uint8 cosine 9.01 -> 7.61, uint8 dot 7.61 -> 6.57,
// int8 L2 7.70 -> 6.61; 256 queries 3.12 -> 2.72 (f32) / 2.70 -> 2.24 (uint8).  Growth: doubling for the half-precision kernel
// with several query groups (its exact evaluations are the expensive part), x4 otherwise (fewer launches).
#include <cstdlib>
#define VGB_PREPASS_DENOM_DEFAULT 512
static inline int vgb_stage_bounds(long long ntiles, long long pre_tiles, long long *bounds, int max_stages, int default_growth_pct = 400) {
    const int growth_pct = vg_sw(SW_VG_BATCH_STAGES, default_growth_pct);
    int n = 0;
    bounds[0] = 0;
    if (pre_tiles > 0 && growth_pct > 100) {
        long long b = 2 * pre_tiles;
        while (b < ntiles && n + 2 < max_stages && ntiles - b > b / 4) {      // (no sliver at the end)
            bounds[++n] = b;
            b = b * growth_pct / 100;
        }
    }
    bounds[++n] = ntiles;
    return n;
}

// ---- the rest of the host side (the merge of a query's lists: vg_batch_merge_launch, vg_batch_units.h)
// the k-step counts (32 bytes of a row each) the kernels with 64-k-step register files are instantiated for; 0: not served
static inline int vgb_ksteps(long long stride_bytes) { return (int)((stride_bytes + 31) / 32); }
static inline int vgb_ntb64(long long stride_bytes) {
    const int ntb = vgb_ksteps(stride_bytes);
    if (ntb <= 8) return 8;
    if (ntb <= 16) return 16;
    if (ntb <= 24) return 24;
    if (ntb <= 32) return 32;
    if (ntb <= 48) return 48;                                     // rows of 1 - 2 KiB: 4-wavefront workgroups
    if (ntb <= 64) return 64;
    return 0;
}

// one kernel launch with `smem` bytes of dynamic LDS (the kernel's limit is raised to it first); 0 or a hipError_t
template <typename Kernel, typename Args>
static inline int vgb_launch(Kernel kernel, int blocks, int threads, size_t smem, hipStream_t stream, const Args &args) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)threads), smem, stream, args);
    return (int)hipGetLastError();
}

// The pre-pass over tiles [0, pre) (pre == 0: none), then the staged real passes above: every pass writes - and every merge reads -
// lists 0 .. a.npart - 1 of a query; a stage after the first starts from the merged keys (a.seed, a.init_keys).  launch_pre(a) /
// launch_stage(a) launch one pass over [a.tile_begin, a.tile_end) - one kernel, or filter then exact evaluation.  How large `pre` is
// stays with the caller: the kernels differ there on purpose.
template <typename Args, typename LaunchPre, typename LaunchStage>
static inline int vgb_run_staged(Args &a, long long ntiles, long long pre, int default_growth_pct, uint64_t *dev_out_keys, hipStream_t stream,
                                 LaunchPre launch_pre, LaunchStage launch_stage) {
    const int npart = a.npart;
    int rc;
    a.npart_total = npart; a.part_base = 0; a.seed = 0; a.init_keys = nullptr;
    if (pre > 0) {
        a.tile_begin = 0; a.tile_end = pre; a.tiles_per_part = (int)((pre + npart - 1) / npart);
        if ((rc = launch_pre(a)) != 0) return rc;
        if ((rc = vg_batch_merge_launch(a.cand, a.nq_pad, a.npart_total, npart, a.k, dev_out_keys, stream)) != 0) return rc;
        a.init_keys = dev_out_keys;
    }
    long long bounds[16];
    const int nstages = vgb_stage_bounds(ntiles, pre, bounds, 16, default_growth_pct);
    for (int s = 0; s < nstages; ++s) {
        a.tile_begin = bounds[s]; a.tile_end = bounds[s + 1];
        a.tiles_per_part = (int)((a.tile_end - a.tile_begin + npart - 1) / npart);
        a.seed = (s > 0) ? 1 : 0;
        if ((rc = launch_stage(a)) != 0) return rc;
        if ((rc = vg_batch_merge_launch(a.cand, a.nq_pad, a.npart_total, npart, a.k, dev_out_keys, stream)) != 0) return rc;
        a.init_keys = dev_out_keys;
    }
    return 0;
}
