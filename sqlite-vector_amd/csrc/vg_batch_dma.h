// vg_batch_dma.h - the device-side primitives of the matrix-core batch kernels (vg_batch.hip, vg_batch_h.hip, vg_batch_hl.hip,
// vg_batch_i8.hip, vg_batch_q8.hip): register vector types, B-operand LDS reads with counted waits, 64-bit DPP minima, the LDS-DMA
// instructions behind every kernel's dma_piece / dma_run / dma_stat_group, and the timing builds' tick macro.  Included through
// vg_batch_common.h.  Everything here is forced inline: a kernel that calls it generates the code it generated with the asm in place.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vg_device.h"

typedef int vgb_i32x4 __attribute__((ext_vector_type(4)));
typedef int vgb_i32x16 __attribute__((ext_vector_type(16)));
typedef float vgb_f32x4 __attribute__((ext_vector_type(4)));
typedef float vgb_f32x16 __attribute__((ext_vector_type(16)));

// VGB_TICK(VGI_TIMING, t0): `const unsigned long long t0 = <shader clock>` in a file's timing build (its *_TIMING switch is 1), nothing
// otherwise (0)
#define VGB_TICK_0(var)
#define VGB_TICK_1(var) const unsigned long long var = __builtin_readcyclecounter()
#define VGB_TICK_ON(on, var) VGB_TICK_##on(var)
#define VGB_TICK(on, var) VGB_TICK_ON(on, var)

// ---- the B operand: one ds_read_b128 per MFMA, issued several k-steps ahead of its use
// (free functions: clang rejects asm operands that name captured variables inside a generic lambda)
template <int OFF, typename V4>
__device__ __forceinline__ void vgb_lds_read128(V4 &dst, uint32_t lds_addr) {
    static_assert(sizeof(V4) == 16, "four 32-bit registers");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(lds_addr), "n"(OFF) : "memory");
}
template <int N, typename V4>
__device__ __forceinline__ void vgb_wait_lds(V4 &v) {               // v is usable once at most N later LDS reads are in flight
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N));
}

template <int CTRL> __device__ __forceinline__ uint64_t vgb_dpp64(uint64_t v) {
    return ((uint64_t)vg_dpp_u32<CTRL>((uint32_t)(v >> 32)) << 32) | vg_dpp_u32<CTRL>((uint32_t)v);
}
__device__ __forceinline__ uint64_t vgb_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- LDS-DMA: global_load_lds_dwordx4 moves 16 bytes per lane from  sbase (SGPR pair) + lane_goff (VGPR) [+ offset]  to LDS byte
// M0 + 16 * lane [+ offset]; lanes switched off in EXEC move nothing.  M0 (and EXEC, where a mask applies) are saved and restored
// around the instruction; an instruction must stand between the write of M0 and the load that reads it (the s_nop, or the EXEC set-up).
// From inline asm because the compiler's waitcnt pass does not see these loads: it cannot put "s_waitcnt vmcnt(0)" in front of every
// ds_read of the CURRENT tile while the NEXT one is in flight.  The callers wait for completion themselves (s_waitcnt vmcnt).
// sbase, lds_dst and exec_mask are "s" operands: they must be wave-uniform AND the compiler must know it.  The per-kernel lambdas that
// call these (dma_piece, dma_run, dma_share, dma_tile, dma_stat_group) have to inline into the kernel - a lambda left as a real
// function receives what it captures through memory, the tile counter becomes a VGPR and the "s" operands no longer assemble.  A
// kernel large enough for the compiler's heuristics to decide otherwise (vg_batch_h.hip) marks every lambda always_inline.
#define VGB_DMA_FIRST "global_load_lds_dwordx4 %1, %2\n\t"
#define VGB_DMA_NEXT(off) "global_load_lds_dwordx4 %1, %2 offset:" #off "\n\t"
#define VGB_DMA_RUN(loads) "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" loads "s_mov_b32 m0, %0"

// N (1 .. 4) whole 1-KiB pieces that are contiguous in memory and in LDS, back to back under one M0 set-up (the instruction offset
// moves the global and the LDS address alike), all lanes
template <int N>
__device__ __forceinline__ void vgb_dma_run(uint32_t lane_goff, const uint8_t *sbase, uint32_t lds_dst) {
    static_assert(N >= 1 && N <= 4, "one to four pieces per M0 set-up");
    uint32_t keep;
    if constexpr (N == 1)
        asm volatile(VGB_DMA_RUN(VGB_DMA_FIRST) : "=&s"(keep) : "v"(lane_goff), "s"(sbase), "s"(lds_dst) : "memory");
    else if constexpr (N == 2)
        asm volatile(VGB_DMA_RUN(VGB_DMA_FIRST VGB_DMA_NEXT(1024)) : "=&s"(keep) : "v"(lane_goff), "s"(sbase), "s"(lds_dst) : "memory");
    else if constexpr (N == 3)
        asm volatile(VGB_DMA_RUN(VGB_DMA_FIRST VGB_DMA_NEXT(1024) VGB_DMA_NEXT(2048))
                     : "=&s"(keep) : "v"(lane_goff), "s"(sbase), "s"(lds_dst) : "memory");
    else
        asm volatile(VGB_DMA_RUN(VGB_DMA_FIRST VGB_DMA_NEXT(1024) VGB_DMA_NEXT(2048) VGB_DMA_NEXT(3072))
                     : "=&s"(keep) : "v"(lane_goff), "s"(sbase), "s"(lds_dst) : "memory");
}
#undef VGB_DMA_FIRST
#undef VGB_DMA_NEXT
#undef VGB_DMA_RUN

// one piece under a lane mask: the lanes of exec_mask move their 16 bytes, the others nothing - no branch, so a k loop that issues it
// stays ONE basic block and the scheduler can keep the B-operand reads several MFMAs ahead of their use
__device__ __forceinline__ void vgb_dma_masked(uint32_t lane_goff, const uint8_t *sbase, uint32_t lds_dst, uint64_t exec_mask) {
    uint32_t keep;
    uint64_t keep_exec;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %4\n\ts_and_b64 exec, exec, %5\n\t"
                 "global_load_lds_dwordx4 %2, %3\n\ts_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(keep_exec) : "v"(lane_goff), "s"(sbase), "s"(lds_dst), "s"(exec_mask) : "memory", "scc");
}
// the same with EXEC set up before M0 and an s_nop behind it: what vg_batch_h.hip's dma_stat_group has always issued.  Kept as a
// variant of its own because folding it into vgb_dma_masked would change that kernel family's instruction stream.
__device__ __forceinline__ void vgb_dma_masked_exec_first(uint32_t lane_goff, const uint8_t *sbase, uint32_t lds_dst, uint64_t exec_mask) {
    uint32_t keep;
    uint64_t keep_exec;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_and_b64 exec, exec, %5\n\t"
                 "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\t"
                 "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(keep_exec) : "v"(lane_goff), "s"(sbase), "s"(lds_dst), "s"(exec_mask) : "memory", "scc");
}
