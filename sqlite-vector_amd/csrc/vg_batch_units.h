// vg_batch_units.h - the host entry points of the batch kernel units, declared ONCE: vg_batch.hip, vg_batch_i8.hip, vg_batch_h.hip,
// vg_batch_hl.hip and vg_batch_q8.hip define them, vg_batch_api.hip (and vg_api.hip, for the row norms) calls them, and the units
// compiled several times from one source (build.py: -DVGI_TU_PRE, -DVGH_TU=, -DVGHL_TU=) call each other through them.  The caller
// and every defining unit include this header: with C linkage a parameter list that drifted would link and run, here it does not
// compile.  Launchers return 0 or a hipError_t (-1: the shape is not served) and only enqueue on `stream`.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define VG_BPAIR_CAP 2048               // candidate pairs per filter wavefront and stage (a batch that overflows one falls back to the fused kernel)
#define VG_BPAIR_CAP_LONG 8192          // ... of the long-row kernel (64 KB per region, 1024 regions: its fallback is one scan per query)

struct BatchArgsH;                      // vg_batch_h_defs.h
struct BatchArgsI8;                     // vg_batch_i8.hip

extern "C" {

// ---- vg_batch.hip: f32 rows on the f32 matrix cores; the merge every batch kernel ends its passes in; the f32 row norms
size_t vg_batch_lds_bytes(long long stride_bytes, int k);                   // 0: rows / k it does not serve
int vg_batch_lists_per_query(long long n_rows, int npart);
int vg_batch_launch(const float *dev_rows, long long n_rows, long long stride_bytes,
                    const float *dev_queries, int nq_pad, int nq_real, int k, int mode, int root,
                    const float *dev_xnorm, uint64_t *dev_cand, int npart, int tiles_per_part,
                    uint64_t *dev_out_keys, hipStream_t stream);
// per query: its lists in the candidate buffer -> the final k keys
int vg_batch_merge_launch(const uint64_t *dev_cand, int nq_pad, int lists_per_query, int npart, int k,
                          uint64_t *dev_out_keys, hipStream_t stream);
int vg_rownorm_launch(const float *dev_rows, long long row0, long long n, long long stride_bytes, float *dev_out,
                      hipStream_t stream);

// ---- vg_batch_i8.hip: uint8 / int8 rows on the integer matrix cores
size_t vg_batch_i8_lds_bytes(long long stride_bytes, int k);
int vg_batch_i8_queries_per_block(long long stride_bytes);
int vg_i8_rowstat_launch(const uint8_t *dev_rows, long long row0, long long n, long long stride, int is_u8,
                         uint32_t *dev_stat, uint8_t *dev_flipped, hipStream_t stream);
int vg_batch_i8_launch(const uint8_t *dev_rows_signed, long long n_rows, long long stride_bytes,
                       const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int mode, int root, int is_u8,
                       const uint32_t *dev_row_stat, uint64_t *dev_cand, int npart,
                       int tiles_per_part, uint64_t *dev_out_keys, hipStream_t stream);
int vgi_launch_pre(const BatchArgsI8 *a, int ntb, int blocks, size_t smem, hipStream_t stream);     // -DVGI_TU_PRE
int vgi_launch_real(const BatchArgsI8 *a, int ntb, int blocks, size_t smem, hipStream_t stream);

// ---- vg_batch_h.hip: f16 / bf16 rows (and f32 rows through their bf16 shadow copy) - matrix-core filter + exact re-evaluation;
// the conversion passes behind the derived copies of a corpus
size_t vg_batch_h_lds_bytes(long long stride_bytes, int k);
int vg_batch_h_queries_per_block(long long stride_bytes);
int vg_batch_h_plan(long long stride_bytes, int k, int nq, int *waves, int *blocks_per_cu);
int vg_batch_h_split(long long stride_bytes, int k);                        // the split form is on for such rows
int vg_batch_h_launch(const uint8_t *dev_rows, int rows_tiled, long long n_rows, long long stride_bytes, int dim, int type_code,
                      const uint8_t *dev_xrows, long long xstride_bytes,
                      const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int mode, int root,
                      const float *dev_row_nn, uint64_t *dev_cand, int npart, int tiles_per_part,
                      uint64_t *dev_out_keys, unsigned long long *dev_evals, int waves,
                      uint64_t *dev_pairs, uint32_t *dev_pair_counts, int pair_cap, hipStream_t stream);
int vg_tile_major_launch(const uint8_t *dev_rows, long long row0, long long n, long long stride, uint8_t *dev_out, hipStream_t stream);
int vg_f32_to_bf16_launch(const uint8_t *dev_rows, long long row0, long long n, long long stride, int dim,
                          uint8_t *dev_out, long long ostride, hipStream_t stream);
int vg_f32_to_bf16_tm_launch(const uint8_t *dev_rows, long long row0, long long n, long long stride, int dim,
                             uint8_t *dev_out, long long ostride, hipStream_t stream);
// its units: the real pass (f16: unit 0, bf16: -DVGH_TU=1, f32: 3), the bound pass (2, 4, 5), the split form's filter and exact
// kernels (6, 7, 8; vg_batch_q8.hip evaluates its pairs with the exact ones)
int vgh_launch_real_f16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_real_bf16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_real_f32(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_bound_f16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_bound_bf16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_bound_f32(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_filter_f16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_filter_bf16(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_filter_f32(const BatchArgsH *a, int ntb, int waves, int blocks, size_t smem, hipStream_t stream);
int vgh_launch_exact_f16(const BatchArgsH *a, int ntb, int waves, int regions, size_t smem, hipStream_t stream);
int vgh_launch_exact_bf16(const BatchArgsH *a, int ntb, int waves, int regions, size_t smem, hipStream_t stream);
int vgh_launch_exact_f32(const BatchArgsH *a, int ntb, int waves, int regions, size_t smem, hipStream_t stream);

// ---- vg_batch_hl.hip: rows of 1025 .. 3072 elements, the K dimension split over the wavefronts of a workgroup
int vg_batch_hl_serves(long long stride_bytes, int k);
int vg_batch_hl_queries_per_block(long long stride_bytes);
int vg_batch_hl_regions(long long stride_bytes, int nq_pad, int npart);
int vg_batch_hl_query_norms(const uint8_t *dev_queries, long long stride_bytes, int dim, int type_code, int nq_real, int nq_pad,
                            float *dev_out, hipStream_t stream);
int vg_batch_hl_launch(const uint8_t *dev_rows, long long n_rows, long long stride_bytes, int dim, int type_code,
                       const uint8_t *dev_xrows, long long xstride_bytes,
                       const uint8_t *dev_queries, int nq_pad, int nq_real, int k, int mode, int root,
                       const float *dev_row_nn, const float *dev_query_nn, uint64_t *dev_cand, int npart,
                       uint64_t *dev_out_keys, unsigned long long *dev_evals,
                       uint64_t *dev_pairs, uint32_t *dev_pair_counts, int pair_cap, hipStream_t stream);
// its units: bound f16 (-DVGHL_TU=0, + the entry points), filter f16 (1, + the exact kernels), bound / filter bf16 (2, 3), f32 (4, 5)
int vghl_bound_f16(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_filter_f16(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_bound_bf16(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_filter_bf16(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_bound_f32(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_filter_f32(const BatchArgsH *a, int ntbp, int blocks, size_t smem, hipStream_t stream);
int vghl_exact_f16(const BatchArgsH *a, int sets, int blocks, size_t smem, hipStream_t stream);
int vghl_exact_bf16(const BatchArgsH *a, int sets, int blocks, size_t smem, hipStream_t stream);
int vghl_exact_f32(const BatchArgsH *a, int sets, int blocks, size_t smem, hipStream_t stream);
// (vg_batch_q8.hip's pairs over rows beyond 4 KiB f32 / 2 KiB f16 - bf16, where vgh_launch_exact_* has too few chunks per lane:
//  `waves` 32-query regions per query group, one region per block)
int vghl_exact_regions_f16(const BatchArgsH *a, int waves, int regions, size_t smem, hipStream_t stream);
int vghl_exact_regions_bf16(const BatchArgsH *a, int waves, int regions, size_t smem, hipStream_t stream);
int vghl_exact_regions_f32(const BatchArgsH *a, int waves, int regions, size_t smem, hipStream_t stream);

// ---- vg_batch_q8.hip: the integer matrix cores as the filter over the tile-major int8 shadow copy
int vg_batch_q8_serves(long long q8stride_bytes, long long xstride_bytes, int k);
int vg_batch_q8_queries_per_block(void);
int vg_batch_q8_workgroups_per_cu(long long q8stride_bytes);
int vg_batch_q8_padded_queries(int nq, long long q8stride_bytes);
int vg_batch_q8_max_partitions(void);
int vg_batch_q8_max_queries(void);
int vg_batch_q8_regions(int nq_pad, int npart);
size_t vg_batch_q8_work_bytes(int nq_pad, long long q8stride_bytes, long long xstride_bytes);
size_t vg_batch_q8_work_stat_offset(int nq_pad, long long q8stride_bytes, long long xstride_bytes);
size_t vg_batch_q8_work_perm_offset(int nq_pad, long long q8stride_bytes, long long xstride_bytes);
int vg_q8_rstat_launch(const void *dev_q8stat, const float *dev_xnorm, long long row0, long long n, void *dev_out, int nn_squared, hipStream_t stream);
int vg_batch_q8_launch(const uint8_t *dev_rows_tm, const void *dev_rstat, long long n_rows, long long q8stride, int dim,
                       const uint8_t *dev_xrows, long long xstride, const float *dev_xnorm,
                       const uint8_t *dev_xqueries, void *dev_qwork, int nq_pad, int nq_real, int k, int mode, int root,
                       uint64_t *dev_cand, int npart, uint64_t *dev_out_keys, unsigned long long *dev_evals,
                       uint64_t *dev_pairs, uint32_t *dev_pair_counts, int pair_cap, int type_code, hipStream_t stream);
size_t vg_batch_q8_pack_bytes(int nq_pad, int k);
int vg_batch_q8_pack_launch(const uint64_t *dev_keys, const void *dev_qwork, int nq_pad, long long q8stride, long long xstride, int k,
                            const uint32_t *dev_overflow_flag, const unsigned long long *dev_evals, void *dev_out, hipStream_t stream);

}   // extern "C"
