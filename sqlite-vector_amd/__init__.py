"""sqlite-vector_amd: MI355X-native brute-force distance scan + top-k behind sqlite-vector's SQL surface.

This Python module is plumbing only: it builds and loads the two native artefacts and exposes a thin ctypes
view of the C-ABI (include/vectorgpu.h) for tests and bench.py.  The product is

    libvectorgpu.so   HIP kernels + C-ABI                     (csrc/*.hip, hipcc --offload-arch=gfx950)
    vector.so         the SQLite loadable extension, plain C  (ext/vector_ext.c; exports sqlite3_vector_init)

Nothing here computes a distance: without the HIP library / a GPU every call raises.  The package never imports
anything from oracle/ (that is test infrastructure).

The directory name contains a '-', so load it with importlib (see __graft_entry__.load_package) or put the repo
root on sys.path and use importlib.import_module("sqlite-vector_amd").
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VG_LIB_PATH") or os.path.join(HERE, "libvectorgpu.so")   # override: A/B kernel builds
EXT_PATH = os.path.join(HERE, "vector.so")         # must be named vector.* (entry point sqlite3_vector_init)

# enums (same numbering as the reference, distance-cpu.h:36-58)
F32, F16, BF16, U8, I8 = 1, 2, 3, 4, 5
L2, SQUARED_L2, COSINE, DOT, L1 = 1, 2, 3, 4, 5
HAMMING = 6                  # not a metric of the reference: differing bits of packed bit vectors, U8 corpora only (pack_bits)
JACCARD = 7                  # not a metric of the reference either: 1 - |q AND x| / |q OR x| of packed bit vectors, U8 corpora only
TANIMOTO = JACCARD           # (the same distance under its other name)
QUANT_U8, QUANT_S8 = 1, 2
TIE_POSITION, TIE_REFERENCE = 0, 1
KEY_EMPTY = 0xFFFFFFFFFFFFFFFF
HALF_TYPES = True            # f16 / bf16 scan kernels are built in
TYPE_SIZE = {F32: 4, F16: 2, BF16: 2, U8: 1, I8: 1}


class VectorGpuError(RuntimeError):
    pass


_lib = None


# The engine reads its VG_* environment switches when the library is loaded and whenever a corpus / shard set is created - not per query
# (csrc/vg_switches.h).  Tests and tools flip switches between two calls on one corpus: with AUTO_RELOAD every call through this module
# re-reads them first (a few microseconds); bench.py turns it off and calls reload_switches() where it changes the environment.
AUTO_RELOAD = True


def reload_switches():
    _load().vg_reload_switches()


def lib():
    L = _load()
    if AUTO_RELOAD:
        L.vg_reload_switches()
    return L


def _load():
    """Load libvectorgpu.so (fails loudly if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VectorGpuError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    sig = {
        "vg_device_count": (i32, []),
        "vg_backend_name": (C.c_char_p, []),
        "vg_last_error": (C.c_char_p, []),
        "vg_corpus_create": (i32, [i32, i32, i32, i64, C.POINTER(vp)]),
        "vg_corpus_destroy": (None, [vp]),
        "vg_corpus_clear": (i32, [vp]),
        "vg_corpus_reserve": (i32, [vp, i64]),
        "vg_corpus_trim": (i32, [vp]),
        "vg_corpus_clone": (i32, [vp, vp]),
        "vg_shards_clone": (i32, [vp, vp]),
        "vg_shards_trim": (i32, [vp]),
        "vg_corpus_rows": (i64, [vp]),
        "vg_corpus_dim": (i32, [vp]),
        "vg_corpus_type": (i32, [vp]),
        "vg_corpus_device": (i32, [vp]),
        "vg_corpus_hbm_bytes": (i64, [vp]),
        "vg_corpus_set_rowid_base": (i32, [vp, i64]),
        "vg_corpus_append": (i32, [vp, vp, i64, i64, vp]),
        "vg_corpus_append_records": (i32, [vp, vp, i64]),
        "vg_corpus_append_device": (i32, [vp, vp, i64, i64, vp]),
        "vg_scan_topk": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_device": (i32, [vp, i32, vp, i32, vp, vp]),
        "vg_key_distance": (C.c_float, [C.c_uint64]),
        "vg_key_position": (C.c_uint32, [C.c_uint64]),
        "vg_merge_keys": (i32, [vp, i32, i32, vp, i32, vp, vp]),
        "vg_scan_topk_keys": (i32, [vp, i32, vp, i32, vp, C.POINTER(i32)]),
        "vg_scan_topk_enqueue": (i32, [vp, i32, vp, i32]),
        "vg_scan_topk_collect": (i32, [vp, vp]),
        "vg_scan_topk_batch_keys": (i32, [vp, i32, vp, i32, i32, vp, vp]),
        "vg_shards_create": (i32, [vp, i32, i32, i32, i64, C.POINTER(vp)]),
        "vg_shards_destroy": (None, [vp]),
        "vg_shards_clear": (i32, [vp]),
        "vg_shards_count": (i32, [vp]),
        "vg_shards_rows": (i64, [vp]),
        "vg_shards_shard": (vp, [vp, i32]),
        "vg_shards_reserve": (i32, [vp, i64]),
        "vg_shards_set_rowid_base": (i32, [vp, i64]),
        "vg_shards_append": (i32, [vp, vp, i64, i64, vp]),
        "vg_shards_append_records": (i32, [vp, vp, i64]),
        "vg_shards_rowid_at": (i64, [vp, i64]),
        "vg_shards_scan_topk": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_batch": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_shards_scan_distances": (i32, [vp, i32, vp, vp]),
        "vg_shards_minmax": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]),
        "vg_shards_quantize_rows": (i32, [vp, C.c_float, C.c_float, i32, i64, i64, vp]),
        "vg_merge_keys_batch": (i32, [vp, i32, i32, i32, vp, i32, vp, vp, vp]),
        "vg_scan_distances": (i32, [vp, i32, vp, vp]),
        "vg_scan_distances_device": (i32, [vp, i32, vp, vp, vp]),
        "vg_corpus_rowid_at": (i64, [vp, i64]),
        "vg_scan_topk_batch": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_quantize_query": (i32, [i32, vp, i32, C.c_float, C.c_float, i32, vp]),
        "vg_corpus_minmax": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i32)]),
        "vg_corpus_quantize_rows": (i32, [vp, C.c_float, C.c_float, i32, i64, i64, vp]),
        "vg_set_profiling": (i32, [vp, i32]),
        "vg_last_kernel_ms": (i32, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "vg_profile_mean_ms": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "vg_scan_kernel_name": (C.c_char_p, [vp, i32]),
        "vg_plan_scan_shape": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_batch_h_plan": (i32, [i64, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "vg_profile_mean_ms_ex": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "vg_corpus_find_rowid": (i64, [vp, i64]),
        "vg_corpus_patch_rows": (i32, [vp, vp, i64, vp, i64]),
        "vg_corpus_delete_rows": (i32, [vp, vp, i64]),
        "vg_shards_find_rowid": (i64, [vp, i64]),
        "vg_shards_patch_rows": (i32, [vp, vp, i64, vp, i64]),
        "vg_shards_delete_rows": (i32, [vp, vp, i64]),
        "vg_filter_exact_evals": (i32, [vp, C.POINTER(C.c_ulonglong)]),
        "vg_filter_guard_cooldown": (i32, [vp]),
        "vg_batch_filter_exact_evals": (i32, [vp, C.POINTER(C.c_ulonglong)]),
        "vg_reload_switches": (None, []),
        "vg_batch_last_path": (i32, [vp]),
        "vg_batch_q8_status": (i32, [vp]),
        "vg_batch_h_split_off": (i32, [vp]),
        "vg_corpus_set_scan_filter": (i32, [vp, i32]),
        "vg_corpus_set_tie_order": (i32, [vp, i32]),
        "vg_corpus_tie_order": (i32, [vp]),
        "vg_corpus_tie_stats": (i32, [vp, vp]),
        "vg_corpus_pass_ms": (i32, [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_longlong)]),
        "vg_shards_set_tie_order": (i32, [vp, i32]),
        "vg_shards_set_scan_filter": (i32, [vp, i32]),
        "vg_shards_set_gather": (i32, [vp, i32]),
        "vg_shards_gather_stats": (i32, [vp, vp]),
        "vg_shards_tie_stats": (i32, [vp, vp]),
        "vg_shards_threaded": (i32, [vp]),
        "vg_slab_scan_begin": (i32, [i32, i32, i32, i32, vp, i32, i32, i64, i64, vp]),
        "vg_slab_scan_rows": (i32, [vp, vp, i64, i64, vp]),
        "vg_slab_scan_records": (i32, [vp, vp, i64]),
        "vg_slab_scan_finish": (i32, [vp, vp, vp, vp]),
        "vg_slab_scan_all": (i32, [vp, vp, vp, vp]),
        "vg_slab_scan_destroy": (None, [vp]),
        "vg_device_memory": (i32, [i32, vp, vp]),
        "vg_host_alloc": (i32, [C.c_size_t, C.POINTER(C.c_void_p)]),
        "vg_host_free": (None, [vp]),
        "vg_corpus_device_bytes": (i32, [vp, vp]),
        "vg_shards_device_bytes": (i32, [vp, vp]),
        "vg_shards_rowids": (i32, [vp, i64, i64, vp]),
        "vg_scan_topk_reference": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_stat_rows_appended": (C.c_longlong, []),
        "vg_reference_topk_replay": (i32, [vp, i64, i32, i64, vp, vp]),
        "vg_reference_topk_replay_slabs": (i32, [vp, i64, i32, i64, i64, vp, vp]),
        "vg_scan_distances_resident": (i32, [vp, i32, vp]),
        "vg_resident_distances_fetch": (i32, [vp, i64, i64, vp]),
        "vg_resident_distances_below": (i32, [vp, i64, C.c_float, vp, i64, C.POINTER(i64)]),
        "vg_scan_within": (i32, [vp, i32, vp, C.c_double, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_within_fetch": (i32, [vp, i64, i64, vp, vp]),
        "vg_scan_within_keys": (i32, [vp, i64, i64, vp]),
        "vg_shards_scan_within": (i32, [vp, i32, vp, C.c_double, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_shards_scan_within_fetch": (i32, [vp, i64, i64, vp, vp]),
        "vg_scan_within_masked": (i32, [vp, i32, vp, C.c_double, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_shards_scan_within_masked": (i32, [vp, i32, vp, C.c_double, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_within_batch_masked": (i32, [vp, i32, vp, i32, vp, i64, vp, vp]),
        "vg_shards_scan_within_batch_masked": (i32, [vp, i32, vp, i32, vp, i64, vp, vp]),
        "vg_within_batch_masked_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_within_batch_masked_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        # labeled range scans: every row of a label (of a set of labels) within a distance; the batch: a label and a radius per query
        "vg_scan_within_labeled": (i32, [vp, i32, vp, C.c_double, i64, C.c_uint32, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_within_labelset": (i32, [vp, i32, vp, C.c_double, i64, vp, i64, i32, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_within_batch_labeled": (i32, [vp, i32, vp, i32, vp, vp, i64, vp, vp]),
        "vg_within_batch_labeled_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_scan_within_labeled": (i32, [vp, i32, vp, C.c_double, i64, C.c_uint32, C.POINTER(i64), C.POINTER(i64)]),
        "vg_shards_scan_within_labelset": (i32, [vp, i32, vp, C.c_double, i64, vp, i64, i32, C.POINTER(i64), C.POINTER(i64)]),
        "vg_shards_scan_within_batch_labeled": (i32, [vp, i32, vp, i32, vp, vp, i64, vp, vp]),
        "vg_shards_within_batch_labeled_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_within_set_initial_capacity": (i32, [vp, i64]),
        "vg_within_last_launches": (i32, [vp]),
        "vg_shards_within_set_initial_capacity": (i32, [vp, i64]),
        "vg_shards_within_last_launches": (i32, [vp]),
        "vg_corpus_set_mask_bits": (i32, [vp, vp, i64]),
        "vg_corpus_set_mask_rowids": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "vg_corpus_clear_mask": (i32, [vp]),
        "vg_corpus_mask_count": (i64, [vp]),
        "vg_scan_topk_masked": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_masked_keys": (i32, [vp, i32, vp, i32, vp, C.POINTER(i32)]),
        "vg_shards_set_mask_bits": (i32, [vp, vp, i64]),
        "vg_shards_set_mask_rowids": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "vg_shards_clear_mask": (i32, [vp]),
        "vg_shards_mask_count": (i64, [vp]),
        "vg_shards_scan_topk_masked": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_batch_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_scan_topk_batch_masked_keys": (i32, [vp, i32, vp, i32, i32, vp, vp]),
        "vg_shards_scan_topk_batch_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_batch_masked_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        # labeled scans: a uint32 label per row on the handle, each query names one
        "vg_corpus_set_labels": (i32, [vp, vp, i64]),
        "vg_corpus_clear_labels": (i32, [vp]),
        "vg_corpus_has_labels": (i32, [vp]),
        "vg_scan_topk_labeled": (i32, [vp, i32, vp, i32, C.c_uint32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_labeled_keys": (i32, [vp, i32, vp, i32, C.c_uint32, vp, C.POINTER(i32)]),
        "vg_scan_topk_batch_labeled": (i32, [vp, i32, vp, i32, vp, i32, vp, vp, vp]),
        "vg_scan_topk_batch_labeled_keys": (i32, [vp, i32, vp, i32, vp, i32, vp, vp]),
        "vg_batch_labeled_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_set_labels": (i32, [vp, vp, i64]),
        "vg_shards_clear_labels": (i32, [vp]),
        "vg_shards_has_labels": (i32, [vp]),
        "vg_shards_scan_topk_labeled": (i32, [vp, i32, vp, i32, C.c_uint32, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_batch_labeled": (i32, [vp, i32, vp, i32, vp, i32, vp, vp, vp]),
        # grouped scans: the k nearest labels, each by its best row
        "vg_scan_topk_grouped": (i32, [vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_keys": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_masked": (i32, [vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_masked_keys": (i32, [vp, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_merge_keys_grouped": (i32, [vp, vp, i32, i32, vp, i32, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_grouped": (i32, [vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_grouped_masked": (i32, [vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32)]),
        # grouped batch scans: the same for many queries, in shared passes
        "vg_scan_topk_batch_grouped": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "vg_scan_topk_batch_grouped_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_scan_topk_batch_grouped_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "vg_scan_topk_batch_grouped_masked_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, vp]),
        "vg_shards_scan_topk_batch_grouped": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "vg_shards_scan_topk_batch_grouped_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp]),
        "vg_batch_grouped_plan": (i32, [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        # capped scans: the k nearest rows, at most per_label of one label
        "vg_scan_topk_capped": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_masked_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]),
        "vg_merge_keys_capped": (i32, [vp, vp, i32, i32, vp, i32, i32, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_capped": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_capped_masked": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, C.POINTER(i32)]),
        # capped batch scans: the same for many queries, in shared passes
        "vg_scan_topk_batch_capped": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "vg_scan_topk_batch_capped_keys": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp]),
        "vg_scan_topk_batch_capped_masked": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "vg_scan_topk_batch_capped_masked_keys": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp]),
        "vg_shards_scan_topk_batch_capped": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "vg_shards_scan_topk_batch_capped_masked": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "vg_batch_capped_plan": (i32, [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        # label-set scans: the labeled / grouped / capped scans over the rows whose label is in (exclude: not in) a set of labels
        "vg_scan_topk_labelset": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_labelset_keys": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_labelset": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_labelset_keys": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_labelset": (i32, [vp, i32, vp, i32, i32, vp, i64, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_labelset_keys": (i32, [vp, i32, vp, i32, i32, vp, i64, i32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_batch_labelset": (i32, [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp]),
        "vg_scan_topk_batch_labelset_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp]),
        "vg_batch_labelset_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_scan_topk_labelset": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_batch_labelset": (i32, [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp]),
        "vg_shards_scan_topk_grouped_labelset": (i32, [vp, i32, vp, i32, vp, i64, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_topk_capped_labelset": (i32, [vp, i32, vp, i32, i32, vp, i64, i32, vp, vp, vp, C.POINTER(i32)]),
        "vg_corpus_set_values": (i32, [vp, vp, i64]),
        "vg_corpus_clear_values": (i32, [vp]),
        "vg_corpus_has_values": (i32, [vp]),
        "vg_shards_set_values": (i32, [vp, vp, i64]),
        "vg_shards_clear_values": (i32, [vp]),
        "vg_shards_has_values": (i32, [vp]),
        "vg_scan_topk_valued": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_valued_keys": (i32, [vp, i32, vp, i32, i64, i64, vp, C.POINTER(i32)]),
        "vg_scan_topk_valued_labeled": (i32, [vp, i32, vp, i32, i64, i64, C.c_uint32, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_valued_labeled_keys": (i32, [vp, i32, vp, i32, i64, i64, C.c_uint32, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_valued": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_grouped_valued_keys": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_valued": (i32, [vp, i32, vp, i32, i32, i64, i64, vp, vp, vp, C.POINTER(i32)]),
        "vg_scan_topk_capped_valued_keys": (i32, [vp, i32, vp, i32, i32, i64, i64, vp, vp, C.POINTER(i32)]),
        "vg_scan_within_valued": (i32, [vp, i32, vp, C.c_double, i64, i64, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_topk_batch_valued": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
        "vg_scan_topk_batch_valued_keys": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]),
        "vg_batch_valued_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_valued_scan_topk": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, C.POINTER(i32)]),
        "vg_shards_valued_scan_topk_labeled": (i32, [vp, i32, vp, i32, i64, i64, C.c_uint32, vp, vp, C.POINTER(i32)]),
        "vg_shards_valued_scan_topk_batch": (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
        "vg_shards_valued_scan_topk_grouped": (i32, [vp, i32, vp, i32, i64, i64, vp, vp, vp, C.POINTER(i32)]),
        "vg_shards_valued_scan_topk_capped": (i32, [vp, i32, vp, i32, i32, i64, i64, vp, vp, vp, C.POINTER(i32)]),
        "vg_shards_scan_within_valued": (i32, [vp, i32, vp, C.c_double, i64, i64, i64, C.POINTER(i64), C.POINTER(i64)]),
        "vg_scan_within_batch": (i32, [vp, i32, vp, i32, vp, i64, vp, vp]),
        "vg_scan_within_batch_fetch": (i32, [vp, i32, i64, i64, vp, vp]),
        "vg_scan_within_batch_keys": (i32, [vp, i32, i64, i64, vp]),
        "vg_shards_scan_within_batch": (i32, [vp, i32, vp, i32, vp, i64, vp, vp]),
        "vg_shards_scan_within_batch_fetch": (i32, [vp, i32, i64, i64, vp, vp]),
        "vg_within_batch_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_within_batch_set_initial_capacity": (i32, [vp, i64]),
        "vg_within_batch_last_launches": (i32, [vp]),
        "vg_shards_within_batch_plan": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "vg_shards_within_batch_set_initial_capacity": (i32, [vp, i64]),
        "vg_shards_within_batch_last_launches": (i32, [vp]),
        # paged scans: the next k rows behind a (distance, rowid) cursor / behind the last key of the previous page
        "vg_after_floor": (i32, [C.c_double, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(i32)]),
    }
    for pre in ("vg_scan_topk_", "vg_shards_scan_topk_"):
        for m in ("", "_masked"):
            sig[pre + "after" + m] = (i32, [vp, i32, vp, i32, C.c_double, i64, vp, vp, C.POINTER(i32)])
            sig[pre + "after" + m + "_keys"] = (i32, [vp, i32, vp, i32, C.c_uint64, vp, C.POINTER(i32)])
            sig[pre + "batch_after" + m] = (i32, [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp])
            sig[pre + "batch_after" + m + "_keys"] = (i32, [vp, i32, vp, i32, i32, vp, vp, vp])
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    L._sig = sig
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise VectorGpuError("vectorgpu error %d: %s" % (rc, lib().vg_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().vg_device_count()


def backend_name():
    return lib().vg_backend_name().decode()


def pack_bits(x):
    """rows of bits for a U8 corpus scanned with HAMMING or JACCARD (= TANIMOTO): a 2-D array of bools or numbers [n, d] -> uint8
    [n, ceil(d / 8)].  A bit is 1 where the entry is true or > 0; the first dimension is the most significant bit of the first byte
    (np.packbits); tail bits are 0, so they add nothing to a Hamming distance nor to the intersection or union of a Jaccard distance.
    The query of either metric is one such row."""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("pack_bits: a 2-D array is needed, got %d-D" % x.ndim)
    bits = x if x.dtype == np.bool_ else x > 0
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="big"))


def hamming_reference(rows_u8, q_u8):
    """popcount(q XOR row) of every row on the host, float32 [n]: what a HAMMING scan returns as distances (spot checks, tests)"""
    rows = np.asarray(rows_u8)
    q = np.asarray(q_u8)
    if rows.dtype != np.uint8 or q.dtype != np.uint8 or rows.ndim != 2 or q.shape != (rows.shape[1],):
        raise ValueError("hamming_reference: uint8 rows [n, d] and a uint8 query [d] are needed")
    return np.unpackbits(rows ^ q[None, :], axis=1).sum(axis=1, dtype=np.int64).astype(np.float32)


def jaccard_reference(rows_u8, q_u8):
    """(u - i) / u with i = popcount(q AND row), u = popcount(q OR row) of every row on the host, float32 [n], 0 where u == 0: what
    a JACCARD scan returns as distances, bit for bit - one float32 division of two exactly converted integers (spot checks, tests)"""
    rows = np.asarray(rows_u8)
    q = np.asarray(q_u8)
    if rows.dtype != np.uint8 or q.dtype != np.uint8 or rows.ndim != 2 or q.shape != (rows.shape[1],):
        raise ValueError("jaccard_reference: uint8 rows [n, d] and a uint8 query [d] are needed")
    i = np.unpackbits(rows & q[None, :], axis=1).sum(axis=1, dtype=np.int64)
    u = np.unpackbits(rows | q[None, :], axis=1).sum(axis=1, dtype=np.int64)
    out = np.zeros(rows.shape[0], dtype=np.float32)
    np.divide((u - i).astype(np.float32), u.astype(np.float32), out=out, where=u > 0)
    return out


def plan_batch_half_form(stride_bytes, k, nq):
    """(wavefronts per workgroup, workgroups per CU) of an f16 / bf16 / f32-via-bf16 batch, or None if the matrix-core kernel does not
    serve such rows - host logic only"""
    w, b = C.c_int(0), C.c_int(0)
    if lib().vg_batch_h_plan(stride_bytes, k, nq, C.byref(w), C.byref(b)) != 0:
        return None
    return w.value, b.value


def plan_scan_shape(vtype, dim, metric):
    """(lanes per row, 16-byte chunks per lane, long-row kernel?) the plain scan would launch with - host logic only, no device"""
    lpr, u, lng = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_plan_scan_shape(vtype, dim, metric, C.byref(lpr), C.byref(u), C.byref(lng)))
    return lpr.value, u.value, bool(lng.value)


def batch_masked_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_masked serves this corpus with; 0 queries per pass =
    one single masked scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_masked_plan(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def _scan_topk_batch_masked(fn, h, metric, queries, k):
    queries = np.ascontiguousarray(queries)
    nq = queries.shape[0]
    ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
    dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
    cnt = np.zeros(max(nq, 1), dtype=np.int32)
    _check(fn(h, metric, _ptr(queries), nq, k, _ptr(ids), _ptr(dist), _ptr(cnt)))
    return ids, dist, cnt[:nq]


LABEL_NONE = 0xFFFFFFFF                             # VG_LABEL_NONE: a row with this label matches no query


def batch_labeled_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_labeled serves this corpus with; 0 queries per pass =
    one single labeled scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_labeled_plan(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def _labels_u32(labels):
    a = np.asarray(labels)
    if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > LABEL_NONE):
        raise ValueError("labels are integers in 0 .. 2^32 - 1 (LABEL_NONE = 2^32 - 1: no label)")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)


class _LabeledOps:
    """the labeled scans, shared by Corpus and Shards (`_lprefix`: vg_corpus / vg_shards, `_sprefix`: vg_ / vg_shards_): a uint32 label
    per scan position on the handle, a query names the label its rows must carry; ascending (distance, scan position) order"""

    def set_labels(self, labels):
        """one label per scan position (len == rows); LABEL_NONE marks a row no query matches"""
        lab = _labels_u32(labels)
        _check(getattr(lib(), self._lprefix + "_set_labels")(self.h, _ptr(lab), lab.size))

    def clear_labels(self):
        _check(getattr(lib(), self._lprefix + "_clear_labels")(self.h))

    def has_labels(self):
        return bool(getattr(lib(), self._lprefix + "_has_labels")(self.h))

    def scan_topk_labeled(self, metric, query, k, label):
        """the k nearest rows whose label is `label`: (rowids, distances)"""
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(getattr(lib(), self._sprefix + "scan_topk_labeled")(self.h, metric, _ptr(query), k, int(label), _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch_labeled(self, metric, queries, labels, k):
        """scan_topk_labeled for every row of `queries` with its own label, in shared passes: (rowids [nq, k], distances [nq, k],
        counts [nq]); the slots of query i behind counts[i] are not written"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        lab = _labels_u32(labels)
        if lab.size != nq:
            raise ValueError("scan_topk_batch_labeled takes one label per query")
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        _check(getattr(lib(), self._sprefix + "scan_topk_batch_labeled")(self.h, metric, _ptr(queries), nq, _ptr(lab), k, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids, dist, cnt[:nq]


class _GroupedOps:
    """the grouped scans, shared by Corpus and Shards (`_sprefix`: vg_ / vg_shards_): the k nearest labels (set_labels), each represented
    by its best row; ascending (distance, scan position) order"""

    def scan_topk_grouped(self, metric, query, k, masked=False):
        """order the labeled rows with a finite distance (masked: whose mask bit is set) by (distance, scan position), keep the first row
        of each label, return the first k kept: (rowids, distances, labels); fewer than k labels present give fewer results"""
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        lab = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = getattr(lib(), self._sprefix + "scan_topk_grouped" + ("_masked" if masked else ""))
        _check(fn(self.h, metric, _ptr(query), k, _ptr(ids), _ptr(dist), _ptr(lab), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], lab[:cnt.value]

    def scan_topk_batch_grouped(self, metric, queries, k, masked=False):
        """scan_topk_grouped for every row of `queries`, in shared passes: (rowids [nq, k], distances [nq, k], labels [nq, k],
        counts [nq]); the slots of query i behind counts[i] are not written"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        lab = np.zeros((nq, max(k, 1)), dtype=np.uint32)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        fn = getattr(lib(), self._sprefix + "scan_topk_batch_grouped" + ("_masked" if masked else ""))
        _check(fn(self.h, metric, _ptr(queries), nq, k, _ptr(ids), _ptr(dist), _ptr(lab), _ptr(cnt)))
        return ids, dist, lab, cnt[:nq]

    def scan_topk_capped(self, metric, query, k, per_label, masked=False):
        """order the labeled rows with a finite distance (masked: whose mask bit is set) by (distance, scan position), keep a row iff
        fewer than `per_label` rows of its label have been kept, return the first k kept: (rowids, distances, labels); per_label = 1
        is scan_topk_grouped, per_label above k behaves as k"""
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        lab = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = getattr(lib(), self._sprefix + "scan_topk_capped" + ("_masked" if masked else ""))
        _check(fn(self.h, metric, _ptr(query), k, per_label, _ptr(ids), _ptr(dist), _ptr(lab), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], lab[:cnt.value]

    def scan_topk_batch_capped(self, metric, queries, k, per_label, masked=False):
        """scan_topk_capped for every row of `queries`, in shared passes, one `per_label` for the whole batch: (rowids [nq, k],
        distances [nq, k], labels [nq, k], counts [nq]); the slots of query i behind counts[i] are not written"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        lab = np.zeros((nq, max(k, 1)), dtype=np.uint32)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        fn = getattr(lib(), self._sprefix + "scan_topk_batch_capped" + ("_masked" if masked else ""))
        _check(fn(self.h, metric, _ptr(queries), nq, k, per_label, _ptr(ids), _ptr(dist), _ptr(lab), _ptr(cnt)))
        return ids, dist, lab, cnt[:nq]


def batch_labelset_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_labelset serves this corpus with; 0 queries per pass =
    one single label-set scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_labelset_plan(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def _labelset_u32(labels):
    """one label set -> contiguous uint32; integers in 0 .. 2^32 - 2 (LABEL_NONE names no row), order and duplicates as given"""
    a = np.asarray(labels)
    if a.size == 0:
        return np.zeros(0, dtype=np.uint32)
    if a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) >= LABEL_NONE:
        raise ValueError("a label set holds integers in 0 .. 2^32 - 2 (LABEL_NONE names no row)")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)


def labelset_csr(sets):
    """the per-query label sets of scan_topk_batch_labelset in CSR form: (flat uint32 [total], offsets int64 [nq + 1]) - pure host
    code, no device.  `sets`: a sequence (list, or a tuple of another length than 2) of nq integer arrays, one set each - or a
    (flat, offsets) pair, a TUPLE of length 2, which is validated and passed through.  Labels are integers in 0 .. 2^32 - 2
    (LABEL_NONE and negative values: ValueError); offsets start at 0, do not decrease and end at len(flat).  Sorting and
    de-duplication are the engine's job: the flat array keeps the caller's order and duplicates."""
    if isinstance(sets, tuple) and len(sets) == 2:
        flat = _labelset_u32(sets[0])
        off = np.asarray(sets[1])
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError("offsets: a 1-d integer array of nq + 1 entries")
        off = np.ascontiguousarray(off, dtype=np.int64)
        if int(off[0]) != 0 or int(off[-1]) != flat.size or (np.diff(off) < 0).any():
            raise ValueError("offsets start at 0, do not decrease and end at len(flat)")
        return flat, off
    parts = [_labelset_u32(s) for s in sets]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts])
    flat = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    return np.ascontiguousarray(flat, dtype=np.uint32), off


class _LabelsetOps:
    """the label-set scans, shared by Corpus and Shards (`_sprefix`: vg_ / vg_shards_): the labeled, grouped and capped scans over
    the rows whose label (set_labels) is in a set of labels - exclude=True: is a label and not in it.  Order and duplicates in a set
    mean nothing; an unlabeled row is never allowed; the row mask is neither read nor written"""

    def scan_topk_labelset(self, metric, query, k, labels, exclude=False):
        """the k nearest allowed rows: (rowids, distances); an empty set allows nothing (exclude: every labeled row)"""
        query = np.ascontiguousarray(query)
        lab = _labelset_u32(labels)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        fn = getattr(lib(), self._sprefix + "scan_topk_labelset")
        _check(fn(self.h, metric, _ptr(query), k, _ptr(lab), lab.size, 1 if exclude else 0, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch_labelset(self, metric, queries, sets, k, exclude=False):
        """scan_topk_labelset for every row of `queries` under its own set (labelset_csr: nq arrays, or a (flat, offsets) pair), one
        `exclude` for the batch, in shared passes: (rowids [nq, k], distances [nq, k], counts [nq]); the slots of query i behind
        counts[i] are not written"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        flat, off = labelset_csr(sets)
        if off.size != nq + 1:
            raise ValueError("scan_topk_batch_labelset takes one label set per query")
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        fn = getattr(lib(), self._sprefix + "scan_topk_batch_labelset")
        _check(fn(self.h, metric, _ptr(queries), nq, k, _ptr(flat), _ptr(off), 1 if exclude else 0, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids, dist, cnt[:nq]

    def scan_topk_grouped_labelset(self, metric, query, k, labels, exclude=False):
        """scan_topk_grouped over the allowed rows: (rowids, distances, labels).  Paging: exclude=True with the labels returned so far"""
        query = np.ascontiguousarray(query)
        lab = _labelset_u32(labels)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        out = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = getattr(lib(), self._sprefix + "scan_topk_grouped_labelset")
        _check(fn(self.h, metric, _ptr(query), k, _ptr(lab), lab.size, 1 if exclude else 0, _ptr(ids), _ptr(dist), _ptr(out), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], out[:cnt.value]

    def scan_topk_capped_labelset(self, metric, query, k, per_label, labels, exclude=False):
        """scan_topk_capped over the allowed rows: (rowids, distances, labels)"""
        query = np.ascontiguousarray(query)
        lab = _labelset_u32(labels)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        out = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = getattr(lib(), self._sprefix + "scan_topk_capped_labelset")
        _check(fn(self.h, metric, _ptr(query), k, per_label, _ptr(lab), lab.size, 1 if exclude else 0, _ptr(ids), _ptr(dist), _ptr(out), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], out[:cnt.value]


def batch_valued_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_valued serves this corpus with - batch_masked_plan's
    figures; 0 queries per pass = one single valued scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_valued_plan(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


VALUE_MIN, VALUE_MAX = -(1 << 63), (1 << 63) - 1   # the open ends of a value interval (lo=None / hi=None)


def _value_bound(v, open_end):
    if v is None:
        return open_end
    v = int(v)
    if v < VALUE_MIN or v > VALUE_MAX:
        raise ValueError("a value bound is an int64")
    return v


def _values_i64(values):
    a = np.asarray(values)
    if a.size and (a.dtype.kind not in "iu" or (a.dtype.kind == "u" and a.dtype.itemsize == 8 and int(a.max()) > VALUE_MAX)):
        raise ValueError("values are integers that fit an int64")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)


class _ValuedOps:
    """the value-range scans, shared by Corpus and Shards (`_lprefix`: vg_corpus / vg_shards, `_sprefix`: vg_ / vg_shards_): an int64
    value per scan position on the handle (set_values), a query names the closed interval [lo, hi] its rows' values must lie in -
    lo=None / hi=None: the open end.  lo > hi allows nothing.  Values, labels and row mask are independent; the row mask is neither
    read nor written"""

    _VALUED_TOPK = {"": "vg_scan_topk_valued", "labeled": "vg_scan_topk_valued_labeled", "batch": "vg_scan_topk_batch_valued",
                    "grouped": "vg_scan_topk_grouped_valued", "capped": "vg_scan_topk_capped_valued"}

    def _valued_topk(self, form):
        """the top-k entry point of a form: vg_scan_topk_* on a corpus, vg_shards_valued_scan_topk[_<form>] over shards"""
        if self._sprefix == "vg_":
            return getattr(lib(), self._VALUED_TOPK[form])
        return getattr(lib(), "vg_shards_valued_scan_topk" + ("_" + form if form else ""))

    def set_values(self, values):
        """one int64 value per scan position (len == rows); any int64 is a value"""
        val = _values_i64(values)
        _check(getattr(lib(), self._lprefix + "_set_values")(self.h, _ptr(val), val.size))

    def clear_values(self):
        _check(getattr(lib(), self._lprefix + "_clear_values")(self.h))

    def has_values(self):
        return bool(getattr(lib(), self._lprefix + "_has_values")(self.h))

    def scan_topk_valued(self, metric, query, k, lo, hi, label=None):
        """the k nearest rows whose value lies in [lo, hi] - label: and whose label (set_labels) is `label`: (rowids, distances)"""
        query = np.ascontiguousarray(query)
        lo, hi = _value_bound(lo, VALUE_MIN), _value_bound(hi, VALUE_MAX)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        if label is None:
            _check(self._valued_topk("")(self.h, metric, _ptr(query), k, lo, hi, _ptr(ids), _ptr(dist), C.byref(cnt)))
        else:
            fn = self._valued_topk("labeled")
            _check(fn(self.h, metric, _ptr(query), k, lo, hi, int(label), _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch_valued(self, metric, queries, los, his, k, labels=None):
        """scan_topk_valued for every row of `queries` under its own interval (los / his: nq bounds each, a scalar or None is
        broadcast) - labels: and its own label - in shared passes: (rowids [nq, k], distances [nq, k], counts [nq]); the slots of
        query i behind counts[i] are not written"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]

        def bounds(b, open_end):
            if b is None or np.ndim(b) == 0:
                return np.full(nq, _value_bound(b, open_end), dtype=np.int64)
            b = [_value_bound(x, open_end) for x in (b.tolist() if isinstance(b, np.ndarray) else list(b))]
            return np.array(b, dtype=np.int64)

        lo, hi = bounds(los, VALUE_MIN), bounds(his, VALUE_MAX)
        if lo.size != nq or hi.size != nq:
            raise ValueError("scan_topk_batch_valued takes one interval per query")
        lab = None
        if labels is not None:
            lab = _labels_u32(labels)
            if lab.size != nq:
                raise ValueError("scan_topk_batch_valued takes one label per query")
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        fn = self._valued_topk("batch")
        _check(fn(self.h, metric, _ptr(queries), nq, k, _ptr(lo), _ptr(hi), None if lab is None else _ptr(lab), _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids, dist, cnt[:nq]

    def scan_topk_grouped_valued(self, metric, query, k, lo, hi):
        """scan_topk_grouped over the rows whose value lies in [lo, hi] - filter by value, group by label: (rowids, distances, labels)"""
        query = np.ascontiguousarray(query)
        lo, hi = _value_bound(lo, VALUE_MIN), _value_bound(hi, VALUE_MAX)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        out = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = self._valued_topk("grouped")
        _check(fn(self.h, metric, _ptr(query), k, lo, hi, _ptr(ids), _ptr(dist), _ptr(out), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], out[:cnt.value]

    def scan_topk_capped_valued(self, metric, query, k, per_label, lo, hi):
        """scan_topk_capped over the rows whose value lies in [lo, hi]: (rowids, distances, labels)"""
        query = np.ascontiguousarray(query)
        lo, hi = _value_bound(lo, VALUE_MIN), _value_bound(hi, VALUE_MAX)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        out = np.zeros(max(k, 1), dtype=np.uint32)
        cnt = C.c_int(0)
        fn = self._valued_topk("capped")
        _check(fn(self.h, metric, _ptr(query), k, per_label, lo, hi, _ptr(ids), _ptr(dist), _ptr(out), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value], out[:cnt.value]

    def scan_within_valued(self, metric, query, radius, lo, hi, limit=None):
        """scan_within among the rows whose value lies in [lo, hi]: (rowids, distances, matches)"""
        lo, hi = _value_bound(lo, VALUE_MIN), _value_bound(hi, VALUE_MAX)
        fn = getattr(lib(), self._sprefix + "scan_within_valued")
        scan = lambda h, metric, q, r, lim, m, held: fn(h, metric, q, r, lim, lo, hi, m, held)
        return _scan_within(scan, getattr(lib(), self._sprefix + "scan_within_fetch"), self.h, metric, query, radius, limit)


def batch_capped_plan(corpus, metric, masked=False):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_capped serves this corpus with; 0 queries per pass =
    one single capped scan per query (f16 / bf16, long rows, an instance left out of the table) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_capped_plan(corpus.h, metric, 1 if masked else 0, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def batch_grouped_plan(corpus, metric, masked=False):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_topk_batch_grouped serves this corpus with; 0 queries per pass =
    one single grouped scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().vg_batch_grouped_plan(corpus.h, metric, 1 if masked else 0, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def merge_keys_grouped(keys, labels, pos_offsets, k):
    """vg_merge_keys_grouped: keys / labels [n_lists, list_len] -> (keys with global positions, labels), one row per label - host only"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    n_lists, list_len = keys.shape
    off = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.int64)
    out_keys = np.zeros(max(k, 1), dtype=np.uint64)
    out_lab = np.zeros(max(k, 1), dtype=np.uint32)
    cnt = C.c_int(0)
    _check(lib().vg_merge_keys_grouped(_ptr(keys), _ptr(labels), n_lists, list_len, _ptr(off), k, _ptr(out_keys), _ptr(out_lab), C.byref(cnt)))
    return out_keys[:cnt.value], out_lab[:cnt.value]


def merge_keys_capped(keys, labels, pos_offsets, k, per_label):
    """vg_merge_keys_capped: keys / labels [n_lists, list_len] -> (keys with global positions, labels), at most per_label rows of a
    label - host only"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    n_lists, list_len = keys.shape
    off = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.int64)
    out_keys = np.zeros(max(k, 1), dtype=np.uint64)
    out_lab = np.zeros(max(k, 1), dtype=np.uint32)
    cnt = C.c_int(0)
    _check(lib().vg_merge_keys_capped(_ptr(keys), _ptr(labels), n_lists, list_len, _ptr(off), k, per_label, _ptr(out_keys), _ptr(out_lab),
                                      C.byref(cnt)))
    return out_keys[:cnt.value], out_lab[:cnt.value]


AFTER_START = (float("-inf"), -(1 << 63))          # the cursor in front of every row


def after_floor(after_dist, first_pos_behind):
    """(floor key, empty?) of a paged scan's cursor (vg_after_floor) - host arithmetic only, no device"""
    floor, empty = C.c_uint64(0), C.c_int(0)
    _check(lib().vg_after_floor(float(after_dist), int(first_pos_behind), C.byref(floor), C.byref(empty)))
    return floor.value, bool(empty.value)


def _after_name(obj, batch, masked, keys):
    return ("vg_shards_scan_topk_" if isinstance(obj, Shards) else "vg_scan_topk_") + ("batch_after" if batch else "after") + \
        ("_masked" if masked else "") + ("_keys" if keys else "")


def _scan_topk_after(obj, metric, query, k, after, masked):
    query = np.ascontiguousarray(query)
    d, r = AFTER_START if after is None else after
    ids = np.zeros(max(k, 1), dtype=np.int64)
    dist = np.zeros(max(k, 1), dtype=np.float64)
    cnt = C.c_int(0)
    _check(getattr(lib(), _after_name(obj, False, masked, False))(obj.h, metric, _ptr(query), k, float(d), int(r), _ptr(ids), _ptr(dist), C.byref(cnt)))
    return ids[:cnt.value], dist[:cnt.value]


def _scan_topk_after_keys(obj, metric, query, k, after_key, masked):
    query = np.ascontiguousarray(query)
    keys = np.zeros(max(k, 1), dtype=np.uint64)
    cnt = C.c_int(0)
    _check(getattr(lib(), _after_name(obj, False, masked, True))(obj.h, metric, _ptr(query), k, int(after_key or 0), _ptr(keys), C.byref(cnt)))
    return keys[:cnt.value]


def _scan_topk_batch_after(obj, metric, queries, k, after, masked):
    queries = np.ascontiguousarray(queries)
    nq = queries.shape[0]
    cur = [AFTER_START] * nq if after is None else [AFTER_START if a is None else a for a in after]
    if len(cur) != nq:
        raise ValueError("one cursor per query")
    ad = np.array([float(a[0]) for a in cur] or [0.0], dtype=np.float64)
    ar = np.array([int(a[1]) for a in cur] or [0], dtype=np.int64)
    ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
    dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
    cnt = np.zeros(max(nq, 1), dtype=np.int32)
    _check(getattr(lib(), _after_name(obj, True, masked, False))(obj.h, metric, _ptr(queries), nq, k, _ptr(ad), _ptr(ar), _ptr(ids), _ptr(dist), _ptr(cnt)))
    return ids, dist, cnt[:nq]


def _scan_topk_batch_after_keys(obj, metric, queries, k, after_keys, masked):
    queries = np.ascontiguousarray(queries)
    nq = queries.shape[0]
    ak = np.zeros(max(nq, 1), dtype=np.uint64) if after_keys is None else np.ascontiguousarray(after_keys, dtype=np.uint64)
    if after_keys is not None and len(ak) != nq:
        raise ValueError("one cursor key per query")
    keys = np.zeros((nq, max(k, 1)), dtype=np.uint64)
    cnt = np.zeros(max(nq, 1), dtype=np.int32)
    _check(getattr(lib(), _after_name(obj, True, masked, True))(obj.h, metric, _ptr(queries), nq, k, _ptr(ak), _ptr(keys), _ptr(cnt)))
    return keys, cnt[:nq]


class _PagedScans:
    """paged scans ("search after"), shared by Corpus and Shards: the next k rows behind a cursor, in ascending (distance, scan
    position) order; masked=True reads the handle's row mask"""

    def scan_topk_after(self, metric, query, k, after=None, masked=False):
        """the next k rows behind `after` = (distance, rowid) of the previous page's last row (None: from the start): (rowids, distances)"""
        return _scan_topk_after(self, metric, query, k, after, masked)

    def scan_topk_after_keys(self, metric, query, k, after_key=None, masked=False):
        """the same with the cursor as the previous page's last packed key (None: from the start), returning packed keys; any rowid layout"""
        return _scan_topk_after_keys(self, metric, query, k, after_key, masked)

    def scan_topk_batch_after(self, metric, queries, k, after=None, masked=False):
        """scan_topk_after for every row of `queries`, a cursor each (`after`: a list of (distance, rowid) pairs or None entries):
        (rowids [nq, k], distances [nq, k], counts [nq]); slots behind a query's count stay zero"""
        return _scan_topk_batch_after(self, metric, queries, k, after, masked)

    def scan_topk_batch_after_keys(self, metric, queries, k, after_keys=None, masked=False):
        """the same with one cursor key per query: (keys [nq, k], counts [nq])"""
        return _scan_topk_batch_after_keys(self, metric, queries, k, after_keys, masked)


def _wb_prefix(obj):
    return "vg_shards_within_batch_" if isinstance(obj, Shards) else "vg_within_batch_"


def within_batch_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_within_batch serves this corpus (or shard set) with; 0 queries
    per pass = one single range scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(getattr(lib(), _wb_prefix(corpus) + "plan")(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def within_batch_masked_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_within_batch_masked serves this corpus (or shard set) with; 0
    queries per pass = one single masked range scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(getattr(lib(), _wb_prefix(corpus) + "masked_plan")(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def within_batch_labeled_plan(corpus, metric):
    """(queries per pass, lanes per row, 16-byte chunks per lane) scan_within_batch_labeled serves this corpus (or shard set) with; 0
    queries per pass = one single labeled range scan per query (f16 / bf16, long rows) - host logic only"""
    nq, lpr, u = C.c_int(0), C.c_int(0), C.c_int(0)
    _check(getattr(lib(), _wb_prefix(corpus) + "labeled_plan")(corpus.h, metric, C.byref(nq), C.byref(lpr), C.byref(u)))
    return nq.value, lpr.value, u.value


def set_within_batch_initial_capacity(corpus, keys_per_query):
    """keys the device region of each query of the next scan_within_batch calls starts with (0: the default) - vectorgpu_diag.h"""
    _check(getattr(lib(), _wb_prefix(corpus) + "set_initial_capacity")(corpus.h, int(keys_per_query)))


def within_batch_last_launches(corpus):
    """scan kernel launches of the last scan_within_batch: its passes, plus one per pass that overflowed and ran once more"""
    return int(getattr(lib(), _wb_prefix(corpus) + "last_launches")(corpus.h))


def _scan_within(scan, fetch, h, metric, query, radius, limit):
    query = np.ascontiguousarray(query)
    m, held = C.c_int64(0), C.c_int64(0)
    _check(scan(h, metric, _ptr(query), float(radius), 0 if limit is None else max(int(limit), 0), C.byref(m), C.byref(held)))
    n = 0 if (limit is not None and limit <= 0) else held.value
    ids, dist = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
    if n:
        _check(fetch(h, 0, n, _ptr(ids), _ptr(dist)))
    return ids, dist, m.value


def _scan_within_batch(scan, fetch, h, metric, queries, radii, limit):
    queries = np.ascontiguousarray(queries)
    if queries.ndim != 2:
        raise ValueError("scan_within_batch takes a 2-d array of queries")
    nq = queries.shape[0]
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (nq,)) if np.ndim(radii) == 0 else np.asarray(radii, dtype=np.float64).ravel())
    if radii.size != nq:
        raise ValueError("scan_within_batch: %d radii for %d queries" % (radii.size, nq))
    m, held = np.zeros(max(nq, 1), dtype=np.int64), np.zeros(max(nq, 1), dtype=np.int64)
    _check(scan(h, metric, _ptr(queries), nq, _ptr(radii), 0 if limit is None else max(int(limit), 0), _ptr(m), _ptr(held)))
    out = []
    for i in range(nq):
        n = 0 if (limit is not None and limit <= 0) else int(held[i])
        ids, dist = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
        if n:
            _check(fetch(h, i, 0, n, _ptr(ids), _ptr(dist)))
        out.append((ids, dist, int(m[i])))
    return out


class _WithinLabeledOps:
    """the labeled range scans, shared by Corpus and Shards (`_sprefix`: vg_ / vg_shards_): every row that carries an allowed label
    (set_labels) and lies within `radius` of the query, ascending (distance, scan position); return shapes are scan_within's and
    scan_within_batch's, and the results are held where those hold theirs.  The row mask is neither read nor written"""

    def _within_fetch(self, batch):
        return getattr(lib(), self._sprefix + ("scan_within_batch_fetch" if batch else "scan_within_fetch"))

    def scan_within_labeled(self, metric, query, radius, label, limit=None):
        """scan_within among the rows whose label is `label`: (rowids, distances, matches)"""
        fn = getattr(lib(), self._sprefix + "scan_within_labeled")
        scan = lambda h, metric, q, r, lim, m, held: fn(h, metric, q, r, lim, int(label), m, held)
        return _scan_within(scan, self._within_fetch(False), self.h, metric, query, radius, limit)

    def scan_within_labelset(self, metric, query, radius, labels, exclude=False, limit=None):
        """scan_within among the rows whose label is in `labels` - exclude=True: is a label and not in it; an empty set allows nothing
        (exclude: every labeled row): (rowids, distances, matches)"""
        lab = _labelset_u32(labels)
        fn = getattr(lib(), self._sprefix + "scan_within_labelset")
        scan = lambda h, metric, q, r, lim, m, held: fn(h, metric, q, r, lim, _ptr(lab), lab.size, 1 if exclude else 0, m, held)
        return _scan_within(scan, self._within_fetch(False), self.h, metric, query, radius, limit)

    def scan_within_batch_labeled(self, metric, queries, labels, radii, limit=None):
        """scan_within_labeled for every row of `queries` with its own label and its own radius (a scalar radius is broadcast), in
        shared passes: a list of (rowids, distances, matches) per query, in the caller's order"""
        lab = _labels_u32(labels)
        if lab.size != np.shape(queries)[0]:
            raise ValueError("scan_within_batch_labeled takes one label per query")
        fn = getattr(lib(), self._sprefix + "scan_within_batch_labeled")
        scan = lambda h, metric, qs, nq, r, lim, m, held: fn(h, metric, qs, nq, _ptr(lab), r, lim, m, held)
        return _scan_within_batch(scan, self._within_fetch(True), self.h, metric, queries, radii, limit)

    def within_batch_labeled_plan(self, metric):
        return within_batch_labeled_plan(self, metric)


def _set_mask(obj, prefix, rows, bits, positions, rowids):
    """Corpus.set_mask / Shards.set_mask: bits | positions | rowids -> the handle's row mask; returns the rows allowed"""
    if (bits is not None) + (positions is not None) + (rowids is not None) != 1:
        raise ValueError("set_mask takes exactly one of bits, positions, rowids")
    L = lib()
    if rowids is not None:
        ids = np.ascontiguousarray(rowids, dtype=np.int64).ravel()
        n_set = C.c_int64(0)
        _check(getattr(L, prefix + "_set_mask_rowids")(obj.h, _ptr(ids), ids.size, C.byref(n_set)))
        return n_set.value
    if positions is not None:
        flags = np.zeros(rows, dtype=bool)
        flags[np.asarray(positions, dtype=np.int64).ravel()] = True
        bits = flags
    bits = np.asarray(bits)
    if bits.dtype == np.uint64:                              # packed words: every bit they hold, up to the rows held
        words, n_bits = np.ascontiguousarray(bits).ravel(), min(int(bits.size) * 64, int(rows))
    else:
        flags = np.ascontiguousarray(bits, dtype=bool).ravel()
        n_bits = int(flags.size)
        words = np.zeros((n_bits + 63) // 64, dtype=np.uint64)
        words.view(np.uint8)[:(n_bits + 7) // 8] = np.packbits(flags, bitorder="little")
    _check(getattr(L, prefix + "_set_mask_bits")(obj.h, _ptr(words), n_bits))
    return int(getattr(L, prefix + "_mask_count")(obj.h))


class Corpus(_PagedScans, _LabeledOps, _GroupedOps, _LabelsetOps, _WithinLabeledOps, _ValuedOps):
    """One HBM-resident corpus shard (opaque vg_corpus handle)."""
    _lprefix, _sprefix = "vg_corpus", "vg_"

    def __init__(self, vtype, dim, device=0, capacity=0):
        self.h = C.c_void_p()
        self.vtype, self.dim = vtype, dim
        _check(lib().vg_corpus_create(device, vtype, dim, capacity, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().vg_corpus_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @property
    def rows(self):
        return lib().vg_corpus_rows(self.h)

    def append(self, rows, rowids=None):
        rows = np.ascontiguousarray(rows)
        assert rows.ndim == 2 and rows.shape[1] * rows.itemsize >= self.dim * TYPE_SIZE[self.vtype]
        ids = None if rowids is None else np.ascontiguousarray(rowids, dtype=np.int64)
        _check(lib().vg_corpus_append(self.h, _ptr(rows), rows.shape[0], rows.strides[0], _ptr(ids)))

    def append_strided(self, buf, n_rows, stride, rowids=None):
        buf = np.ascontiguousarray(buf)
        ids = None if rowids is None else np.ascontiguousarray(rowids, dtype=np.int64)
        _check(lib().vg_corpus_append(self.h, _ptr(buf), n_rows, stride, _ptr(ids)))

    def append_records(self, records, n):
        records = np.ascontiguousarray(records)
        _check(lib().vg_corpus_append_records(self.h, _ptr(records), n))

    def append_device(self, dev_ptr, n_rows, stride, rowids=None):
        ids = None if rowids is None else np.ascontiguousarray(rowids, dtype=np.int64)
        _check(lib().vg_corpus_append_device(self.h, C.c_void_p(dev_ptr), n_rows, stride, _ptr(ids)))

    def set_rowid_base(self, base):
        _check(lib().vg_corpus_set_rowid_base(self.h, base))

    def scan_topk(self, metric, query, k):
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(lib().vg_scan_topk(self.h, metric, _ptr(query), k, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_device(self, metric, dev_query_ptr, k, dev_keys_ptr, stream=None):
        _check(lib().vg_scan_topk_device(self.h, metric, C.c_void_p(dev_query_ptr), k, C.c_void_p(dev_keys_ptr),
                                         C.c_void_p(stream) if stream else None))

    def scan_distances(self, metric, query):
        query = np.ascontiguousarray(query)
        out = np.empty(self.rows, dtype=np.float32)
        _check(lib().vg_scan_distances(self.h, metric, _ptr(query), _ptr(out)))
        return out

    def scan_within(self, metric, query, radius, limit=None):
        """every row with distance <= radius (finite), ordered by (distance, scan position): (rowids, distances, matches); with a
        limit the first `limit` of them, `matches` still counting all"""
        return _scan_within(lib().vg_scan_within, lib().vg_scan_within_fetch, self.h, metric, query, radius, limit)

    # masked scans: a row mask on the handle (a bitmap over scan positions), read by the four *_masked scans only
    def set_mask(self, bits=None, positions=None, rowids=None):
        """the rows a masked scan may return - exactly one of: `bits` (bool per scan position, or packed uint64 words: bit p & 63 of
        word p >> 6), `positions` (scan positions), `rowids` (those not held are ignored).  Returns the number of rows allowed."""
        return _set_mask(self, "vg_corpus", self.rows, bits, positions, rowids)

    def clear_mask(self):
        _check(lib().vg_corpus_clear_mask(self.h))

    def mask_count(self):
        """rows the mask allows, -1 without a mask"""
        return int(lib().vg_corpus_mask_count(self.h))

    def scan_topk_masked(self, metric, query, k):
        """the k nearest ALLOWED rows, ascending (distance, scan position): (rowids, distances)"""
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(lib().vg_scan_topk_masked(self.h, metric, _ptr(query), k, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch_masked(self, metric, queries, k):
        """scan_topk_masked for every row of `queries` in shared passes over the allowed rows: (rowids [nq, k], distances [nq, k],
        counts [nq]) like scan_topk_batch; slots behind a query's count stay zero"""
        return _scan_topk_batch_masked(lib().vg_scan_topk_batch_masked, self.h, metric, queries, k)

    def scan_within_masked(self, metric, query, radius, limit=None):
        """scan_within among the ALLOWED rows: (rowids, distances, matches); it holds its result where scan_within does"""
        return _scan_within(lib().vg_scan_within_masked, lib().vg_scan_within_fetch, self.h, metric, query, radius, limit)

    def scan_within_batch_masked(self, metric, queries, radii, limit=None):
        """scan_within_masked for every row of `queries` in shared passes over the allowed rows, a radius each (a scalar is
        broadcast): a list of (rowids, distances, matches) per query; it holds its results where scan_within_batch does"""
        return _scan_within_batch(lib().vg_scan_within_batch_masked, lib().vg_scan_within_batch_fetch, self.h, metric, queries, radii, limit)

    def clone(self):
        """a second corpus with the same rows, rowids, switches and row mask (vg_corpus_clone)"""
        other = Corpus.__new__(Corpus)
        other.h = C.c_void_p()
        other.vtype, other.dim = self.vtype, self.dim
        _check(lib().vg_corpus_clone(self.h, C.byref(other.h)))
        return other

    def within_keys(self, n):
        """the first n keys the last scan_within holds (positions local to this corpus): what a multi-shard caller merges"""
        keys = np.zeros(n, dtype=np.uint64)
        if n:
            _check(lib().vg_scan_within_keys(self.h, 0, n, _ptr(keys)))
        return keys

    def set_within_initial_capacity(self, keys):
        """keys the device buffer of the next range scans starts with (0: the default) - vectorgpu_diag.h"""
        _check(lib().vg_within_set_initial_capacity(self.h, keys))

    def within_last_launches(self):
        return int(lib().vg_within_last_launches(self.h))

    def scan_within_batch(self, metric, queries, radii, limit=None):
        """scan_within for every row of `queries` in shared passes over the corpus, a radius each (a scalar is broadcast): a list of
        (rowids, distances, matches) per query; `limit` is per query"""
        return _scan_within_batch(lib().vg_scan_within_batch, lib().vg_scan_within_batch_fetch, self.h, metric, queries, radii, limit)

    def within_batch_keys(self, query, n):
        """the first n keys the last scan_within_batch holds for `query` (positions local to this corpus)"""
        keys = np.zeros(n, dtype=np.uint64)
        _check(lib().vg_scan_within_batch_keys(self.h, query, 0, n, _ptr(keys)))
        return keys

    def within_batch_plan(self, metric):
        return within_batch_plan(self, metric)

    def within_batch_masked_plan(self, metric):
        return within_batch_masked_plan(self, metric)

    def set_within_batch_initial_capacity(self, keys_per_query):
        set_within_batch_initial_capacity(self, keys_per_query)

    def within_batch_last_launches(self):
        return within_batch_last_launches(self)

    def scan_topk_batch(self, metric, queries, k):
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        _check(lib().vg_scan_topk_batch(self.h, metric, _ptr(queries), nq, k, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids, dist, cnt

    def scan_topk_batch_keys(self, metric, queries, k):
        """per-query packed keys (positions local to this corpus): uint64 [nq, k] (VG_KEY_EMPTY padded), counts [nq]"""
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        keys = np.full((nq, max(k, 1)), KEY_EMPTY, dtype=np.uint64)
        cnt = np.zeros(nq, dtype=np.int32)
        _check(lib().vg_scan_topk_batch_keys(self.h, metric, _ptr(queries), nq, k, _ptr(keys), _ptr(cnt)))
        for i in range(nq):                                    # entries past the count are unspecified: pad them
            keys[i, cnt[i]:] = KEY_EMPTY
        return keys, cnt

    def minmax(self):
        lo, hi, neg = C.c_float(0), C.c_float(0), C.c_int(0)
        _check(lib().vg_corpus_minmax(self.h, C.byref(lo), C.byref(hi), C.byref(neg)))
        return lo.value, hi.value, bool(neg.value)

    def quantize_rows(self, scale, offset, qtype, row0=0, n_rows=None):
        n = self.rows - row0 if n_rows is None else n_rows
        out = np.empty((n, self.dim), dtype=np.uint8)
        _check(lib().vg_corpus_quantize_rows(self.h, scale, offset, qtype, row0, n, _ptr(out)))
        return out

    def set_profiling(self, on=True):
        _check(lib().vg_set_profiling(self.h, 1 if on else 0))

    def last_kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().vg_last_kernel_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def profile_mean_ms(self):
        n, a, b = C.c_int(0), C.c_float(0), C.c_float(0)
        _check(lib().vg_profile_mean_ms(self.h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def kernel_name(self, metric):
        return lib().vg_scan_kernel_name(self.h, metric).decode()

    def profile_mean_ms_ex(self):
        """(launches, scan kernel ms, merge ms, pre-pass ms) - the scan figure is ONE kernel"""
        n, a, b, p = C.c_int(0), C.c_float(0), C.c_float(0), C.c_float(0)
        _check(lib().vg_profile_mean_ms_ex(self.h, C.byref(n), C.byref(a), C.byref(b), C.byref(p)))
        return n.value, a.value, b.value, p.value

    def filter_exact_evals(self):
        v = C.c_ulonglong(0)
        _check(lib().vg_filter_exact_evals(self.h, C.byref(v)))
        return v.value

    def filter_guard_cooldown(self):
        """> 0: the selectivity guard has sent this corpus' next that many single scans to the plain kernel"""
        return int(lib().vg_filter_guard_cooldown(self.h))

    def find_rowid(self, rowid):
        return int(lib().vg_corpus_find_rowid(self.h, rowid))

    def patch_rows(self, positions, rows):
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        rows = np.ascontiguousarray(rows)
        _check(lib().vg_corpus_patch_rows(self.h, _ptr(positions), positions.shape[0], _ptr(rows), rows.strides[0]))

    def delete_rows(self, positions):
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        _check(lib().vg_corpus_delete_rows(self.h, _ptr(positions), positions.shape[0]))

    def device_bytes(self):
        """(row matrix, derived per-row copies / statistics, working buffers) in bytes on the device"""
        out = np.zeros(3, dtype=np.int64)
        _check(lib().vg_corpus_device_bytes(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def batch_q8_status(self):
        """how the last attempt at the int8 batch filter ended (vectorgpu_diag.h)"""
        return lib().vg_batch_q8_status(self.h)

    def batch_half_split_off(self):
        """True once a split-form batch over this corpus overflowed a pair region: the fused kernel answers from then on"""
        return bool(lib().vg_batch_h_split_off(self.h))

    def last_batch_path(self):
        """1 f32 matrix-core kernel, 2 int8, 3 half-precision kernel, 4 its long-row form, 5 multi-query scan, 6 one scan per query"""
        return lib().vg_batch_last_path(self.h)

    def batch_filter_exact_evals(self):
        v = C.c_ulonglong(0)
        _check(lib().vg_batch_filter_exact_evals(self.h, C.byref(v)))
        return v.value

    def set_scan_filter(self, mode):
        _check(lib().vg_corpus_set_scan_filter(self.h, mode))

    def set_tie_order(self, mode):
        """TIE_POSITION (default) or TIE_REFERENCE: the reference's slot-history result among equal distances"""
        _check(lib().vg_corpus_set_tie_order(self.h, mode))

    def pass_ms(self, which):
        """(kernel ms, rows) of the last "minmax" / "quantize" / "q8_shadow" pass over this corpus"""
        ms, rows = C.c_float(0), C.c_longlong(0)
        _check(lib().vg_corpus_pass_ms(self.h, {"minmax": 0, "quantize": 1, "q8_shadow": 2}[which], C.byref(ms), C.byref(rows)))
        return ms.value, rows.value

    def clear(self):
        _check(lib().vg_corpus_clear(self.h))

    def reserve(self, n):
        """room for n rows in all (vg_corpus_reserve): never shrinks"""
        _check(lib().vg_corpus_reserve(self.h, n))

    def trim(self):
        """give back what a reservation holds beyond the rows that arrived (vg_corpus_trim)"""
        _check(lib().vg_corpus_trim(self.h))

    def tie_stats(self):
        """reference-order scans so far: {scans, with_a_tie_among_the_k_plus_1_best, fused_replays, store_mode_replays}"""
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().vg_corpus_tie_stats(self.h, _ptr(out)))
        return dict(zip(("scans", "with_a_tie_among_the_k_plus_1_best", "fused_replays", "store_mode_replays"), (int(x) for x in out)))


class SlabScan:
    """One query over a table handed over slab by slab (include/vectorgpu.h: vg_slab_scan_*): the device holds two slabs."""

    def __init__(self, vtype, dim, metric, query, k, slab_rows, tie_order=0, device=0, rowid_base=1):
        self.h = C.c_void_p()
        self.k = k
        query = np.ascontiguousarray(query)
        _check(lib().vg_slab_scan_begin(device, vtype, dim, metric, _ptr(query), k, tie_order, slab_rows, rowid_base, C.byref(self.h)))

    def rows(self, rows, rowids=None):
        rows = np.ascontiguousarray(rows)
        ids = None if rowids is None else np.ascontiguousarray(rowids, dtype=np.int64)
        _check(lib().vg_slab_scan_rows(self.h, _ptr(rows), rows.shape[0], rows.strides[0] if rows.ndim == 2 else 0, None if ids is None else _ptr(ids)))

    def records(self, recs, n):
        recs = np.ascontiguousarray(recs)
        _check(lib().vg_slab_scan_records(self.h, _ptr(recs), n))

    def finish(self):
        ids = np.zeros(max(self.k, 1), dtype=np.int64)
        dist = np.zeros(max(self.k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(lib().vg_slab_scan_finish(self.h, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def all(self):
        """k = 0 scans, after finish(): (distances, rowids) of every row in scan order"""
        n = C.c_int64(0)
        pd, pi = C.c_void_p(), C.c_void_p()
        _check(lib().vg_slab_scan_all(self.h, C.byref(n), C.byref(pd), C.byref(pi)))
        if n.value == 0:
            return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)
        d = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_float)), shape=(n.value,)).copy()
        i = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_int64)), shape=(n.value,)).copy()
        return d, i

    def close(self):
        if self.h:
            lib().vg_slab_scan_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


def device_memory(device=0):
    f, t = C.c_longlong(0), C.c_longlong(0)
    _check(lib().vg_device_memory(device, C.byref(f), C.byref(t)))
    return f.value, t.value


class Shards(_PagedScans, _LabeledOps, _GroupedOps, _LabelsetOps, _WithinLabeledOps, _ValuedOps):
    """One logical corpus dealt block-cyclically over several devices of this process (opaque vg_shards handle)."""
    _lprefix, _sprefix = "vg_shards", "vg_shards_"

    def __init__(self, vtype, dim, devices, block_rows=0):
        self.h = C.c_void_p()
        self.vtype, self.dim = vtype, dim
        devs = (C.c_int * len(devices))(*devices)
        _check(lib().vg_shards_create(devs, len(devices), vtype, dim, block_rows, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().vg_shards_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    @property
    def rows(self):
        return lib().vg_shards_rows(self.h)

    def shard_rows(self):
        return [lib().vg_corpus_rows(lib().vg_shards_shard(self.h, i)) for i in range(lib().vg_shards_count(self.h))]

    def reserve(self, n):
        _check(lib().vg_shards_reserve(self.h, n))

    def clear(self):
        _check(lib().vg_shards_clear(self.h))

    def trim(self):
        _check(lib().vg_shards_trim(self.h))

    def clone(self):
        """a second shard set with the same rows, rowids and switches (vg_shards_clone)"""
        other = Shards.__new__(Shards)
        other.h = C.c_void_p()
        other.vtype, other.dim = self.vtype, self.dim
        _check(lib().vg_shards_clone(self.h, C.byref(other.h)))
        return other

    def find_rowid(self, rowid):
        """global scan position of `rowid`, -1 not held, -2 no lookup (vg_shards_find_rowid)"""
        return int(lib().vg_shards_find_rowid(self.h, rowid))

    def patch_rows(self, positions, rows):
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        rows = np.ascontiguousarray(rows)
        _check(lib().vg_shards_patch_rows(self.h, _ptr(positions), positions.shape[0], _ptr(rows), rows.strides[0]))

    def delete_rows(self, positions):
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        _check(lib().vg_shards_delete_rows(self.h, _ptr(positions), positions.shape[0]))

    def append(self, rows, rowids=None):
        rows = np.ascontiguousarray(rows)
        ids = None if rowids is None else np.ascontiguousarray(rowids, dtype=np.int64)
        _check(lib().vg_shards_append(self.h, _ptr(rows), rows.shape[0], rows.strides[0], _ptr(ids)))

    def append_records(self, records, n):
        records = np.ascontiguousarray(records)
        _check(lib().vg_shards_append_records(self.h, _ptr(records), n))

    def rowid_at(self, pos):
        return lib().vg_shards_rowid_at(self.h, pos)

    def rowids(self, pos0, n):
        out = np.zeros(n, dtype=np.int64)
        _check(lib().vg_shards_rowids(self.h, pos0, n, _ptr(out)))
        return out

    def set_tie_order(self, mode):
        _check(lib().vg_shards_set_tie_order(self.h, mode))

    def set_scan_filter(self, mode):
        _check(lib().vg_shards_set_scan_filter(self.h, mode))

    def set_gather(self, mode):
        """candidate gather: "host" (every shard copies its 64 keys back) or "rccl" (one grouped ncclAllGather over xGMI)"""
        _check(lib().vg_shards_set_gather(self.h, {"host": 0, "rccl": 1}[mode]))

    def gather_stats(self):
        out = np.zeros(2, dtype=np.uint64)
        serving = lib().vg_shards_gather_stats(self.h, _ptr(out))
        return {"host": int(out[0]), "rccl": int(out[1]), "rccl_serving": bool(serving)}

    @property
    def threaded(self):
        """every query's per-shard work runs on the handle's persistent host threads (one per shard)"""
        return bool(lib().vg_shards_threaded(self.h))

    def tie_stats(self):
        """reference-order scans of this handle so far (same four counters as Corpus.tie_stats)"""
        out = np.zeros(4, dtype=np.uint64)
        _check(lib().vg_shards_tie_stats(self.h, _ptr(out)))
        return dict(zip(("scans", "with_a_tie_among_the_k_plus_1_best", "fused_replays", "store_mode_replays"), (int(x) for x in out)))

    def scan_topk(self, metric, query, k):
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(lib().vg_shards_scan_topk(self.h, metric, _ptr(query), k, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch(self, metric, queries, k):
        queries = np.ascontiguousarray(queries)
        nq = queries.shape[0]
        ids = np.zeros((nq, max(k, 1)), dtype=np.int64)
        dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
        cnt = np.zeros(nq, dtype=np.int32)
        _check(lib().vg_shards_scan_topk_batch(self.h, metric, _ptr(queries), nq, k, _ptr(ids), _ptr(dist), _ptr(cnt)))
        return ids, dist, cnt

    def set_mask(self, bits=None, positions=None, rowids=None):
        """Corpus.set_mask over GLOBAL scan positions: the bits are dealt out to the shards like the rows"""
        return _set_mask(self, "vg_shards", self.rows, bits, positions, rowids)

    def clear_mask(self):
        _check(lib().vg_shards_clear_mask(self.h))

    def mask_count(self):
        return int(lib().vg_shards_mask_count(self.h))

    def scan_topk_masked(self, metric, query, k):
        """Corpus.scan_topk_masked over all shards, merged by (distance, global scan position)"""
        query = np.ascontiguousarray(query)
        ids = np.zeros(max(k, 1), dtype=np.int64)
        dist = np.zeros(max(k, 1), dtype=np.float64)
        cnt = C.c_int(0)
        _check(lib().vg_shards_scan_topk_masked(self.h, metric, _ptr(query), k, _ptr(ids), _ptr(dist), C.byref(cnt)))
        return ids[:cnt.value], dist[:cnt.value]

    def scan_topk_batch_masked(self, metric, queries, k):
        """Corpus.scan_topk_batch_masked over all shards, merged per query by (distance, global scan position)"""
        return _scan_topk_batch_masked(lib().vg_shards_scan_topk_batch_masked, self.h, metric, queries, k)

    def scan_within(self, metric, query, radius, limit=None):
        """Corpus.scan_within over all shards, merged by (distance, global scan position): (rowids, distances, matches)"""
        return _scan_within(lib().vg_shards_scan_within, lib().vg_shards_scan_within_fetch, self.h, metric, query, radius, limit)

    def scan_within_masked(self, metric, query, radius, limit=None):
        """Corpus.scan_within_masked over all shards (each over its own bits), merged like scan_within"""
        return _scan_within(lib().vg_shards_scan_within_masked, lib().vg_shards_scan_within_fetch, self.h, metric, query, radius, limit)

    def scan_within_batch_masked(self, metric, queries, radii, limit=None):
        """Corpus.scan_within_batch_masked over all shards, merged per query by (distance, global scan position)"""
        return _scan_within_batch(lib().vg_shards_scan_within_batch_masked, lib().vg_shards_scan_within_batch_fetch, self.h, metric, queries, radii, limit)

    def set_within_initial_capacity(self, keys):
        _check(lib().vg_shards_within_set_initial_capacity(self.h, keys))

    def within_last_launches(self):
        return int(lib().vg_shards_within_last_launches(self.h))

    def scan_within_batch(self, metric, queries, radii, limit=None):
        """Corpus.scan_within_batch over all shards, merged per query by (distance, global scan position)"""
        return _scan_within_batch(lib().vg_shards_scan_within_batch, lib().vg_shards_scan_within_batch_fetch, self.h, metric, queries, radii, limit)

    def within_batch_plan(self, metric):
        return within_batch_plan(self, metric)

    def within_batch_masked_plan(self, metric):
        return within_batch_masked_plan(self, metric)

    def set_within_batch_initial_capacity(self, keys_per_query):
        set_within_batch_initial_capacity(self, keys_per_query)

    def within_batch_last_launches(self):
        return within_batch_last_launches(self)

    def scan_distances(self, metric, query):
        query = np.ascontiguousarray(query)
        out = np.empty(self.rows, dtype=np.float32)
        _check(lib().vg_shards_scan_distances(self.h, metric, _ptr(query), _ptr(out)))
        return out

    def minmax(self):
        lo, hi, neg = C.c_float(0), C.c_float(0), C.c_int(0)
        _check(lib().vg_shards_minmax(self.h, C.byref(lo), C.byref(hi), C.byref(neg)))
        return lo.value, hi.value, bool(neg.value)

    def quantize_rows(self, scale, offset, qtype, row0=0, n_rows=None):
        n = self.rows - row0 if n_rows is None else n_rows
        out = np.empty((n, self.dim), dtype=np.uint8)
        _check(lib().vg_shards_quantize_rows(self.h, scale, offset, qtype, row0, n, _ptr(out)))
        return out


def quantize_query(src_type, src, scale, offset, qtype):
    src = np.ascontiguousarray(src)
    dst = np.empty(src.shape[0], dtype=np.uint8 if qtype == QUANT_U8 else np.int8)
    _check(lib().vg_quantize_query(src_type, _ptr(src), src.shape[0], scale, offset, qtype, _ptr(dst)))
    return dst


def reference_topk_replay(dist, k, below_cap=0):
    """host replay of the reference's slot algorithm over a distance stream -> (positions, distances)"""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    pos = np.zeros(max(k, 1), dtype=np.int64)
    out = np.zeros(max(k, 1), dtype=np.float64)
    cnt = lib().vg_reference_topk_replay(_ptr(dist), dist.shape[0], k, below_cap, _ptr(pos), _ptr(out))
    if cnt < 0:
        raise VectorGpuError("vg_reference_topk_replay: bad arguments")
    return pos[:cnt], out[:cnt]


def reference_topk_replay_slabs(dist, k, slab_rows, below_cap=0):
    """the same stream handed over slab by slab (the out-of-core scan's continuation of the slot state) -> (positions, distances)"""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    pos = np.zeros(max(k, 1), dtype=np.int64)
    out = np.zeros(max(k, 1), dtype=np.float64)
    cnt = lib().vg_reference_topk_replay_slabs(_ptr(dist), dist.shape[0], k, slab_rows, below_cap, _ptr(pos), _ptr(out))
    if cnt < 0:
        raise VectorGpuError("vg_reference_topk_replay_slabs: bad arguments")
    return pos[:cnt], out[:cnt]


def merge_keys_batch(keys, pos_offsets, k):
    """keys: (n_lists, nq, list_len) uint64 -> (global positions [nq, k], distances [nq, k], counts [nq])."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n_lists, nq, list_len = keys.shape
    off = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.int64)
    pos = np.zeros((nq, max(k, 1)), dtype=np.int64)
    dist = np.zeros((nq, max(k, 1)), dtype=np.float64)
    cnt = np.zeros(nq, dtype=np.int32)
    if lib().vg_merge_keys_batch(_ptr(keys), n_lists, nq, list_len, _ptr(off), k, _ptr(pos), _ptr(dist), _ptr(cnt)) != 0:
        raise VectorGpuError("vg_merge_keys_batch: bad arguments")
    return pos, dist, cnt


def merge_keys(keys, pos_offsets, k):
    """keys: (n_lists, list_len) uint64 array of per-shard candidate lists -> (global positions, distances)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    n_lists, list_len = keys.shape
    off = None if pos_offsets is None else np.ascontiguousarray(pos_offsets, dtype=np.int64)
    pos = np.zeros(max(k, 1), dtype=np.int64)
    dist = np.zeros(max(k, 1), dtype=np.float64)
    cnt = lib().vg_merge_keys(_ptr(keys), n_lists, list_len, _ptr(off), k, _ptr(pos), _ptr(dist))
    return pos[:cnt], dist[:cnt]
