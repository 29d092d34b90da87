"""The refusals of the shard layer's fused scan forms that are answered before a handle is read, and of the two host label merges,
word for word - without a device.

Every vg_shards_scan_topk_* entry point of the masked, labeled, label-set, grouped, capped and paged forms is called with a NULL
handle, a NULL query and a NULL count pointer; vg_merge_keys_grouped / _capped with NULL lists, n_lists < 1 and a global position
that does not fit a key.  The messages are literals, recorded before the shard layer's entry points were folded onto one scaffold
(point 4): a message names the function the text below says it names, not the one that was called."""
import ctypes as C

import numpy as np
import pytest

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
KEY_EMPTY = 0xFFFFFFFFFFFFFFFF

# entry point (without the vg_shards_scan_topk_ prefix) -> the name its "NULL argument" carries
NULL_ARGUMENT = {
    "masked": "vg_shards_scan_topk_masked",
    "batch_masked": "vg_shards_scan_topk_batch_masked",
    "labeled": "vg_shards_scan_topk_labeled",
    "batch_labeled": "vg_shards_scan_topk_batch_labeled",
    "labelset": "vg_shards_scan_topk_labelset",
    "batch_labelset": "vg_shards_scan_topk_batch_labelset",
    "grouped": "vg_shards_scan_topk_grouped",
    "grouped_masked": "vg_shards_scan_topk_grouped",
    "batch_grouped": "vg_shards_scan_topk_batch_grouped",
    "batch_grouped_masked": "vg_shards_scan_topk_batch_grouped_masked",
    "capped": "vg_shards_scan_topk_capped",
    "capped_masked": "vg_shards_scan_topk_capped",
    "batch_capped": "vg_shards_scan_topk_batch_capped",
    "batch_capped_masked": "vg_shards_scan_topk_batch_capped_masked",
    "grouped_labelset": "vg_shards_scan_topk_grouped_labelset",
    "capped_labelset": "vg_shards_scan_topk_capped_labelset",
    # the paged scans answer in the name of the corpus entry point, the _keys forms in the name of their rowid twin
    "after": "vg_scan_topk_after",
    "after_keys": "vg_scan_topk_after",
    "after_masked": "vg_scan_topk_after_masked",
    "after_masked_keys": "vg_scan_topk_after_masked",
    "batch_after": "vg_scan_topk_batch_after",
    "batch_after_keys": "vg_scan_topk_batch_after",
    "batch_after_masked": "vg_scan_topk_batch_after_masked",
    "batch_after_masked_keys": "vg_scan_topk_batch_after_masked",
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package().lib()


def _arguments(lib, name, keep):
    """valid-looking arguments for `name` after its ctypes signature: every pointer at zeroed memory no call may read before it has
    refused (the handle too), every integer 3 (nq, k, per_label, exclude, n_labels), cursors 0; `keep` holds what they point at"""
    args = []
    for t in lib._sig[name][1]:
        if t is C.c_void_p:
            keep.append(np.zeros(1 << 12, dtype=np.uint8))
            args.append(keep[-1].ctypes.data_as(C.c_void_p))
        elif t is C.c_double:
            args.append(0.0)
        elif t in (C.c_int32, C.c_int, C.c_int64, C.c_uint32, C.c_uint64):
            args.append(3)
        else:                                                   # POINTER(int32): the single forms' count
            keep.append(C.c_int(7))
            args.append(C.byref(keep[-1]))
    return args


@pytest.mark.parametrize("stem", sorted(NULL_ARGUMENT))
def test_null_handle_query_and_count_pointer(lib, stem):
    name = "vg_shards_scan_topk_" + stem
    want = NULL_ARGUMENT[stem] + ": NULL argument"
    n_args = len(lib._sig[name][1])
    for null_at in (0, 2, n_args - 1):                          # the handle, the query / queries, the count(s)
        keep = []
        args = _arguments(lib, name, keep)
        args[null_at] = None
        assert getattr(lib, name)(*args) == VG_ERR_INVALID, (name, null_at)
        assert lib.vg_last_error().decode() == want, (name, null_at)


def test_the_fused_forms_are_all_here(lib):
    """every vg_shards_scan_topk_* the library binds, but the plain scan and its batch, is in the table above"""
    bound = {n[len("vg_shards_scan_topk_"):] for n in lib._sig if n.startswith("vg_shards_scan_topk_")}
    assert bound - {"batch"} == set(NULL_ARGUMENT)


def test_host_label_merges(lib):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vg_last_error().decode()
    keys = np.array([[(5 << 32) | 1, KEY_EMPTY]], dtype=np.uint64)
    labels = np.array([[4, 0xFFFFFFFF]], dtype=np.uint32)
    far = np.array([1 << 32], dtype=np.int64)                   # list 0 starts at global position 2^32
    out_keys, out_labels = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint32)
    for fn, extra, who, least in ((lib.vg_merge_keys_grouped, (), "vg_merge_keys_grouped", "n_lists, list_len and k must be at least 1"),
                                  (lib.vg_merge_keys_capped, (2,), "vg_merge_keys_capped", "n_lists, list_len, k and per_label must be at least 1")):
        cnt = C.c_int(7)
        assert fn(None, p(labels), 1, 2, None, 4, *extra, p(out_keys), p(out_labels), C.byref(cnt)) == VG_ERR_INVALID
        assert err() == who + ": NULL argument" and cnt.value == 0
        cnt = C.c_int(7)
        assert fn(p(keys), p(labels), 0, 2, None, 4, *extra, p(out_keys), p(out_labels), C.byref(cnt)) == VG_ERR_INVALID
        assert err() == who + ": " + least and cnt.value == 0
        cnt = C.c_int(7)
        assert fn(p(keys), p(labels), 1, 2, p(far), 4, *extra, p(out_keys), p(out_labels), C.byref(cnt)) == VG_ERR_UNSUPPORTED
        assert err() == who + ": a global position does not fit a key's 32 bits" and cnt.value == 0
        # (and the same list where it fits: one row, its position moved by the offset)
        near = np.array([10], dtype=np.int64)
        assert fn(p(keys), p(labels), 1, 2, p(near), 4, *extra, p(out_keys), p(out_labels), C.byref(cnt)) == 0
        assert cnt.value == 1 and int(out_keys[0]) == (5 << 32) | 11 and int(out_labels[0]) == 4

