"""CPU-only checks of the label-set scans' host side: labelset_csr (the per-query sets of scan_topk_batch_labelset in CSR form) and the
C symbols of the four families - no device needed."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def test_list_array_and_pair_input(pkg):
    sets = [[3, 1, 2], [], np.array([7], dtype=np.uint32), (9, 9, 0), np.array([], dtype=np.int64), [4294967294]]
    flat, off = pkg.labelset_csr(sets)
    assert flat.dtype == np.uint32 and off.dtype == np.int64 and flat.flags.c_contiguous and off.flags.c_contiguous
    assert flat.tolist() == [3, 1, 2, 7, 9, 9, 0, 4294967294]      # the caller's order and duplicates: normalising is the engine's job
    assert off.tolist() == [0, 3, 3, 4, 7, 7, 8]
    # an array of equal-length sets is a sequence of sets
    flat2, off2 = pkg.labelset_csr(np.array([[1, 2], [2, 2], [5, 0]]))
    assert flat2.tolist() == [1, 2, 2, 2, 5, 0] and off2.tolist() == [0, 2, 4, 6]
    # a (flat, offsets) pair is validated and passed through
    flat3, off3 = pkg.labelset_csr((flat, off))
    assert np.array_equal(flat3, flat) and np.array_equal(off3, off)
    flat4, off4 = pkg.labelset_csr(([5, 5, 1], [0, 0, 3]))
    assert flat4.tolist() == [5, 5, 1] and off4.tolist() == [0, 0, 3] and flat4.dtype == np.uint32 and off4.dtype == np.int64
    # two sets are a LIST of two; no sets at all
    assert pkg.labelset_csr([[1, 2], [0, 2]])[1].tolist() == [0, 2, 4]
    flat5, off5 = pkg.labelset_csr([])
    assert flat5.size == 0 and off5.tolist() == [0]
    assert pkg.labelset_csr([[], []])[1].tolist() == [0, 0, 0]


def test_rejections(pkg):
    for bad in ([[1, pkg.LABEL_NONE]], [[-1]], [[1.5]], [[0], [2 ** 32]], ([1, pkg.LABEL_NONE], [0, 2]), ([-3], [0, 1])):
        with pytest.raises(ValueError):
            pkg.labelset_csr(bad)
    for off in ([1, 2], [0, 1], [0, 2, 1, 3], [0, 4], [], [[0, 3]], [0.0, 3.0]):
        with pytest.raises(ValueError):
            pkg.labelset_csr(([1, 2, 3], off))


def test_symbols_and_constants(pkg):
    lib = pkg.lib()
    for name in ("vg_scan_topk_labelset", "vg_scan_topk_labelset_keys", "vg_scan_topk_grouped_labelset", "vg_scan_topk_grouped_labelset_keys",
                 "vg_scan_topk_capped_labelset", "vg_scan_topk_capped_labelset_keys", "vg_scan_topk_batch_labelset",
                 "vg_scan_topk_batch_labelset_keys", "vg_batch_labelset_plan", "vg_shards_scan_topk_labelset",
                 "vg_shards_scan_topk_batch_labelset", "vg_shards_scan_topk_grouped_labelset", "vg_shards_scan_topk_capped_labelset"):
        assert hasattr(lib, name), name
    for cls in (pkg.Corpus, pkg.Shards):
        for m in ("scan_topk_labelset", "scan_topk_batch_labelset", "scan_topk_grouped_labelset", "scan_topk_capped_labelset"):
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(pkg.batch_labelset_plan)
    # NULL handles are refused by the argument checks, before any device is touched
    import ctypes as C
    cnt = C.c_int(5)
    assert lib.vg_scan_topk_labelset(None, pkg.L2, None, 5, None, 0, 0, None, None, C.byref(cnt)) == 1
    assert lib.vg_scan_topk_batch_labelset(None, pkg.L2, None, 1, 5, None, None, 0, None, None, None) == 1
    assert lib.vg_shards_scan_topk_grouped_labelset(None, pkg.L2, None, 5, None, 0, 0, None, None, None, C.byref(cnt)) == 1
    assert lib.vg_shards_scan_topk_capped_labelset(None, pkg.L2, None, 5, 0, None, 0, 0, None, None, None, C.byref(cnt)) == 1
