"""The grouped batch scans' surface without a device: the C-ABI symbols are exported and bound, and the plan and the argument errors
that the other batch entry points answer before they touch a device (NULL, nq < 1) are answered the same way.  (No SQL modules: the
grouped scans have no SQL form - DESIGN.md 3.16 says why.)"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg

VG_ERR_INVALID = 1
SYMBOLS = ("vg_scan_topk_batch_grouped", "vg_scan_topk_batch_grouped_keys", "vg_scan_topk_batch_grouped_masked",
           "vg_scan_topk_batch_grouped_masked_keys", "vg_shards_scan_topk_batch_grouped", "vg_shards_scan_topk_batch_grouped_masked",
           "vg_batch_grouped_plan")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def test_symbols_are_exported_and_bound(pkg):
    lib = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), "libvectorgpu.so does not export %s" % name
        assert name in lib._sig, "the ctypes table does not bind %s" % name
    assert callable(pkg.batch_grouped_plan)
    for cls in (pkg.Corpus, pkg.Shards):
        assert callable(getattr(cls, "scan_topk_batch_grouped"))


def test_plan_and_argument_errors_match_the_other_batch_entry_points(pkg):
    lib = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nq, lpr, u = C.c_int(7), C.c_int(7), C.c_int(7)
    # the plan: a NULL corpus, like vg_batch_masked_plan
    assert lib.vg_batch_masked_plan(None, dg.L2, C.byref(nq), C.byref(lpr), C.byref(u)) == VG_ERR_INVALID
    for masked in (0, 1):
        assert lib.vg_batch_grouped_plan(None, dg.L2, masked, C.byref(nq), C.byref(lpr), C.byref(u)) == VG_ERR_INVALID
    assert "corpus is NULL" in lib.vg_last_error().decode()
    # NULL arguments, and nq < 1 (answered before the handle is looked at: the handle here is zeroed memory no call may read)
    q = np.zeros((2, 8), dtype=np.float32)
    ids, dist = np.zeros((2, 5), dtype=np.int64), np.zeros((2, 5), dtype=np.float64)
    lab, keys = np.zeros((2, 5), dtype=np.uint32), np.zeros((2, 5), dtype=np.uint64)
    cnt = np.full(2, 7, dtype=np.int32)
    fake = np.zeros(1 << 16, dtype=np.uint8)
    assert lib.vg_scan_topk_batch_masked(None, dg.L2, p(q), 2, 5, p(ids), p(dist), p(cnt)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_batch_masked(p(fake), dg.L2, p(q), 0, 5, p(ids), p(dist), p(cnt)) == VG_ERR_INVALID
    for stem in ("vg_scan_topk_batch_grouped", "vg_scan_topk_batch_grouped_masked", "vg_shards_scan_topk_batch_grouped",
                 "vg_shards_scan_topk_batch_grouped_masked"):
        fn = getattr(lib, stem)
        assert fn(None, dg.L2, p(q), 2, 5, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert "NULL argument" in lib.vg_last_error().decode(), stem
        assert fn(p(fake), dg.L2, None, 2, 5, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert fn(p(fake), dg.L2, p(q), 2, 5, p(ids), p(dist), p(lab), None) == VG_ERR_INVALID, stem
        if "shards" not in stem:                                # (a shards handle is looked at first: how many shards it holds)
            assert fn(p(fake), dg.L2, p(q), 0, 5, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
            assert "nq must be at least 1" in lib.vg_last_error().decode(), stem
    for stem in ("vg_scan_topk_batch_grouped_keys", "vg_scan_topk_batch_grouped_masked_keys"):
        fn = getattr(lib, stem)
        assert fn(None, dg.L2, p(q), 2, 5, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert fn(p(fake), dg.L2, p(q), 0, 5, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert fn(p(fake), dg.L2, p(q), -3, 5, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem

