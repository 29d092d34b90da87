"""The capped batch scans' surface without a device: the C-ABI symbols are exported and bound, and the plan and the argument errors
that the grouped batch and the single capped scan answer before they touch a device (NULL, nq < 1, per_label < 1) are answered the
same way, with the same messages.  (No SQL modules: the capped scans have no SQL form - DESIGN.md 3.17 / 3.18 say why.)"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg

VG_ERR_INVALID = 1
SCANS = ("vg_scan_topk_batch_capped", "vg_scan_topk_batch_capped_masked")
KEYS = ("vg_scan_topk_batch_capped_keys", "vg_scan_topk_batch_capped_masked_keys")
SHARDS = ("vg_shards_scan_topk_batch_capped", "vg_shards_scan_topk_batch_capped_masked")
SYMBOLS = SCANS + KEYS + SHARDS + ("vg_batch_capped_plan",)


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
    assert callable(pkg.batch_capped_plan)
    for cls in (pkg.Corpus, pkg.Shards):
        assert callable(getattr(cls, "scan_topk_batch_capped"))


def test_plan_and_argument_errors_match_the_grouped_batch_and_the_single_capped_scan(pkg):
    lib = pkg.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.vg_last_error().decode()
    nq, lpr, u = C.c_int(7), C.c_int(7), C.c_int(7)
    # the plan: a NULL corpus, like vg_batch_grouped_plan
    for masked in (0, 1):
        assert lib.vg_batch_grouped_plan(None, dg.L2, masked, C.byref(nq), C.byref(lpr), C.byref(u)) == VG_ERR_INVALID
        want = err()
        assert lib.vg_batch_capped_plan(None, dg.L2, masked, C.byref(nq), C.byref(lpr), C.byref(u)) == VG_ERR_INVALID
        assert err() == want and "corpus is NULL" in want
    # NULL arguments, nq < 1 and per_label < 1 (answered before the handle is looked at: the handle here is zeroed memory no call may read)
    q = np.zeros((2, 8), dtype=np.float32)
    ids, dist = np.zeros((2, 5), dtype=np.int64), np.zeros((2, 5), dtype=np.float64)
    lab, keys = np.zeros((2, 5), dtype=np.uint32), np.zeros((2, 5), dtype=np.uint64)
    cnt = np.full(2, 7, dtype=np.int32)
    one = C.c_int(7)
    fake = np.zeros(1 << 16, dtype=np.uint8)

    def grouped_says(stem, *args):
        """the message of the grouped batch's entry point of the same form, with the capped name in place of its own"""
        twin = stem.replace("capped", "grouped")
        assert getattr(lib, twin)(*args) == VG_ERR_INVALID, twin
        return err().replace(twin, stem)

    for stem in SCANS + SHARDS:
        fn = getattr(lib, stem)
        want = grouped_says(stem, None, dg.L2, p(q), 2, 5, p(ids), p(dist), p(lab), p(cnt))
        assert fn(None, dg.L2, p(q), 2, 5, 3, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert err() == want and "NULL argument" in want, stem
        assert fn(p(fake), dg.L2, None, 2, 5, 3, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert fn(p(fake), dg.L2, p(q), 2, 5, 3, p(ids), p(dist), p(lab), None) == VG_ERR_INVALID, stem
        if "shards" in stem:                                    # (a shards handle is looked at first: how many shards it holds)
            continue
        want = grouped_says(stem, p(fake), dg.L2, p(q), 0, 5, p(ids), p(dist), p(lab), p(cnt))
        assert fn(p(fake), dg.L2, p(q), 0, 5, 3, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert err() == want and "nq must be at least 1" in want, stem
        # per_label < 1: the single capped scan's message, the counts zeroed first
        single = stem.replace("_batch", "")
        assert getattr(lib, single)(p(fake), dg.L2, p(q), 5, 0, p(ids), p(dist), p(lab), C.byref(one)) == VG_ERR_INVALID, single
        want = err().replace(single + ":", stem + ":")
        for m in (0, -2):
            cnt[:] = 7
            assert fn(p(fake), dg.L2, p(q), 2, 5, m, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem
            assert err() == want and "per_label must be at least 1" in want, stem
            assert not cnt.any(), stem
        cnt[:] = 7
        assert fn(p(fake), dg.L2, p(q), 2, 0, 3, p(ids), p(dist), p(lab), p(cnt)) == VG_ERR_INVALID, stem          # k = 0
        assert "k must be at least 1" in err() and not cnt.any(), stem
    for stem in KEYS:
        fn = getattr(lib, stem)
        assert fn(None, dg.L2, p(q), 2, 5, 3, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert "NULL argument" in err(), stem
        assert fn(p(fake), dg.L2, p(q), 0, 5, 3, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert fn(p(fake), dg.L2, p(q), -3, 5, 3, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert "nq must be at least 1" in err(), stem
        cnt[:] = 7
        assert fn(p(fake), dg.L2, p(q), 2, 5, 0, p(keys), p(lab), p(cnt)) == VG_ERR_INVALID, stem
        assert "per_label must be at least 1" in err() and not cnt.any(), stem
