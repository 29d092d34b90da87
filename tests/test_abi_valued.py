"""The value-range entry points without a device: every one refuses a NULL handle with VG_ERR_INVALID - the count(s) zeroed first
where it has any - instead of touching anything, and the Python surface has the methods on Corpus and Shards.  No GPU."""
import ctypes as C

import numpy as np
import pytest

VG_ERR_INVALID = 1


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def test_every_valued_entry_point_refuses_null_handles(pkg):
    lib = pkg.lib()
    buf = np.zeros(64, dtype=np.uint64)
    lo = np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b = p(buf)
    for prefix in ("vg_corpus", "vg_shards"):
        assert getattr(lib, prefix + "_set_values")(None, p(lo), 4) == VG_ERR_INVALID
        assert getattr(lib, prefix + "_clear_values")(None) == VG_ERR_INVALID
        assert getattr(lib, prefix + "_has_values")(None) == 0
    single = {
        "scan_topk_valued": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, b, b, cnt),
        "scan_topk_valued_labeled": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, 3, b, b, cnt),
        "scan_topk_grouped_valued": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, b, b, b, cnt),
        "scan_topk_capped_valued": lambda fn, cnt: fn(None, 1, b, 5, 2, 0, 9, b, b, b, cnt),
    }
    keys = {
        "scan_topk_valued_keys": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, b, cnt),
        "scan_topk_valued_labeled_keys": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, 3, b, cnt),
        "scan_topk_grouped_valued_keys": lambda fn, cnt: fn(None, 1, b, 5, 0, 9, b, b, cnt),
        "scan_topk_capped_valued_keys": lambda fn, cnt: fn(None, 1, b, 5, 2, 0, 9, b, b, cnt),
    }
    for name, call in list(single.items()) + list(keys.items()):
        cnt = C.c_int(7)
        assert call(getattr(lib, "vg_" + name), C.byref(cnt)) == VG_ERR_INVALID, name
    # over shards the five top-k forms are vg_shards_valued_scan_topk[_labeled | _grouped | _capped | _batch]
    shard_of = {"scan_topk_valued": "", "scan_topk_valued_labeled": "_labeled", "scan_topk_grouped_valued": "_grouped", "scan_topk_capped_valued": "_capped"}
    for name, call in single.items():
        cnt = C.c_int(7)
        assert call(getattr(lib, "vg_shards_valued_scan_topk" + shard_of[name]), C.byref(cnt)) == VG_ERR_INVALID, name
    # per_label < 1 is refused before anything touches a handle, the count zeroed first
    for fn in (lib.vg_scan_topk_capped_valued, lib.vg_shards_valued_scan_topk_capped):
        cnt = C.c_int(7)
        assert fn(None, 1, b, 5, 0, 0, 9, b, b, b, C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    cnt = C.c_int(7)
    assert lib.vg_scan_topk_capped_valued_keys(None, 1, b, 5, 0, 0, 9, b, b, C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    for fn in (lib.vg_scan_within_valued, lib.vg_shards_scan_within_valued):
        m, h = C.c_int64(7), C.c_int64(7)
        assert fn(None, 1, b, 1.0, 0, 0, 9, C.byref(m), C.byref(h)) == VG_ERR_INVALID and m.value == 0 and h.value == 0
    counts = np.full(4, 7, dtype=np.int32)
    assert lib.vg_scan_topk_batch_valued(None, 1, b, 4, 5, p(lo), p(lo), None, b, b, p(counts)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_batch_valued_keys(None, 1, b, 4, 5, p(lo), p(lo), None, b, p(counts)) == VG_ERR_INVALID
    assert lib.vg_shards_valued_scan_topk_batch(None, 1, b, 4, 5, p(lo), p(lo), None, b, b, p(counts)) == VG_ERR_INVALID
    assert lib.vg_batch_valued_plan(None, 1, None, None, None) == VG_ERR_INVALID


def test_python_surface(pkg):
    for cls in (pkg.Corpus, pkg.Shards):
        for name in ("set_values", "clear_values", "has_values", "scan_topk_valued", "scan_topk_batch_valued", "scan_topk_grouped_valued",
                     "scan_topk_capped_valued", "scan_within_valued"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert callable(pkg.batch_valued_plan)
    assert pkg.VALUE_MIN == -(1 << 63) and pkg.VALUE_MAX == (1 << 63) - 1
    if pkg.device_count() < 1:                                  # no silent fallback: without a device there is no handle to ask
        with pytest.raises(pkg.VectorGpuError):
            pkg.Corpus(pkg.F32, 8)
