"""vg_merge_keys_capped (host only): the merge of several corpora's capped lists, against a python model of the four-step contract
(order by (distance, global position), keep a row iff fewer than per_label rows of its label are kept, first k).  With per_label = 1
it must be vg_merge_keys_grouped."""
import ctypes as C

import numpy as np
import pytest

import capped_cases as cc
import grouped_cases as gc

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
E = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def _lists(rows, list_len):
    """rows: per list a sequence of (distance, position, label), any order -> (keys, labels) sorted and padded"""
    keys = np.full((len(rows), list_len), E, dtype=np.uint64)
    labels = np.full((len(rows), list_len), gc.NONE, dtype=np.uint32)
    for l, ents in enumerate(rows):
        ents = sorted((gc.key(d, p), lab) for d, p, lab in ents)
        for j, (kk, lab) in enumerate(ents):
            keys[l, j] = kk
            labels[l, j] = lab
    return keys, labels


def _check(pkg, keys, labels, off, k, m, ctx=None):
    gk, gl = pkg.merge_keys_capped(keys, labels, off, k, m)
    wk, wl = cc.merge_model(keys, labels, off, k, m)
    assert gk.tolist() == wk and gl.tolist() == wl, ctx
    assert np.all(np.diff(gk.astype(object)) > 0), ctx
    assert len(gl) == 0 or np.unique(gl, return_counts=True)[1].max() <= m, ctx
    if m == 1:
        ok, ol = pkg.merge_keys_grouped(keys, labels, off, k)
        assert gk.tolist() == ok.tolist() and gl.tolist() == ol.tolist(), ctx
    return gk, gl


def test_random_lists_with_offsets_and_labels_repeated_across_lists(pkg):
    rng = np.random.default_rng(17)
    for trial in range(20):
        n_lists = int(rng.integers(1, 6))
        list_len = int(rng.integers(1, 65))
        n_labels = int(rng.integers(1, 30))
        rows = []
        for l in range(n_lists):
            cnt = int(rng.integers(0, list_len + 1))
            labs = rng.integers(0, n_labels, cnt)                # a label repeats inside a list and across lists
            labs[rng.random(cnt) < 0.1] = gc.NONE                # ... and some rows carry none
            pos = rng.permutation(1000)[:cnt]
            dist = rng.integers(0, 12, cnt).astype(np.float32) / 4 - 1       # few levels: equal distances are routine
            rows.append([(float(d), int(p), int(lb)) for d, p, lb in zip(dist, pos, labs)])
        keys, labels = _lists(rows, list_len)
        off = [1000 * l for l in range(n_lists)]
        for k in (1, 5, 20, 64):
            for m in (1, 3, k):
                _check(pkg, keys, labels, off, k, m, ctx=(trial, k, m))


def test_rows_of_one_label_compete_across_lists(pkg):
    rows = [[(1.0, 3, 10), (2.0, 4, 10), (2.5, 5, 11)],
            [(0.5, 0, 10), (3.0, 9, 12)],
            [(0.75, 7, 10), (0.8, 2, 11), (4.0, 1, 10)]]
    keys, labels = _lists(rows, 4)
    gk, gl = _check(pkg, keys, labels, [0, 100, 200], 5, 2)
    assert gl.tolist() == [10, 10, 11, 11, 12]
    assert [int(x) & 0xFFFFFFFF for x in gk] == [100, 207, 202, 5, 109]
    gk, gl = _check(pkg, keys, labels, [0, 100, 200], 5, 3)
    assert gl.tolist() == [10, 10, 11, 10, 11]
    gk, gl = _check(pkg, keys, labels, [0, 100, 200], 5, 1)
    assert gl.tolist() == [10, 11, 12]                           # fewer than k eligible entries
    gk, gl = _check(pkg, keys, labels, None, 64, 64)             # no offsets, no effective cap: every entry, in key order
    assert len(gk) == 8


def test_equal_distances_resolve_by_global_position(pkg):
    rows = [[(2.0, 50, 1), (2.0, 60, 1)],
            [(2.0, 5, 1), (2.0, 7, 3)],                          # global 105 / 107: behind list 0's rows
            [(2.0, 0, 1)]]                                       # global 20: in front of everything
    keys, labels = _lists(rows, 3)
    gk, gl = _check(pkg, keys, labels, [0, 100, 20], 4, 2)
    assert gl.tolist() == [1, 1, 3]
    assert [int(x) & 0xFFFFFFFF for x in gk] == [20, 50, 107]


def test_short_lists_none_labels_and_fewer_than_k_eligible(pkg):
    keys, labels = _lists([[], [(1.0, 1, 4), (2.0, 2, 4)], []], 8)      # lists of nothing but VG_KEY_EMPTY around a short one
    for m, n in ((1, 1), (2, 2), (3, 2)):
        gk, gl = _check(pkg, keys, labels, [0, 10, 20], 64, m)
        assert gl.tolist() == [4] * n and int(gk[0]) == gc.key(1.0, 11)
    assert len(_check(pkg, *_lists([[], []], 4), None, 5, 3)[0]) == 0
    keys, labels = _lists([[(1.0, 1, gc.NONE), (2.0, 2, 5), (3.0, 3, gc.NONE), (4.0, 4, 5)]], 4)
    assert _check(pkg, keys, labels, None, 4, 3)[1].tolist() == [5, 5]
    rows = [[(float(i), i, i % 9) for i in range(64)], [(float(i) + 0.5, i, (i * 7) % 11) for i in range(64)]]
    keys, labels = _lists(rows, 64)
    for k in (1, 20, 64):
        for m in (1, 3, k):
            gk, gl = _check(pkg, keys, labels, [0, 64], k, m)
            assert len(gk) == min(k, sum(min(m, int(c)) for c in np.unique(labels, return_counts=True)[1]))


def test_argument_errors(pkg):
    lib = pkg.lib()
    keys, labels = _lists([[(1.0, 1, 4)]], 4)
    ok = np.zeros(4, dtype=np.uint64); ol = np.zeros(4, dtype=np.uint32); cnt = C.c_int(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda kp, lp, nl, ll, k, m, okp, olp, cp: lib.vg_merge_keys_capped(kp, lp, nl, ll, None, k, m, okp, olp, cp)
    assert call(p(keys), p(labels), 1, 4, 2, 2, p(ok), p(ol), C.byref(cnt)) == 0 and cnt.value == 1
    for bad in ((None, p(labels), 1, 4, 2, 2, p(ok), p(ol), C.byref(cnt)), (p(keys), None, 1, 4, 2, 2, p(ok), p(ol), C.byref(cnt)),
                (p(keys), p(labels), 1, 4, 2, 2, None, p(ol), C.byref(cnt)), (p(keys), p(labels), 1, 4, 2, 2, p(ok), None, C.byref(cnt)),
                (p(keys), p(labels), 0, 4, 2, 2, p(ok), p(ol), C.byref(cnt)), (p(keys), p(labels), 1, 0, 2, 2, p(ok), p(ol), C.byref(cnt)),
                (p(keys), p(labels), 1, 4, 0, 2, p(ok), p(ol), C.byref(cnt)), (p(keys), p(labels), 1, 4, 2, 0, p(ok), p(ol), C.byref(cnt)),
                (p(keys), p(labels), 1, 4, 2, -1, p(ok), p(ol), C.byref(cnt))):
        cnt.value = 7
        assert call(*bad) == VG_ERR_INVALID, bad
        assert cnt.value == 0
    assert call(p(keys), p(labels), 1, 4, 2, 2, p(ok), p(ol), None) == VG_ERR_INVALID
    off = np.array([1 << 32], dtype=np.int64)                   # a global position beyond a key's 32 bits
    assert lib.vg_merge_keys_capped(p(keys), p(labels), 1, 4, p(off), 2, 2, p(ok), p(ol), C.byref(cnt)) == VG_ERR_UNSUPPORTED


def test_scan_entry_points_reject_a_bad_cap_without_a_device(pkg):
    """per_label < 1 is refused before anything touches a handle"""
    lib = pkg.lib()
    cnt = C.c_int(7)
    buf = np.zeros(64, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.vg_scan_topk_capped_keys(None, 1, p(buf), 5, 0, p(buf), p(buf), C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    assert lib.vg_scan_topk_capped_masked_keys(None, 1, p(buf), 5, 0, p(buf), p(buf), C.byref(cnt)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_capped(None, 1, p(buf), 5, 3, p(buf), p(buf), p(buf), C.byref(cnt)) == VG_ERR_INVALID      # NULL handle
