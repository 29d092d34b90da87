"""vg_merge_keys_grouped (host only): the label-deduping merge of several corpora's grouped lists, against a python model of the
three-step contract (order by (distance, global position), first row of each label, first k)."""
import ctypes as C

import numpy as np
import pytest

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


def _check(pkg, keys, labels, off, k, ctx=None):
    gk, gl = pkg.merge_keys_grouped(keys, labels, off, k)
    wk, wl = gc.merge_model(keys, labels, off, k)
    assert gk.tolist() == wk and gl.tolist() == wl, ctx
    assert len(set(gl.tolist())) == len(gl) and np.all(np.diff(gk.astype(object)) > 0), ctx
    return gk, gl


def test_random_lists_with_labels_shared_across_lists(pkg):
    rng = np.random.default_rng(7)
    for trial in range(20):
        n_lists = int(rng.integers(1, 6))
        list_len = int(rng.integers(1, 65))
        n_labels = int(rng.integers(1, 90))
        rows = []
        for l in range(n_lists):
            cnt = int(rng.integers(0, list_len + 1))
            labs = rng.permutation(n_labels)[:cnt]               # a list is distinct by label, like a grouped scan's
            pos = rng.permutation(1000)[:len(labs)]
            dist = rng.integers(0, 12, len(labs)).astype(np.float32) / 4 - 1       # few levels: equal distances are routine
            rows.append([(float(d), int(p), int(lb)) for d, p, lb in zip(dist, pos, labs)])
        keys, labels = _lists(rows, list_len)
        off = [1000 * l for l in range(n_lists)]
        for k in (1, 5, 64):
            _check(pkg, keys, labels, off, k, ctx=(trial, k))


def test_best_key_of_a_label_in_the_last_list(pkg):
    rows = [[(1.0, 3, 10), (2.0, 4, 11)],
            [(1.5, 0, 10), (3.0, 9, 12)],
            [(0.5, 7, 11), (0.75, 2, 10)]]                       # the best rows of labels 10 and 11 sit in the last list
    keys, labels = _lists(rows, 4)
    gk, gl = _check(pkg, keys, labels, [0, 100, 200], 5)
    assert gl.tolist() == [11, 10, 12]
    assert [int(x) & 0xFFFFFFFF for x in gk] == [207, 202, 109]
    assert [pkg.lib().vg_key_distance(C.c_uint64(int(x))) for x in gk] == [0.5, 0.75, 3.0]


def test_equal_distances_resolve_by_global_position(pkg):
    rows = [[(2.0, 50, 1), (2.0, 60, 2)],
            [(2.0, 5, 1), (2.0, 7, 3)],                          # global 105 / 107: behind list 0's rows
            [(2.0, 0, 2)]]                                       # global 20: in front of everything
    keys, labels = _lists(rows, 3)
    gk, gl = _check(pkg, keys, labels, [0, 100, 20], 3)
    assert gl.tolist() == [2, 1, 3]
    assert [int(x) & 0xFFFFFFFF for x in gk] == [20, 50, 107]
    gk, gl = _check(pkg, keys, labels, None, 3)                  # no offsets: positions as they are
    assert [int(x) & 0xFFFFFFFF for x in gk] == [0, 5, 7] and gl.tolist() == [2, 1, 3]


def test_padding_k_beyond_the_labels_and_k_1_and_64(pkg):
    keys, labels = _lists([[], [(1.0, 1, 4)], []], 8)            # lists of nothing but VG_KEY_EMPTY
    gk, gl = _check(pkg, keys, labels, [0, 10, 20], 64)
    assert gl.tolist() == [4] and int(gk[0]) == gc.key(1.0, 11)
    assert len(_check(pkg, _lists([[], []], 4)[0], _lists([[], []], 4)[1], None, 5)[0]) == 0
    rows = [[(float(i), i, 100 + i) for i in range(64)], [(float(i) + 0.5, i, 100 + (i * 7) % 80) for i in range(64)]]
    keys, labels = _lists(rows, 64)
    for k in (1, 64):
        gk, gl = _check(pkg, keys, labels, [0, 64], k)
        assert len(gk) == k
    gk, gl = _check(pkg, keys, labels, [0, 64], 200)             # k larger than the number of labels: every label once
    assert len(gl) == len(set(labels.reshape(-1).tolist()))
    # a row without a label inside a list is skipped
    keys, labels = _lists([[(1.0, 1, gc.NONE), (2.0, 2, 5)]], 4)
    assert _check(pkg, keys, labels, None, 4)[1].tolist() == [5]


def test_argument_errors(pkg):
    lib = pkg.lib()
    keys, labels = _lists([[(1.0, 1, 4)]], 4)
    ok = np.zeros(4, dtype=np.uint64); ol = np.zeros(4, dtype=np.uint32); cnt = C.c_int(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda kp, lp, nl, ll, k, okp, olp, cp: lib.vg_merge_keys_grouped(kp, lp, nl, ll, None, k, okp, olp, cp)
    assert call(p(keys), p(labels), 1, 4, 2, p(ok), p(ol), C.byref(cnt)) == 0 and cnt.value == 1
    for bad in ((None, p(labels), 1, 4, 2, p(ok), p(ol), C.byref(cnt)), (p(keys), None, 1, 4, 2, p(ok), p(ol), C.byref(cnt)),
                (p(keys), p(labels), 1, 4, 2, None, p(ol), C.byref(cnt)), (p(keys), p(labels), 1, 4, 2, p(ok), None, C.byref(cnt)),
                (p(keys), p(labels), 0, 4, 2, p(ok), p(ol), C.byref(cnt)), (p(keys), p(labels), 1, 0, 2, p(ok), p(ol), C.byref(cnt)),
                (p(keys), p(labels), 1, 4, 0, p(ok), p(ol), C.byref(cnt))):
        cnt.value = 7
        assert call(*bad) == VG_ERR_INVALID, bad
        assert cnt.value == 0
    assert call(p(keys), p(labels), 1, 4, 2, p(ok), p(ol), None) == VG_ERR_INVALID
    off = np.array([1 << 32], dtype=np.int64)                   # a global position beyond a key's 32 bits
    assert lib.vg_merge_keys_grouped(p(keys), p(labels), 1, 4, p(off), 2, p(ok), p(ol), C.byref(cnt)) == VG_ERR_UNSUPPORTED
