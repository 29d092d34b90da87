"""Label-set scans, single forms (vg_scan_topk_labelset, vg_scan_topk_grouped_labelset, vg_scan_topk_capped_labelset): the rows whose
label is in a set of labels, or - exclude - is a label and not in it.

Contract (include/vectorgpu.h): the masked / grouped-masked / capped-masked contract with "allowed" decided by the set; the handle's row
mask is neither read nor written.  Everything here is exact: rowids, order, distance bits, labels.

  * every shape x layout (labeled_cases.layouts + `unique`) x set (empty, one, three with an absent label, 70, every label present,
    duplicates in descending order) x exclude: scan_topk_labelset against scan_distances of the same handle filtered here, k in
    (1, 20, 64); the grouped and capped (per_label 1 and 3) forms against set_mask(allowed) + the masked form;
  * a one-label set is scan_topk_labeled; exclude over S is include over the present labels not in S;
  * four pages of 5 by exclusion are the first 20 of the grouped order, on a layout where one label owns the 64 nearest rows;
  * the row mask survives and changes no answer; re-set_labels is seen (no stale bitmap); error codes; 3 logical shards == one corpus.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
import labelset_cases as ls

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
KS = (1, 20, 64)


@pytest.fixture(scope="module")
def pkg():
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import __graft_entry__ as g
    p = g.load_package()
    if p.device_count() < 1:
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    return p


def assert_same3(got, want, ctx=None):
    lc.assert_same(got[:2], want[0], want[1], ctx=ctx)
    assert np.asarray(got[2]).tolist() == np.asarray(want[2]).tolist(), ctx


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape_layout_and_set(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 61 + dim)
    q = lc.data(vt, 1, dim, 62 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    user_mask = np.random.default_rng(dim).random(n) < 0.4
    for metric in metrics:
        own = c.scan_distances(metric, q)
        for lname, labels in ls.layouts(n).items():
            c.set_labels(labels)
            c.clear_mask()
            have = ls.present(labels)
            got = {}
            for sname, s in ls.sets_for(labels).items():
                for ex in (False, True):
                    for k in KS:
                        got[(sname, ex, k)] = c.scan_topk_labelset(metric, q, k, s, exclude=ex)
                    got[(sname, ex, "g")] = c.scan_topk_grouped_labelset(metric, q, 20, s, exclude=ex)
                    for m in (1, 3):
                        got[(sname, ex, "c", m)] = c.scan_topk_capped_labelset(metric, q, 20, m, s, exclude=ex)
            # with a row mask on the handle: the same answers, and the mask is what it was
            assert c.set_mask(bits=user_mask) == int(user_mask.sum())
            mask_before = c.scan_topk_masked(metric, q, 20)
            for sname, s in ls.sets_for(labels).items():
                for ex in (False, True):
                    lc.assert_same(c.scan_topk_labelset(metric, q, 20, s, exclude=ex), *got[(sname, ex, 20)], ctx=(lname, sname, ex, "under a mask"))
                    assert_same3(c.scan_topk_grouped_labelset(metric, q, 20, s, exclude=ex), got[(sname, ex, "g")], ctx=(lname, sname, ex, "grouped under a mask"))
            assert c.mask_count() == int(user_mask.sum())
            lc.assert_same(c.scan_topk_masked(metric, q, 20), *mask_before, ctx=(lname, "mask after"))
            for sname, s in ls.sets_for(labels).items():
                for ex in (False, True):
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, sname, ex)
                    allow = ls.allowed(labels, s, ex)
                    for k in KS:
                        lc.assert_same(got[(sname, ex, k)], *lc.expected(own, allow, k), ctx=ctx + (k,))
                    if sname == "empty":
                        assert len(got[(sname, ex, 20)][0]) == (min(20, int((labels != ls.NONE).sum())) if ex else 0), ctx
                    if sname == "one" and not ex:
                        lc.assert_same(got[(sname, ex, 20)], *c.scan_topk_labeled(metric, q, 20, int(s[0])), ctx=ctx + ("labeled",))
                    if ex:                                       # exclude over S == include over the present labels not in S
                        rest = np.setdiff1d(have, np.asarray(s, dtype=np.int64).astype(np.uint32))
                        lc.assert_same(got[(sname, ex, 20)], *c.scan_topk_labelset(metric, q, 20, rest), ctx=ctx + ("complement",))
                    c.set_mask(bits=allow)
                    assert_same3(got[(sname, ex, "g")], c.scan_topk_grouped(metric, q, 20, masked=True), ctx=ctx + ("grouped",))
                    for m in (1, 3):
                        assert_same3(got[(sname, ex, "c", m)], c.scan_topk_capped(metric, q, 20, m, masked=True), ctx=ctx + ("capped", m))
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64), (dg.F16, 384)], ids=["f32-384", "u8-64", "f16-384"])
def test_paging_grouped_results_by_exclusion(pkg, vt, dim):
    n = lc.N
    rows = lc.data(vt, n, dim, 71 + dim)
    q = lc.data(vt, 1, dim, 72 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    # `hot`: one label owns the 64 nearest rows; the others are spread over 40 labels, some rows carry none
    rng = np.random.default_rng(7)
    labels = rng.integers(0, 40, n).astype(np.uint32)
    labels[rng.random(n) < 0.1] = ls.NONE
    labels[np.lexsort((np.arange(n), own))[:64]] = 1000
    c.set_labels(labels)
    order = ls.grouped_order(own, labels, np.ones(n, dtype=bool))
    assert labels[order[0]] == 1000 and len(order) >= 20
    seen, ids, dist, labs = [], [], [], []
    for page in range(4):
        pi, pd, pl = c.scan_topk_grouped_labelset(dg.L2, q, 5, np.array(seen, dtype=np.int64), exclude=True)
        assert len(pi) == 5 and not set(pl.tolist()) & set(seen), page
        seen += pl.tolist(); ids += pi.tolist(); dist += pd.tolist(); labs += pl.tolist()
    lc.assert_same((np.array(ids), np.array(dist)), order[:20] + 1, own[order[:20]], ctx="pages")
    assert labs == labels[order[:20]].tolist()
    c.close()


def test_relabeling_is_seen_and_words_of_the_bitmap(pkg):
    dim = 64
    rows = lc.data(dg.U8, 130, dim, 5)
    q = lc.data(dg.U8, 1, dim, 6)[0]
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    labels = (np.arange(130) % 7).astype(np.uint32)
    labels[64] = 50; labels[129] = 51; labels[10] = ls.NONE
    c.set_labels(labels)
    for s in ([50, 51], [3], [50, 3, 51, 3]):
        for ex in (False, True):
            for k in (5, 64):
                lc.assert_same(c.scan_topk_labelset(dg.L2, q, k, s, exclude=ex), *lc.expected(own, ls.allowed(labels, s, ex), k), ctx=(s, ex, k))
    assert sorted(c.scan_topk_labelset(dg.L2, q, 5, [50, 51])[0].tolist()) == [65, 130]
    # other labels, the same call: the new answer (no stale bitmap, no stale membership)
    qs = np.ascontiguousarray(np.repeat(q[None, :], 5, axis=0))
    before = c.scan_topk_batch_labelset(dg.L2, qs, [[50, 51]] * 5, 5)
    relabeled = np.roll(labels, 3)
    c.set_labels(relabeled)
    lc.assert_same(c.scan_topk_labelset(dg.L2, q, 5, [50, 51]), *lc.expected(own, ls.allowed(relabeled, [50, 51], False), 5))
    assert sorted(c.scan_topk_labelset(dg.L2, q, 5, [50, 51])[0].tolist()) == [3, 68]
    after = c.scan_topk_batch_labelset(dg.L2, qs, [[50, 51]] * 5, 5)
    assert before[2].tolist() == [2] * 5 and after[2].tolist() == [2] * 5
    assert sorted(after[0][4, :2].tolist()) == [3, 68] and sorted(before[0][4, :2].tolist()) == [65, 130]
    c.close()


def test_contract(pkg):
    n, dim = 2001, 100
    rows = lc.data(dg.F32, n, dim, 21)
    q = lc.data(dg.F32, 1, dim, 22)[0]
    labels = np.random.default_rng(3).integers(0, 4, n).astype(np.uint32)
    labels[::9] = ls.NONE
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    calls = {
        "topk": lambda k, s, ex=False: c.scan_topk_labelset(dg.L2, q, k, s, exclude=ex),
        "grouped": lambda k, s, ex=False: c.scan_topk_grouped_labelset(dg.L2, q, k, s, exclude=ex),
        "capped": lambda k, s, ex=False: c.scan_topk_capped_labelset(dg.L2, q, k, 2, s, exclude=ex),
    }
    lib = pkg.lib()
    none_set = np.array([1, ls.NONE], dtype=np.uint32)           # (the Python layer refuses LABEL_NONE itself: through the C symbols)
    out_i, out_d, out_l = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.float64), np.zeros(64, dtype=np.uint32)
    import ctypes as C
    cnt = C.c_int(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, call in calls.items():
        assert lc.error_code(pkg, lambda: call(5, [1])) == VG_ERR_INVALID, name                       # no labels
    c.set_labels(labels)
    for name, call in calls.items():
        assert lc.error_code(pkg, lambda: call(0, [1])) == VG_ERR_INVALID, name
        assert lc.error_code(pkg, lambda: call(65, [1])) == VG_ERR_UNSUPPORTED, name
        assert len(call(5, [])[0]) == 0, name                                                         # an empty set: nothing, no error
        assert len(call(5, [], True)[0]) == (4 if name == "grouped" else 5), name                     # ... excluded: every labeled row (4 labels)
        assert (labels[call(64, [], True)[0] - 1] != ls.NONE).all(), name
        with pytest.raises(ValueError):
            call(5, [1, ls.NONE])
        with pytest.raises(ValueError):
            call(5, [-1])
    assert lib.vg_scan_topk_labelset(c.h, dg.L2, ptr(q), 5, ptr(none_set), 2, 0, ptr(out_i), ptr(out_d), C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    assert lib.vg_scan_topk_grouped_labelset(c.h, dg.L2, ptr(q), 5, ptr(none_set), 2, 1, ptr(out_i), ptr(out_d), ptr(out_l), C.byref(cnt)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_capped_labelset(c.h, dg.L2, ptr(q), 5, 2, ptr(none_set), 2, 0, ptr(out_i), ptr(out_d), ptr(out_l), C.byref(cnt)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_labelset(c.h, dg.L2, ptr(q), 5, ptr(none_set), -1, 0, ptr(out_i), ptr(out_d), C.byref(cnt)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped_labelset(dg.L2, q, 5, 0, [1])) == VG_ERR_INVALID     # per_label < 1
    assert lc.error_code(pkg, lambda: c.scan_topk_labelset(99, q, 5, [1])) == VG_ERR_INVALID
    res = c.scan_topk_labelset(dg.L2, q, 20, [2, 0])
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    lc.assert_same(c.scan_topk_labelset(dg.L2, q, 20, [0, 2, 2]), *res)
    c.close()
    e = pkg.Corpus(dg.F32, dim)                                 # an empty corpus: VG_OK, count 0
    assert lc.error_code(pkg, lambda: e.scan_topk_labelset(dg.L2, q, 5, [1])) == VG_ERR_INVALID
    e.set_labels(np.zeros(0, dtype=np.uint32))
    for ex in (False, True):
        assert len(e.scan_topk_labelset(dg.L2, q, 5, [1], exclude=ex)[0]) == 0
        assert len(e.scan_topk_grouped_labelset(dg.L2, q, 5, [1], exclude=ex)[0]) == 0
        assert len(e.scan_topk_capped_labelset(dg.L2, q, 5, 2, [1], exclude=ex)[0]) == 0
    e.close()


@pytest.mark.parametrize("vt,dim,metric", [(dg.U8, 64, dg.COSINE), (dg.F32, 384, dg.L2), (dg.F16, 384, dg.L2), (dg.F32, 4100, dg.L2)],
                         ids=["u8-64", "f32-384", "f16-384", "f32-4100"])
def test_three_logical_shards_equal_one_corpus(pkg, vt, dim, metric):
    n = lc.N
    rows = lc.data(vt, n, dim, 81 + dim)
    q = lc.data(vt, 1, dim, 82 + dim)[0]
    rowids = np.arange(n, dtype=np.int64) * 3 + 7
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0, 0, 0], block_rows=64)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    with pytest.raises(pkg.VectorGpuError):
        sh.scan_topk_labelset(metric, q, 5, [1])                 # no labels
    for lname, labels in ls.layouts(n).items():
        c.set_labels(labels)
        sh.set_labels(labels)
        for sname, s in ls.sets_for(labels).items():
            for ex in (False, True):
                for k in KS:
                    ctx = (lname, sname, ex, k)
                    lc.assert_same(sh.scan_topk_labelset(metric, q, k, s, exclude=ex), *c.scan_topk_labelset(metric, q, k, s, exclude=ex), ctx=ctx)
                    assert_same3(sh.scan_topk_grouped_labelset(metric, q, k, s, exclude=ex), c.scan_topk_grouped_labelset(metric, q, k, s, exclude=ex), ctx=ctx)
                    for m in (1, 3):
                        assert_same3(sh.scan_topk_capped_labelset(metric, q, k, m, s, exclude=ex), c.scan_topk_capped_labelset(metric, q, k, m, s, exclude=ex), ctx=ctx + (m,))
    assert lc.error_code(pkg, lambda: sh.scan_topk_labelset(metric, q, 65, [1])) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: sh.scan_topk_grouped_labelset(metric, q, 0, [1])) == VG_ERR_INVALID
    sh.close()
    c.close()
