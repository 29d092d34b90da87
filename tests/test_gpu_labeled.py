"""Labeled scans, single form (vg_scan_topk_labeled): a label per row on the handle, a query names one label.

Contract (include/vectorgpu.h): scan_topk_masked with "allowed" meaning labels[p] == label - ascending (distance, scan position), NaN /
+Inf never, every distance the float scan_distances reports for that row, bit for bit.

  * every shape: rowids, order and distance bits equal to scan_distances of the same handle filtered by label here, and to
    scan_topk_masked under the host-built bitmap of the label; the user's own mask is neither read nor changed;
  * the bitmap kernel's second word (65 rows), an empty corpus, a label no row carries, rows without a label;
  * lifetime of the labels (append / delete / clear drop, patch / reserve / trim keep, clone copies) and the error codes.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5


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


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape_against_own_distances_and_masked_scan(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 11 + dim)
    qs = lc.data(vt, 2, dim, 12 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    user_mask = np.random.default_rng(dim).random(n) < 0.4
    for metric in metrics:
        own = [c.scan_distances(metric, q) for q in qs]
        for name, (labels, asked) in lc.layouts(n).items():
            c.set_labels(labels)
            assert c.has_labels()
            assert c.set_mask(bits=user_mask) == int(user_mask.sum())
            mask_before = c.scan_topk_masked(metric, qs[0], 20)
            got = {}
            for label in asked:
                for qi in range(2):
                    for k in ((1, 20, 64) if qi == 0 else (20,)):
                        got[(label, qi, k)] = c.scan_topk_labeled(metric, qs[qi], k, label)
            # the user's mask: neither read (the answers below name rows outside it) nor changed
            assert c.mask_count() == int(user_mask.sum())
            lc.assert_same(c.scan_topk_masked(metric, qs[0], 20), *mask_before, ctx=(name, "mask after"))
            for label in asked:
                allowed = labels == label
                c.set_mask(bits=allowed)
                for (lb, qi, k), res in got.items():
                    if lb != label:
                        continue
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name, label, qi, k)
                    ids, dist = lc.expected(own[qi], allowed, k)
                    lc.assert_same(res, ids, dist, ctx=ctx)
                    lc.assert_same(res, *c.scan_topk_masked(metric, qs[qi], k), ctx=ctx)
                    if label in (lc.ABSENT, 8):
                        assert len(res[0]) == 0, ctx
    c.close()


def test_second_word_of_the_bitmap_and_an_empty_corpus(pkg):
    dim = 64
    rows = lc.data(dg.U8, 65, dim, 5)
    q = lc.data(dg.U8, 1, dim, 6)[0]
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    labels = np.full(65, 1, dtype=np.uint32)
    labels[64] = 3
    labels[10] = lc.NONE
    c.set_labels(labels)
    for label, k in ((3, 5), (1, 64), (1, 20), (2, 5)):
        lc.assert_same(c.scan_topk_labeled(dg.L2, q, k, label), *lc.expected(own, labels == label, k), ctx=(label, k))
    assert c.scan_topk_labeled(dg.L2, q, 5, 3)[0].tolist() == [65]
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # no rows: labels of length 0 are labels
    assert lc.error_code(pkg, lambda: e.scan_topk_labeled(dg.L2, q, 5, 1)) == VG_ERR_INVALID
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert e.has_labels()
    assert len(e.scan_topk_labeled(dg.L2, q, 5, 1)[0]) == 0
    e.close()


def test_lifetime_of_the_labels_and_error_codes(pkg):
    n, dim = 2001, 100
    rows = lc.data(dg.F32, n, dim, 21)
    q = lc.data(dg.F32, 1, dim, 22)[0]
    labels = np.random.default_rng(3).integers(0, 4, n).astype(np.uint32)
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)

    def check(corpus, lab, label=2, k=20):
        res = corpus.scan_topk_labeled(dg.L2, q, k, label)
        lc.assert_same(res, *lc.expected(corpus.scan_distances(dg.L2, q), lab == label, k))
        return res

    assert not c.has_labels()
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 5, 1)) == VG_ERR_INVALID           # no labels
    assert lc.error_code(pkg, lambda: c.set_labels(labels[:-1])) == VG_ERR_INVALID                     # n != rows
    assert not c.has_labels()
    plain_before = c.scan_topk(dg.L2, q, 10)
    c.set_labels(labels)
    plain_after = c.scan_topk(dg.L2, q, 10)                     # scans that name no label ignore the labels
    assert all(np.array_equal(a, b) for a, b in zip(plain_before, plain_after))
    assert lc.error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 5)) == VG_ERR_INVALID               # labels are no mask
    res = check(c, labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 0, 1)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 65, 1)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 5, lc.NONE)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(99, q, 5, 1)) == VG_ERR_INVALID
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    lc.assert_same(c.scan_topk_labeled(dg.L2, q, 20, 2), *res)
    c.set_tie_order(pkg.TIE_POSITION)
    # clone copies; reserve and trim keep
    d = c.clone()
    assert d.has_labels()
    lc.assert_same(check(d, labels), *res)
    d.close()
    c.reserve(3 * n)
    assert c.has_labels()
    lc.assert_same(check(c, labels), *res)
    c.trim()
    assert c.has_labels()
    lc.assert_same(check(c, labels), *res)
    # patch keeps: the patched row is found under its old label at its new distance
    far = int(lc.expected(c.scan_distances(dg.L2, q), labels == 2, n)[0][-1] - 1)          # the farthest row of label 2 ...
    c.patch_rows(np.array([far], dtype=np.int64), q[None, :].copy())                        # ... becomes the query itself
    assert c.has_labels()
    res2 = check(c, labels)
    assert res2[0][0] == far + 1 and res2[1][0] == 0.0
    # clear_labels, then append / delete / clear each drop
    c.clear_labels()
    assert not c.has_labels()
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 5, 1)) == VG_ERR_INVALID
    c.set_labels(labels)
    c.append(rows[:3])
    assert not c.has_labels()
    assert lc.error_code(pkg, lambda: c.scan_topk_labeled(dg.L2, q, 5, 1)) == VG_ERR_INVALID
    c.set_labels(np.zeros(c.rows, dtype=np.uint32))
    c.delete_rows(np.array([1, 7], dtype=np.int64))
    assert not c.has_labels()
    c.set_labels(np.zeros(c.rows, dtype=np.uint32))
    c.clear()
    assert not c.has_labels()
    c.close()
