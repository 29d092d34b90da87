"""Capped scans (vg_scan_topk_capped[_masked]): the k nearest rows, at most m = per_label of one label.

Contract (include/vectorgpu.h): the rows with a finite distance and a label (masked form: and a set mask bit), ordered by (distance,
scan position); a row is kept iff fewer than m rows of its label have been kept; the first k rows kept.  Every comparison here is
exact - rowids, labels and distance bits - against capped_cases.expected over the distances scan_distances returns on the same handle.

  * every shape of labeled_cases.SHAPES x the seven label layouts of grouped_cases x six (k, m); m = 1 must equal scan_topk_grouped,
    `unique` (and m = 64 on a layout without NONE) must equal scan_topk, `hot` is the case a top-64-then-cap gets wrong;
  * larger corpora, where one wavefront sees hundreds of rows and a full label's worst kept row is replaced inside a list;
  * the masked form, several shards with every label on all of them, the f16 shape of six chunks per lane, and the error codes.
"""
import numpy as np
import pytest

import capped_cases as cc
import datagen as dg
import grouped_cases as gc
import labeled_cases as lc

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
KMS = ((1, 1), (20, 1), (20, 3), (64, 2), (64, 5), (64, 64))


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
def test_every_shape_and_layout_against_own_distances(pkg, vt, dim, per_pass, metrics):
    n = gc.N
    rows = lc.data(vt, n, dim, 31 + dim)
    q = lc.data(vt, 1, dim, 32 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    for metric in metrics:
        own = c.scan_distances(metric, q)
        for name, labels in gc.layouts(n, own).items():
            c.set_labels(labels)
            for k, m in KMS:
                ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name, k, m)
                got = c.scan_topk_capped(metric, q, k, m)
                cc_want = cc.expected(own, labels, None, k, m)
                gc.assert_same(got, *cc_want, ctx=ctx)
                if m == 1:
                    gc.assert_same(got, *c.scan_topk_grouped(metric, q, k), ctx=ctx)
                if name == "unique" or (m == 64 and name != "some_none"):
                    lc.assert_same(c.scan_topk(metric, q, k), got[0], got[1], ctx=ctx)
                if name == "uniform5":
                    assert len(got[0]) == min(k, 5 * m), ctx
                if name == "all_one":
                    assert len(got[0]) == min(k, m), ctx
                if name == "hot":                               # one label owns the 500 nearest rows: m of it, then the others
                    lab = got[2].tolist()
                    assert len(lab) == k and lab[:min(k, m)] == [1] * min(k, m) and 1 not in lab[m:], ctx
    c.close()


def _corpus(pkg, vt, n, dim, seed):
    rows = lc.data(vt, n, dim, seed)
    q = lc.data(vt, 1, dim, seed + 1)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    return c, q


@pytest.mark.parametrize("groups", [7, 1000], ids=["mod7", "mod1000"])
def test_large_uint8_corpus_replaces_inside_a_full_label(pkg, groups):
    n = 200_000
    c, q = _corpus(pkg, dg.U8, n, 64, 51)
    labels = (np.arange(n) % groups).astype(np.uint32)
    c.set_labels(labels)
    for metric in (dg.L2, dg.COSINE):
        own = c.scan_distances(metric, q)
        for k, m in ((20, 3), (64, 3)):
            got = c.scan_topk_capped(metric, q, k, m)
            gc.assert_same(got, *cc.expected(own, labels, None, k, m), ctx=(groups, metric, k, m))
            assert len(got[0]) == min(k, 3 * groups)
    c.close()


def test_large_f32_corpus_with_a_hot_label(pkg):
    n = 60_000
    c, q = _corpus(pkg, dg.F32, n, 384, 61)
    own = c.scan_distances(dg.L2, q)
    labels = gc.hot(own, 500)
    c.set_labels(labels)
    plain_ids, _ = c.scan_topk(dg.L2, q, 64)
    assert len(set(labels[plain_ids - 1].tolist())) == 1         # what a top-64-then-cap would see: one label
    for m in (1, 2, 3, 5):
        for k in (20, 64):
            got = c.scan_topk_capped(dg.L2, q, k, m)
            gc.assert_same(got, *cc.expected(own, labels, None, k, m), ctx=(k, m))
            lab = got[2].tolist()
            assert len(lab) == k and lab[:m] == [1] * m and 1 not in lab[m:], (k, m)
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64), (dg.F16, 384), (dg.F32, 4100)], ids=["f32-384", "uint8-64", "f16-384", "f32-4100"])
def test_masked_form(pkg, vt, dim):
    n, k, m = gc.N, 20, 3
    c, q = _corpus(pkg, vt, n, dim, 71 + dim)
    own = c.scan_distances(dg.L2, q)
    labels = np.random.default_rng(dim).integers(0, 30, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, k, m, masked=True)) == VG_ERR_INVALID      # no mask set
    allowed = np.random.default_rng(dim + 1).random(n) < 0.5
    c.set_mask(bits=allowed)
    got = c.scan_topk_capped(dg.L2, q, k, m, masked=True)
    gc.assert_same(got, *cc.expected(own, labels, allowed, k, m), ctx="half the rows")
    assert len(got[0]) == k and allowed[got[0] - 1].all()
    gc.assert_same(c.scan_topk_capped(dg.L2, q, k, m), *cc.expected(own, labels, None, k, m), ctx="the unmasked form ignores the mask")
    # the rows the free answer kept are cleared: every label's next allowed rows move up
    free_ids, _, _ = cc.expected(own, labels, None, 64, m)
    allowed = np.ones(n, dtype=bool)
    allowed[free_ids - 1] = False
    c.set_mask(bits=allowed)
    got = c.scan_topk_capped(dg.L2, q, k, m, masked=True)
    gc.assert_same(got, *cc.expected(own, labels, allowed, k, m), ctx="kept rows cleared")
    assert not set(got[0].tolist()) & set(free_ids.tolist())
    c.set_mask(bits=np.zeros(n, dtype=bool))                    # an empty mask: no result
    assert len(c.scan_topk_capped(dg.L2, q, k, m, masked=True)[0]) == 0
    c.close()


def test_three_shards_with_every_label_on_all_of_them(pkg):
    n, dim = gc.N, 100
    rows = lc.data(dg.F32, n, dim, 81)
    q = lc.data(dg.F32, 1, dim, 82)[0]
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    s = pkg.Shards(dg.F32, dim, [0, 0, 0], block_rows=64)       # blocks of 64 rows dealt out in turn
    s.append(rows)
    own = c.scan_distances(dg.L2, q)
    hot = gc.hot(own, 500)                                      # label 1's nearest rows are spread over the three shards
    for labels in ((np.arange(n) % 50).astype(np.uint32), (np.arange(n) % 7).astype(np.uint32), hot):
        c.set_labels(labels)
        s.set_labels(labels)
        for k, m in ((20, 3), (64, 5)):
            one = c.scan_topk_capped(dg.L2, q, k, m)
            gc.assert_same(one, *cc.expected(own, labels, None, k, m), ctx=(k, m))
            gc.assert_same(s.scan_topk_capped(dg.L2, q, k, m), *one, ctx=(k, m, "shards"))
    labels = (np.arange(n) % 50).astype(np.uint32)
    allowed = np.random.default_rng(5).random(n) < 0.3
    for h in (c, s):
        h.set_labels(labels)
        h.set_mask(bits=allowed)
    for k, m in ((20, 3), (64, 5)):
        want = cc.expected(own, labels, allowed, k, m)
        gc.assert_same(c.scan_topk_capped(dg.L2, q, k, m, masked=True), *want)
        gc.assert_same(s.scan_topk_capped(dg.L2, q, k, m, masked=True), *want)
    s.close()
    c.close()


def test_error_codes_and_an_empty_corpus(pkg):
    n, dim = 2001, 100
    c, q = _corpus(pkg, dg.F32, n, dim, 91)
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 5, 2)) == VG_ERR_INVALID                # no labels
    labels = np.random.default_rng(3).integers(0, 9, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 0, 2)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 65, 2)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 5, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 5, -3)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(99, q, 5, 2)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.L2, q, 5, 2, masked=True)) == VG_ERR_INVALID   # no mask
    own = c.scan_distances(dg.L2, q)
    res = c.scan_topk_capped(dg.L2, q, 20, 3)
    gc.assert_same(res, *cc.expected(own, labels, None, 20, 3))
    gc.assert_same(c.scan_topk_capped(dg.L2, q, 20, 1000), *cc.expected(own, labels, None, 20, 20))      # m above k behaves as k
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    gc.assert_same(c.scan_topk_capped(dg.L2, q, 20, 3), *res)
    c.set_tie_order(pkg.TIE_POSITION)
    gc.assert_same(c.scan_topk_grouped(dg.L2, q, 20), *gc.expected(own, labels, None, 20))                # the grouped scan still works
    c.close()
    s = pkg.Shards(dg.F32, dim, [0, 0], block_rows=64)
    s.append(lc.data(dg.F32, 300, dim, 92))
    assert lc.error_code(pkg, lambda: s.scan_topk_capped(dg.L2, q, 5, 2)) == VG_ERR_INVALID                # no labels
    s.set_labels((np.arange(300) % 4).astype(np.uint32))
    assert lc.error_code(pkg, lambda: s.scan_topk_capped(dg.L2, q, 0, 2)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: s.scan_topk_capped(dg.L2, q, 65, 2)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: s.scan_topk_capped(dg.L2, q, 5, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: s.scan_topk_capped(dg.L2, q, 5, 2, masked=True)) == VG_ERR_INVALID
    s.close()
    e = pkg.Corpus(dg.F32, dim)                                 # no rows: labels of length 0 are labels, nothing is launched
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert len(e.scan_topk_capped(dg.L2, q, 5, 2)[0]) == 0
    e.close()


def test_f16_rows_of_six_chunks_per_lane(pkg):
    """2049 .. 3072 halves: the one f16 shape of 6 chunks per lane.  L2 and L1 are served (and exact); the cosine and dot kernels of that
    shape do not fit the register file, so the capped forms refuse them like the grouped ones (VG_ERR_UNSUPPORTED) and the handle goes
    on working."""
    n, dim = 301, 3072
    c, q = _corpus(pkg, dg.F16, n, dim, 71)
    labels = (np.arange(n) // 4).astype(np.uint32)
    c.set_labels(labels)
    c.set_mask(bits=np.arange(n) % 3 != 0)
    for metric in (dg.L2, dg.L1):
        own = c.scan_distances(metric, q)
        gc.assert_same(c.scan_topk_capped(metric, q, 20, 3), *cc.expected(own, labels, None, 20, 3), ctx=metric)
        gc.assert_same(c.scan_topk_capped(metric, q, 20, 3, masked=True), *cc.expected(own, labels, np.arange(n) % 3 != 0, 20, 3), ctx=metric)
    for metric in (dg.COSINE, dg.DOT):
        for masked in (False, True):
            assert lc.error_code(pkg, lambda: c.scan_topk_capped(metric, q, 20, 3, masked=masked)) == VG_ERR_UNSUPPORTED, (metric, masked)
        assert len(c.scan_topk(metric, q, 20)[0]) == 20                  # the plain scan of that shape is untouched
    c.close()
