"""Grouped scans (vg_scan_topk_grouped[_masked]): the k nearest labels, each represented by its best row.

Contract (include/vectorgpu.h): the rows with a finite distance and a label (masked form: and a set mask bit), ordered by (distance,
scan position); the first row of each label; the first k of those.  Every comparison here is exact - rowids, labels and distance bits -
against grouped_cases.expected over the distances scan_distances returns on the same handle.

  * every shape of labeled_cases.SHAPES (five types, a padding chunk, 1 / 3 / 6 chunks per lane, long rows) x seven label layouts x
    k = 1, 20, 64; `unique` must equal scan_topk, `hot` is the case a top-64-then-dedupe gets wrong;
  * larger corpora, where one wavefront sees hundreds of rows and entries are replaced inside a list;
  * the masked form, several shards with every label on all of them, and the error codes.
"""
import numpy as np
import pytest

import datagen as dg
import grouped_cases as gc
import labeled_cases as lc

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
            for k in KS:
                ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name, k)
                got = c.scan_topk_grouped(metric, q, k)
                want = gc.expected(own, labels, None, k)
                gc.assert_same(got, *want, ctx=ctx)
                if name == "uniform5":
                    assert len(got[0]) == min(k, 5), ctx
                if name == "all_one":
                    assert len(got[0]) == 1, ctx
                if name == "unique":
                    lc.assert_same(c.scan_topk(metric, q, k), got[0], got[1], ctx=ctx)
                if name == "hot":                               # one label owns the 500 nearest rows: still k groups
                    assert len(got[0]) == k and got[2][0] == 1 and len(set(got[2].tolist())) == k, ctx
    c.close()


def _corpus(pkg, vt, n, dim, seed):
    rows = lc.data(vt, n, dim, seed)
    q = lc.data(vt, 1, dim, seed + 1)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    return c, q


@pytest.mark.parametrize("groups,ks", [(7, KS), (1000, (64,))], ids=["mod7", "mod1000"])
def test_large_uint8_corpus_replaces_inside_the_lists(pkg, groups, ks):
    n = 200_000
    c, q = _corpus(pkg, dg.U8, n, 64, 51)
    labels = (np.arange(n) % groups).astype(np.uint32)
    c.set_labels(labels)
    for metric in (dg.L2, dg.COSINE):
        own = c.scan_distances(metric, q)
        for k in ks:
            got = c.scan_topk_grouped(metric, q, k)
            gc.assert_same(got, *gc.expected(own, labels, None, k), ctx=(groups, metric, k))
            assert len(got[0]) == min(k, groups)
    c.close()


def test_large_f32_corpus_with_a_hot_label(pkg):
    n = 60_000
    c, q = _corpus(pkg, dg.F32, n, 384, 61)
    own = c.scan_distances(dg.L2, q)
    labels = gc.hot(own, 500)
    c.set_labels(labels)
    plain_ids, _ = c.scan_topk(dg.L2, q, 64)
    assert len(set(labels[plain_ids - 1].tolist())) == 1         # what a top-64-then-dedupe would see: one group
    for k in KS:
        got = c.scan_topk_grouped(dg.L2, q, k)
        gc.assert_same(got, *gc.expected(own, labels, None, k), ctx=k)
        assert len(got[0]) == k
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64), (dg.F16, 384), (dg.F32, 4100)], ids=["f32-384", "uint8-64", "f16-384", "f32-4100"])
def test_masked_form(pkg, vt, dim):
    n = gc.N
    c, q = _corpus(pkg, vt, n, dim, 71 + dim)
    own = c.scan_distances(dg.L2, q)
    labels = np.random.default_rng(dim).integers(0, 30, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(dg.L2, q, 5, masked=True)) == VG_ERR_INVALID      # no mask set
    free_ids, _, free_lab = gc.expected(own, labels, None, 64)
    # every group's best row cleared: the representative becomes the group's next allowed row
    allowed = np.ones(n, dtype=bool)
    allowed[free_ids - 1] = False
    c.set_mask(bits=allowed)
    for k in KS:
        got = c.scan_topk_grouped(dg.L2, q, k, masked=True)
        gc.assert_same(got, *gc.expected(own, labels, allowed, k), ctx=("best cleared", k))
        assert not set(got[0].tolist()) & set(free_ids.tolist())
    assert len(c.scan_topk_grouped(dg.L2, q, 64, masked=True)[0]) == 30
    # a whole group cleared (the nearest one), and a random mask
    allowed = labels != free_lab[0]
    c.set_mask(bits=allowed)
    got = c.scan_topk_grouped(dg.L2, q, 64, masked=True)
    gc.assert_same(got, *gc.expected(own, labels, allowed, 64), ctx="group cleared")
    assert len(got[0]) == 29 and int(free_lab[0]) not in got[2].tolist()
    allowed = np.random.default_rng(dim + 1).random(n) < 0.1
    c.set_mask(bits=allowed)
    gc.assert_same(c.scan_topk_grouped(dg.L2, q, 20, masked=True), *gc.expected(own, labels, allowed, 20), ctx="random mask")
    gc.assert_same(c.scan_topk_grouped(dg.L2, q, 20), *gc.expected(own, labels, None, 20), ctx="the unmasked form ignores the mask")
    # an empty mask: no result
    c.set_mask(bits=np.zeros(n, dtype=bool))
    assert len(c.scan_topk_grouped(dg.L2, q, 20, masked=True)[0]) == 0
    c.close()


def test_three_shards_with_every_label_on_several_shards(pkg):
    n, dim = gc.N, 100
    rows = lc.data(dg.F32, n, dim, 81)
    q = lc.data(dg.F32, 1, dim, 82)[0]
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    s = pkg.Shards(dg.F32, dim, [0, 0, 0], block_rows=64)       # blocks of 64 rows dealt out in turn
    s.append(rows)
    own = c.scan_distances(dg.L2, q)
    for name, labels in gc.layouts(n, own).items():
        if name in ("unique", "all_one"):
            continue
        c.set_labels(labels)
        s.set_labels(labels)
        for k in KS:
            one = c.scan_topk_grouped(dg.L2, q, k)
            gc.assert_same(one, *gc.expected(own, labels, None, k), ctx=(name, k))
            gc.assert_same(s.scan_topk_grouped(dg.L2, q, k), *one, ctx=(name, k, "shards"))
    labels = (np.arange(n) % 50).astype(np.uint32)              # every label on all three shards
    allowed = np.random.default_rng(5).random(n) < 0.3
    for h in (c, s):
        h.set_labels(labels)
        h.set_mask(bits=allowed)
    want = gc.expected(own, labels, allowed, 64)
    gc.assert_same(c.scan_topk_grouped(dg.L2, q, 64, masked=True), *want)
    gc.assert_same(s.scan_topk_grouped(dg.L2, q, 64, masked=True), *want)
    s.close()
    c.close()


def test_error_codes_and_an_empty_corpus(pkg):
    n, dim = 2001, 100
    c, q = _corpus(pkg, dg.F32, n, dim, 91)
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(dg.L2, q, 5)) == VG_ERR_INVALID                  # no labels
    labels = np.random.default_rng(3).integers(0, 9, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(dg.L2, q, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(dg.L2, q, 65)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(99, q, 5)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_grouped(dg.L2, q, 5, masked=True)) == VG_ERR_INVALID     # no mask
    own = c.scan_distances(dg.L2, q)
    res = c.scan_topk_grouped(dg.L2, q, 20)
    gc.assert_same(res, *gc.expected(own, labels, None, 20))
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    gc.assert_same(c.scan_topk_grouped(dg.L2, q, 20), *res)
    c.set_tie_order(pkg.TIE_POSITION)
    lc.assert_same(c.scan_topk_labeled(dg.L2, q, 5, int(res[2][0])), *lc.expected(own, labels == res[2][0], 5))   # the labeled scan still works
    c.close()
    e = pkg.Corpus(dg.F32, dim)                                 # no rows: labels of length 0 are labels, nothing is launched
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert len(e.scan_topk_grouped(dg.L2, q, 5)[0]) == 0
    e.close()


def test_f16_rows_of_six_chunks_per_lane(pkg):
    """2049 .. 3072 halves: the one f16 shape of 6 chunks per lane.  L2 and L1 are served (and exact); the cosine and dot kernels of that
    shape do not fit the register file, so the grouped forms refuse them (VG_ERR_UNSUPPORTED) and the handle goes on working."""
    n, dim = 301, 3072
    c, q = _corpus(pkg, dg.F16, n, dim, 71)
    labels = (np.arange(n) // 2).astype(np.uint32)
    c.set_labels(labels)
    c.set_mask(bits=np.arange(n) % 3 != 0)
    for metric in (dg.L2, dg.L1):
        own = c.scan_distances(metric, q)
        gc.assert_same(c.scan_topk_grouped(metric, q, 20), *gc.expected(own, labels, None, 20), ctx=metric)
        gc.assert_same(c.scan_topk_grouped(metric, q, 20, masked=True), *gc.expected(own, labels, np.arange(n) % 3 != 0, 20), ctx=metric)
    for metric in (dg.COSINE, dg.DOT):
        for masked in (False, True):
            assert lc.error_code(pkg, lambda: c.scan_topk_grouped(metric, q, 20, masked=masked)) == VG_ERR_UNSUPPORTED, (metric, masked)
        assert len(c.scan_topk(metric, q, 20)[0]) == 20                  # the plain scan of that shape is untouched
    c.close()
