"""Label-set batch scans (vg_scan_topk_batch_labelset): each query of a batch names its own SET of labels, one `exclude` for the batch.

Contract (include/vectorgpu.h): query i's answer is what scan_topk_labelset(metric, q_i, k, sets[i], exclude) is contracted to return,
in caller order; the slots behind counts[i] are not written.

  * uint8 / int8 and the fallback shapes: exact against the handle's own distances filtered here, and equal to the single form;
  * f32 multi-query shapes: bit for bit scan_topk_batch_masked under each distinct set's bitmap - both run the multi-query arithmetic
    under one launch shape - and within the project's tolerance (batch_reference.completeness_tol) of a float64 numpy reference;
  * nq in (1, 4, 5, 9, 33, 37): 33 and 37 cross the 32-query membership group, ragged against 4 and 2 per pass; every query its own
    set, all queries one set, one query under several sets, equal sets apart in caller order, every label but one; sets that are
    searched in LDS and (`unique`: 3000 labels a set, more than two of them in a group) in global memory; the plan per shape; error codes; 3 logical shards.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
import labelset_cases as ls
from batch_reference import completeness_tol
from test_gpu_labeled_batch import _answer, _judge_f64

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
def test_every_shape(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 31 + dim)
    qs = lc.data(vt, ls.MAXQ, dim, 32 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    f32_multi = vt == dg.F32 and per_pass != 0
    x64 = dg.storage_to_f64(vt, rows) if f32_multi else None
    all_layouts = ls.layouts(n)
    for mi, metric in enumerate(metrics):
        assert pkg.batch_labelset_plan(c, metric)[0] == per_pass, (dim, metric)
        assert pkg.batch_labelset_plan(c, metric) == pkg.batch_masked_plan(c, metric)      # one launch shape with the masked batch
        own = [c.scan_distances(metric, qs[i]) for i in range(ls.MAXQ)]
        ref = [lc.f64_distances(metric, qs[i], x64) for i in range(ls.MAXQ)] if f32_multi else None
        twins = {}                                               # (query row, k, allowed rows) -> the masked batch's answer
        # every layout under the first metric; the others: rows without a label, and every row its own label
        names = list(all_layouts) if mi == 0 else ["some_none", "unique"]
        for lname in names:
            labels = all_layouts[lname]
            c.set_labels(labels)
            for mname, (mq, msets) in ls.mixes(labels, qs).items():
                qidx = [0] * ls.MAXQ if mname == "one_query_many_sets" else list(range(ls.MAXQ))
                for ex in (False, True):
                    allow = [ls.allowed(labels, s, ex) for s in msets]
                    for nq in ls.NQS:
                        # every k on the full batch of one layout; k = 20 everywhere
                        for k in (KS if (lname == "some_none" and nq == ls.MAXQ) else (20,)):
                            res = c.scan_topk_batch_labelset(metric, mq[:nq], msets[:nq], k, exclude=ex)
                            assert res[0].shape == (nq, k) and len(res[2]) == nq
                            for i in range(nq):
                                ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, mname, ex, nq, k, i)
                                if not f32_multi:                # integer sums / the single scans themselves: the handle's own floats
                                    lc.assert_same(_answer(res, i), *lc.expected(own[qidx[i]], allow[i], k), ctx=ctx)
                                    if k == 20 and nq == 5:
                                        lc.assert_same(_answer(res, i), *c.scan_topk_labelset(metric, mq[i], k, msets[i], exclude=ex), ctx=ctx)
                                else:
                                    _judge_f64(_answer(res, i), ref[qidx[i]], allow[i], metric, mq[i], k, ctx)
                                    key = (qidx[i], k, allow[i].tobytes())
                                    if key not in twins:         # bit for bit the masked batch under this set's bitmap
                                        c.set_mask(bits=allow[i])
                                        twins[key] = _answer(c.scan_topk_batch_masked(metric, np.ascontiguousarray(mq[i:i + 1]), k), 0)
                                    lc.assert_same(_answer(res, i), *twins[key], ctx=ctx + ("masked twin",))
    c.close()


def test_contract(pkg):
    n, dim, nq = 2001, 64, 6
    rows = lc.data(dg.U8, n, dim, 41)
    qs = lc.data(dg.U8, nq, dim, 42)
    labels = np.random.default_rng(4).integers(0, 3, n).astype(np.uint32)
    sets = [[2], [0, 1], [], [1, 1, 0], [2, 7], [5]]
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labelset(dg.L2, qs, sets, 5)) == VG_ERR_INVALID          # no labels
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labelset(dg.L2, qs, sets, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labelset(dg.L2, qs, sets, 65)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labelset(dg.L2, qs[:0], [], 5)) == VG_ERR_INVALID        # nq = 0
    with pytest.raises(ValueError):
        c.scan_topk_batch_labelset(dg.L2, qs, sets[:5], 5)       # a set per query
    # through the C symbol: VG_LABEL_NONE in a set, offsets that decrease - VG_ERR_INVALID with the counts zeroed first
    import ctypes as C
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ids, dist = np.zeros((nq, 5), dtype=np.int64), np.zeros((nq, 5), dtype=np.float64)
    flat = np.array([2, 0, 1, ls.NONE, 1, 2, 5], dtype=np.uint32)
    good = np.array([0, 1, 3, 4, 5, 6, 7], dtype=np.int64)
    bad = np.array([0, 1, 3, 2, 5, 6, 7], dtype=np.int64)
    for f, o in ((flat, good), (np.array([2, 0, 1, 1, 1, 2, 5], dtype=np.uint32), bad)):
        cnt = np.full(nq, 9, dtype=np.int32)
        assert lib.vg_scan_topk_batch_labelset(c.h, dg.L2, ptr(qs), nq, 5, ptr(f), ptr(o), 0, ptr(ids), ptr(dist), ptr(cnt)) == VG_ERR_INVALID
        assert not cnt.any()
    cnt = np.full(nq, 9, dtype=np.int32)
    assert lib.vg_scan_topk_batch_labelset(c.h, dg.L2, ptr(qs), nq, 65, ptr(flat), ptr(good), 0, ptr(ids), ptr(dist), ptr(cnt)) == VG_ERR_UNSUPPORTED
    assert not cnt.any()
    # caller order: query i's rows are allowed by ITS set; an empty set counts 0 and is no error; (flat, offsets) input
    res = c.scan_topk_batch_labelset(dg.L2, qs, sets, 20)
    assert res[2].tolist() == [20, 20, 0, 20, 20, 0]
    for i in range(nq):
        assert np.isin(labels[res[0][i, :res[2][i]] - 1], sets[i]).all(), i
    pair = pkg.labelset_csr(sets)
    again = c.scan_topk_batch_labelset(dg.L2, qs, pair, 20)
    assert all(np.array_equal(a, b) for a, b in zip(res, again))
    exc = c.scan_topk_batch_labelset(dg.L2, qs, sets, 20, exclude=True)
    assert exc[2].tolist() == [20, 20, 20, 20, 20, 20]
    for i in range(nq):
        assert not np.isin(labels[exc[0][i] - 1], sets[i]).any(), i
    # the slots behind counts[i] are not written, and tie_order does not matter
    rare = np.zeros(n, dtype=np.uint32); rare[5] = 1; rare[n - 1] = 1
    c.set_labels(rare)
    ids, dist, cnt = c.scan_topk_batch_labelset(dg.L2, qs, sets, 20)
    assert cnt.tolist() == [0, 20, 0, 20, 0, 0] and not ids[0].any() and not ids[5].any()
    ids, dist, cnt = c.scan_topk_batch_labelset(dg.L2, qs, [[1], [1, 9], [0], [1], [], [1]], 20)
    assert cnt.tolist() == [2, 2, 20, 2, 0, 2] and not ids[0, 2:].any() and not ids[4].any()
    c.set_tie_order(pkg.TIE_REFERENCE)
    again = c.scan_topk_batch_labelset(dg.L2, qs, [[1], [1, 9], [0], [1], [], [1]], 20)
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], dist) and np.array_equal(again[2], cnt)
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: every count 0
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert not e.scan_topk_batch_labelset(dg.L2, qs, sets, 20)[2].any()
    assert not e.scan_topk_batch_labelset(dg.L2, qs, sets, 20, exclude=True)[2].any()
    e.close()


@pytest.mark.parametrize("vt,dim,metric", [(dg.U8, 64, dg.COSINE), (dg.F32, 384, dg.L2), (dg.F16, 384, dg.L2), (dg.F32, 1536, dg.COSINE)],
                         ids=["u8-64", "f32-384", "f16-384", "f32-1536"])
def test_three_logical_shards_equal_one_corpus(pkg, vt, dim, metric):
    n = lc.N
    rows = lc.data(vt, n, dim, 51 + dim)
    qs = lc.data(vt, ls.MAXQ, dim, 52 + dim)
    rowids = np.arange(n, dtype=np.int64) * 3 + 7
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0, 0, 0], block_rows=64)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    with pytest.raises(pkg.VectorGpuError):
        sh.scan_topk_batch_labelset(dg.L2, qs[:3], [[0]] * 3, 5)                             # no labels
    for lname in ("some_none", "runs200", "unique"):
        labels = ls.layouts(n)[lname]
        c.set_labels(labels)
        sh.set_labels(labels)
        for mname, (mq, msets) in ls.mixes(labels, qs).items():
            for ex in (False, True):
                for nq in (5, 37):
                    for k in (KS if nq == 37 else (20,)):
                        one = c.scan_topk_batch_labelset(metric, mq[:nq], msets[:nq], k, exclude=ex)
                        many = sh.scan_topk_batch_labelset(metric, mq[:nq], msets[:nq], k, exclude=ex)
                        assert one[2].tolist() == many[2].tolist(), (lname, mname, ex, nq, k)
                        for i in range(nq):
                            lc.assert_same(_answer(many, i), *_answer(one, i), ctx=(lname, mname, ex, nq, k, i))
    sh.close()
    c.close()
