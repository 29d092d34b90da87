"""Value-range batch scans (vg_scan_topk_batch_valued): each query of a batch names its own interval [lo, hi] - and, with labels=, its own label.

Contract (include/vectorgpu.h): query i's answer is what scan_topk_valued(metric, q_i, k, los[i], his[i], label=labels[i]) is contracted
to return, in caller order; the slots behind counts[i] are not written.

  * uint8 / int8 and the fallback shapes: exact against the handle's own distances filtered here, and equal to the single form;
  * f32 multi-query shapes: bit for bit scan_topk_batch_masked under each distinct condition's bitmap - both run the multi-query
    arithmetic under one launch shape - and within the project's tolerance (batch_reference.completeness_tol) of a float64 numpy reference;
  * nq in (1, 4, 5, 9, 33, 37): 33 and 37 cross the 32-query membership group, ragged against 4 and 2 per pass; every query its own
    interval, all queries one interval, one query under many intervals, equal conditions apart in caller order - each with and without
    per-query labels; the plan per shape; error codes; 3 logical shards.
"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
import valued_cases as vc
from batch_reference import completeness_tol  # noqa: F401  (the tolerance _judge_f64 applies)
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
    qs = lc.data(vt, vc.MAXQ, dim, 32 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    f32_multi = vt == dg.F32 and per_pass != 0
    x64 = dg.storage_to_f64(vt, rows) if f32_multi else None
    lay = vc.layouts(n)
    labels = lc.layouts(n)["some_none"][0]
    c.set_labels(labels)
    for mi, metric in enumerate(metrics):
        assert pkg.batch_valued_plan(c, metric)[0] == per_pass, (dim, metric)
        assert pkg.batch_valued_plan(c, metric) == pkg.batch_masked_plan(c, metric)        # one launch shape with the masked batch
        own = [c.scan_distances(metric, qs[i]) for i in range(vc.MAXQ)]
        ref = [lc.f64_distances(metric, qs[i], x64) for i in range(vc.MAXQ)] if f32_multi else None
        twins = {}                                               # (query row, k, allowed rows) -> the masked batch's answer
        # the full layout x mix product under the first metric; the others: the two layouts a wrong compare shows on
        for lname in (list(lay) if mi == 0 else ["extremes", "low_word_only"]):
            values = lay[lname]
            c.set_values(values)
            for with_labels in (False, True):
                for mname, (mq, los, his, qlab) in vc.mixes(values, qs, labels if with_labels else None).items():
                    qidx = [0] * vc.MAXQ if mname == "one_query_many_intervals" else list(range(vc.MAXQ))
                    allow = [vc.allowed(values, los[i], his[i], labels, None if qlab is None else qlab[i]) for i in range(vc.MAXQ)]
                    for nq in vc.NQS:
                        # every k on the full batch of one layout; k = 20 everywhere
                        for k in (KS if (lname == "extremes" and nq == vc.MAXQ) else (20,)):
                            res = c.scan_topk_batch_valued(metric, mq[:nq], los[:nq], his[:nq], k, labels=None if qlab is None else qlab[:nq])
                            assert res[0].shape == (nq, k) and len(res[2]) == nq
                            for i in range(nq):
                                ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, mname, with_labels, nq, k, i)
                                if not f32_multi:                # integer sums / the single scans themselves: the handle's own floats
                                    lc.assert_same(_answer(res, i), *lc.expected(own[qidx[i]], allow[i], k), ctx=ctx)
                                    if k == 20 and nq == 5:
                                        single = c.scan_topk_valued(metric, mq[i], k, los[i], his[i], label=None if qlab is None else qlab[i])
                                        lc.assert_same(_answer(res, i), *single, ctx=ctx + ("single",))
                                else:
                                    _judge_f64(_answer(res, i), ref[qidx[i]], allow[i], metric, mq[i], k, ctx)
                                    key = (qidx[i], k, allow[i].tobytes())
                                    if key not in twins:         # bit for bit the masked batch under this condition's bitmap
                                        c.set_mask(bits=allow[i])
                                        twins[key] = _answer(c.scan_topk_batch_masked(metric, np.ascontiguousarray(mq[i:i + 1]), k), 0)
                                    lc.assert_same(_answer(res, i), *twins[key], ctx=ctx + ("masked twin",))
    c.close()


def test_contract(pkg):
    n, dim, nq = 2001, 64, 6
    rows = lc.data(dg.U8, n, dim, 41)
    qs = lc.data(dg.U8, nq, dim, 42)
    values = np.arange(n, dtype=np.int64) - 1000
    labels = (np.arange(n) % 3).astype(np.uint32)
    los, his = [0, -5, 1, 500, vc.I64_MIN, 5000], [99, 5, 0, 500, -999, 6000]
    qlab = np.array([0, 1, 2, 2, 0, 1], dtype=np.uint32)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(dg.L2, qs, los, his, 5)) == VG_ERR_INVALID          # no values
    c.set_values(values)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(dg.L2, qs, los, his, 5, labels=qlab)) == VG_ERR_INVALID          # no labels
    assert c.scan_topk_batch_valued(dg.L2, qs, los, his, 5)[2].tolist() == [5, 5, 0, 1, 2, 0]           # ... which only labels= needs
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(dg.L2, qs, los, his, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(dg.L2, qs, los, his, 65)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(dg.L2, qs[:0], [], [], 5)) == VG_ERR_INVALID        # nq = 0
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_valued(99, qs, los, his, 5)) == VG_ERR_INVALID
    with pytest.raises(ValueError):
        c.scan_topk_batch_valued(dg.L2, qs, los[:5], his, 5)     # an interval per query
    with pytest.raises(ValueError):
        c.scan_topk_batch_valued(dg.L2, qs, los, his, 5, labels=qlab[:5])
    # through the C symbol: VG_LABEL_NONE among the query labels, k = 65, NULL bounds - the counts zeroed first
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ids, dist = np.zeros((nq, 5), dtype=np.int64), np.zeros((nq, 5), dtype=np.float64)
    lo64, hi64 = np.array(los, dtype=np.int64), np.array(his, dtype=np.int64)
    bad = qlab.copy(); bad[3] = lc.NONE
    cnt = np.full(nq, 9, dtype=np.int32)
    assert lib.vg_scan_topk_batch_valued(c.h, dg.L2, ptr(qs), nq, 5, ptr(lo64), ptr(hi64), ptr(bad), ptr(ids), ptr(dist), ptr(cnt)) == VG_ERR_INVALID
    assert not cnt.any()
    cnt = np.full(nq, 9, dtype=np.int32)
    assert lib.vg_scan_topk_batch_valued(c.h, dg.L2, ptr(qs), nq, 65, ptr(lo64), ptr(hi64), None, ptr(ids), ptr(dist), ptr(cnt)) == VG_ERR_UNSUPPORTED
    assert not cnt.any()
    cnt = np.full(nq, 9, dtype=np.int32)
    assert lib.vg_scan_topk_batch_valued(c.h, dg.L2, ptr(qs), nq, 5, ptr(lo64), ptr(hi64), None, None, ptr(dist), ptr(cnt)) == VG_ERR_INVALID
    assert not cnt.any()
    assert lib.vg_scan_topk_batch_valued(c.h, dg.L2, ptr(qs), nq, 5, None, ptr(hi64), None, ptr(ids), ptr(dist), ptr(cnt)) == VG_ERR_INVALID
    assert lib.vg_scan_topk_batch_valued(c.h, dg.L2, ptr(qs), nq, 5, ptr(lo64), ptr(hi64), None, ptr(ids), ptr(dist), None) == VG_ERR_INVALID
    # caller order: query i's rows lie in ITS interval (and carry ITS label); lo > hi counts 0 and is no error
    res = c.scan_topk_batch_valued(dg.L2, qs, los, his, 20)
    assert res[2].tolist() == [20, 11, 0, 1, 2, 0]
    for i in range(nq):
        v = values[res[0][i, :res[2][i]] - 1]
        assert ((v >= los[i]) & (v <= his[i])).all(), i
    lab = c.scan_topk_batch_valued(dg.L2, qs, los, his, 20, labels=qlab)
    want = [int(vc.allowed(values, los[i], his[i], labels, qlab[i]).sum()) for i in range(nq)]
    assert lab[2].tolist() == [min(20, w) for w in want]
    for i in range(nq):
        assert (labels[lab[0][i, :lab[2][i]] - 1] == qlab[i]).all(), i
    # scalars and None broadcast: one interval for the batch
    one = c.scan_topk_batch_valued(dg.L2, qs, None, -990, 20)
    assert one[2].tolist() == [11] * nq
    # the slots behind counts[i] are not written, and tie_order does not matter
    ids, dist, cnt = res
    assert not ids[2].any() and not ids[5].any() and not ids[3, 1:].any() and not dist[4, 2:].any()
    c.set_tie_order(pkg.TIE_REFERENCE)
    again = c.scan_topk_batch_valued(dg.L2, qs, los, his, 20)
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], dist) and np.array_equal(again[2], cnt)
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: every count 0
    e.set_values(np.zeros(0, dtype=np.int64))
    assert not e.scan_topk_batch_valued(dg.L2, qs, los, his, 20)[2].any()
    e.close()
