"""Labeled batch scans (vg_scan_topk_batch_labeled): each query of a batch names its own label.

Contract (include/vectorgpu.h): query i's answer is what scan_topk_labeled(metric, q_i, k, labels[i]) is contracted to return, in
caller order; the slots behind counts[i] are not written.

  * uint8 / int8 and the fallback shapes: identical to nq single labeled scans (and to the handle's own distances filtered here);
  * f32: bit for bit scan_topk_batch_masked run per distinct label under that label's bitmap - both run the multi-query arithmetic
    under one launch shape - and within the project's 1e-5 relative tolerance of a float64 numpy reference over the labeled rows;
  * nq in {1, 4, 5, 9} (ragged against 4 and 2 per pass), k in {1, 20, 64}; mixed labels inside one pass, one query under several
    labels, all queries one label; the plan per shape; error codes; 3 logical shards on one device == one corpus.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
from batch_reference import completeness_tol

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
NQS = (1, 4, 5, 9)
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


def _answer(res, i):
    ids, dist, cnt = res
    return ids[i, :cnt[i]], dist[i, :cnt[i]]


def _mixes(qs, asked):
    """name -> (queries, a label each): 9 queries, cut to nq by the caller"""
    rng = np.random.default_rng(len(asked))
    mixed = np.array([asked[j] for j in rng.integers(0, len(asked), 9)], dtype=np.uint32)
    mixed[:len(asked)] = asked[::-1]                            # every asked label is there, and NOT in ascending order
    dup = np.ascontiguousarray(np.repeat(qs[:1], 9, axis=0))    # one query, a different label each time round
    return {"mixed": (qs, mixed), "one_query_many_labels": (dup, np.array([asked[j % len(asked)] for j in range(9)], dtype=np.uint32)),
            "all_one_label": (qs, np.full(9, asked[0], dtype=np.uint32))}


def _judge_f64(got, ref, allowed, metric, q, k, ctx):
    """one f32 answer against float64 distances `ref` of every row: count, membership, per-row value, nothing better left behind -
    each within 1e-5 relative (the suite's slack for dot and cosine, whose values cancel: batch_reference.completeness_tol)"""
    gi, gd = got
    assert len(gi) == min(k, int(allowed.sum())), ctx
    if len(gi) == 0:
        return
    pos = gi - 1
    assert allowed[pos].all() and len(set(pos.tolist())) == len(pos), ctx
    q_l1 = float(np.abs(q.astype(np.float64)).sum())
    for p, d in zip(pos, gd):
        assert abs(d - ref[p]) <= completeness_tol(metric, q_l1, ref[p]), (ctx, p, d, ref[p])
    assert np.all(np.diff(gd) >= 0), ctx
    if len(gi) == k:
        out = allowed.copy()
        out[pos] = False
        if out.any():
            assert float(ref[out].min()) >= float(gd[-1]) - completeness_tol(metric, q_l1, gd[-1]), ctx


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 31 + dim)
    qs = lc.data(vt, 9, dim, 32 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    f32_multi = vt == dg.F32 and per_pass != 0
    x64 = dg.storage_to_f64(vt, rows) if f32_multi else None
    for metric in metrics:
        assert pkg.batch_labeled_plan(c, metric)[0] == per_pass, (dim, metric)
        assert pkg.batch_labeled_plan(c, metric) == pkg.batch_masked_plan(c, metric)       # one launch shape with the masked batch
        own = [c.scan_distances(metric, qs[i]) for i in range(9)]
        ref = [lc.f64_distances(metric, qs[i], x64) for i in range(9)] if f32_multi else None
        for lname, (labels, asked) in lc.layouts(n).items():
            c.set_labels(labels)
            for mname, (mq, mlab) in _mixes(qs, asked).items():
                qidx = [0] * 9 if mname == "one_query_many_labels" else list(range(9))
                for nq in NQS:
                    # every k on one layout and the full batch; k = 20 everywhere
                    for k in (KS if (lname == "uniform5" or nq == 9) else (20,)):
                        res = c.scan_topk_batch_labeled(metric, mq[:nq], mlab[:nq], k)
                        assert res[0].shape == (nq, k) and len(res[2]) == nq
                        for i in range(nq):
                            ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, mname, nq, k, i)
                            allowed = labels == mlab[i]
                            if not f32_multi:                   # integer sums / the single scans themselves: the handle's own floats
                                lc.assert_same(_answer(res, i), *lc.expected(own[qidx[i]], allowed, k), ctx=ctx)
                                if k == 20 and nq == 5:
                                    lc.assert_same(_answer(res, i), *c.scan_topk_labeled(metric, mq[i], k, int(mlab[i])), ctx=ctx)
                            else:
                                _judge_f64(_answer(res, i), ref[qidx[i]], allowed, metric, mq[i], k, ctx)
                        if f32_multi and (nq == 9 or k == 20):  # bit for bit the masked batch under each label's bitmap
                            for label in np.unique(mlab[:nq]):
                                sel = np.nonzero(mlab[:nq] == label)[0]
                                c.set_mask(bits=labels == label)
                                mres = c.scan_topk_batch_masked(metric, np.ascontiguousarray(mq[sel]), k)
                                for j, i in enumerate(sel):
                                    lc.assert_same(_answer(res, i), *_answer(mres, j), ctx=(dim, metric, lname, mname, nq, k, i, "masked twin"))
    c.close()


def test_contract(pkg):
    n, dim, nq = 2001, 64, 6
    rows = lc.data(dg.U8, n, dim, 41)
    qs = lc.data(dg.U8, nq, dim, 42)
    labels = np.random.default_rng(4).integers(0, 3, n).astype(np.uint32)
    ql = np.array([2, 0, 1, 0, 2, 1], dtype=np.uint32)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labeled(dg.L2, qs, ql, 5)) == VG_ERR_INVALID           # no labels
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labeled(dg.L2, qs, ql, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labeled(dg.L2, qs, ql, 65)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labeled(dg.L2, qs[:0], ql[:0], 5)) == VG_ERR_INVALID   # nq = 0
    bad = ql.copy(); bad[3] = lc.NONE
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_labeled(dg.L2, qs, bad, 5)) == VG_ERR_INVALID
    # caller order, not label order: query i's rows carry ITS label
    ids, dist, cnt = c.scan_topk_batch_labeled(dg.L2, qs, ql, 20)
    for i in range(nq):
        assert cnt[i] == 20 and (labels[ids[i] - 1] == ql[i]).all(), i
    # the slots behind counts[i] are not written, and tie_order does not matter
    rare = labels.copy(); rare[:] = 0; rare[5] = 1; rare[n - 1] = 1
    c.set_labels(rare)
    ids, dist, cnt = c.scan_topk_batch_labeled(dg.L2, qs, ql, 20)
    assert cnt.tolist() == [0, 20, 2, 20, 0, 2] and not ids[0].any() and not ids[2, 2:].any()
    c.set_tie_order(pkg.TIE_REFERENCE)
    again = c.scan_topk_batch_labeled(dg.L2, qs, ql, 20)
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], dist) and np.array_equal(again[2], cnt)
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: every count 0
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert not e.scan_topk_batch_labeled(dg.L2, qs, ql, 20)[2].any()
    e.close()


@pytest.mark.parametrize("vt,dim,metrics", [(dg.U8, 64, lc.L2_COS), (dg.F32, 384, (dg.L2,)), (dg.F16, 384, (dg.L2,)),
                                            (dg.F32, 1536, lc.L2_COS), (dg.I8, 100, lc.L2_COS), (dg.F32, 4100, (dg.L2,))],
                         ids=["u8-64", "f32-384", "f16-384", "f32-1536", "i8-100", "f32-4100"])
def test_three_logical_shards_equal_one_corpus(pkg, vt, dim, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 51 + dim)
    qs = lc.data(vt, 9, dim, 52 + dim)
    rowids = np.arange(n, dtype=np.int64) * 3 + 7
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0, 0, 0], block_rows=64)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    with pytest.raises(pkg.VectorGpuError):
        sh.scan_topk_batch_labeled(dg.L2, qs, np.zeros(9, dtype=np.uint32), 5)               # no labels
    assert not sh.has_labels()
    for lname, (labels, asked) in lc.layouts(n).items():
        c.set_labels(labels)
        sh.set_labels(labels)
        assert sh.has_labels()
        for metric in metrics:
            for label in asked:
                for k in KS:
                    one = c.scan_topk_labeled(metric, qs[0], k, label)
                    lc.assert_same(sh.scan_topk_labeled(metric, qs[0], k, label), *one, ctx=(lname, metric, label, k))
                    assert (labels[(one[0] - 7) // 3] == label).all()
            for mname, (mq, mlab) in _mixes(qs, asked).items():
                for nq in NQS:
                    for k in (KS if nq == 9 else (20,)):
                        one = c.scan_topk_batch_labeled(metric, mq[:nq], mlab[:nq], k)
                        many = sh.scan_topk_batch_labeled(metric, mq[:nq], mlab[:nq], k)
                        assert one[2].tolist() == many[2].tolist(), (lname, mname, nq, k)
                        for i in range(nq):
                            lc.assert_same(_answer(many, i), *_answer(one, i), ctx=(lname, mname, metric, nq, k, i))
    sh.clear_labels()
    assert not sh.has_labels()
    sh.close()
    c.close()
