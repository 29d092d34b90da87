"""Capped batch scans (vg_scan_topk_batch_capped[_masked]): the k nearest rows, at most m = per_label of one label, for many queries.

Contract (include/vectorgpu.h): query i of a batch gets exactly what the capped contract gives for query i alone - the rows with a
finite distance and a label (masked form: and a set mask bit), ordered by (distance, scan position); a row is kept iff fewer than m
rows of its label have been kept; the first k rows kept.  One m covers the batch.  Every comparison is exact: rowids, labels, and
distance bits.

The expectation for query i is capped_cases.expected over the handle's own floats for the path under test (the grouped batch test's
rule):
  * uint8 / int8, and every fallback shape (plan 0: one single capped scan per query): scan_distances - the integer sums are
    identical, the fallback is the single scan;
  * f32 on a multi-query shape: the multi kernel's summation order may differ from the single scan's, so the distances come from
    scan_within_batch (radius = the largest finite float, limit = n): the same kernel, plan and per-pair arithmetic; rows it does not
    return are non-finite.  batch_capped_plan must equal batch_masked_plan first, so the launch shape is known to be shared, and the
    `uniform5` layout is anchored to float64 numpy as well (the cap, per-row value, order, nothing better left behind).

Left out of the kernel tables for their registers: the MASKED instances at 6 chunks per lane, 2 queries per pass,
of cosine (f32 / uint8 / int8) and of f32 L2 - they spill, like their grouped twins.  batch_capped_plan(masked=True) reports 0 for
those shapes (f32 x 1536 here) and the batch answers through single masked capped scans; the unmasked plan of every shape is the
`per_pass` column.
"""
import os
import re

import numpy as np
import pytest

import capped_cases as cc
from capped_cases import _judge_f64
import datagen as dg
import grouped_cases as gc
import labeled_cases as lc

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
KMS = ((1, 1), (20, 3), (64, 5), (64, 64))
NQS = (1, 3, 4, 9)


def _fused_slice():
    """VG_FUSED_SLICE as the source has it (vg_multi_masked.hip): queries go up in slices of this many"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sqlite-vector_amd", "csrc", "vg_multi_masked.hip")
    m = re.search(r"^#define\s+VG_FUSED_SLICE\s+(\d+)\s*$", open(src).read(), re.M)
    assert m, "VG_FUSED_SLICE is no longer a plain #define in vg_multi_masked.hip"
    return int(m.group(1))


FUSED_SLICE = _fused_slice()
FLT_MAX = float(np.finfo(np.float32).max)


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
    ids, dist, lab, cnt = res
    return ids[i, :cnt[i]], dist[i, :cnt[i]], lab[i, :cnt[i]]


def _path_distances(pkg, c, vt, metric, qs, masked=False):
    """per query: the handle's own floats for the path the capped batch takes on this corpus"""
    plan = pkg.batch_capped_plan(c, metric, masked)
    if vt != dg.F32 or plan[0] == 0:
        return [c.scan_distances(metric, q) for q in qs]
    assert plan == pkg.batch_masked_plan(c, metric), (plan, "the capped batch shares the masked batch's launch shape")
    n = c.rows
    out = []
    for ids, dist, _ in c.scan_within_batch(metric, qs, FLT_MAX, limit=n):
        d = np.full(n, np.inf, dtype=np.float32)
        d[ids - 1] = dist.astype(np.float32)
        out.append(d)
    return out


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape_and_layout(pkg, vt, dim, per_pass, metrics):
    n = gc.N
    rows = lc.data(vt, n, dim, 31 + dim)
    qs = lc.data(vt, 9, dim, 32 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    c.set_mask(bits=np.ones(n, dtype=bool))                      # (for the masked twin; the unmasked capped form ignores it)
    integer = vt in (dg.U8, dg.I8)
    x64 = dg.storage_to_f64(vt, rows) if vt == dg.F32 and per_pass else None
    for metric in metrics:
        assert pkg.batch_capped_plan(c, metric)[0] == per_pass, (dim, metric)
        own = _path_distances(pkg, c, vt, metric, qs)
        ref = [lc.f64_distances(metric, qs[i], x64) for i in range(9)] if x64 is not None else None
        for name, labels in gc.layouts(n, own[0]).items():
            c.set_labels(labels)
            for k, m in KMS:
                want = [cc.expected(own[i], labels, None, k, m) for i in range(9)]
                single = [c.scan_topk_capped(metric, qs[i], k, m) for i in range(9)] if integer else None
                for nq in NQS:
                    res = c.scan_topk_batch_capped(metric, qs[:nq], k, m)
                    assert res[0].shape == (nq, k) and len(res[3]) == nq
                    gres = c.scan_topk_batch_grouped(metric, qs[:nq], k) if m == 1 else None
                    plain = name == "unique" or (m == 64 and name != "some_none")
                    mres = c.scan_topk_batch_masked(metric, qs[:nq], k) if plain else None
                    for i in range(nq):
                        ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name, nq, k, m, i)
                        got = _answer(res, i)
                        gc.assert_same(got, *want[i], ctx=ctx)
                        assert res[3][i] == len(want[i][0]), ctx
                        if m == 1:                               # the grouped batch, bit for bit: counts too
                            gc.assert_same(got, *_answer(gres, i), ctx=(ctx, "grouped twin"))
                            assert res[3][i] == gres[3][i], ctx
                        if plain:                                # no effective cap: the masked batch under an all-set mask
                            lc.assert_same(got[:2], mres[0][i, :mres[2][i]], mres[1][i, :mres[2][i]], ctx=(ctx, "masked twin"))
                        if integer:
                            gc.assert_same(got, *single[i], ctx=(ctx, "single"))
                        if name == "hot" and i == 0:             # one label owns the 500 nearest rows: m of it, then the others
                            lab = got[2].tolist()
                            assert len(lab) == k and lab[:min(k, m)] == [1] * min(k, m) and 1 not in lab[m:], ctx
                        if name == "uniform5" and x64 is not None:
                            _judge_f64(got, ref[i], labels, metric, qs[i], k, m, ctx)
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64)], ids=["f32-384", "uint8-64"])
def test_queries_of_one_pass_do_not_share_a_list(pkg, vt, dim):
    """the same query in all four slots of a pass and another one behind, and a batch whose query 2 is the one the `hot` layout was
    built around: a list, an mlab register or a cap count crossing between queries would make the copies differ or move the hot
    label's rows into another query's answer"""
    n = gc.N
    rows = lc.data(vt, n, dim, 131 + dim)
    two = lc.data(vt, 2, dim, 132 + dim)
    copies = np.ascontiguousarray(np.concatenate([np.repeat(two[:1], 4, axis=0), two[1:]]))
    four = np.ascontiguousarray(lc.data(vt, 4, dim, 133 + dim))
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = _path_distances(pkg, c, vt, dg.L2, copies)
    own4 = _path_distances(pkg, c, vt, dg.L2, four)

    def single(q, own_q, labels, k, m):
        """the single-call answer: the single scan itself where its floats are the batch's (integers), the contract over the path's
        own floats otherwise"""
        want = cc.expected(own_q, labels, None, k, m)
        if vt != dg.F32:
            gc.assert_same(c.scan_topk_capped(dg.L2, q, k, m), *want, ctx=("single", k, m))
        return want

    for name, labels in gc.layouts(n, own[0]).items():
        c.set_labels(labels)
        for k, m in KMS:
            res = c.scan_topk_batch_capped(dg.L2, copies, k, m)
            first = _answer(res, 0)
            gc.assert_same(first, *single(copies[0], own[0], labels, k, m), ctx=(name, k, m))
            for i in (1, 2, 3):
                gc.assert_same(_answer(res, i), *first, ctx=(name, k, m, i))
            gc.assert_same(_answer(res, 4), *single(copies[4], own[4], labels, k, m), ctx=(name, k, m, "the other query"))
    labels = gc.hot(own4[2], 500)                               # query 2, not 0, is the one next to the hot label
    c.set_labels(labels)
    for k, m in KMS:
        res = c.scan_topk_batch_capped(dg.L2, four, k, m)
        for i in range(4):
            gc.assert_same(_answer(res, i), *single(four[i], own4[i], labels, k, m), ctx=("hot around query 2", k, m, i))
        lab = res[2][2, :res[3][2]].tolist()
        assert len(lab) == k and lab[:min(k, m)] == [1] * min(k, m) and 1 not in lab[m:], (k, m)
    c.close()


def _corpus(pkg, vt, n, dim, seed, nq):
    rows = lc.data(vt, n, dim, seed)
    qs = lc.data(vt, nq, dim, seed + 1)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    return c, qs


@pytest.mark.parametrize("groups", [7, 1000], ids=["mod7", "mod1000"])
def test_large_uint8_corpus_replaces_inside_a_full_label(pkg, groups):
    n, nq = 200_000, 5                                          # one full pass and one ragged
    c, qs = _corpus(pkg, dg.U8, n, 64, 51, nq)
    labels = (np.arange(n) % groups).astype(np.uint32)
    c.set_labels(labels)
    for metric in (dg.L2, dg.COSINE):
        own = [c.scan_distances(metric, q) for q in qs]
        for k, m in ((20, 3), (64, 3)):
            res = c.scan_topk_batch_capped(metric, qs, k, m)
            for i in range(nq):
                gc.assert_same(_answer(res, i), *cc.expected(own[i], labels, None, k, m), ctx=(groups, metric, k, m, i))
                assert res[3][i] == min(k, 3 * groups)
    c.close()


def test_large_f32_corpus_with_a_hot_label(pkg):
    n, nq = 60_000, 3
    c, qs = _corpus(pkg, dg.F32, n, 384, 61, nq)
    own = _path_distances(pkg, c, dg.F32, dg.L2, qs)
    labels = gc.hot(own[1], 500)
    c.set_labels(labels)
    plain_ids, _ = c.scan_topk(dg.L2, qs[1], 64)
    for m in (1, 2, 3, 5):
        assert len(set(labels[plain_ids - 1].tolist())) == 1     # what a top-64-then-cap would see for query 1: one label
        for k in (20, 64):
            res = c.scan_topk_batch_capped(dg.L2, qs, k, m)
            for i in range(nq):
                gc.assert_same(_answer(res, i), *cc.expected(own[i], labels, None, k, m), ctx=(k, m, i))
                assert res[3][i] == k
            lab = res[2][1].tolist()
            assert lab[:m] == [1] * m and 1 not in lab[m:], (k, m)
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64), (dg.F32, 1536), (dg.F16, 384), (dg.F32, 4100)],
                         ids=["f32-384", "uint8-64", "f32-1536", "f16-384", "f32-4100"])
def test_masked_form(pkg, vt, dim):
    n, nq = gc.N, 5
    c, qs = _corpus(pkg, vt, n, dim, 71 + dim, nq)
    labels = np.random.default_rng(dim).integers(0, 30, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs, 5, 3, masked=True)) == VG_ERR_INVALID      # no mask set
    if (vt, dim) == (dg.F32, 1536):                             # the instance that was left out: the fallback, and the plan says so
        assert pkg.batch_capped_plan(c, dg.L2, masked=True)[0] == 0 and pkg.batch_capped_plan(c, dg.L2)[0] == 2
    own = _path_distances(pkg, c, vt, dg.L2, qs, masked=True)
    own_free = _path_distances(pkg, c, vt, dg.L2, qs, masked=False)

    def check(allowed, kms, what):
        for k, m in kms:
            res = c.scan_topk_batch_capped(dg.L2, qs, k, m, masked=True)
            for i in range(nq):
                want = cc.expected(own[i], labels, allowed, k, m)
                gc.assert_same(_answer(res, i), *want, ctx=(what, k, m, i))
                assert res[3][i] == len(want[0])
        return res

    # half the rows allowed; the unmasked form ignores the mask
    allowed = np.random.default_rng(dim + 1).random(n) < 0.5
    c.set_mask(bits=allowed)
    res = check(allowed, KMS, "half the rows")
    assert all(allowed[res[0][i, :res[3][i]] - 1].all() for i in range(nq))
    res = c.scan_topk_batch_capped(dg.L2, qs, 20, 3)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *cc.expected(own_free[i], labels, None, 20, 3), ctx=("the unmasked form ignores the mask", i))
    # the rows the free answer kept (for query 0) are cleared: every label's next allowed rows move up
    free_ids, _, _ = cc.expected(own[0], labels, None, 64, 3)
    allowed = np.ones(n, dtype=bool)
    allowed[free_ids - 1] = False
    c.set_mask(bits=allowed)
    res = check(allowed, ((20, 3), (64, 3)), "kept rows cleared")
    assert res[3][0] == 64 and not set(res[0][0].tolist()) & set(free_ids.tolist())
    # an empty mask: every count 0
    c.set_mask(bits=np.zeros(n, dtype=bool))
    assert not c.scan_topk_batch_capped(dg.L2, qs, 20, 3, masked=True)[3].any()
    c.close()


def test_three_shards_with_every_label_on_all_of_them(pkg):
    n, dim, nq = gc.N, 100, 5
    rows = lc.data(dg.F32, n, dim, 81)
    qs = lc.data(dg.F32, nq, dim, 82)
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    s = pkg.Shards(dg.F32, dim, [0, 0, 0], block_rows=64)       # blocks of 64 rows dealt out in turn
    s.append(rows)
    labels = (np.arange(n) % 50).astype(np.uint32)
    allowed = np.random.default_rng(5).random(n) < 0.3
    for h in (c, s):
        h.set_labels(labels)
        h.set_mask(bits=allowed)
    for masked in (False, True):
        own = _path_distances(pkg, c, dg.F32, dg.L2, qs, masked=masked)
        for k, m in KMS:
            one = c.scan_topk_batch_capped(dg.L2, qs, k, m, masked=masked)
            many = s.scan_topk_batch_capped(dg.L2, qs, k, m, masked=masked)
            assert one[3].tolist() == many[3].tolist()
            for i in range(nq):
                gc.assert_same(_answer(one, i), *cc.expected(own[i], labels, allowed if masked else None, k, m), ctx=(masked, k, m, i))
                gc.assert_same(_answer(many, i), *_answer(one, i), ctx=(masked, k, m, i, "shards"))
    s.close()
    c.close()


def test_a_batch_larger_than_one_slice(pkg):
    n, dim, nq, k, m = gc.N, 64, FUSED_SLICE + 1, 20, 3
    c, qs = _corpus(pkg, dg.U8, n, dim, 101, nq)
    labels = np.random.default_rng(6).integers(0, 40, n).astype(np.uint32)
    c.set_labels(labels)
    res = c.scan_topk_batch_capped(dg.L2, qs, k, m)
    assert res[0].shape == (nq, k)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *cc.expected(c.scan_distances(dg.L2, qs[i]), labels, None, k, m), ctx=i)
    c.close()


def test_error_codes_and_an_empty_corpus(pkg):
    n, dim, nq = 2001, 100, 5
    c, qs = _corpus(pkg, dg.F32, n, dim, 91, nq)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs, 5, 3)) == VG_ERR_INVALID                # no labels
    labels = np.random.default_rng(3).integers(0, 9, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs, 0, 3)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs, 65, 3)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs, 5, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(99, qs, 5, 3)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.L2, qs[:0], 5, 3)) == VG_ERR_INVALID           # nq = 0
    own = _path_distances(pkg, c, dg.F32, dg.L2, qs)
    res = c.scan_topk_batch_capped(dg.L2, qs, 20, 2)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *cc.expected(own[i], labels, None, 20, 2), ctx=i)
    assert (res[3] == 18).all() and not res[0][:, 18:].any()     # 9 labels x 2; the slots behind counts[i] are not written
    above = c.scan_topk_batch_capped(dg.L2, qs, 20, 1000)        # m above k behaves as k
    at_k = c.scan_topk_batch_capped(dg.L2, qs, 20, 20)
    assert all(np.array_equal(a, b) for a, b in zip(above, at_k))
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    again = c.scan_topk_batch_capped(dg.L2, qs, 20, 2)
    assert all(np.array_equal(a, b) for a, b in zip(again, res))
    c.set_tie_order(pkg.TIE_POSITION)
    c.close()
    e = pkg.Corpus(dg.F32, dim)                                 # no rows: labels of length 0 are labels, nothing is launched
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert not e.scan_topk_batch_capped(dg.L2, qs, 5, 3)[3].any()
    e.close()


def test_f16_rows_of_six_chunks_per_lane_are_refused_like_the_single_form(pkg):
    n, dim, nq = 301, 3072, 3
    c, qs = _corpus(pkg, dg.F16, n, dim, 71, nq)
    labels = (np.arange(n) // 4).astype(np.uint32)
    c.set_labels(labels)
    res = c.scan_topk_batch_capped(dg.L2, qs, 20, 3)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *cc.expected(c.scan_distances(dg.L2, qs[i]), labels, None, 20, 3), ctx=i)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_capped(dg.COSINE, qs, 20, 3)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_capped(dg.COSINE, qs[0], 20, 3)) == VG_ERR_UNSUPPORTED      # as the single form has it
    assert len(c.scan_topk(dg.COSINE, qs[0], 20)[0]) == 20      # the handle's plain scans still work
    c.close()
