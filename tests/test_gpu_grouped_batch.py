"""Grouped batch scans (vg_scan_topk_batch_grouped[_masked]): the k nearest labels, each by its best row, for many queries.

Contract (include/vectorgpu.h): query i of a batch gets exactly what the grouped contract gives for query i alone - the rows with a
finite distance and a label (masked form: and a set mask bit), ordered by (distance, scan position); the first row of each label; the
first k of those.  Every comparison is exact: rowids, labels, and distance bits.

The expectation for query i is grouped_cases.expected over the handle's own floats for the path under test:
  * uint8 / int8, and every fallback shape (plan 0: one single grouped scan per query): scan_distances - the integer sums are
    identical, the fallback is the single scan;
  * f32 on a multi-query shape: the multi kernel's summation order may differ from the single scan's, so the distances come from
    scan_within_batch (radius = the largest finite float, limit = n): the same kernel, plan and per-pair arithmetic; rows it does not
    return are non-finite.  batch_grouped_plan must equal batch_masked_plan first, so the launch shape is known to be shared, and the
    `uniform5` layout is anchored to float64 numpy as well (membership, per-row value, nothing better left behind).

Left out of the kernel tables for their registers: the MASKED instances at 6 chunks per lane, 2 queries per pass,
of cosine (f32 / uint8 / int8) and of f32 L2 - they spill.  batch_grouped_plan(masked=True) reports 0 for those shapes (f32 x 1536
here) and the batch answers through single masked grouped scans; the unmasked plan of every shape is the `per_pass` column.
"""
import os
import re

import numpy as np
import pytest

import datagen as dg
import grouped_cases as gc
import labeled_cases as lc
from batch_reference import completeness_tol

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
KS = (1, 20, 64)
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
    """per query: the handle's own floats for the path the grouped batch takes on this corpus"""
    plan = pkg.batch_grouped_plan(c, metric, masked)
    if vt != dg.F32 or plan[0] == 0:
        return [c.scan_distances(metric, q) for q in qs]
    assert plan == pkg.batch_masked_plan(c, metric), (plan, "the grouped batch shares the masked batch's launch shape")
    n = c.rows
    out = []
    for ids, dist, _ in c.scan_within_batch(metric, qs, FLT_MAX, limit=n):
        d = np.full(n, np.inf, dtype=np.float32)
        d[ids - 1] = dist.astype(np.float32)
        out.append(d)
    return out


def _judge_f64(got, ref, labels, metric, q, k, ctx):
    """one f32 answer against float64 distances of every row: distinct labels, count, per-row value, order, and no label left
    behind whose best row is better than the last one returned - each within 1e-5 relative (batch_reference.completeness_tol)"""
    gi, gd, gl = got
    present = np.unique(labels[labels != gc.NONE])
    assert len(gi) == min(k, len(present)), ctx
    pos = gi - 1
    assert (labels[pos] == gl).all() and len(set(gl.tolist())) == len(gl), ctx
    q_l1 = float(np.abs(q.astype(np.float64)).sum())
    for p, d, l in zip(pos, gd, gl):
        assert abs(d - ref[p]) <= completeness_tol(metric, q_l1, ref[p]), (ctx, p, d, ref[p])
        assert ref[labels == l].min() >= ref[p] - completeness_tol(metric, q_l1, ref[p]), (ctx, "not its group's best row", l)
    assert np.all(np.diff(gd) >= 0), ctx
    left = ~np.isin(labels, gl) & (labels != gc.NONE)
    if len(gi) == k and left.any():
        assert float(ref[left].min()) >= float(gd[-1]) - completeness_tol(metric, q_l1, gd[-1]), ctx


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape_and_layout(pkg, vt, dim, per_pass, metrics):
    n = gc.N
    rows = lc.data(vt, n, dim, 31 + dim)
    qs = lc.data(vt, 9, dim, 32 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    integer = vt in (dg.U8, dg.I8)
    x64 = dg.storage_to_f64(vt, rows) if vt == dg.F32 and per_pass else None
    for metric in metrics:
        assert pkg.batch_grouped_plan(c, metric)[0] == per_pass, (dim, metric)
        own = _path_distances(pkg, c, vt, metric, qs)
        ref = [lc.f64_distances(metric, qs[i], x64) for i in range(9)] if x64 is not None else None
        for name, labels in gc.layouts(n, own[0]).items():
            c.set_labels(labels)
            if name == "unique":
                c.set_mask(bits=np.ones(n, dtype=bool))
            for nq in NQS:
                for k in KS:
                    res = c.scan_topk_batch_grouped(metric, qs[:nq], k)
                    assert res[0].shape == (nq, k) and len(res[3]) == nq
                    mres = c.scan_topk_batch_masked(metric, qs[:nq], k) if name == "unique" else None
                    for i in range(nq):
                        ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name, nq, k, i)
                        got = _answer(res, i)
                        want = gc.expected(own[i], labels, None, k)
                        gc.assert_same(got, *want, ctx=ctx)
                        assert res[3][i] == len(want[0]), ctx
                        if integer:
                            gc.assert_same(got, *c.scan_topk_grouped(metric, qs[i], k), ctx=(ctx, "single"))
                        if name == "unique":                    # every row its own group: the masked batch under an all-set mask
                            lc.assert_same(got[:2], mres[0][i, :mres[2][i]], mres[1][i, :mres[2][i]], ctx=(ctx, "masked twin"))
                        if name == "hot" and i == 0:
                            assert len(got[0]) == k and got[2][0] == 1 and len(set(got[2].tolist())) == k, ctx
                        if name == "uniform5" and x64 is not None:
                            _judge_f64(got, ref[i], labels, metric, qs[i], k, ctx)
            if name == "unique":
                c.clear_mask()
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64)], ids=["f32-384", "uint8-64"])
def test_copies_of_one_query_in_one_pass_agree(pkg, vt, dim):
    """the same query in all four slots of a pass, and another one behind: a list or an mlab register crossing between queries
    would make the copies differ"""
    n = gc.N
    rows = lc.data(vt, n, dim, 131 + dim)
    two = lc.data(vt, 2, dim, 132 + dim)
    qs = np.ascontiguousarray(np.concatenate([np.repeat(two[:1], 4, axis=0), two[1:]]))
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = _path_distances(pkg, c, vt, dg.L2, qs)
    for name, labels in gc.layouts(n, own[0]).items():
        c.set_labels(labels)
        for k in KS:
            res = c.scan_topk_batch_grouped(dg.L2, qs, k)
            first = _answer(res, 0)
            gc.assert_same(first, *gc.expected(own[0], labels, None, k), ctx=(name, k))
            for i in (1, 2, 3):
                gc.assert_same(_answer(res, i), *first, ctx=(name, k, i))
            gc.assert_same(_answer(res, 4), *gc.expected(own[4], labels, None, k), ctx=(name, k, "the other query"))
    c.close()


def _corpus(pkg, vt, n, dim, seed, nq):
    rows = lc.data(vt, n, dim, seed)
    qs = lc.data(vt, nq, dim, seed + 1)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    return c, qs


@pytest.mark.parametrize("groups", [7, 1000], ids=["mod7", "mod1000"])
def test_large_uint8_corpus_replaces_inside_the_lists(pkg, groups):
    n, nq, k = 200_000, 6, 64
    c, qs = _corpus(pkg, dg.U8, n, 64, 51, nq)
    labels = (np.arange(n) % groups).astype(np.uint32)
    c.set_labels(labels)
    for metric in (dg.L2, dg.COSINE):
        res = c.scan_topk_batch_grouped(metric, qs, k)
        for i in range(nq):
            own = c.scan_distances(metric, qs[i])
            gc.assert_same(_answer(res, i), *gc.expected(own, labels, None, k), ctx=(groups, metric, i))
            assert res[3][i] == min(k, groups)
    c.close()


def test_large_f32_corpus_with_a_hot_label(pkg):
    n, nq, k = 60_000, 6, 64
    c, qs = _corpus(pkg, dg.F32, n, 384, 61, nq)
    own = _path_distances(pkg, c, dg.F32, dg.L2, qs)
    labels = gc.hot(own[0], 500)
    c.set_labels(labels)
    res = c.scan_topk_batch_grouped(dg.L2, qs, k)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *gc.expected(own[i], labels, None, k), ctx=i)
        assert res[3][i] == k
    assert res[2][0, 0] == 1
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64), (dg.F32, 1536), (dg.F16, 384), (dg.F32, 4100)],
                         ids=["f32-384", "uint8-64", "f32-1536", "f16-384", "f32-4100"])
def test_masked_form(pkg, vt, dim):
    n, nq = gc.N, 5
    c, qs = _corpus(pkg, vt, n, dim, 71 + dim, nq)
    labels = np.random.default_rng(dim).integers(0, 30, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.L2, qs, 5, masked=True)) == VG_ERR_INVALID      # no mask set
    own = _path_distances(pkg, c, vt, dg.L2, qs, masked=True)
    own_free = _path_distances(pkg, c, vt, dg.L2, qs, masked=False)

    def check(allowed, ks, what):
        for k in ks:
            res = c.scan_topk_batch_grouped(dg.L2, qs, k, masked=True)
            for i in range(nq):
                want = gc.expected(own[i], labels, allowed, k)
                gc.assert_same(_answer(res, i), *want, ctx=(what, k, i))
                assert res[3][i] == len(want[0])
        return res

    free_ids, _, free_lab = gc.expected(own[0], labels, None, 64)
    # the best row (for query 0) of every group cleared: the representative becomes the group's next allowed row
    allowed = np.ones(n, dtype=bool)
    allowed[free_ids - 1] = False
    c.set_mask(bits=allowed)
    res = check(allowed, KS, "best cleared")
    assert res[3][0] == 30 and not set(res[0][0].tolist()) & set(free_ids.tolist())
    # a whole group cleared (query 0's nearest one)
    allowed = labels != free_lab[0]
    c.set_mask(bits=allowed)
    res = check(allowed, (64,), "group cleared")
    assert (res[3] == 29).all() and int(free_lab[0]) not in res[2].tolist()
    # a random 10 % mask; the unmasked form ignores it
    allowed = np.random.default_rng(dim + 1).random(n) < 0.1
    c.set_mask(bits=allowed)
    check(allowed, (20,), "random mask")
    res = c.scan_topk_batch_grouped(dg.L2, qs, 20)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *gc.expected(own_free[i], labels, None, 20), ctx=("the unmasked form ignores the mask", i))
    # an empty mask: every count 0
    c.set_mask(bits=np.zeros(n, dtype=bool))
    assert not c.scan_topk_batch_grouped(dg.L2, qs, 20, masked=True)[3].any()
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
        for k in KS:
            one = c.scan_topk_batch_grouped(dg.L2, qs, k, masked=masked)
            many = s.scan_topk_batch_grouped(dg.L2, qs, k, masked=masked)
            assert one[3].tolist() == many[3].tolist()
            for i in range(nq):
                gc.assert_same(_answer(one, i), *gc.expected(own[i], labels, allowed if masked else None, k), ctx=(masked, k, i))
                gc.assert_same(_answer(many, i), *_answer(one, i), ctx=(masked, k, i, "shards"))
    s.close()
    c.close()


def test_a_batch_larger_than_one_slice(pkg):
    n, dim, nq, k = gc.N, 64, FUSED_SLICE + 1, 20
    c, qs = _corpus(pkg, dg.U8, n, dim, 101, nq)
    labels = np.random.default_rng(6).integers(0, 40, n).astype(np.uint32)
    c.set_labels(labels)
    res = c.scan_topk_batch_grouped(dg.L2, qs, k)
    assert res[0].shape == (nq, k)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *gc.expected(c.scan_distances(dg.L2, qs[i]), labels, None, k), ctx=i)
    c.close()


def test_error_codes_and_an_empty_corpus(pkg):
    n, dim, nq = 2001, 100, 5
    c, qs = _corpus(pkg, dg.F32, n, dim, 91, nq)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.L2, qs, 5)) == VG_ERR_INVALID                  # no labels
    labels = np.random.default_rng(3).integers(0, 9, n).astype(np.uint32)
    c.set_labels(labels)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.L2, qs, 0)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.L2, qs, 65)) == VG_ERR_UNSUPPORTED
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(99, qs, 5)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.L2, qs[:0], 5)) == VG_ERR_INVALID             # nq = 0
    own = _path_distances(pkg, c, dg.F32, dg.L2, qs)
    res = c.scan_topk_batch_grouped(dg.L2, qs, 20)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *gc.expected(own[i], labels, None, 20), ctx=i)
    assert (res[3] == 9).all() and not res[0][:, 9:].any()       # the slots behind counts[i] are not written
    c.set_tie_order(pkg.TIE_REFERENCE)                          # the order does not follow tie_order
    again = c.scan_topk_batch_grouped(dg.L2, qs, 20)
    assert all(np.array_equal(a, b) for a, b in zip(again, res))
    c.set_tie_order(pkg.TIE_POSITION)
    c.close()
    e = pkg.Corpus(dg.F32, dim)                                 # no rows: labels of length 0 are labels, nothing is launched
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert not e.scan_topk_batch_grouped(dg.L2, qs, 5)[3].any()
    e.close()


def test_f16_rows_of_six_chunks_per_lane_are_refused_like_the_single_form(pkg):
    n, dim, nq = 301, 3072, 3
    c, qs = _corpus(pkg, dg.F16, n, dim, 71, nq)
    labels = (np.arange(n) // 2).astype(np.uint32)
    c.set_labels(labels)
    res = c.scan_topk_batch_grouped(dg.L2, qs, 20)
    for i in range(nq):
        gc.assert_same(_answer(res, i), *gc.expected(c.scan_distances(dg.L2, qs[i]), labels, None, 20), ctx=i)
    assert lc.error_code(pkg, lambda: c.scan_topk_batch_grouped(dg.COSINE, qs, 20)) == VG_ERR_UNSUPPORTED
    assert len(c.scan_topk(dg.COSINE, qs[0], 20)[0]) == 20      # the handle's plain scans still work
    assert len(c.scan_topk(dg.L2, qs[0], 20)[0]) == 20
    c.close()
