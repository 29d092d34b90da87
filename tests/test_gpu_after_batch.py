"""Paged batch scans (vg_scan_topk_batch_after[_masked]): nq queries, a cursor each, through the binding.

Every query's rows equal what the single form (scan_topk_after) returns for that query and cursor, bit for bit: uint8 / int8 and the
fallbacks by their arithmetic, f32 because a shape whose multi-query launch shape differs from the single scan's (another summation
order) is answered by one single paged scan per query.  nq in (1, 4, 5, 9) makes ragged passes for both
plans (4 and 2 queries per pass); one query starts at the start cursor, one is exhausted, two share a query vector."""
import numpy as np
import pytest

import datagen as dg
from test_gpu_after import START, _behind, _order
from test_gpu_masked import _assert_same, _error_code

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1
NQS = (1, 4, 5, 9)


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


def _queries_and_cursors(c, vt, dim, metric, nq, seed, low, masked):
    """nq queries (two share a vector), a cursor each taken from the single form's own pages: the start cursor, an exhausted one, and
    cursors 1, 2, ... pages deep"""
    qs = [dg.query(vt, dim, seed + i, low_entropy=low) for i in range(nq)]
    if nq >= 4:
        qs[3] = qs[2]                                        # the same vector, different cursors
    cursors = []
    for i in range(nq):
        if i == 0:
            cursors.append(START)
        elif i == 1:
            cursors.append((float("inf"), 0) if nq % 2 else (3.0e38, 1 << 40))          # nothing / next to nothing behind it
        else:
            after = START
            for _ in range(i - 1):
                gi, gd = c.scan_topk_after(metric, qs[i], 20, after=after, masked=masked)
                if len(gi) == 0:
                    break
                after = (float(gd[-1]), int(gi[-1]))
            cursors.append(after)
    return np.stack(qs), cursors


def _check_batch(obj, single, vt, dim, metric, nq, k, low, masked, seed, ctx, allowed=None):
    qs, cursors = _queries_and_cursors(single, vt, dim, metric, nq, seed, low, masked)
    ids, dist, cnt = obj.scan_topk_batch_after(metric, qs, k, after=cursors, masked=masked)
    assert ids.shape == (nq, k) and len(cnt) == nq
    for i in range(nq):
        si, sd = single.scan_topk_after(metric, qs[i], k, after=cursors[i], masked=masked)
        _assert_same((ids[i, :cnt[i]], dist[i, :cnt[i]]), si, sd, ctx=(ctx, nq, k, i))
    rowids = np.arange(single.rows, dtype=np.int64) * 3 + 11                # (every corpus of this file is appended with these)
    for i in range(nq):                                                      # every count from the stream's distances and the contract
        own = single.scan_distances(metric, qs[i])
        want_ids, _ = _behind(own, _order(own, allowed if masked else None), rowids, cursors[i], k)
        assert cnt[i] == len(want_ids) and ids[i, :cnt[i]].tolist() == want_ids.tolist(), (ctx, nq, k, i)
    if nq >= 2:
        assert cnt[1] == 0                                                   # the exhausted query
        assert cnt[0] == min(k, single.rows if not masked else single.mask_count())
    if nq >= 4:
        assert cursors[2] != cursors[3] and ids[2, :cnt[2]].tolist() != ids[3, :cnt[3]].tolist()
    return qs, cursors


# uint8 / int8: both plans (U <= 3: 4 queries per pass; U = 4 / 6: 2), a partial last batch of rows, every metric
@pytest.mark.parametrize("vt,dim", [(dg.U8, 35), (dg.U8, 384), (dg.I8, 768), (dg.U8, 1024), (dg.I8, 1536), (dg.I8, 17)])
@pytest.mark.parametrize("masked", [False, True])
def test_int8_batch_equals_single(pkg, vt, dim, masked):
    n = 2531
    rows = dg.corpus(vt, n, dim, 700 + dim, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    allowed = np.random.default_rng(dim).random(n) < 0.35
    if masked:
        assert _error_code(pkg, lambda: c.scan_topk_batch_after(dg.L2, rows[:2], 5, masked=True)) == VG_ERR_INVALID     # no mask set
        c.set_mask(bits=allowed)
    plans = set()
    for metric in dg.ALL_METRICS:
        plans.add(pkg.batch_masked_plan(c, metric)[0])
        for nq in NQS:
            for k in (1, 20, 64):
                _check_batch(c, c, vt, dim, metric, nq, k, True, masked, 710 + dim, (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], masked), allowed)
    assert plans <= {2, 4} and plans, "these shapes are served by the multi-query kernel"
    if masked:
        c.set_mask(bits=np.zeros(n, dtype=bool))                       # an empty mask: every count 0, no launch
        _, _, cnt = c.scan_topk_batch_after(dg.L2, rows[:5], 20, masked=True)
        assert cnt.tolist() == [0] * 5
    c.close()


# f32: bit equality with the single form for EVERY dim.  Where the multi-query launch shape is the plain scan's (same lanes per row, same
# chunks per lane: the same summation order) the multi-query kernel answers; elsewhere the batch is nq single paged scans.  Both routes
# occur among these dims (asserted in test_f32_routes).
F32_DIMS = [4, 16, 100, 128, 256, 384, 512, 1000, 1536]     # (128, 256, 512: the plain scan takes 4 chunks per lane, the multi-query plan 2)


@pytest.mark.parametrize("dim", F32_DIMS)
@pytest.mark.parametrize("masked", [False, True])
def test_f32_batch_equals_single(pkg, dim, masked):
    n, vt = 2531, dg.F32
    rows = dg.corpus(vt, n, dim, 800 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows, np.arange(n, dtype=np.int64) * 3 + 11)
    allowed = np.random.default_rng(dim).random(n) < 0.35
    if masked:
        c.set_mask(bits=allowed)
    for metric in (dg.L2, dg.COSINE, dg.DOT, dg.L1):
        for nq in NQS:
            _check_batch(c, c, vt, dim, metric, nq, 20, False, masked, 810 + dim, (dim, dg.METRIC_NAMES[metric], masked), allowed)
    c.close()


def test_f32_routes(pkg):
    """among the dims above some run the multi-query kernel and some the per-query fallback (host logic only)"""
    same = set()
    for dim in F32_DIMS:
        c = pkg.Corpus(dg.F32, dim)
        nqpp, lpr, u = pkg.batch_masked_plan(c, dg.L2)
        same.add(nqpp in (2, 4) and (lpr, u) == pkg.plan_scan_shape(dg.F32, dim, dg.L2)[:2])
        c.close()
    assert same == {True, False}


# the fallbacks: f16 / bf16 and long rows are one single paged scan per query - same answers, by construction and checked
@pytest.mark.parametrize("vt,dim", [(dg.F16, 384), (dg.BF16, 100), (dg.F32, 4100), (dg.U8, 9000)])
@pytest.mark.parametrize("masked", [False, True])
def test_fallback_shapes(pkg, vt, dim, masked):
    n = 2531 if dim < 4000 else 1003
    low = vt == dg.U8
    rows = dg.corpus(vt, n, dim, 900 + dim, low_entropy=low)
    c = pkg.Corpus(vt, dim)
    c.append(rows, np.arange(n, dtype=np.int64) * 3 + 11)
    allowed = np.random.default_rng(dim).random(n) < 0.35
    if masked:
        c.set_mask(bits=allowed)
    assert pkg.batch_masked_plan(c, dg.L2)[0] == 0
    for metric in (dg.L2, dg.DOT):
        for nq in (1, 5):
            _check_batch(c, c, vt, dim, metric, nq, 20, low, masked, 910 + dim, (dg.TYPE_NAMES[vt], dim, metric, masked), allowed)
    c.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_shards_equal_one_corpus(pkg, n_shards):
    n, dim, vt = 2531, 100, dg.U8
    rows = dg.corpus(vt, n, dim, 81, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    allowed = np.random.default_rng(9).random(n) < 0.3
    for masked in (False, True):
        if masked:
            assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed)
        for metric in (dg.L2, dg.DOT, dg.L1):
            for nq in NQS:
                qs, cursors = _check_batch(sh, c, vt, dim, metric, nq, 20, True, masked, 90, (n_shards, metric, masked), allowed)
                # and the key forms agree: keys over global positions == one corpus' keys
                first = c.scan_topk_batch_after_keys(metric, qs, 20, masked=masked)
                ak = np.array([int(first[0][i, first[1][i] - 1]) if first[1][i] else 0 for i in range(nq)], dtype=np.uint64)
                ka, ca = c.scan_topk_batch_after_keys(metric, qs, 20, after_keys=ak, masked=masked)
                kb, cb = sh.scan_topk_batch_after_keys(metric, qs, 20, after_keys=ak, masked=masked)
                assert ca.tolist() == cb.tolist()
                for i in range(nq):
                    assert ka[i, :ca[i]].tolist() == kb[i, :cb[i]].tolist()
    sh.close()
    c.close()
