"""Masked batch scans (vg_scan_topk_batch_masked): one row mask, many queries per pass, through the binding.

Contract (include/vectorgpu.h): query i's answer is what scan_topk_masked is contracted to return for it - only allowed rows, ascending
(distance, scan position) whatever the tie_order, NaN / +Inf never, fewer than k rows when fewer allowed rows qualify.

  * uint8 / int8: every query bit for bit equal to the pinned CPU oracle's distances masked and sorted here, and to scan_topk_masked;
  * mask shapes per kernel form (4 and 2 queries per pass, 2 and 64 rows per batch), ragged batches;
  * f32: where the masked-batch plan's launch shape is the plain scan's, the engine's own stream masked here, bit for bit; every query
    judged against the oracle (count, membership, per-row tolerance, order, completeness) - no query left out;
  * shapes without a multi-query form (f16 / bf16, long rows): the single masked scans, bit for bit;
  * contract, lifecycle of the mask, batches larger than a staging slice, logical shards == one corpus.
"""
import numpy as np
import pytest

import datagen as dg
from batch_reference import completeness_tol
from test_gpu_masked import _assert_same, _expected, _mask_shapes, _mask_with_tie_at
from test_gpu_within import _float_tolerance

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


def _error_code(pkg, fn):
    with pytest.raises(pkg.VectorGpuError) as ei:
        fn()
    return int(str(ei.value).split("error ")[1].split(":")[0])


def _answer(res, i):
    ids, dist, cnt = res
    return ids[i, :cnt[i]], dist[i, :cnt[i]]


def _queries(vt, nq, dim, seed, low_entropy=False):
    return np.ascontiguousarray(dg.corpus(vt, nq, dim, seed, low_entropy))


# ------------------------------------------------------------------------------------------------- 1. uint8 / int8, bit for bit

# 64 / 256 / 768 bytes: 1 / 2 / 3 chunks per lane, 4 queries per pass.  1024 bytes: the PLAIN scan runs 4 chunks per lane, but the
# multi-query plan first asks for a shape of at most 3 (64 chunks = 32 lanes x 2) and finds one: 4 queries per pass as well.  The
# 2-queries-per-pass form needs a row no shape of <= 3 chunks per lane covers (more than 192 chunks): 4096 bytes = 64 lanes x 4.
@pytest.mark.parametrize("vt,dim,per_pass", [(dg.U8, 64, 4), (dg.U8, 256, 4), (dg.I8, 768, 4), (dg.U8, 1024, 4), (dg.U8, 4096, 2)])
def test_int8_bit_exact_vs_oracle_and_single_scans(pkg, orc, vt, dim, per_pass):
    n, nq = 2500, 9                                            # 9 queries: ragged against 4 and against 2 per pass
    rng = np.random.default_rng(1900 + dim)
    for low in (False, True):
        rows = dg.corpus(vt, n, dim, 400 + dim, low_entropy=low)
        qs = _queries(vt, nq, dim, 1401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            assert pkg.batch_masked_plan(c, metric)[0] == per_pass, (dim, metric)     # the multi-query form serves the shape
            want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(nq)]
            tie_mask = _mask_with_tie_at(want[0], 20, rng)      # the 20th place of query 0 falls inside a group of equal distances
            if low and dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
                assert tie_mask is not None, "the low-entropy case is there for ties at the k-th place"
            for allowed in (rng.random(n) < 0.5, rng.random(n) < 0.1, tie_mask):
                if allowed is None:
                    continue
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                for k in (1, 20, 64):
                    res = c.scan_topk_batch_masked(metric, qs, k)
                    for i in range(nq):
                        ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, k, i)
                        ids, dist = _expected(want[i], allowed, k)
                        _assert_same(_answer(res, i), ids, dist, ctx=ctx)
                        _assert_same(c.scan_topk_masked(metric, qs[i], k), ids, dist, ctx=ctx)
        c.close()


# ------------------------------------------------------------------------------------------------- f32 against the oracle

def _judge(got, want, tol, allowed, metric, q, k, ctx):
    """one query of a batch against the oracle's distances `want` (float32 per row, all finite): count, membership, per-row tolerance,
    order, and nothing better left behind"""
    gi, gd = got
    n_allowed = int(allowed.sum())
    assert len(gi) == min(k, n_allowed), (ctx, len(gi), n_allowed)
    if len(gi) == 0:
        return
    pos = gi - 1
    assert allowed[pos].all() and len(set(pos.tolist())) == len(pos), ctx
    assert np.all(np.abs(gd - want[pos].astype(np.float64)) <= tol[pos]), (ctx, float(np.max(np.abs(gd - want[pos]) - tol[pos])))
    assert np.all(np.diff(gd) >= 0), ctx
    same = np.diff(gd) == 0
    assert np.all(np.diff(pos)[same] > 0), ctx                 # equal distances: ascending rowid
    if len(gi) == k:                                           # (fewer than k: every allowed row came back)
        kth = float(gd[-1])
        slack = completeness_tol(metric, float(np.abs(q.astype(np.float64)).sum()), kth)
        out = allowed.copy()
        out[pos] = False
        if out.any():
            best_out = float(want[out].min())
            assert best_out >= kth - slack, (ctx, best_out, kth, slack)


# ------------------------------------------------------------------------------------------------- 2. mask shapes per kernel form

@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.F32, 4), (dg.U8, 64), (dg.F32, 1024)])
def test_mask_shapes(pkg, orc, vt, dim):
    metrics = (dg.L2, dg.COSINE, dg.DOT)
    low = vt == dg.U8
    for n in (37, 30001):
        assert n % 64 and n % 2
        rows = dg.corpus(vt, n, dim, 610 + dim, low_entropy=low)
        qs = _queries(vt, 5, dim, 1611 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        shapes = _mask_shapes(n)
        for metric in metrics:
            per_pass, lpr, u = pkg.batch_masked_plan(c, metric)
            assert per_pass == (2 if dim == 1024 else 4), (dim, metric, per_pass)
            same_shape = (lpr, u) == pkg.plan_scan_shape(vt, dim, metric)[:2]
            if (vt, dim) == (dg.F32, 384):
                assert same_shape and (lpr, u) == (32, 3)
            exact = same_shape or vt == dg.U8                  # integer sums do not depend on the launch shape
            own = [c.scan_distances(metric, qs[i]) for i in range(5)]
            if not exact:
                want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(5)]
                tol = [_float_tolerance(want[i], vt, metric, qs[i], rows) for i in range(5)]
            for name, allowed in shapes.items():
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                top = [_expected(own[i], allowed, 20) for i in range(5)]          # (its first entry is the k = 1 answer)
                for nq in (1, 3, 4, 5):
                    for k in (1, 20):
                        res = c.scan_topk_batch_masked(metric, qs[:nq], k)
                        assert res[0].shape == (nq, k) and len(res[2]) == nq
                        for i in range(nq):
                            ctx = (dg.TYPE_NAMES[vt], dim, n, dg.METRIC_NAMES[metric], name, nq, k, i)
                            if exact:
                                _assert_same(_answer(res, i), top[i][0][:k], top[i][1][:k], ctx=ctx)
                            else:
                                _judge(_answer(res, i), want[i], tol[i], allowed, metric, qs[i], k, ctx)
                        if name == "empty":
                            assert not res[2].any()
                        if name == "fewer_than_k" and k == 20:
                            assert res[2].tolist() == [min(n, 7)] * nq
        c.close()


# ------------------------------------------------------------------------------------------------- 3. f32, every query judged

@pytest.mark.parametrize("dim", [4, 100, 128, 200, 384, 512, 1024])
def test_f32_every_query_against_the_oracle(pkg, orc, dim):
    n, nq = 2531, 9
    rows = dg.corpus(dg.F32, n, dim, 700 + dim)
    qs = _queries(dg.F32, nq, dim, 701 + dim)
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    rng = np.random.default_rng(77 + dim)
    for metric in dg.ALL_METRICS:
        assert pkg.batch_masked_plan(c, metric)[0] in (2, 4), (dim, metric)
        want = [orc.scan_distances(orc.AVX2, metric, dg.F32, qs[i], rows) for i in range(nq)]
        assert all(np.isfinite(w).all() for w in want)
        tol = [_float_tolerance(want[i], dg.F32, metric, qs[i], rows) for i in range(nq)]
        for density in (0.5, 0.05):
            allowed = rng.random(n) < density
            assert c.set_mask(bits=allowed) == int(allowed.sum())
            for k in (1, 20, 64):
                res = c.scan_topk_batch_masked(metric, qs, k)
                for i in range(nq):
                    _judge(_answer(res, i), want[i], tol[i], allowed, metric, qs[i], k, (dg.METRIC_NAMES[metric], dim, density, k, i))
    c.close()


# ------------------------------------------------------------------------------------------------- 4. fallback shapes

@pytest.mark.parametrize("vt,dim", [(dg.F16, 384), (dg.BF16, 100), (dg.F32, 4100)])
def test_fallback_shapes_are_the_single_masked_scans(pkg, vt, dim):
    eq, erows = dg.edge_rows(vt, dim, 90)
    rows = np.ascontiguousarray(np.concatenate([dg.corpus(vt, 1500, dim, 800 + dim), erows, dg.corpus(vt, 501, dim, 801 + dim)]))
    n = len(rows)
    qs = np.ascontiguousarray(np.stack([eq] + [dg.query(vt, dim, 802 + dim + i) for i in range(4)]))
    nq = len(qs)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    rng = np.random.default_rng(31 + dim)
    special = False
    for metric in dg.ALL_METRICS:
        assert pkg.batch_masked_plan(c, metric)[0] == 0, (vt, dim, metric)
        own = [c.scan_distances(metric, qs[i]) for i in range(nq)]
        special = special or any(bool(np.isnan(o).any() or np.isposinf(o).any()) for o in own)
        masks = [np.ones(n, dtype=bool), rng.random(n) < 0.3]
        masks[1][1500:1500 + len(erows)] = True                 # the NaN / Inf rows are allowed under both
        for allowed in masks:
            c.set_mask(bits=allowed)
            for k in (1, 20, 64):
                res = c.scan_topk_batch_masked(metric, qs, k)
                for i in range(nq):
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], k, i)
                    gi, gd = _answer(res, i)
                    si, sd = c.scan_topk_masked(metric, qs[i], k)
                    _assert_same((gi, gd), si, sd, ctx=ctx)
                    ids, dist = _expected(own[i], allowed, k)
                    _assert_same((gi, gd), ids, dist, ctx=ctx)
                    assert np.all(gd < np.inf), ctx             # NaN / +Inf never come back
    assert special, "the edge rows are there for their NaN / Inf distances"
    c.close()


# ------------------------------------------------------------------------------------------------- 5. contract and lifecycle

def test_contract_and_lifecycle(pkg):
    n, dim, nq = 4001, 100, 6
    rows = dg.corpus(dg.F32, n, dim, 31)
    qs = _queries(dg.F32, nq, dim, 33)
    allowed = np.random.default_rng(6).random(n) < 0.2
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    # f32 x 100 runs 16 lanes x 2 chunks in the plain scan, and two chunks per lane fit the 4-queries-per-pass form: one launch shape,
    # so the batch carries the single masked scan's bits
    assert pkg.batch_masked_plan(c, dg.L2) == (4, 16, 2) and pkg.plan_scan_shape(dg.F32, dim, dg.L2)[:2] == (16, 2)

    def check(corpus, k=20):
        """the batch against the single masked scans, bit for bit"""
        res = corpus.scan_topk_batch_masked(dg.L2, qs, k)
        for i in range(nq):
            _assert_same(_answer(res, i), *corpus.scan_topk_masked(dg.L2, qs[i], k), ctx=i)
        return res

    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 5)) == VG_ERR_INVALID       # no mask
    before = c.scan_topk_batch(dg.L2, qs, 10)
    c.set_mask(bits=allowed)
    after = c.scan_topk_batch(dg.L2, qs, 10)                   # the unmasked batch does not see the mask
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    res = check(c)
    assert res[2].tolist() == [20] * nq and allowed[res[0] - 1].all()
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 0)) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, -3)) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 65)) == VG_ERR_UNSUPPORTED
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs[:0], 5)) == VG_ERR_INVALID  # nq = 0
    # tie_order = reference: the same answer
    c.set_tie_order(pkg.TIE_REFERENCE)
    res_ref = c.scan_topk_batch_masked(dg.L2, qs, 20)
    c.set_tie_order(pkg.TIE_POSITION)
    for a, b in zip(res, res_ref):
        assert np.array_equal(a, b)
    # an empty mask: every count 0
    c.set_mask(bits=np.zeros(n, dtype=bool))
    assert not c.scan_topk_batch_masked(dg.L2, qs, 20)[2].any()
    c.set_mask(bits=allowed)
    # clone keeps the mask
    d = c.clone()
    assert d.mask_count() == int(allowed.sum())
    for a, b in zip(res, check(d)):
        assert np.array_equal(a, b)
    d.close()
    # patch_rows keeps it, the next masked batch answers from the new bytes
    best = int(res[0][0, 0] - 1)
    c.patch_rows(np.array([best], dtype=np.int64), np.full((1, dim), 1000.0, dtype=np.float32))
    assert c.mask_count() == int(allowed.sum())
    res2 = check(c)
    assert res2[0][0, 0] != res[0][0, 0] and (best + 1) not in res2[0][0].tolist()
    # append, delete_rows and clear each drop it
    c.append(rows[:3])
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 5)) == VG_ERR_INVALID
    c.set_mask(bits=np.ones(c.rows, dtype=bool))
    c.delete_rows(np.array([1, 7], dtype=np.int64))
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 5)) == VG_ERR_INVALID
    c.set_mask(bits=np.ones(c.rows, dtype=bool))
    c.clear()
    assert _error_code(pkg, lambda: c.scan_topk_batch_masked(dg.L2, qs, 5)) == VG_ERR_INVALID
    c.close()


def test_a_batch_larger_than_one_staging_slice(pkg):
    n, dim, nq = 3000, 64, 300
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    qs = _queries(dg.U8, nq, dim, 72, low_entropy=True)
    allowed = np.random.default_rng(5).random(n) < 0.3
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    c.set_mask(bits=allowed)
    assert pkg.batch_masked_plan(c, dg.L2)[0] == 4
    res = c.scan_topk_batch_masked(dg.L2, qs, 20)
    for i in range(nq):
        si, sd = c.scan_topk_masked(dg.L2, qs[i], 20)
        _assert_same(_answer(res, i), si, sd, ctx=i)
    c.close()


# ------------------------------------------------------------------------------------------------- 6. shards equal one corpus

@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
def test_shards_equal_one_corpus(pkg, n_shards):
    n, dim, nq = 5003, 100, 5
    rows = dg.corpus(dg.U8, n, dim, 81, low_entropy=True)
    qs = _queries(dg.U8, nq, dim, 82, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(dg.U8, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    with pytest.raises(pkg.VectorGpuError):
        sh.scan_topk_batch_masked(dg.L2, qs, 5)                # no mask
    rng = np.random.default_rng(9)
    masks = {"half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.02, "all": np.ones(n, dtype=bool), "empty": np.zeros(n, dtype=bool)}
    m = np.zeros(n, dtype=bool); m[35:47] = True; m[n - 3:] = True; masks["runs_over_block_borders"] = m
    for name, allowed in masks.items():
        assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed) == int(allowed.sum())
        for metric in (dg.L2, dg.DOT, dg.L1):
            own = [c.scan_distances(metric, qs[i]) for i in range(nq)]
            for k in (1, 20, 64):
                one = c.scan_topk_batch_masked(metric, qs, k)
                many = sh.scan_topk_batch_masked(metric, qs, k)
                for i in range(nq):
                    ids, dist = _expected(own[i], allowed, k, rowids)
                    _assert_same(_answer(one, i), ids, dist, ctx=("corpus", name, metric, k, i))
                    _assert_same(_answer(many, i), ids, dist, ctx=("shards", n_shards, name, metric, k, i))
    sh.close()
    c.close()
