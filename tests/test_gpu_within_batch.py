"""Batch range scans (vg_scan_within_batch): many queries, a radius each, through the binding.

Contract (include/vectorgpu.h): query i's answer is what scan_within is contracted to return for (q_i, radii[i]) - the rows with
(double)d <= radii[i], NaN / +Inf never, ascending (distance, scan position), `limit` per query with the count of all matches kept.

  * uint8 / int8: every query bit for bit equal to the pinned CPU oracle's distances filtered here, and to scan_within; radii on tied
    distances, below the minimum and +Inf, different radii inside one pass, limits;
  * f32 against the oracle outside the tolerance band (the band's share is asserted before the engine is called);
  * f32, same arithmetic: the engine's own stream filtered here where the batch plan's launch shape is the plain scan's, the
    multi-query top-k scan's floats where it is not;
  * shapes without a multi-query form (f16 / bf16, long rows): the single range scans, bit for bit;
  * overflow of a query's region: complete answers, one more launch per overflowed pass;
  * contract, batches larger than a staging slice, logical shards == one corpus;
  * the shards' merge, single and batch form, against the oracle's order with equal distances in every shard.
"""
import numpy as np
import pytest

import datagen as dg
from test_gpu_within import _assert_same, _expected, _float_tolerance, _own_radii, _radii_at_ranks

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1
N, NQ = 2500, 9                                                # 9 queries: ragged against 4 and against 2 per pass


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


def _queries(vt, nq, dim, seed, low_entropy=False):
    return np.ascontiguousarray(dg.corpus(vt, nq, dim, seed, low_entropy))


def _passes(nq, per_pass):
    return (nq + per_pass - 1) // per_pass


# ------------------------------------------------------------------------------------------------- uint8 / int8, bit for bit

# the shapes of test_gpu_masked_batch.py: 1 / 2 / 3 chunks per lane at 4 queries per pass (1024 bytes: the multi-query plan finds a
# 2-chunk shape), and 4096 bytes = 64 lanes x 4 chunks, the 2-per-pass form
@pytest.mark.parametrize("vt,dim,per_pass", [(dg.U8, 64, 4), (dg.U8, 256, 4), (dg.I8, 768, 4), (dg.U8, 1024, 4), (dg.U8, 4096, 2)])
def test_int8_bit_exact_vs_oracle_and_single_scans(pkg, orc, vt, dim, per_pass):
    for low in (False, True):
        rows = dg.corpus(vt, N, dim, 400 + dim, low_entropy=low)
        qs = _queries(vt, NQ, dim, 1401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            assert pkg.within_batch_plan(c, metric)[0] == per_pass, (dim, metric)      # the multi-query form serves the shape
            want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(NQ)]
            per_query = [_radii_at_ranks(want[i]) for i in range(NQ)]
            tied = False
            for rnd in range(max(len(r) for r in per_query)):
                # rotated: the queries of one pass hold different radii (on a tied distance, below the minimum, +Inf side by side)
                radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
                exp = [_expected(want[i], radii[i]) for i in range(NQ)]
                tied = tied or any(np.isfinite(radii[i]) and int(np.sum(want[i] == np.float32(radii[i]))) > 1 for i in range(NQ))
                res = c.scan_within_batch(metric, qs, radii)
                assert len(res) == NQ
                for i in range(NQ):
                    ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, rnd, i, radii[i])
                    _assert_same(res[i], exp[i][0], exp[i][1], ctx=ctx)
                    _assert_same(c.scan_within(metric, qs[i], radii[i]), exp[i][0], exp[i][1], ctx=ctx)
                if rnd in (1, 3):                              # limits, as _check_with_limits (test_gpu_within.py) sets them
                    m0 = len(exp[rnd][0])
                    for limit in sorted(set([1, max(1, m0 // 2), max(1, m0 - 1), max(1, m0), m0 + 1, m0 + 1000])):
                        res = c.scan_within_batch(metric, qs, radii, limit=limit)
                        for i in range(NQ):
                            _assert_same(res[i], exp[i][0][:limit], exp[i][1][:limit], matches=len(exp[i][0]),
                                         ctx=(dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, rnd, i, "limit", limit))
            if low and dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
                assert tied, "the low-entropy case is there for radii on a tied distance"
        c.close()


# ------------------------------------------------------------------------------------------------- f32 against the oracle

# inputs for which the ORACLE ALONE keeps the band inside its cap (checked on the CPU for all 9 queries, 5 metrics, 4 quantiles)
@pytest.mark.parametrize("dim,seed_rows,seed_q,per_pass", [(35, 2535, 2536, 4), (384, 2884, 2885, 4), (768, 3268, 3269, 4), (1000, 4500, 4501, 2)])
def test_f32_vs_oracle_outside_the_tolerance_band(pkg, orc, dim, seed_rows, seed_q, per_pass):
    vt = dg.F32
    rows = dg.corpus(vt, N, dim, seed_rows)
    qs = _queries(vt, NQ, dim, seed_q)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    for metric in dg.ALL_METRICS:
        assert pkg.within_batch_plan(c, metric)[0] == per_pass, (dim, metric)
        want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(NQ)]
        tol = [_float_tolerance(want[i], vt, metric, qs[i], rows) for i in range(NQ)]
        for quant in (0.001, 0.01, 0.1, 0.5):
            j = max(1, int(round(quant * N)))
            radii, inside, band = [], [], []
            for i in range(NQ):
                assert np.isfinite(want[i]).all()
                w = want[i].astype(np.float64)
                s = np.sort(w)
                radii.append(0.5 * (s[j - 1] + s[j]))          # the midpoint of two consecutive oracle distances: j rows match
                inside.append(w <= radii[i])
                band.append(np.abs(w - radii[i]) <= tol[i])
                # a condition, not a measurement: asserted before the engine is called
                assert int(band[i].sum()) <= max(3, 0.01 * int(inside[i].sum())), (metric, dim, quant, i, int(band[i].sum()), int(inside[i].sum()))
            res = c.scan_within_batch(metric, qs, radii)
            for i in range(NQ):
                ids, dist, matches = res[i]
                ctx = (dg.METRIC_NAMES[metric], dim, quant, i)
                got = np.zeros(N, dtype=bool)
                got[ids - 1] = True
                assert len(ids) == matches and len(set(ids.tolist())) == matches, ctx
                assert np.array_equal(got[~band[i]], inside[i][~band[i]]), (ctx, np.nonzero((got != inside[i]) & ~band[i])[0][:5])
                assert np.all(dist <= radii[i]) and np.all(np.diff(dist) >= 0), ctx
                assert np.all(np.abs(dist - want[i][ids - 1].astype(np.float64)) <= tol[i][ids - 1]), ctx
    c.close()


# ------------------------------------------------------------------------------------------------- f32, same arithmetic

def test_f32_same_arithmetic(pkg):
    vt = dg.F32
    seen_same, seen_other = False, []
    for dim in (35, 128, 256, 384, 512, 768, 1000, 1024):
        rows = dg.corpus(vt, N, dim, 600 + dim)
        qs = _queries(vt, NQ, dim, 1601 + dim)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            per_pass, lpr, u = pkg.within_batch_plan(c, metric)
            assert per_pass in (2, 4), (dim, metric)
            if (lpr, u) == pkg.plan_scan_shape(vt, dim, metric)[:2]:
                # the plain scan's launch shape: the engine's own stream filtered on the host, bit for bit
                seen_same = True
                own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
                per_query = [_own_radii(own[i]) for i in range(NQ)]
                for rnd in range(max(len(r) for r in per_query)):
                    radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
                    res = c.scan_within_batch(metric, qs, radii)
                    for i in range(NQ):
                        ids, dist = _expected(own[i], radii[i])
                        _assert_same(res[i], ids, dist, ctx=(dg.METRIC_NAMES[metric], dim, rnd, i, radii[i]))
            else:
                # another lane decomposition: the floats are the multi-query top-k scan's (k = 64 keeps the batch on that kernel)
                seen_other.append((dim, metric))
                tids, tdist, tcnt = c.scan_topk_batch(metric, qs, 64)
                assert pkg.lib().vg_batch_last_path(c.h) == 5, (dim, metric)
                assert (tcnt == 64).all()
                radii = [float(tdist[i, 39]) for i in range(NQ)]
                res = c.scan_within_batch(metric, qs, radii)
                for i in range(NQ):
                    m = int(np.sum(tdist[i] <= radii[i]))
                    assert 40 <= m < 64, (dim, metric, i, m)   # (the whole group of the 40th distance lies inside the list)
                    _assert_same(res[i], tids[i, :m], tdist[i, :m].astype(np.float32), ctx=(dg.METRIC_NAMES[metric], dim, i))
        c.close()
    assert seen_same and seen_other, "both launch-shape cases are meant to be covered"


# ------------------------------------------------------------------------------------------------- shapes without a multi-query form

@pytest.mark.parametrize("vt,dim", [(dg.F16, 384), (dg.BF16, 384), (dg.F32, 4096)])
def test_shapes_without_a_multi_query_form_equal_the_single_scans(pkg, vt, dim):
    rows = dg.corpus(vt, N, dim, 800 + dim)
    qs = _queries(vt, NQ, dim, 1801 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    for metric in dg.ALL_METRICS:
        assert pkg.within_batch_plan(c, metric)[0] == 0, (vt, dim, metric)
        own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
        per_query = [_own_radii(own[i]) for i in range(NQ)]
        for rnd in (0, 2, 5):
            radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
            for limit in (None, 7):
                res = c.scan_within_batch(metric, qs, radii, limit=limit)
                for i in range(NQ):
                    single = c.scan_within(metric, qs[i], radii[i], limit=limit)
                    _assert_same(res[i], single[0], single[1].astype(np.float32), matches=single[2], ctx=(dg.TYPE_NAMES[vt], metric, rnd, i, limit))
                    ids, dist = _expected(own[i], radii[i])
                    assert res[i][2] == len(ids) and res[i][0].tolist() == ids[:len(res[i][0])].tolist()
        # the single range scan keeps its own result apart, on this path too
        single = c.scan_within(metric, qs[0], per_query[0][1])
        keys = c.within_keys(len(single[0]))
        launches = c.within_last_launches()
        c.scan_within_batch(metric, qs, [per_query[i][3] for i in range(NQ)])
        assert c.within_keys(len(single[0])).tolist() == keys.tolist() and c.within_last_launches() == launches
        with pytest.raises(pkg.VectorGpuError):
            c.within_keys(len(single[0]) + 1)
    c.close()


# ------------------------------------------------------------------------------------------------- overflow

@pytest.mark.parametrize("vt,dim,per_pass", [(dg.U8, 64, 4), (dg.U8, 4096, 2), (dg.F32, 384, 4)])
def test_overflow_relaunches_only_the_pass_that_overflowed(pkg, vt, dim, per_pass):
    rows = dg.corpus(vt, N, dim, 900 + dim)
    qs = _queries(vt, NQ, dim, 1901 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    metric = dg.L2
    assert pkg.within_batch_plan(c, metric)[0] == per_pass
    own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
    big = 5                                                    # one query of one pass matches 1000 rows, all others 20 or fewer
    radii = []
    for i in range(NQ):
        s = np.sort(own[i])
        rank = 1000 if i == big else 3 + i
        radii.append(0.5 * (float(s[rank - 1]) + float(s[rank])) if s[rank - 1] < s[rank] else float(s[rank - 1]))
    exp = [_expected(own[i], radii[i]) for i in range(NQ)]
    assert len(exp[big][0]) >= 1000 and all(len(exp[i][0]) <= 20 for i in range(NQ) if i != big)
    exact = vt != dg.F32 or pkg.within_batch_plan(c, metric)[1:] == pkg.plan_scan_shape(vt, dim, metric)[:2]
    assert exact
    pkg.set_within_batch_initial_capacity(c, 64)
    try:
        for limit in (None, 17):
            res = c.scan_within_batch(metric, qs, radii, limit=limit)
            assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 1
            for i in range(NQ):
                ids, dist = exp[i]
                cut = len(ids) if limit is None else limit
                _assert_same(res[i], ids[:cut], dist[:cut], matches=len(ids), ctx=(dim, i, limit))
        # two passes overflow: two more launches
        radii2 = list(radii)
        radii2[0] = radii[big]
        res = c.scan_within_batch(metric, qs, radii2)
        assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 2
        for i in range(NQ):
            ids, dist = _expected(own[i], radii2[i])
            _assert_same(res[i], ids, dist, ctx=(dim, i, "two passes"))
    finally:
        pkg.set_within_batch_initial_capacity(c, 0)
    res = c.scan_within_batch(metric, qs, radii)               # a capacity that fits: the passes, nothing more
    assert c.within_batch_last_launches() == _passes(NQ, per_pass)
    for i in range(NQ):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=(dim, i, "fits"))
    c.close()


def test_more_matches_than_the_host_sorts(pkg):
    """a query with more than 4096 matches goes through the device sort; with a limit only `limit` keys come back"""
    n, dim = 6000, 64
    rows = dg.corpus(dg.U8, n, dim, 950, low_entropy=True)
    qs = _queries(dg.U8, 5, dim, 951, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = [c.scan_distances(dg.L2, qs[i]) for i in range(5)]
    radii = [float("inf"), float(np.sort(own[1])[10]), float(np.sort(own[2])[5000]), float(np.sort(own[3])[4096]), float(np.sort(own[4])[4094])]
    for cap in (0, 100):
        pkg.set_within_batch_initial_capacity(c, cap)
        for limit in (None, 33, 5000):
            res = c.scan_within_batch(dg.L2, qs, radii, limit=limit)
            for i in range(5):
                ids, dist = _expected(own[i], radii[i])
                cut = len(ids) if limit is None else limit
                _assert_same(res[i], ids[:cut], dist[:cut], matches=len(ids), ctx=(cap, limit, i))
    pkg.set_within_batch_initial_capacity(c, 0)
    c.close()


# ------------------------------------------------------------------------------------------------- contract

def test_contract(pkg):
    dim = 16
    c = pkg.Corpus(dg.U8, dim)
    qs = _queries(dg.U8, 3, dim, 11)
    res = c.scan_within_batch(dg.L2, qs, 1e9)                  # an empty corpus: every count 0
    assert [(len(r[0]), len(r[1]), r[2]) for r in res] == [(0, 0, 0)] * 3
    assert c.within_batch_last_launches() == 0
    rows = dg.corpus(dg.U8, N, dim, 12)
    c.append(rows)
    assert _error_code(pkg, lambda: c.scan_within_batch(dg.L2, qs, [1.0, float("nan"), 2.0])) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_within_batch(dg.L2, qs[:0], [])) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_within_batch(99, qs, 1.0)) == VG_ERR_INVALID
    m = np.full(3, 7, dtype=np.int64)
    h = np.full(3, 7, dtype=np.int64)
    bad = np.array([1.0, float("nan"), 2.0])
    assert pkg.lib().vg_scan_within_batch(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(bad), 0, pkg._ptr(m), pkg._ptr(h)) == VG_ERR_INVALID
    assert m.tolist() == [0, 0, 0] and h.tolist() == [0, 0, 0]  # the counts are zeroed first
    m[:], h[:] = 7, 7                                           # a NULL argument zeroes the counts too
    assert pkg.lib().vg_scan_within_batch(c.h, dg.L2, None, 3, pkg._ptr(bad), 0, pkg._ptr(m), pkg._ptr(h)) == VG_ERR_INVALID
    assert m.tolist() == [0, 0, 0] and h.tolist() == [0, 0, 0]
    m[:], h[:] = 7, 7
    assert pkg.lib().vg_scan_within_batch(c.h, dg.L2, pkg._ptr(qs), 3, None, 0, pkg._ptr(m), pkg._ptr(h)) == VG_ERR_INVALID
    assert m.tolist() == [0, 0, 0] and h.tolist() == [0, 0, 0]
    m[:], h[:] = 7, 7
    assert pkg.lib().vg_scan_within_batch(c.h, 99, pkg._ptr(qs), 3, pkg._ptr(bad), 0, pkg._ptr(m), pkg._ptr(h)) == VG_ERR_INVALID
    assert m.tolist() == [0, 0, 0] and h.tolist() == [0, 0, 0]

    own = [c.scan_distances(dg.L2, qs[i]) for i in range(3)]
    radii = [float(np.sort(own[i])[10 * (i + 1)]) for i in range(3)]
    exp = [_expected(own[i], radii[i]) for i in range(3)]
    res = c.scan_within_batch(dg.L2, qs, radii)
    for i in range(3):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=i)
    same = c.scan_within_batch(dg.L2, qs, radii[1])            # a scalar radius is broadcast
    for i in range(3):
        ids, dist = _expected(own[i], radii[1])
        _assert_same(same[i], ids, dist, ctx=("scalar", i))
    res = c.scan_within_batch(dg.L2, qs, radii)
    # fetch / keys outside what is held
    L = pkg.lib()
    n0 = len(exp[0][0])
    assert _error_code(pkg, lambda: pkg._check(L.vg_scan_within_batch_fetch(c.h, 3, 0, 1, None, None))) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: pkg._check(L.vg_scan_within_batch_fetch(c.h, -1, 0, 1, None, None))) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: pkg._check(L.vg_scan_within_batch_fetch(c.h, 0, n0, 1, None, None))) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: pkg._check(L.vg_scan_within_batch_fetch(c.h, 0, -1, 2, None, None))) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.within_batch_keys(0, n0 + 1)) == VG_ERR_INVALID
    keys = c.within_batch_keys(0, n0)
    assert ((keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == exp[0][0].tolist()
    # the single scans on the handle still answer, and keep their own result apart
    tids, tdist = c.scan_topk(dg.L2, qs[0], 10)
    order = np.lexsort((np.arange(N), own[0]))[:10]
    assert tids.tolist() == (order + 1).tolist()
    _assert_same(c.scan_within(dg.L2, qs[2], radii[2]), exp[2][0], exp[2][1])
    assert c.within_batch_keys(0, n0).tolist() == keys.tolist()
    # a row mask on the handle is not read
    c.set_mask(bits=np.arange(N) % 2 == 0)
    res = c.scan_within_batch(dg.L2, qs, radii)
    for i in range(3):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=("mask", i))
    c.clear_mask()
    c.clear()                                                   # a cleared corpus holds no result
    assert _error_code(pkg, lambda: pkg._check(L.vg_scan_within_batch_fetch(c.h, 0, 0, 1, None, None))) == VG_ERR_INVALID
    c.close()


def test_a_batch_larger_than_a_staging_slice(pkg):
    n, dim, nq = N, 16, 300
    rows = dg.corpus(dg.U8, n, dim, 21, low_entropy=True)
    qs = _queries(dg.U8, nq, dim, 22, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    rng = np.random.default_rng(23)
    per_pass = pkg.within_batch_plan(c, dg.L2)[0]
    assert per_pass == 4
    ranks = rng.integers(0, 60, nq)
    single = []
    radii = []
    for i in range(nq):
        own = c.scan_distances(dg.L2, qs[i])
        radii.append(float(np.sort(own)[ranks[i]]))
        single.append(c.scan_within(dg.L2, qs[i], radii[i]))
        ids, dist = _expected(own, radii[i])
        _assert_same(single[i], ids, dist, ctx=i)
    res = c.scan_within_batch(dg.L2, qs, radii)
    assert c.within_batch_last_launches() == _passes(nq, per_pass)
    for i in range(nq):
        _assert_same(res[i], single[i][0], single[i][1].astype(np.float32), ctx=i)
    c.close()


# ------------------------------------------------------------------------------------------------- shards

@pytest.mark.parametrize("vt,dim", [(dg.U8, 100), (dg.F32, 384)])
def test_shards_equal_one_corpus(pkg, vt, dim):
    """4 logical shards on one device, block_rows = 256: the same kernels per shard, merged per query by global position"""
    low = vt == dg.U8
    rows = dg.corpus(vt, N, dim, 81 + dim, low_entropy=low)
    qs = _queries(vt, NQ, dim, 82 + dim, low_entropy=low)
    rowids = np.arange(N, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0] * 4, block_rows=256)
    for r0 in range(0, N, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    assert sh.within_batch_plan(dg.L2) == c.within_batch_plan(dg.L2)
    for metric in (dg.L2, dg.DOT, dg.L1):
        own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
        ranks = [0, 40, 700, N // 2, N - 1, 3, 12, 100, 1]
        radii = [float(np.sort(own[i])[ranks[i]]) for i in range(NQ)]
        radii[4] = float("inf")
        for limit in (None, 1, 33):
            one = c.scan_within_batch(metric, qs, radii, limit=limit)
            many = sh.scan_within_batch(metric, qs, radii, limit=limit)
            for i in range(NQ):
                ids, dist = _expected(own[i], radii[i], rowids)
                cut = len(ids) if limit is None else limit
                if vt == dg.U8 or c.within_batch_plan(metric)[1:] == pkg.plan_scan_shape(vt, dim, metric)[:2]:
                    _assert_same(one[i], ids[:cut], dist[:cut], matches=len(ids), ctx=("corpus", metric, i, limit))
                _assert_same(many[i], one[i][0], one[i][1].astype(np.float32), matches=one[i][2], ctx=("shards", metric, i, limit))
    sh.set_within_batch_initial_capacity(32)
    many = sh.scan_within_batch(dg.L2, qs, float("inf"))
    assert sh.within_batch_last_launches() == 2 * _passes(NQ, c.within_batch_plan(dg.L2)[0])   # every pass of every shard overflowed
    for i in range(NQ):
        ids, dist = _expected(c.scan_distances(dg.L2, qs[i]), float("inf"), rowids)
        _assert_same(many[i], ids, dist, ctx=("shards, overflow", i))
    sh.close()
    c.close()


def test_shards_merge_vs_oracle_with_ties_across_shards(pkg, orc):
    """The merge of the shards' held keys, single and batch form, against the order computed HERE from the pinned oracle's distances -
    not against the other entry point: 40 distinct uint8 rows repeated over 3000 positions, so that every distance is held by rows of
    all 3 shards and the order inside a distance is the global scan position's; 1 query and 5 (two passes at 4 per pass); limits that
    cut inside a run of equal distances, and above the match count.  uint8 distances are exact: equality, bit for bit."""
    vt, dim, n, S, B = dg.U8, 64, 3000, 3, 256
    rows = np.ascontiguousarray(dg.corpus(vt, 40, dim, 9140)[np.random.default_rng(9141).integers(0, 40, n)])
    qs = _queries(vt, 5, dim, 9142)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    sh = pkg.Shards(vt, dim, [0] * S, block_rows=B)
    sh.append(rows, rowids)
    shard_of = (np.arange(n) // B) % S
    for metric in (dg.SQUARED_L2, dg.L2):
        assert sh.within_batch_plan(metric)[0] == 4
        want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(5)]
        radii = [float(np.sort(want[i])[n // 3 + 100 * i]) for i in range(5)]
        exp = [_expected(want[i], radii[i], rowids) for i in range(5)]
        m0 = len(exp[0][0])
        tie = next(j for j in range(m0 // 2, m0) if exp[0][1][j - 1] == exp[0][1][j])      # a cut between two rows of one distance ...
        held_by = shard_of[(exp[0][0] - 11) // 3][exp[0][1] == exp[0][1][tie]]
        assert len(set(held_by.tolist())) == S, "... that rows of every shard hold"
        for limit in (None, 7, tie, max(len(e[0]) for e in exp) + 10):
            cut = n if limit is None else limit
            ctx = (dg.METRIC_NAMES[metric], limit)
            _assert_same(sh.scan_within(metric, qs[0], radii[0], limit=limit), exp[0][0][:cut], exp[0][1][:cut], matches=m0, ctx=(ctx, "single"))
            one = sh.scan_within_batch(metric, qs[:1], radii[:1], limit=limit)
            assert len(one) == 1
            _assert_same(one[0], exp[0][0][:cut], exp[0][1][:cut], matches=m0, ctx=(ctx, "batch of 1"))
            five = sh.scan_within_batch(metric, qs, radii, limit=limit)
            assert len(five) == 5
            for i in range(5):
                _assert_same(five[i], exp[i][0][:cut], exp[i][1][:cut], matches=len(exp[i][0]), ctx=(ctx, "batch of 5", i))
    sh.close()
