"""Masked batch range scans (vg_scan_within_batch_masked): one row mask, many queries, a radius each, through the binding.

Contract (include/vectorgpu.h): query i's answer is what scan_within_masked is contracted to return for (q_i, radii[i]).

  * uint8 / int8: every query bit for bit equal to the pinned CPU oracle's distances masked and filtered here, and to scan_within_masked;
  * f32: scan_within_batch with the same radii restricted to the allowed rows on the host, bit for bit and count for count, wherever
    the masked plan reports the unmasked plan's launch shape (the arithmetic of a (query, row) pair depends on the lane decomposition,
    not on the mask) - the unmasked batch is anchored to the oracle by test_gpu_within_batch.py; the single masked scans where the
    plan routes a shape to the fallback;
  * every mask shape, per-query independence inside one batch, overflow (only the overflowed pass runs again), shapes without a
    multi-query form, a batch larger than a staging slice, logical shards == one corpus, the contract's errors.
"""
import numpy as np
import pytest

import datagen as dg
from test_gpu_masked import _mask_shapes
from test_gpu_within import _assert_same, _expected, _own_radii, _radii_at_ranks

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


def _expected_masked(dist, allowed, radius, rowids=None):
    d = np.where(np.asarray(allowed, dtype=bool), np.asarray(dist, dtype=np.float32), np.float32(np.nan))
    return _expected(d, radius, rowids)


def _restrict(res, allowed, rowid_to_pos=lambda ids: ids - 1):
    """a (rowids, distances, matches) result restricted to the allowed rows on the host (a result without a limit)"""
    ids, dist, _ = res
    keep = allowed[rowid_to_pos(ids)]
    return ids[keep], dist[keep].astype(np.float32)


# ------------------------------------------------------------------------------------------------- uint8 / int8, bit for bit

@pytest.mark.parametrize("vt,dim", [(dg.U8, 64), (dg.U8, 256), (dg.I8, 768), (dg.U8, 1024), (dg.U8, 4096)])
def test_int8_bit_exact_vs_oracle_and_single_scans(pkg, orc, vt, dim):
    rng = np.random.default_rng(2900 + dim)
    for low in (False, True):
        rows = dg.corpus(vt, N, dim, 400 + dim, low_entropy=low)
        qs = _queries(vt, NQ, dim, 1401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            per_pass = pkg.within_batch_masked_plan(c, metric)[0]
            assert per_pass in (0, 2, 4), (dim, metric)
            want = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) for i in range(NQ)]
            for density in (0.5, 0.1):
                allowed = rng.random(N) < density
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                per_query = [_radii_at_ranks(want[i][allowed]) for i in range(NQ)]
                for rnd in range(max(len(r) for r in per_query)):
                    # rotated: the queries of one pass hold different radii (on a tied distance, below the minimum, +Inf side by side)
                    radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
                    exp = [_expected_masked(want[i], allowed, radii[i]) for i in range(NQ)]
                    res = c.scan_within_batch_masked(metric, qs, radii)
                    assert len(res) == NQ
                    if per_pass:
                        assert c.within_batch_last_launches() == _passes(NQ, per_pass)
                    for i in range(NQ):
                        ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, density, rnd, i, radii[i])
                        _assert_same(res[i], exp[i][0], exp[i][1], ctx=ctx)
                        _assert_same(c.scan_within_masked(metric, qs[i], radii[i]), exp[i][0], exp[i][1], ctx=ctx)
                    if rnd in (1, 3):
                        m0 = len(exp[rnd][0])
                        for limit in sorted(set([1, max(1, m0 // 2), max(1, m0 - 1), max(1, m0), m0 + 1, m0 + 1000])):
                            res = c.scan_within_batch_masked(metric, qs, radii, limit=limit)
                            for i in range(NQ):
                                _assert_same(res[i], exp[i][0][:limit], exp[i][1][:limit], matches=len(exp[i][0]),
                                             ctx=(dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, rnd, i, "limit", limit))
        c.close()


# ------------------------------------------------------------------------------------------------- f32: the unmasked batch, restricted

def test_f32_equals_the_unmasked_batch_restricted_to_the_mask(pkg):
    vt = dg.F32
    rng = np.random.default_rng(31)
    for dim in (35, 128, 384, 768, 1000):
        rows = dg.corpus(vt, N, dim, 600 + dim)
        qs = _queries(vt, NQ, dim, 1601 + dim)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            plan = pkg.within_batch_masked_plan(c, metric)
            own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
            per_query = [_own_radii(own[i]) for i in range(NQ)]
            for density in (0.5, 0.05):
                allowed = rng.random(N) < density
                c.set_mask(bits=allowed)
                for rnd in (0, 1, 3, 5, 7):
                    radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
                    res = c.scan_within_batch_masked(metric, qs, radii)
                    if plan[0] == 0:
                        # routed to the fallback: nq single masked range scans
                        for i in range(NQ):
                            single = c.scan_within_masked(metric, qs[i], radii[i])
                            _assert_same(res[i], single[0], single[1].astype(np.float32), matches=single[2], ctx=(dim, metric, rnd, i, "fallback"))
                        continue
                    assert plan[1:] == pkg.within_batch_plan(c, metric)[1:], (dim, metric)        # the same lane decomposition
                    assert c.within_batch_last_launches() == _passes(NQ, plan[0])
                    unmasked = c.scan_within_batch(metric, qs, radii)
                    for i in range(NQ):
                        ids, dist = _restrict(unmasked[i], allowed)
                        _assert_same(res[i], ids, dist, ctx=(dg.METRIC_NAMES[metric], dim, density, rnd, i, radii[i]))
        c.close()


# ------------------------------------------------------------------------------------------------- mask shapes

@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 64)])
def test_mask_shapes(pkg, vt, dim):
    n, nq = 70001, 5
    low = vt == dg.U8
    rows = dg.corpus(vt, n, dim, 610 + dim, low_entropy=low)
    qs = _queries(vt, nq, dim, 1611 + dim, low_entropy=low)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    metric = dg.L2
    plan = pkg.within_batch_masked_plan(c, metric)
    own = [c.scan_distances(metric, qs[i]) for i in range(nq)]
    ranks = [0, 7, n // 50, n // 3, n - 1]
    radii = [float(np.sort(own[i])[ranks[i]]) for i in range(nq)]
    radii[4] = float("inf")
    if vt == dg.F32 and plan[0] and plan[1:] != pkg.plan_scan_shape(vt, dim, metric)[:2]:
        base = [(r[0], r[1].astype(np.float32)) for r in c.scan_within_batch(metric, qs, radii)]      # another lane decomposition than the stream's
    else:
        base = [_expected(own[i], radii[i]) for i in range(nq)]
    for name, allowed in _mask_shapes(n).items():
        assert c.set_mask(bits=allowed) == int(allowed.sum())
        res = c.scan_within_batch_masked(metric, qs, radii)
        if name == "empty":
            assert c.within_batch_last_launches() == 0
        elif plan[0]:
            assert c.within_batch_last_launches() == _passes(nq, plan[0])
        for i in range(nq):
            ids, dist = base[i]
            keep = allowed[ids - 1]
            _assert_same(res[i], ids[keep], dist[keep], ctx=(dg.TYPE_NAMES[vt], name, i))
    c.close()


# ------------------------------------------------------------------------------------------------- per-query independence, overflow

@pytest.mark.parametrize("vt,dim", [(dg.U8, 64), (dg.U8, 4096), (dg.F32, 384)])
def test_queries_of_one_batch_are_independent_and_only_the_overflowed_pass_runs_again(pkg, vt, dim):
    rows = dg.corpus(vt, N, dim, 900 + dim)
    qs = _queries(vt, NQ, dim, 1901 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    metric = dg.L2
    per_pass, lpr, u = pkg.within_batch_masked_plan(c, metric)
    assert per_pass in (2, 4)
    assert vt != dg.F32 or (lpr, u) == pkg.plan_scan_shape(vt, dim, metric)[:2]      # the stream's floats are the batch's
    allowed = np.random.default_rng(4).random(N) < 0.5
    c.set_mask(bits=allowed)
    own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
    big = 5                                                    # one query matches 600 allowed rows: past its region of 64 keys
    radii = []
    for i in range(NQ):
        s = np.sort(own[i][allowed])
        rank = 600 if i == big else 3 + i
        radii.append(0.5 * (float(s[rank - 1]) + float(s[rank])) if s[rank - 1] < s[rank] else float(s[rank - 1]))
    radii[0] = float("-inf")                                   # nothing
    radii[4] = float("inf")                                    # every allowed row, in the pass of `big` (at 4 and at 2 per pass)
    exp = [_expected_masked(own[i], allowed, radii[i]) for i in range(NQ)]
    assert len(exp[0][0]) == 0 and len(exp[big][0]) >= 600 and len(exp[4][0]) == int(allowed.sum())
    assert all(0 < len(exp[i][0]) <= 20 for i in range(1, NQ) if i not in (big, 4))
    assert big // per_pass == 4 // per_pass
    pkg.set_within_batch_initial_capacity(c, 64)
    try:
        for limit in (None, 17):
            res = c.scan_within_batch_masked(metric, qs, radii, limit=limit)
            assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 1         # only the pass that overflowed ran again
            for i in range(NQ):
                ids, dist = exp[i]
                cut = len(ids) if limit is None else limit
                _assert_same(res[i], ids[:cut], dist[:cut], matches=len(ids), ctx=(dim, i, limit))
        radii2 = list(radii)
        radii2[8] = float("inf")                                   # the last (ragged) pass overflows too
        res = c.scan_within_batch_masked(metric, qs, radii2)
        assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 2
        for i in range(NQ):
            ids, dist = _expected_masked(own[i], allowed, radii2[i])
            _assert_same(res[i], ids, dist, ctx=(dim, i, "two passes"))
        # 40 allowed matches that are some 80 matches overall: the allowed ones fit 64 keys - no pass runs again
        s = np.sort(own[2][allowed])
        r40 = 0.5 * (float(s[39]) + float(s[40])) if s[39] < s[40] else float(s[39])
        fits = [r40 if i == 2 else float("-inf") for i in range(NQ)]
        ids, dist = _expected_masked(own[2], allowed, r40)
        assert len(ids) <= 64 < int(np.sum(own[2] <= r40))
        res = c.scan_within_batch_masked(metric, qs, fits)
        assert c.within_batch_last_launches() == _passes(NQ, per_pass)
        _assert_same(res[2], ids, dist, ctx="fits")
        assert all(res[i][2] == 0 for i in range(NQ) if i != 2)
    finally:
        pkg.set_within_batch_initial_capacity(c, 0)
    c.close()


# ------------------------------------------------------------------------------------------------- shapes without a multi-query form

@pytest.mark.parametrize("vt,dim", [(dg.F16, 384), (dg.BF16, 384), (dg.F32, 4096)])
def test_shapes_without_a_multi_query_form_equal_the_single_scans(pkg, vt, dim):
    rows = dg.corpus(vt, N, dim, 800 + dim)
    qs = _queries(vt, NQ, dim, 1801 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    allowed = np.random.default_rng(12).random(N) < 0.3
    c.set_mask(bits=allowed)
    for metric in dg.ALL_METRICS:
        assert pkg.within_batch_masked_plan(c, metric)[0] == 0, (vt, dim, metric)
        own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
        per_query = [_own_radii(own[i]) for i in range(NQ)]
        for rnd in (0, 2, 5):
            radii = [per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)]
            for limit in (None, 7):
                res = c.scan_within_batch_masked(metric, qs, radii, limit=limit)
                for i in range(NQ):
                    single = c.scan_within_masked(metric, qs[i], radii[i], limit=limit)
                    _assert_same(res[i], single[0], single[1].astype(np.float32), matches=single[2], ctx=(dg.TYPE_NAMES[vt], metric, rnd, i, limit))
                    ids, dist = _expected_masked(own[i], allowed, radii[i])
                    cut = len(ids) if limit is None else limit
                    _assert_same(res[i], ids[:cut], dist[:cut], matches=len(ids), ctx=(dg.TYPE_NAMES[vt], metric, rnd, i, limit, "stream"))
    c.close()


def test_a_batch_larger_than_a_staging_slice(pkg):
    n, dim, nq = N, 64, 300
    rows = dg.corpus(dg.U8, n, dim, 21, low_entropy=True)
    qs = _queries(dg.U8, nq, dim, 22, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    rng = np.random.default_rng(23)
    allowed = rng.random(n) < 0.4
    c.set_mask(bits=allowed)
    per_pass = pkg.within_batch_masked_plan(c, dg.L2)[0]
    assert per_pass in (2, 4)
    ranks = rng.integers(0, 60, nq)
    radii, exp = [], []
    for i in range(nq):
        own = c.scan_distances(dg.L2, qs[i])
        radii.append(float(np.sort(own[allowed])[ranks[i]]))
        exp.append(_expected_masked(own, allowed, radii[i]))
    res = c.scan_within_batch_masked(dg.L2, qs, radii)
    assert c.within_batch_last_launches() == _passes(nq, per_pass)
    for i in range(nq):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=i)
    c.close()


# ------------------------------------------------------------------------------------------------- shards

@pytest.mark.parametrize("n_shards", [3, 8])
@pytest.mark.parametrize("vt,dim", [(dg.U8, 100), (dg.F32, 384)])
def test_shards_equal_one_corpus(pkg, n_shards, vt, dim):
    low = vt == dg.U8
    rows = dg.corpus(vt, N, dim, 81 + dim, low_entropy=low)
    qs = _queries(vt, NQ, dim, 82 + dim, low_entropy=low)
    rowids = np.arange(N, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, N, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    assert sh.within_batch_masked_plan(dg.L2) == c.within_batch_masked_plan(dg.L2)
    assert _error_code(pkg, lambda: sh.scan_within_batch_masked(dg.L2, qs, 1.0)) == VG_ERR_INVALID      # no mask
    rng = np.random.default_rng(10)
    one_shard = np.zeros(N, dtype=bool)                            # every set bit in blocks of one shard
    for b in range(1, N // 40, n_shards):
        one_shard[b * 40:b * 40 + 40:3] = True
    for name, allowed in (("half", rng.random(N) < 0.5), ("sparse", rng.random(N) < 0.02), ("one_shard_only", one_shard)):
        assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed) == int(allowed.sum())
        for metric in (dg.L2, dg.DOT, dg.L1):
            own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
            ranks = [0, 40, 700, N // 2, N - 1, 3, 12, 100, 1]
            radii = [float(np.sort(own[i])[ranks[i]]) for i in range(NQ)]
            radii[4] = float("inf")
            exact = vt == dg.U8 or c.within_batch_masked_plan(metric)[1:] == pkg.plan_scan_shape(vt, dim, metric)[:2]
            for limit in (None, 1, 33):
                one = c.scan_within_batch_masked(metric, qs, radii, limit=limit)
                many = sh.scan_within_batch_masked(metric, qs, radii, limit=limit)
                for i in range(NQ):
                    if exact:
                        ids, dist = _expected_masked(own[i], allowed, radii[i], rowids)
                        cut = len(ids) if limit is None else limit
                        _assert_same(one[i], ids[:cut], dist[:cut], matches=len(ids), ctx=("corpus", name, metric, i, limit))
                    _assert_same(many[i], one[i][0], one[i][1].astype(np.float32), matches=one[i][2], ctx=("shards", n_shards, name, metric, i, limit))
    sh.close()
    c.close()


# ------------------------------------------------------------------------------------------------- contract

def test_contract(pkg):
    L = pkg.lib()
    dim = 16
    c = pkg.Corpus(dg.U8, dim)
    qs = _queries(dg.U8, 3, dim, 11)
    rows = dg.corpus(dg.U8, N, dim, 12)
    c.append(rows)
    good = np.array([1.0, 5.0, 2.0])
    bad = np.array([1.0, float("nan"), 2.0])

    def raw(h, metric, queries, nq, radii):
        m, held = np.full(3, 7, dtype=np.int64), np.full(3, 7, dtype=np.int64)
        rc = L.vg_scan_within_batch_masked(h, metric, queries, nq, radii, 0, pkg._ptr(m), pkg._ptr(held))
        return rc, m.tolist(), held.tolist()

    zero = [0, 0, 0]
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(good)) == (VG_ERR_INVALID, zero, zero)          # no mask
    allowed = np.arange(N) % 3 == 0
    c.set_mask(bits=allowed)
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(bad)) == (VG_ERR_INVALID, zero, zero)
    assert c.within_batch_last_launches() == 0                                                      # refused before any launch
    assert raw(c.h, 99, pkg._ptr(qs), 3, pkg._ptr(good)) == (VG_ERR_INVALID, zero, zero)
    assert raw(c.h, dg.L2, None, 3, pkg._ptr(good)) == (VG_ERR_INVALID, zero, zero)
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, None) == (VG_ERR_INVALID, zero, zero)
    assert raw(None, dg.L2, pkg._ptr(qs), 3, pkg._ptr(good)) == (VG_ERR_INVALID, zero, zero)
    assert raw(c.h, dg.L2, pkg._ptr(qs), 0, pkg._ptr(good))[0] == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_within_batch_masked(dg.L2, qs[:0], [])) == VG_ERR_INVALID

    own = [c.scan_distances(dg.L2, qs[i]) for i in range(3)]
    radii = [float(np.sort(own[i][allowed])[10 * (i + 1)]) for i in range(3)]
    exp = [_expected_masked(own[i], allowed, radii[i]) for i in range(3)]
    res = c.scan_within_batch_masked(dg.L2, qs, radii)
    for i in range(3):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=i)
    same = c.scan_within_batch_masked(dg.L2, qs, radii[1])          # a scalar radius is broadcast
    for i in range(3):
        ids, dist = _expected_masked(own[i], allowed, radii[1])
        _assert_same(same[i], ids, dist, ctx=("scalar", i))
    res = c.scan_within_batch_masked(dg.L2, qs, radii)
    n0 = len(exp[0][0])
    keys = c.within_batch_keys(0, n0)
    assert ((keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == exp[0][0].tolist()
    assert _error_code(pkg, lambda: c.within_batch_keys(0, n0 + 1)) == VG_ERR_INVALID
    # the single form's held result and the batch form's stay apart, masked or not
    single = c.scan_within_masked(dg.L2, qs[2], radii[2])
    _assert_same(single, exp[2][0], exp[2][1])
    assert c.within_batch_keys(0, n0).tolist() == keys.tolist()
    skeys = c.within_keys(len(single[0]))
    c.scan_within_batch_masked(dg.L2, qs, radii[0])
    assert c.within_keys(len(single[0])).tolist() == skeys.tolist()
    # the unmasked batch overwrites the masked batch's held result, and still does not read the mask
    un = c.scan_within_batch(dg.L2, qs, radii)
    for i in range(3):
        ids, dist = _expected(own[i], radii[i])
        _assert_same(un[i], ids, dist, ctx=("unmasked", i))
    assert len(c.within_batch_keys(0, len(un[0][0]))) == len(un[0][0]) > n0
    # an empty mask: every count 0, no launch
    c.set_mask(positions=[])
    res = c.scan_within_batch_masked(dg.L2, qs, 1e9)
    assert [(len(r[0]), r[2]) for r in res] == [(0, 0)] * 3 and c.within_batch_last_launches() == 0
    c.close()
    # an empty corpus with a mask: every count 0, no launch
    c = pkg.Corpus(dg.U8, dim)
    c.set_mask(bits=np.zeros(0, dtype=bool))
    res = c.scan_within_batch_masked(dg.L2, qs, 1e9)
    assert [(len(r[0]), r[2]) for r in res] == [(0, 0)] * 3 and c.within_batch_last_launches() == 0
    c.close()
