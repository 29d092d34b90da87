"""Range scans (vg_scan_within): every row within a distance of the query, through the C-ABI.

Contract (include/vectorgpu.h): a row matches when its distance d - the float the plain scan computes - satisfies (double)d <= radius;
NaN and +Inf never match; order is ascending (distance, scan position); with a limit the first `limit` matches are returned and the
number of all matches is still reported.

  * uint8 / int8: set, order, distance bits and count equal to the pinned CPU oracle's, radii ON tied distances included;
  * f32 / f16 / bf16: the product's floats are within 1e-5 relative of the oracle's, so rows whose oracle distance lies within that
    tolerance of the radius may fall on either side - they are left out, every other row must agree, and the share left out is bounded;
  * every type and metric: equal to the engine's own vg_scan_distances filtered on the host, bit for bit (the "same arithmetic" claim);
  * overflow of the device buffer (lowered through the diagnostic hook): complete answer, two launches; one when it fits;
  * logical shards on one device == one corpus;
  * 10M x 384 f32 once.
"""
import numpy as np
import pytest

import datagen as dg

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
DIMS_F32 = (1, 3, 4, 5, 16, 35, 100, 128, 384, 768, 1000, 1024, 1536)
DIMS_INT = (1, 3, 15, 16, 17, 35, 100, 384, 768, 1000, 1536, 2048)


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


def _expected(dist, radius, rowids=None):
    """positions (or rowids) and distances of the rows with dist <= radius (NaN / +Inf never), ordered by (distance, position)"""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m = (d.astype(np.float64) <= radius) & (d < np.inf)
    pos = np.nonzero(m)[0]
    order = np.lexsort((pos, d[pos]))
    pos = pos[order]
    ids = pos + 1 if rowids is None else np.asarray(rowids)[pos]
    return ids, d[pos]


def _assert_same(got, ids, dist, matches=None, ctx=None):
    gi, gd, gm = got
    assert gm == (len(ids) if matches is None else matches), ctx
    assert gi.tolist() == ids.tolist(), ctx
    assert np.array_equal(gd.astype(np.float32).view(np.uint32), np.asarray(dist, dtype=np.float32).view(np.uint32)), ctx
    assert np.array_equal(gd, np.asarray(dist, dtype=np.float32).astype(np.float64)), ctx


def _check_with_limits(c, metric, q, radius, ids, dist, ctx):
    _assert_same(c.scan_within(metric, q, radius), ids, dist, ctx=ctx)
    m = len(ids)
    for limit in sorted(set([1, max(1, m // 2), max(1, m - 1), m, m + 1, m + 1000])):
        if limit < 1:
            continue
        _assert_same(c.scan_within(metric, q, radius, limit=limit), ids[:limit], dist[:limit], matches=m, ctx=(ctx, "limit", limit))


def _radii_at_ranks(dist):
    s = np.sort(dist[np.isfinite(dist)])
    n = len(s)
    ranks = sorted(set([0, min(5, n - 1), n // 100, n // 10, n // 2, n - 1]))
    radii = [float(s[r]) for r in ranks]                       # ON a distance some rows hold (several, with low-entropy data)
    vals, counts = np.unique(s, return_counts=True)
    tied = vals[counts > 1]
    if len(tied):
        radii.insert(1, float(tied[len(tied) // 2]))           # certainly equal to a distance held by several rows
    radii.append(float(np.nextafter(s[0], np.float32(-np.inf))))   # below the minimum: no match
    radii.append(float("inf"))
    return radii


@pytest.mark.parametrize("vt", [dg.U8, dg.I8])
@pytest.mark.parametrize("dim", DIMS_INT)
def test_int8_bit_exact_vs_oracle(pkg, orc, vt, dim):
    n = 2500
    for low in (False, True):
        rows = dg.corpus(vt, n, dim, 400 + dim, low_entropy=low)
        q = dg.query(vt, dim, 401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
            tied = False
            for i, radius in enumerate(_radii_at_ranks(want)):
                ids, dist = _expected(want, radius)
                tied = tied or (np.isfinite(radius) and int(np.sum(want == np.float32(radius))) > 1)
                ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, radius)
                if i in (1, 3):
                    _check_with_limits(c, metric, q, radius, ids, dist, ctx)
                else:
                    _assert_same(c.scan_within(metric, q, radius), ids, dist, ctx=ctx)
            if low and dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
                assert tied, "the low-entropy case is there for radii on a tied distance"
        c.close()


def _float_tolerance(want, vt, metric, q, rows):
    """the tolerance _check_float_distances (test_gpu_scan.py) grants each row's distance"""
    w = want.astype(np.float64)
    tol = REL_TOL * np.abs(w)
    if metric == dg.DOT:
        tol = tol + REL_TOL * np.abs(dg.storage_to_f64(vt, rows) * dg.storage_to_f64(vt, q)).sum(axis=1)
    elif metric == dg.COSINE:
        tol = tol + REL_TOL
    return np.maximum(tol, 8 * np.finfo(np.float32).eps * 1.01)


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
@pytest.mark.parametrize("n,dim", [(2500, 35), (2500, 384), (2500, 1000), (20000, 35), (20000, 384), (20000, 1000)])
def test_floats_vs_oracle_outside_the_tolerance_band(pkg, orc, vt, n, dim):
    rows = dg.corpus(vt, n, dim, 500 + dim)
    q = dg.query(vt, dim, 501 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    for metric in dg.ALL_METRICS:
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        assert np.isfinite(want).all()
        tol = _float_tolerance(want, vt, metric, q, rows)
        s = np.sort(want.astype(np.float64))
        for quant in (0.001, 0.01, 0.1, 0.5):
            j = max(1, int(round(quant * n)))
            radius = 0.5 * (s[j - 1] + s[j])                   # the midpoint of two consecutive oracle distances: j rows match
            inside = want.astype(np.float64) <= radius
            band = np.abs(want.astype(np.float64) - radius) <= tol
            n_match = int(inside.sum())
            assert int(band.sum()) <= max(3, 0.01 * n_match), (dg.TYPE_NAMES[vt], metric, n, dim, quant, int(band.sum()), n_match)
            ids, dist, matches = c.scan_within(metric, q, radius)
            got = np.zeros(n, dtype=bool)
            got[ids - 1] = True
            assert len(ids) == matches and len(set(ids.tolist())) == matches
            assert np.array_equal(got[~band], inside[~band]), (dg.TYPE_NAMES[vt], metric, n, dim, quant, np.nonzero((got != inside) & ~band)[0][:5])
            assert np.all(dist <= radius) and np.all(np.diff(dist) >= 0)
            assert np.all(np.abs(dist - want[ids - 1].astype(np.float64)) <= tol[ids - 1])
    c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
def test_nan_inf_rows_never_match(pkg, orc, vt):
    dim = 35
    q, rows = dg.edge_rows(vt, dim, 90)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    special = False
    for metric in dg.ALL_METRICS:
        own = c.scan_distances(metric, q)
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        assert np.array_equal(np.isnan(own), np.isnan(want)) and np.array_equal(np.isposinf(own), np.isposinf(want)), metric
        special = special or bool(np.isnan(own).any() or np.isposinf(own).any())
        for radius in (float("inf"), 1e300, float(np.finfo(np.float32).max)):
            ids, dist, matches = c.scan_within(metric, q, radius)
            eids, edist = _expected(own, radius)
            _assert_same((ids, dist, matches), eids, edist, ctx=(dg.TYPE_NAMES[vt], metric, radius))
            assert matches == int(np.sum(own < np.inf)) and np.isfinite(dist[dist > -np.inf]).all()
        with pytest.raises(pkg.VectorGpuError):
            c.scan_within(metric, q, float("nan"))
    assert special, "the edge rows are there for their NaN / Inf distances"
    c.close()


def _own_radii(own):
    s = np.sort(own[own < np.inf])
    n = len(s)
    out = [float(s[r]) for r in sorted(set([0, min(7, n - 1), n // 50, n // 3, n - 1]))]
    out.append(0.5 * (float(s[n // 7]) + float(s[n // 7 + 1])) if n > n // 7 + 1 else float(s[0]))
    out.append(float(np.nextafter(s[0], np.float32(-np.inf))))
    f = np.float32(s[n // 5])
    out.append(0.5 * (float(f) + float(np.nextafter(f, np.float32(np.inf)))))   # a double BETWEEN two adjacent floats: only f's side matches
    out.append(float("inf"))
    return out


@pytest.mark.parametrize("vt", dg.ALL_TYPES)
def test_equals_the_engines_own_stream(pkg, vt):
    """scan_within(r) == the rows of scan_distances with d <= r, sorted by (d, position): same rowids, order and distance bits, for every
    type and metric, short and long rows, n not a multiple of 1024, explicit rowids"""
    n = 2531
    for dim in (DIMS_F32 + (4100,)) if vt in (dg.F32, dg.F16, dg.BF16) else (DIMS_INT + (9000,)):       # (the last one: long rows)
        rows = dg.corpus(vt, n, dim, 600 + dim, low_entropy=(dim % 2 == 1))
        q = dg.query(vt, dim, 601 + dim, low_entropy=(dim % 2 == 1))
        rowids = np.arange(n, dtype=np.int64) * 3 + 11
        c = pkg.Corpus(vt, dim)
        c.append(rows, rowids)
        for metric in dg.ALL_METRICS:
            own = c.scan_distances(metric, q)
            for radius in _own_radii(own):
                ids, dist = _expected(own, radius, rowids)
                _assert_same(c.scan_within(metric, q, radius), ids, dist, ctx=(dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, radius))
            r = float(np.sort(own)[n // 10])
            ids, dist = _expected(own, r, rowids)
            _check_with_limits(c, metric, q, r, ids, dist, (dg.TYPE_NAMES[vt], metric, dim, "limits"))
        c.close()


def test_tie_order_setting_does_not_change_the_answer(pkg):
    n, dim = 3000, 64
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    q = dg.query(dg.U8, dim, 72, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    r = float(np.sort(own)[200])
    ids, dist = _expected(own, r)
    for mode in (pkg.TIE_REFERENCE, pkg.TIE_POSITION):
        c.set_tie_order(mode)
        _assert_same(c.scan_within(dg.L2, q, r), ids, dist, ctx=mode)
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 100), (dg.F16, 4100)])
def test_overflow_takes_exactly_one_more_launch(pkg, vt, dim):
    n = 20011
    rows = dg.corpus(vt, n, dim, 700 + dim)
    q = dg.query(vt, dim, 701)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    s = np.sort(own)
    c.set_within_initial_capacity(300)
    try:
        for m, launches in ((40, 1), (300, 1), (301, 2), (3000, 2), (9000, 2), (n, 2)):   # (more than 4096 matches: the device sort)
            radius = float("inf") if m == n else 0.5 * (float(s[m - 1]) + float(s[m]))
            ids, dist = _expected(own, radius)
            assert len(ids) == m
            _assert_same(c.scan_within(dg.L2, q, radius), ids, dist, ctx=(m,))
            assert c.within_last_launches() == launches, (m, c.within_last_launches())
            _assert_same(c.scan_within(dg.L2, q, radius, limit=17), ids[:17], dist[:17], matches=m, ctx=(m, "limit"))
        # once grown the buffer is kept: the same radius fits now
        c.scan_within(dg.L2, q, float("inf"))
        assert c.within_last_launches() == 1
    finally:
        c.set_within_initial_capacity(0)
    ids, dist = _expected(own, float("inf"))
    _assert_same(c.scan_within(dg.L2, q, float("inf")), ids, dist)
    assert c.within_last_launches() == 1
    c.close()


def test_empty_corpus_and_bad_arguments(pkg):
    c = pkg.Corpus(pkg.F32, 8)
    q = np.zeros(8, dtype=np.float32)
    ids, dist, m = c.scan_within(dg.L2, q, 1.0)
    assert len(ids) == 0 and m == 0
    c.append(np.ones((5, 8), dtype=np.float32))
    with pytest.raises(pkg.VectorGpuError):
        c.scan_within(99, q, 1.0)
    ids, dist, m = c.scan_within(dg.L2, q, 100.0)
    assert ids.tolist() == [1, 2, 3, 4, 5] and m == 5
    with pytest.raises(pkg.VectorGpuError):
        pkg._check(pkg.lib().vg_scan_within_fetch(c.h, 3, 3, None, None))
    c.clear()
    with pytest.raises(pkg.VectorGpuError):
        pkg._check(pkg.lib().vg_scan_within_fetch(c.h, 0, 1, None, None))
    c.close()


@pytest.mark.parametrize("n_shards", [1, 3, 8])
def test_shards_equal_one_corpus(pkg, n_shards):
    """logical shards on one device, a small block size, low-entropy uint8: ties across shard borders merge by global position"""
    n, dim = 5003, 100
    rows = dg.corpus(dg.U8, n, dim, 81, low_entropy=True)
    q = dg.query(dg.U8, dim, 82, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(dg.U8, dim, [0] * n_shards, block_rows=64)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    sh.set_within_initial_capacity(200)
    first_inf = True
    for metric in (dg.L2, dg.DOT, dg.L1):
        own = c.scan_distances(metric, q)
        s = np.sort(own)
        for radius in (float(s[0]), float(s[40]), float(s[700]), float(s[n // 2]), float("inf"), float(s[0]) - 1.0):
            ids, dist = _expected(own, radius, rowids)
            _assert_same(c.scan_within(metric, q, radius), ids, dist, ctx=("corpus", metric, radius))
            _assert_same(sh.scan_within(metric, q, radius), ids, dist, ctx=("shards", n_shards, metric, radius))
            if radius == float("inf") and first_inf:           # every shard holds more rows than the lowered capacity (and than it grew to so far)
                assert sh.within_last_launches() == 2
                first_inf = False
            for limit in (1, 33, len(ids), len(ids) + 5):
                if limit >= 1:
                    _assert_same(sh.scan_within(metric, q, radius, limit=limit), ids[:limit], dist[:limit], matches=len(ids), ctx=("shards", n_shards, limit))
    sh.close()
    c.close()


def test_full_size_10m_f32(pkg):
    """10M x 384 f32 L2 (the C2 corpus): radii from the 20th and the 10 000th distance; the set equals the engine's stream filtered here"""
    import torch
    N, dim = 10_000_000, 384
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        t = torch.randn((1_000_000, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), 1_000_000, dim * 4)
        del t
    q = np.random.default_rng(43).standard_normal(dim, dtype=np.float32)
    own = c.scan_distances(dg.L2, q)
    part = np.partition(own, (19, 9999))
    for rank in (19, 9999):
        radius = float(part[rank])
        ids, dist = _expected(own, radius)
        assert len(ids) >= rank + 1
        _assert_same(c.scan_within(dg.L2, q, radius), ids, dist, ctx=rank)
        assert c.within_last_launches() == 1
        _assert_same(c.scan_within(dg.L2, q, radius, limit=20), ids[:20], dist[:20], matches=len(ids), ctx=(rank, "limit"))
    tids, tdist = c.scan_topk(dg.L2, q, 20)
    ids, dist, _ = c.scan_within(dg.L2, q, float(part[19]), limit=20)
    assert ids.tolist() == tids.tolist() and np.array_equal(dist, tdist)
    c.close()
