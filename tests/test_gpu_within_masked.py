"""Masked range scans (vg_scan_within_masked): every ALLOWED row within a distance of the query, through the binding.

Contract (include/vectorgpu.h): the conjunction of scan_within's and scan_topk_masked's - a row matches when its bit is set in the
handle's row mask and its distance d (the float scan_distances reports, bit for bit) satisfies (double)d <= radius; NaN / +Inf never;
ascending (distance, scan position) whatever the tie_order; with a limit the first `limit` matches, the count of all still reported.

  * uint8 / int8: rowids, order, distance bits and count equal to the pinned CPU oracle's distances masked, filtered and sorted here,
    radii ON tied distances included, limits below and above the match count;
  * mask shapes per kernel family against the engine's own stream and against scan_within restricted to the allowed rows;
  * NaN / Inf rows, overflow of the device buffer (only ALLOWED matches take room), the mask's lifecycle, the contract's error codes,
    logical shards == one corpus.
"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
from test_gpu_masked import _mask_shapes
from test_gpu_within import DIMS_INT, _assert_same, _expected, _own_radii, _radii_at_ranks

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1


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


def _expected_masked(dist, allowed, radius, rowids=None):
    """_expected (test_gpu_within.py) over the allowed rows only: a row that is not allowed is a row that never matches"""
    d = np.where(np.asarray(allowed, dtype=bool), np.asarray(dist, dtype=np.float32), np.float32(np.nan))
    return _expected(d, radius, rowids)


def _limits(m):
    return [x for x in sorted(set([1, max(1, m // 2), max(1, m - 1), m, m + 1, m + 1000])) if x >= 1]


@pytest.mark.parametrize("vt", [dg.U8, dg.I8])
@pytest.mark.parametrize("dim", DIMS_INT)
def test_int8_bit_exact_vs_oracle(pkg, orc, vt, dim):
    n = 2500
    rng = np.random.default_rng(1900 + dim)
    for low in (False, True):
        rows = dg.corpus(vt, n, dim, 400 + dim, low_entropy=low)
        q = dg.query(vt, dim, 401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
            tied = False
            for density in (0.5, 0.1):
                allowed = rng.random(n) < density
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                # radii at ranks of the ALLOWED rows' distances: on a distance several allowed rows hold, below the minimum, +Inf
                for i, radius in enumerate(_radii_at_ranks(want[allowed])):
                    ids, dist = _expected_masked(want, allowed, radius)
                    tied = tied or (np.isfinite(radius) and int(np.sum(want[allowed] == np.float32(radius))) > 1)
                    ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, density, radius)
                    _assert_same(c.scan_within_masked(metric, q, radius), ids, dist, ctx=ctx)
                    if i in (1, 3):
                        for limit in _limits(len(ids)):            # below, at and above the match count
                            _assert_same(c.scan_within_masked(metric, q, radius, limit=limit), ids[:limit], dist[:limit], matches=len(ids),
                                         ctx=(ctx, "limit", limit))
            if low and dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
                assert tied, "the low-entropy case is there for radii on a distance several allowed rows hold"
        c.close()


# one shape per kernel family (test_gpu_masked.test_mask_shapes): f32 x 384 (double-buffered), f32 x 4 (a batch is a whole mask word),
# uint8 x 64 / x 256 (the ring forms), int8 x 768, f16 x 384 (cached-norm cosine), f32 x 4100 (the long-row kernel)
@pytest.mark.parametrize("vt,dim,sizes", [(dg.F32, 384, (37, 70001)), (dg.F32, 4, (37, 70001)), (dg.U8, 64, (37, 70001)), (dg.U8, 256, (37, 70001)),
                                          (dg.I8, 768, (37, 30001)), (dg.F16, 384, (37, 30001)), (dg.F32, 4100, (37, 5003))])
def test_mask_shapes(pkg, vt, dim, sizes):
    for n in sizes:
        rows = dg.corpus(vt, n, dim, 610 + dim, low_entropy=(vt in (dg.U8, dg.I8)))
        q = dg.query(vt, dim, 611 + dim, low_entropy=(vt in (dg.U8, dg.I8)))
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in (dg.L2, dg.COSINE, dg.DOT):
            own = c.scan_distances(metric, q)
            radii = _own_radii(own)
            unmasked = {r: c.scan_within(metric, q, r) for r in radii}
            stream = {r: _expected(own, r) for r in radii}          # the engine's own stream within r, sorted here (once per radius)
            for name, allowed in _mask_shapes(n).items():
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                for radius in radii:
                    ctx = (dg.TYPE_NAMES[vt], dim, n, dg.METRIC_NAMES[metric], name, radius)
                    ids, dist = stream[radius]
                    ids, dist = ids[allowed[ids - 1]], dist[allowed[ids - 1]]
                    got = c.scan_within_masked(metric, q, radius)
                    _assert_same(got, ids, dist, ctx=ctx)           # ... and restricted to the allowed rows
                    ui, ud, _ = unmasked[radius]                    # scan_within with the same radius, restricted to the allowed rows
                    keep = allowed[ui - 1]
                    _assert_same(got, ui[keep], ud[keep].astype(np.float32), ctx=ctx)
                    if name == "empty":
                        assert got[2] == 0 and c.within_last_launches() == 0, ctx
                    elif name == "all":
                        assert c.within_last_launches() >= 1, ctx
        c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
def test_nan_inf_rows_never_match(pkg, orc, vt):
    dim = 35
    q, rows = dg.edge_rows(vt, dim, 90)
    n = len(rows)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    special = False
    rng = np.random.default_rng(17)
    for metric in dg.ALL_METRICS:
        own = c.scan_distances(metric, q)
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        assert np.array_equal(np.isnan(own), np.isnan(want)) and np.array_equal(np.isposinf(own), np.isposinf(want)), metric
        bad = np.isnan(own) | np.isposinf(own)
        special = special or bool(bad.any())
        for allowed in (np.ones(n, dtype=bool), bad | (rng.random(n) < 0.5)):          # every NaN / Inf row is allowed
            c.set_mask(bits=allowed)
            for radius in (float("inf"), 1e300, float(np.finfo(np.float32).max)):
                ids, dist, matches = c.scan_within_masked(metric, q, radius)
                eids, edist = _expected_masked(own, allowed, radius)
                _assert_same((ids, dist, matches), eids, edist, ctx=(dg.TYPE_NAMES[vt], metric, radius))
                assert not bad[ids - 1].any()
            # +inf: exactly the allowed rows with a finite distance (-Inf, a dot product's, is a distance)
            ids, dist, matches = c.scan_within_masked(metric, q, float("inf"))
            assert sorted(ids.tolist()) == (np.nonzero(allowed & (own < np.inf))[0] + 1).tolist() and matches == len(ids)
    assert special, "the edge rows are there for their NaN / Inf distances"
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.F32, 384), (dg.U8, 100), (dg.F16, 4100)])
def test_overflow_counts_allowed_matches_only(pkg, vt, dim):
    n = 20011
    rows = dg.corpus(vt, n, dim, 700 + dim)
    q = dg.query(vt, dim, 701)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    allowed = np.random.default_rng(3).random(n) < 0.1
    c.set_mask(bits=allowed)
    sa = np.sort(own[allowed])
    c.set_within_initial_capacity(64)
    try:
        # m allowed matches; the radius of m = 60 matches some 600 rows overall, which an unmasked scan filtered on the host would have to hold
        for m, launches in ((60, 1), (64, 1), (65, 2), (700, 2), (len(sa), 2)):
            radius = float("inf") if m == len(sa) else 0.5 * (float(sa[m - 1]) + float(sa[m]))
            ids, dist = _expected_masked(own, allowed, radius)
            assert len(ids) == m
            if m == 60:
                assert int(np.sum(own <= radius)) > 64
            _assert_same(c.scan_within_masked(dg.L2, q, radius), ids, dist, ctx=(m,))
            assert c.within_last_launches() == launches, (m, c.within_last_launches())
            _assert_same(c.scan_within_masked(dg.L2, q, radius, limit=17), ids[:17], dist[:17], matches=m, ctx=(m, "limit"))
    finally:
        c.set_within_initial_capacity(0)
    c.close()


def test_lifecycle(pkg):
    n, dim = 4001, 100
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32)
    allowed = np.random.default_rng(6).random(n) < 0.2
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    r = float(np.sort(own)[400])
    assert _error_code(pkg, lambda: c.scan_within_masked(dg.L2, q, r)) == VG_ERR_INVALID           # no mask
    c.set_mask(bits=allowed)
    ids, dist = _expected_masked(own, allowed, r)
    assert 0 < len(ids) < 400
    _assert_same(c.scan_within_masked(dg.L2, q, r), ids, dist)
    # scan_within behind scan_within_masked ignores the mask, and overwrites the held result (and the reverse)
    uids, udist = _expected(own, r)
    _assert_same(c.scan_within(dg.L2, q, r), uids, udist)
    assert ((c.within_keys(len(uids)) & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == uids.tolist()
    _assert_same(c.scan_within_masked(dg.L2, q, r), ids, dist)
    assert ((c.within_keys(len(ids)) & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == ids.tolist()
    assert _error_code(pkg, lambda: c.within_keys(len(ids) + 1)) == VG_ERR_INVALID
    # clone carries the mask
    d = c.clone()
    _assert_same(d.scan_within_masked(dg.L2, q, r), ids, dist)
    d.close()
    # patch_rows keeps the mask; the patched row's new distance decides
    best = int(ids[0] - 1)
    c.patch_rows(np.array([best], dtype=np.int64), np.full((1, dim), 1000.0, dtype=np.float32))
    assert c.mask_count() == int(allowed.sum())
    own2 = c.scan_distances(dg.L2, q)
    ids2, dist2 = _expected_masked(own2, allowed, r)
    assert best + 1 not in ids2.tolist() and len(ids2) == len(ids) - 1
    _assert_same(c.scan_within_masked(dg.L2, q, r), ids2, dist2)
    outside = int(np.nonzero(allowed & (own2 > r))[0][0])                                        # an allowed row moves INTO the radius
    c.patch_rows(np.array([outside], dtype=np.int64), q.reshape(1, dim).astype(np.float32))
    own3 = c.scan_distances(dg.L2, q)
    ids3, dist3 = _expected_masked(own3, allowed, r)
    assert ids3[0] == outside + 1
    _assert_same(c.scan_within_masked(dg.L2, q, r), ids3, dist3)
    # append drops the mask
    c.append(rows[:3])
    assert c.mask_count() == -1
    assert _error_code(pkg, lambda: c.scan_within_masked(dg.L2, q, r)) == VG_ERR_INVALID
    c.close()


def test_tie_order_setting_does_not_change_the_answer(pkg):
    n, dim = 3000, 64
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    q = dg.query(dg.U8, dim, 72, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    allowed = np.random.default_rng(5).random(n) < 0.3
    r = float(np.sort(own[allowed])[200])
    ids, dist = _expected_masked(own, allowed, r)
    for mode in (pkg.TIE_REFERENCE, pkg.TIE_POSITION):
        c.set_tie_order(mode)
        c.set_mask(bits=allowed)
        _assert_same(c.scan_within_masked(dg.L2, q, r), ids, dist, ctx=mode)
    c.close()


def test_contract(pkg):
    L = pkg.lib()
    c = pkg.Corpus(pkg.F32, 8)
    q = np.zeros(8, dtype=np.float32)

    def raw(h, metric, query, radius):
        m, held = C.c_int64(7), C.c_int64(7)
        rc = L.vg_scan_within_masked(h, metric, query, radius, 0, C.byref(m), C.byref(held))
        return rc, m.value, held.value

    assert raw(c.h, dg.L2, pkg._ptr(q), 1.0) == (VG_ERR_INVALID, 0, 0)                # no mask (an empty corpus too)
    c.set_mask(bits=np.zeros(0, dtype=bool))
    assert raw(c.h, dg.L2, pkg._ptr(q), 1.0) == (0, 0, 0)                             # an empty corpus: nothing, no launch
    assert c.within_last_launches() == 0
    c.append(np.ones((5, 8), dtype=np.float32))
    assert raw(c.h, dg.L2, pkg._ptr(q), 100.0) == (VG_ERR_INVALID, 0, 0)              # the append dropped the mask
    assert c.set_mask(positions=[1, 3]) == 2
    assert raw(c.h, dg.L2, pkg._ptr(q), float("nan")) == (VG_ERR_INVALID, 0, 0)
    assert c.within_last_launches() == 0                                              # refused before any launch
    assert raw(c.h, 99, pkg._ptr(q), 100.0) == (VG_ERR_INVALID, 0, 0)
    assert raw(c.h, dg.L2, None, 100.0) == (VG_ERR_INVALID, 0, 0)
    assert raw(None, dg.L2, pkg._ptr(q), 100.0) == (VG_ERR_INVALID, 0, 0)
    assert raw(c.h, dg.L2, pkg._ptr(q), 100.0) == (0, 2, 2)
    ids, dist, m = c.scan_within_masked(dg.L2, q, 100.0)
    assert ids.tolist() == [2, 4] and m == 2
    ids, dist, m = c.scan_within_masked(dg.L2, q, 100.0, limit=1)
    assert ids.tolist() == [2] and m == 2
    assert c.set_mask(positions=[]) == 0
    assert raw(c.h, dg.L2, pkg._ptr(q), 100.0) == (0, 0, 0) and c.within_last_launches() == 0      # an empty mask: no launch
    c.close()


@pytest.mark.parametrize("n_shards", [1, 3, 8])
@pytest.mark.parametrize("vt,dim", [(dg.U8, 100), (dg.F32, 384)])
def test_shards_equal_one_corpus(pkg, n_shards, vt, dim):
    """logical shards on one device, a block size of 40 rows (a mask word spans block borders); low-entropy uint8: ties across shard
    borders merge by global position"""
    n = 5003
    rows = dg.corpus(vt, n, dim, 81, low_entropy=(vt == dg.U8))
    q = dg.query(vt, dim, 82, low_entropy=(vt == dg.U8))
    rowids = np.arange(n, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    assert _error_code(pkg, lambda: sh.scan_within_masked(dg.L2, q, 1.0)) == VG_ERR_INVALID
    rng = np.random.default_rng(9)
    masks = {"half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.02, "all": np.ones(n, dtype=bool), "empty": np.zeros(n, dtype=bool)}
    m = np.zeros(n, dtype=bool); m[35:47] = True; m[n - 3:] = True; masks["runs_over_block_borders"] = m
    one = np.zeros(n, dtype=bool)                                  # every set bit in blocks of ONE shard (block b -> shard b % S)
    for b in range(1 % n_shards, n // 40, n_shards):
        one[b * 40:b * 40 + 40:3] = True
    masks["one_shard_only"] = one
    sh.set_within_initial_capacity(200)
    tied = False
    for name, allowed in masks.items():
        assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed) == int(allowed.sum())
        for metric in (dg.L2, dg.DOT, dg.L1):
            own = c.scan_distances(metric, q)
            s = np.sort(own[allowed]) if allowed.any() else np.sort(own)
            for radius in (float(s[0]), float(s[min(40, len(s) - 1)]), float(s[len(s) // 2]), float("inf"), float(s[0]) - 1.0):
                ids, dist = _expected_masked(own, allowed, radius, rowids)
                tied = tied or len(set(dist.tolist())) < len(dist)
                _assert_same(c.scan_within_masked(metric, q, radius), ids, dist, ctx=("corpus", name, metric, radius))
                _assert_same(sh.scan_within_masked(metric, q, radius), ids, dist, ctx=("shards", n_shards, name, metric, radius))
                if name == "empty":
                    assert sh.within_last_launches() == 0
                for limit in (1, 33, len(ids) + 5):
                    _assert_same(sh.scan_within_masked(metric, q, radius, limit=limit), ids[:limit], dist[:limit], matches=len(ids),
                                 ctx=("shards", n_shards, name, limit))
    if vt == dg.U8:
        assert tied, "the low-entropy rows are there for equal distances in several shards"
    # the unmasked form on the same handle still ignores the mask
    own = c.scan_distances(dg.L2, q)
    r = float(np.sort(own)[100])
    ids, dist = _expected(own, r, rowids)
    _assert_same(sh.scan_within(dg.L2, q, r), ids, dist)
    sh.clear_mask()
    assert _error_code(pkg, lambda: sh.scan_within_masked(dg.L2, q, r)) == VG_ERR_INVALID
    sh.close()
    c.close()
