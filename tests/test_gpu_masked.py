"""Masked scans (vg_scan_topk_masked): the k nearest rows among an allowed set, through the binding.

Contract (include/vectorgpu.h): a row mask is a bitmap over scan positions on the handle, read by scan_topk_masked only.  The result is
the top-k contract restricted to the allowed rows: ascending (distance, scan position) whatever the tie_order, NaN / +Inf never enter,
fewer than k rows when fewer allowed rows qualify, every distance the float scan_distances reports for that row.

  * uint8 / int8: rowids, order and distance bits equal to the pinned CPU oracle's distances masked and sorted here, ties at the k-th
    place included;
  * mask shapes per kernel family (double-buffered, ring, long rows): full, half, sparse, strided, single rows, runs inside a batch and
    a word, the last partial batch, fewer rows than k, empty;
  * f32 / f16 / bf16: equal to the engine's own scan_distances masked and sorted here, bit for bit, and within the oracle's tolerance
    rank by rank and row by row;
  * NaN / Inf rows, the lifecycle of the mask, logical shards == one corpus, 10M x 384 f32 once.
"""
import numpy as np
import pytest

import datagen as dg
from test_gpu_within import DIMS_F32, DIMS_INT, _float_tolerance

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


def _expected(dist, allowed, k, rowids=None):
    """rowids and distances of the k first allowed rows with a finite distance (NaN / +Inf never) in (distance, position) order"""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pos = np.nonzero(np.asarray(allowed, dtype=bool) & (d < np.inf))[0]
    pos = pos[np.lexsort((pos, d[pos]))][:k]
    ids = pos + 1 if rowids is None else np.asarray(rowids)[pos]
    return ids, d[pos]


def _assert_same(got, ids, dist, ctx=None):
    gi, gd = got
    assert gi.tolist() == ids.tolist(), ctx
    assert np.array_equal(gd.astype(np.float32).view(np.uint32), np.asarray(dist, dtype=np.float32).view(np.uint32)), ctx
    assert np.array_equal(gd, np.asarray(dist, dtype=np.float32).astype(np.float64)), ctx


def _error_code(pkg, fn):
    with pytest.raises(pkg.VectorGpuError) as ei:
        fn()
    return int(str(ei.value).split("error ")[1].split(":")[0])


def _mask_with_tie_at(want, k, rng):
    """a mask under which the k-th place falls INSIDE a group of rows holding one distance: k - 1 rows below a tied value, every row
    holding it, some of the rows above; None when no distance with k - 1 rows below it is held twice"""
    vals, counts = np.unique(want[np.isfinite(want)], return_counts=True)
    for v in vals[counts > 1]:
        below = np.nonzero(want < v)[0]
        if len(below) >= k - 1:
            allowed = (want > v) & (rng.random(len(want)) < 0.3)
            allowed[rng.choice(below, size=k - 1, replace=False)] = True
            allowed[want == v] = True
            return allowed
    return None


@pytest.mark.parametrize("vt", [dg.U8, dg.I8])
@pytest.mark.parametrize("dim", DIMS_INT)
def test_int8_bit_exact_vs_oracle(pkg, orc, vt, dim):
    n = 2500
    rng = np.random.default_rng(900 + dim)
    for low in (False, True):
        rows = dg.corpus(vt, n, dim, 400 + dim, low_entropy=low)
        q = dg.query(vt, dim, 401 + dim, low_entropy=low)
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in dg.ALL_METRICS:
            want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
            tie_mask = _mask_with_tie_at(want, 20, rng)
            if low and dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
                assert tie_mask is not None, "the low-entropy case is there for ties at the k-th place"
            for allowed in (rng.random(n) < 0.5, rng.random(n) < 0.1, tie_mask):
                if allowed is None:
                    continue
                assert c.set_mask(bits=allowed) == int(allowed.sum()) == c.mask_count()
                for k in (1, 20, 64):
                    ids, dist = _expected(want, allowed, k)
                    _assert_same(c.scan_topk_masked(metric, q, k), ids, dist, ctx=(dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, low, k))
                    if allowed is tie_mask and k == 20:       # the cut at the 20th place falls inside a group of rows holding one distance
                        assert len(ids) == 20 and int(np.sum(want[allowed] == dist[-1])) > 1 and int(np.sum(want[allowed] < dist[-1])) == 19
        c.close()


def _mask_shapes(n, rpb_hint=64):
    rng = np.random.default_rng(n)
    shapes = {}
    shapes["all"] = np.ones(n, dtype=bool)
    shapes["half"] = rng.random(n) < 0.5
    shapes["sparse"] = rng.random(n) < 1.0 / 64
    m = np.zeros(n, dtype=bool); m[::64] = True; shapes["every64th"] = m
    for name, p in (("first", 0), ("last", n - 1)):
        m = np.zeros(n, dtype=bool); m[p] = True; shapes[name] = m
    m = np.zeros(n, dtype=bool); m[min(n - 1, 67):min(n, 67 + 23)] = True; shapes["run_in_word"] = m       # starts and ends inside a word and a batch
    m = np.zeros(n, dtype=bool); m[min(n - 1, 5):min(n, 131)] = True; shapes["run_over_words"] = m
    m = np.zeros(n, dtype=bool); m[(n - 1) // rpb_hint * rpb_hint:] = True; shapes["last_partial_batch"] = m
    m = np.zeros(n, dtype=bool); m[rng.choice(n, size=min(n, 7), replace=False)] = True; shapes["fewer_than_k"] = m
    shapes["empty"] = np.zeros(n, dtype=bool)
    return shapes


# one shape per kernel family: f32 x 384 (double-buffered, 2 rows per batch), f32 x 4 (64 rows per batch: a batch is a whole word),
# uint8 x 64 / x 256 (the ring forms, 6 and 4 buffers), int8 x 768, f16 x 384 (cached-norm cosine), f32 x 4100 (the long-row kernel)
@pytest.mark.parametrize("vt,dim,sizes", [(dg.F32, 384, (37, 70001)), (dg.F32, 4, (37, 70001)), (dg.U8, 64, (37, 70001)), (dg.U8, 256, (37, 70001)),
                                          (dg.I8, 768, (37, 30001)), (dg.F16, 384, (37, 30001)), (dg.F32, 4100, (37, 5003))])
def test_mask_shapes(pkg, vt, dim, sizes):
    for n in sizes:
        assert n % 64 and n % 2
        rows = dg.corpus(vt, n, dim, 610 + dim, low_entropy=(vt in (dg.U8, dg.I8)))
        q = dg.query(vt, dim, 611 + dim, low_entropy=(vt in (dg.U8, dg.I8)))
        c = pkg.Corpus(vt, dim)
        c.append(rows)
        for metric in (dg.L2, dg.COSINE, dg.DOT):
            own = c.scan_distances(metric, q)
            for name, allowed in _mask_shapes(n).items():
                assert c.set_mask(bits=allowed) == int(allowed.sum())
                for k in (1, 20):
                    ids, dist = _expected(own, allowed, k)
                    got = c.scan_topk_masked(metric, q, k)
                    _assert_same(got, ids, dist, ctx=(dg.TYPE_NAMES[vt], dim, n, dg.METRIC_NAMES[metric], name, k))
                    if name == "empty":
                        assert len(got[0]) == 0
                    if name == "fewer_than_k" and k == 20:
                        assert len(got[0]) == min(n, 7)
            # the other ways to say the same mask
            allowed = _mask_shapes(n)["sparse"]
            ids, dist = _expected(own, allowed, 20)
            assert c.set_mask(positions=np.nonzero(allowed)[0]) == int(allowed.sum())
            _assert_same(c.scan_topk_masked(metric, q, 20), ids, dist, ctx="positions")
            words = np.zeros((n + 63) // 64, dtype=np.uint64)
            words.view(np.uint8)[:(n + 7) // 8] = np.packbits(allowed, bitorder="little")
            assert c.set_mask(bits=words) == int(allowed.sum())
            _assert_same(c.scan_topk_masked(metric, q, 20), ids, dist, ctx="words")
        c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
@pytest.mark.parametrize("dim", DIMS_F32)
def test_floats_own_stream_and_oracle(pkg, orc, vt, dim):
    n = 2531
    rows = dg.corpus(vt, n, dim, 500 + dim)
    q = dg.query(vt, dim, 501 + dim)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    rng = np.random.default_rng(77 + dim)
    for density in (0.5, 0.05):
        allowed = rng.random(n) < density
        assert c.set_mask(bits=allowed) == int(allowed.sum())
        for metric in dg.ALL_METRICS:
            own = c.scan_distances(metric, q)
            want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
            assert np.isfinite(want).all()
            tol = _float_tolerance(want, vt, metric, q, rows)
            apos = np.nonzero(allowed)[0]
            by_rank = apos[np.lexsort((apos, want[apos]))]                     # allowed rows by oracle distance
            for k in (1, 20, 64):
                ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim, density, k)
                ids, dist = _expected(own, allowed, k, rowids)
                gi, gd = c.scan_topk_masked(metric, q, k)
                _assert_same((gi, gd), ids, dist, ctx=ctx)                     # the same arithmetic as the stream, bit for bit
                assert len(gi) == min(k, len(apos)), ctx
                pos = (gi - 11) // 3
                assert allowed[pos].all(), ctx                                 # every returned row is allowed
                for i in range(len(gi)):                                       # rank by rank against the oracle
                    r = by_rank[i]
                    assert abs(gd[i] - float(want[r])) <= tol[r], (ctx, i, gd[i], float(want[r]), tol[r])
                assert np.all(np.abs(gd - want[pos].astype(np.float64)) <= tol[pos]), ctx      # and each row's own oracle distance
    c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
def test_nan_inf_rows_never_come_back(pkg, orc, vt):
    dim = 35
    q, rows = dg.edge_rows(vt, dim, 90)
    n = len(rows)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    c.set_tie_order(pkg.TIE_POSITION)
    special = False
    for metric in dg.ALL_METRICS:
        own = c.scan_distances(metric, q)
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        assert np.array_equal(np.isnan(own), np.isnan(want)) and np.array_equal(np.isposinf(own), np.isposinf(want)), metric
        special = special or bool(np.isnan(own).any() or np.isposinf(own).any())
        assert c.set_mask(bits=np.ones(n, dtype=bool)) == n                   # every row allowed, the NaN / Inf ones too
        for k in (1, 20, 64):
            ids, dist = _expected(own, np.ones(n, dtype=bool), k)
            gi, gd = c.scan_topk_masked(metric, q, k)
            _assert_same((gi, gd), ids, dist, ctx=(dg.TYPE_NAMES[vt], metric, k))
            assert np.all(gd < np.inf) and len(gi) == min(k, int(np.sum(own < np.inf)))
            ti, td = c.scan_topk(metric, q, k)                                 # an all-ones mask == the plain top-k in position order
            assert gi.tolist() == ti.tolist() and np.array_equal(gd, td), (metric, k)
    assert special, "the edge rows are there for their NaN / Inf distances"
    c.close()


def test_tie_order_setting_does_not_change_the_answer(pkg):
    n, dim = 3000, 64
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    q = dg.query(dg.U8, dim, 72, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    allowed = np.random.default_rng(5).random(n) < 0.3
    ids, dist = _expected(own, allowed, 20)
    for mode in (pkg.TIE_REFERENCE, pkg.TIE_POSITION):
        c.set_tie_order(mode)
        c.set_mask(bits=allowed)
        _assert_same(c.scan_topk_masked(dg.L2, q, 20), ids, dist, ctx=mode)
    c.close()


def test_lifecycle(pkg):
    n, dim = 4001, 100
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32)
    qs = np.stack([dg.query(dg.F32, dim, 33 + i) for i in range(4)])
    allowed = np.random.default_rng(6).random(n) < 0.2
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows)
    assert c.mask_count() == -1
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 5)) == VG_ERR_INVALID          # no mask
    # the other scans do not see the mask
    before = (c.scan_topk(dg.L2, q, 20), c.scan_within(dg.L2, q, float(np.sort(c.scan_distances(dg.L2, q))[50])), c.scan_distances(dg.L2, q),
              c.scan_topk_batch(dg.L2, qs, 10))
    c.set_mask(bits=allowed)
    after = (c.scan_topk(dg.L2, q, 20), c.scan_within(dg.L2, q, float(np.sort(c.scan_distances(dg.L2, q))[50])), c.scan_distances(dg.L2, q),
             c.scan_topk_batch(dg.L2, qs, 10))
    for b, a in zip(before, after):
        if isinstance(b, tuple):
            for x, y in zip(b, a):
                assert np.array_equal(np.asarray(x), np.asarray(y))
        else:
            assert np.array_equal(b, a)
    assert c.mask_count() == int(allowed.sum())
    own = c.scan_distances(dg.L2, q)
    ids, dist = _expected(own, allowed, 20)
    _assert_same(c.scan_topk_masked(dg.L2, q, 20), ids, dist)
    # k outside 1..64
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 65)) == VG_ERR_UNSUPPORTED
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 0)) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, -3)) == VG_ERR_INVALID
    # clone keeps the mask
    d = c.clone()
    assert d.mask_count() == int(allowed.sum())
    _assert_same(d.scan_topk_masked(dg.L2, q, 20), ids, dist)
    d.close()
    # patch_rows keeps it, the next masked scan answers from the new bytes
    best = int(ids[0] - 1)
    far = np.full((1, dim), 1000.0, dtype=np.float32)
    c.patch_rows(np.array([best], dtype=np.int64), far)
    assert c.mask_count() == int(allowed.sum())
    own2 = c.scan_distances(dg.L2, q)
    ids2, dist2 = _expected(own2, allowed, 20)
    assert ids2[0] != ids[0]
    _assert_same(c.scan_topk_masked(dg.L2, q, 20), ids2, dist2)
    # reserve / trim keep it
    pkg._check(pkg.lib().vg_corpus_reserve(c.h, 3 * n))
    pkg._check(pkg.lib().vg_corpus_trim(c.h))
    _assert_same(c.scan_topk_masked(dg.L2, q, 20), ids2, dist2)
    # append, delete_rows and clear each drop it
    c.append(rows[:3])
    assert c.mask_count() == -1
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 5)) == VG_ERR_INVALID
    c.set_mask(bits=np.ones(c.rows, dtype=bool))
    c.delete_rows(np.array([1, 7], dtype=np.int64))
    assert c.mask_count() == -1
    assert _error_code(pkg, lambda: c.scan_topk_masked(dg.L2, q, 5)) == VG_ERR_INVALID
    c.set_mask(bits=np.ones(c.rows, dtype=bool))
    c.clear_mask()
    assert c.mask_count() == -1
    c.set_mask(bits=np.ones(c.rows, dtype=bool))
    c.clear()
    assert c.mask_count() == -1
    # more bits than rows
    c.append(rows[:10])
    with pytest.raises(pkg.VectorGpuError):
        c.set_mask(bits=np.ones(11, dtype=bool))
    # fewer bits than rows: the missing ones are 0
    assert c.set_mask(bits=np.ones(4, dtype=bool)) == 4
    gi, _ = c.scan_topk_masked(dg.L2, q, 64)
    assert sorted(gi.tolist()) == [1, 2, 3, 4]
    c.close()


def test_mask_by_rowids(pkg):
    n, dim = 3001, 64
    rows = dg.corpus(dg.U8, n, dim, 41, low_entropy=True)
    q = dg.query(dg.U8, dim, 42, low_entropy=True)
    rng = np.random.default_rng(8)
    allowed = rng.random(n) < 0.1
    # explicit, ascending, non-contiguous rowids; rowids not held are ignored, duplicates are harmless
    rowids = np.arange(n, dtype=np.int64) * 5 + 100
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, rowids)
    own = c.scan_distances(dg.L1, q)
    ask = np.concatenate([rowids[allowed], rowids[allowed][:50], np.array([0, 101, 99, 5 * n + 100, -7], dtype=np.int64)])
    rng.shuffle(ask)
    assert c.set_mask(rowids=ask) == int(allowed.sum()) == c.mask_count()
    ids, dist = _expected(own, allowed, 64, rowids)
    _assert_same(c.scan_topk_masked(dg.L1, q, 64), ids, dist)
    assert c.set_mask(rowids=np.zeros(0, dtype=np.int64)) == 0
    assert len(c.scan_topk_masked(dg.L1, q, 5)[0]) == 0
    c.close()
    # implicit rowids with a base
    c = pkg.Corpus(dg.U8, dim)
    c.set_rowid_base(1000)
    c.append(rows)
    ask = np.concatenate([np.nonzero(allowed)[0] + 1000, np.array([999, 1000 + n, 3], dtype=np.int64)])
    assert c.set_mask(rowids=ask) == int(allowed.sum())
    ids, dist = _expected(own, allowed, 20, np.arange(n, dtype=np.int64) + 1000)
    _assert_same(c.scan_topk_masked(dg.L1, q, 20), ids, dist)
    c.close()
    # several shards, an empty rowid list: ascending maps give an empty mask, a map that is not ascending is refused all the same
    sh = pkg.Shards(dg.U8, dim, [0, 0], block_rows=4)
    sh.append(rows[:10], np.arange(10, dtype=np.int64) + 1)
    assert sh.set_mask(rowids=np.zeros(0, dtype=np.int64)) == 0 and sh.mask_count() == 0
    sh.close()
    sh = pkg.Shards(dg.U8, dim, [0, 0], block_rows=4)
    sh.append(rows[:10], np.array([5, 4, 9, 1, 2, 3, 8, 7, 6, 10], dtype=np.int64))
    assert _error_code(pkg, lambda: sh.set_mask(rowids=np.zeros(0, dtype=np.int64))) == VG_ERR_UNSUPPORTED
    assert sh.mask_count() == -1
    sh.close()
    # a map that is not ascending: no lookup
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows[:10], np.array([5, 4, 9, 1, 2, 3, 8, 7, 6, 10], dtype=np.int64))
    assert _error_code(pkg, lambda: c.set_mask(rowids=np.array([4], dtype=np.int64))) == VG_ERR_UNSUPPORTED
    assert c.mask_count() == -1
    assert c.set_mask(positions=[1]) == 1                                      # by position it works
    assert c.scan_topk_masked(dg.L1, q, 3)[0].tolist() == [4]
    c.close()


@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
def test_shards_equal_one_corpus(pkg, n_shards):
    """logical shards on one device, a block size of 40 rows (a mask word spans block borders), low-entropy uint8: ties across shard
    borders merge by global position"""
    n, dim = 5003, 100
    rows = dg.corpus(dg.U8, n, dim, 81, low_entropy=True)
    q = dg.query(dg.U8, dim, 82, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(dg.U8, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    assert sh.mask_count() == -1
    rng = np.random.default_rng(9)
    masks = {"half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.02, "all": np.ones(n, dtype=bool), "empty": np.zeros(n, dtype=bool)}
    m = np.zeros(n, dtype=bool); m[35:47] = True; m[n - 3:] = True; masks["runs_over_block_borders"] = m
    for name, allowed in masks.items():
        for how in ("bits", "rowids"):
            if how == "bits":
                assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed) == int(allowed.sum())
            else:
                assert c.set_mask(rowids=rowids[allowed]) == sh.set_mask(rowids=rowids[allowed]) == int(allowed.sum())
            assert sh.mask_count() == int(allowed.sum())
            for metric in (dg.L2, dg.DOT, dg.L1):
                own = c.scan_distances(metric, q)
                for k in (1, 20, 64):
                    ids, dist = _expected(own, allowed, k, rowids)
                    _assert_same(c.scan_topk_masked(metric, q, k), ids, dist, ctx=("corpus", name, how, metric, k))
                    _assert_same(sh.scan_topk_masked(metric, q, k), ids, dist, ctx=("shards", n_shards, name, how, metric, k))
    sh.clear_mask()
    assert sh.mask_count() == -1
    with pytest.raises(pkg.VectorGpuError):
        sh.scan_topk_masked(dg.L2, q, 5)
    sh.close()
    c.close()


def test_full_size_10m_f32(pkg):
    """10M x 384 f32 L2 (the C2 corpus), every row allowed and one in a hundred: equal to the engine's stream masked here"""
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
    rng = np.random.default_rng(44)
    for density in (1.0, 0.01):
        allowed = np.ones(N, dtype=bool) if density == 1.0 else rng.random(N) < density
        assert c.set_mask(bits=allowed) == int(allowed.sum())
        ids, dist = _expected(own, allowed, 20)
        _assert_same(c.scan_topk_masked(dg.L2, q, 20), ids, dist, ctx=density)
    c.close()
