"""Paged scans (vg_scan_topk_after): the next k rows behind a (distance, rowid) cursor, through the binding.

Contract (include/vectorgpu.h): the row at scan position p with distance d (the float scan_distances reports) is behind the cursor
(D, R) iff d < +Inf and (d > D, or d == D and rowid(p) > R); returned are the first k such rows in ascending (distance, scan position)
order.  Expected results are built here from a distance vector sorted by (d, p):
  * uint8 / int8: the pinned CPU oracle's distances; pages of 1, 20 and 64 walked from the start cursor; rowids, order and bits;
  * explicit cursors: inside a run of equal distances (first / middle / last row), an absent rowid, a midpoint double, below the
    minimum, the last key;
  * f32 / f16 / bf16: the engine's own scan_distances bit for bit, the oracle's tolerance rank by rank; NaN / Inf rows;
  * masked forms over the mask shapes of test_gpu_masked, the equalities with the existing scans, the _keys form, the lifecycle,
    rowids that are not ascending, logical shards == one corpus."""
import numpy as np
import pytest

import datagen as dg
from test_gpu_masked import _assert_same, _error_code, _mask_shapes
from test_gpu_within import DIMS_F32, DIMS_INT, _float_tolerance

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
START = (float("-inf"), -(1 << 63))
LONG_INT, LONG_F32 = 9000, 4100            # one long-row dim per type, as test_gpu_within.py has them
WALK_DIMS = (35, 384)                       # walked to exhaustion; the rest: five pages


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


def _order(dist, allowed=None):
    """scan positions of the rows that can be returned at all, in (distance, position) order"""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = d < np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, dtype=bool)
    pos = np.nonzero(ok)[0]
    return pos[np.lexsort((pos, d[pos]))]


def _behind(dist, order, rowids, after, k):
    """the first k rows of `order` behind the cursor, by the contract's predicate"""
    D, R = after
    d = np.asarray(dist, dtype=np.float32)[order].astype(np.float64)
    r = rowids[order]
    keep = (d > D) | ((d == D) & (r > R))
    pos = order[keep][:k]
    return rowids[pos], np.asarray(dist, dtype=np.float32)[pos]


def _walk(scan, k, max_pages=None):
    """pages from the start cursor, each cursor the last row of the page in front"""
    after, ids, dist, pages = START, [], [], 0
    while max_pages is None or pages < max_pages:
        gi, gd = scan(after, k)
        pages += 1
        ids += gi.tolist()
        dist += gd.tolist()
        if len(gi) < k:
            if len(gi):                                      # a short page is the last one: the page behind it is empty
                assert len(scan((float(gd[-1]), int(gi[-1])), k)[0]) == 0
            break
        after = (float(gd[-1]), int(gi[-1]))
    return np.array(ids, dtype=np.int64), np.array(dist, dtype=np.float64), pages


def _key_distances(keys):
    """the distances packed keys carry: the inverse of the order-preserving float image in their high halves"""
    s = (np.asarray(keys, dtype=np.uint64) >> np.uint64(32)).astype(np.uint32)
    b = np.where(s >> 31, s ^ np.uint32(0x80000000), s ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def _tie_runs(dist, order, least=3):
    """(start, length) in `order` of runs of at least `least` equal distances"""
    d = np.asarray(dist, dtype=np.float32)[order]
    runs, i = [], 0
    while i < len(d):
        j = i
        while j + 1 < len(d) and d[j + 1] == d[i]:
            j += 1
        if j - i + 1 >= least:
            runs.append((i, j - i + 1))
        i = j + 1
    return runs


def _explicit_cursors(dist, order, rowids):
    """name -> cursor, placed deterministically"""
    d = np.asarray(dist, dtype=np.float32)
    cur = {}
    runs = _tie_runs(dist, order)
    if runs:
        s, ln = runs[len(runs) // 2]
        for name, j in (("tie_first", s), ("tie_middle", s + ln // 2), ("tie_last", s + ln - 1)):
            cur[name] = (float(d[order[j]]), int(rowids[order[j]]))
    mid = order[len(order) // 2]
    cur["absent_rowid"] = (float(d[mid]), int(rowids[mid]) + 1)            # rowids here step by 3: + 1 is held by no row
    lo, hi = d[order[len(order) // 3]], None
    for p in order[len(order) // 3:]:
        if d[p] > lo:
            hi = d[p]
            break
    if hi is not None:
        cur["midpoint"] = ((float(lo) + float(hi)) / 2.0, 0)
    cur["below_min"] = (float(np.nextafter(d[order[0]], np.float32(-np.inf))) if np.isfinite(d[order[0]]) else -1e300, 1 << 62)
    cur["last_key"] = (float(d[order[-1]]), int(rowids[order[-1]]))
    cur["start"] = START
    cur["past_everything"] = (float("inf"), 0)
    return cur


def _check_cursors(scan, dist, order, rowids, ks=(1, 20), ctx=None):
    cursors = _explicit_cursors(dist, order, rowids)
    for name, after in cursors.items():
        for k in ks:
            ids, dd = _behind(dist, order, rowids, after, k)
            _assert_same(scan(after, k), ids, dd, ctx=(ctx, name, k))
    ids, _ = _behind(dist, order, rowids, cursors["last_key"], 5)
    assert len(ids) == 0
    return cursors


@pytest.mark.parametrize("vt", [dg.U8, dg.I8])
@pytest.mark.parametrize("dim", DIMS_INT + (LONG_INT,))
def test_int8_pages_vs_oracle(pkg, orc, vt, dim):
    n = 2500
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    rows = dg.corpus(vt, n, dim, 400 + dim, low_entropy=True)
    q = dg.query(vt, dim, 401 + dim, low_entropy=True)
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    for metric in dg.ALL_METRICS:
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        order = _order(want)
        ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim)
        if dim <= 100 and metric in (dg.SQUARED_L2, dg.DOT, dg.L1):
            assert _tie_runs(want, order), "the low-entropy corpus is there for runs of equal distances"
        scan = lambda after, k: c.scan_topk_after(metric, q, k, after=after)
        for k in (1, 20, 64):
            pages = None if dim in WALK_DIMS else 5
            gi, gd, npages = _walk(scan, k, pages)
            m = len(order) if pages is None else min(len(order), 5 * k)
            _assert_same((gi, gd), rowids[order[:m]], want[order[:m]], ctx=(ctx, k))      # no row twice, none missing, in order
            if pages is None:
                assert len(set(gi.tolist())) == len(order) == n and npages == n // k + 1
        _check_cursors(scan, want, order, rowids, ctx=ctx)
    c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
@pytest.mark.parametrize("dim", DIMS_F32 + (LONG_F32,))
def test_floats_own_stream_and_oracle(pkg, orc, vt, dim):
    n = 2531
    rows = dg.corpus(vt, n, dim, 500 + dim)
    q = dg.query(vt, dim, 501 + dim)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    for metric in dg.ALL_METRICS:
        own = c.scan_distances(metric, q)
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        assert np.isfinite(want).all()
        tol = _float_tolerance(want, vt, metric, q, rows)
        order = _order(own)
        by_rank = _order(want)
        ctx = (dg.TYPE_NAMES[vt], dg.METRIC_NAMES[metric], dim)
        scan = lambda after, k: c.scan_topk_after(metric, q, k, after=after)
        for k in (20, 64):
            pages = None if (dim in WALK_DIMS and k == 64) else 5
            gi, gd, _ = _walk(scan, k, pages)
            m = n if pages is None else 5 * k
            _assert_same((gi, gd), rowids[order[:m]], own[order[:m]], ctx=(ctx, k))       # the stream's arithmetic, bit for bit
            for i in range(m):                                                            # rank by rank against the oracle
                r = by_rank[i]
                assert abs(gd[i] - float(want[r])) <= tol[r], (ctx, k, i, gd[i], float(want[r]), tol[r])
        _check_cursors(scan, own, order, rowids, ks=(1, 20), ctx=ctx)
    c.close()


@pytest.mark.parametrize("vt", [dg.F32, dg.F16, dg.BF16])
def test_nan_inf_rows_never_come_back(pkg, orc, vt):
    dim = 35
    q, rows = dg.edge_rows(vt, dim, 90)
    n = len(rows)
    rowids = np.arange(n, dtype=np.int64) + 1
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    special = False
    for metric in dg.ALL_METRICS:
        own = c.scan_distances(metric, q)
        special = special or bool(np.isnan(own).any() or np.isposinf(own).any())
        order = _order(own)
        gi, gd, _ = _walk(lambda after, k: c.scan_topk_after(metric, q, k, after=after), 7)
        _assert_same((gi, gd), rowids[order], own[order], ctx=(dg.TYPE_NAMES[vt], metric))
        assert np.all(gd < np.inf) and not np.isnan(gd).any()
        if np.isneginf(own).any():                                                        # a -Inf row is reachable from the start cursor
            first = c.scan_topk_after(metric, q, 1)
            assert first[1][0] == -np.inf and first[0][0] == rowids[order[0]]
    assert special, "the edge rows are there for their NaN / Inf distances"
    c.close()


# one shape per kernel family, as test_gpu_masked.test_mask_shapes: double-buffered, 64 rows per batch, the rings, int8 x 768, f16 with
# cached norms, the long-row kernel
@pytest.mark.parametrize("vt,dim,n", [(dg.F32, 384, 2531), (dg.F32, 4, 2531), (dg.U8, 64, 2531), (dg.U8, 256, 2531), (dg.I8, 768, 2531),
                                      (dg.F16, 384, 2531), (dg.F32, 4100, 2531)])
def test_masked_cursors(pkg, vt, dim, n):
    low = vt in (dg.U8, dg.I8)
    rows = dg.corpus(vt, n, dim, 610 + dim, low_entropy=low)
    q = dg.query(vt, dim, 611 + dim, low_entropy=low)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L2, q, 5, masked=True)) == VG_ERR_INVALID       # no mask set
    for metric in (dg.L2, dg.DOT):
        own = c.scan_distances(metric, q)
        full = _order(own)
        for name, allowed in _mask_shapes(n).items():
            assert c.set_mask(bits=allowed) == int(allowed.sum())
            order = _order(own, allowed)
            scan = lambda after, k: c.scan_topk_after(metric, q, k, after=after, masked=True)
            ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], name)
            if name == "empty":
                assert len(scan(START, 20)[0]) == 0
                continue
            _check_cursors(scan, own, order, rowids, ctx=ctx)
            gi, gd, _ = _walk(scan, 20, 5)
            m = min(len(order), 100)
            _assert_same((gi, gd), rowids[order[:m]], own[order[:m]], ctx=ctx)
            # a cursor on a row that is NOT allowed: pages continue behind it among the allowed rows
            banned = full[~allowed[full]]
            if len(banned):
                p = banned[len(banned) // 2]
                after = (float(own[p]), int(rowids[p]))
                ids, dd = _behind(own, order, rowids, after, 20)
                _assert_same(scan(after, 20), ids, dd, ctx=(ctx, "cursor row not allowed"))
    c.close()


def test_equalities_with_existing_scans_and_key_form(pkg):
    n, dim = 2531, 100
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    q = dg.query(dg.U8, dim, 72, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    c.set_tie_order(pkg.TIE_POSITION)
    for metric in (dg.L2, dg.DOT, dg.L1):
        for k in (1, 20, 64):
            a = c.scan_topk_after(metric, q, k)
            c.set_mask(bits=np.ones(n, dtype=bool))
            b = c.scan_topk_masked(metric, q, k)
            t = c.scan_topk(metric, q, k)
            for other in (b, t):
                assert a[0].tolist() == other[0].tolist() and np.array_equal(a[1], other[1]), (metric, k)
            c.clear_mask()
        # the key form chained by after_key equals the rowid form chained by (distance, rowid); masked too
        for masked in (False, True):
            if masked:
                c.set_mask(bits=np.random.default_rng(3).random(n) < 0.4)
            key, after = None, START
            for _ in range(6):
                keys = c.scan_topk_after_keys(metric, q, 20, after_key=key, masked=masked)
                gi, gd = c.scan_topk_after(metric, q, 20, after=after, masked=masked)
                pos = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
                assert (pos + 1).tolist() == gi.tolist()
                assert np.array_equal(_key_distances(keys), gd)
                key, after = int(keys[-1]), (float(gd[-1]), int(gi[-1]))
            c.clear_mask()
    assert _error_code(pkg, lambda: c.scan_topk_after_keys(dg.L2, q, 5, after_key=0xFFFFFFFFFFFFFFFF)) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L2, q, 5, after=(float("nan"), 0))) == VG_ERR_INVALID
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L2, q, 65)) == VG_ERR_UNSUPPORTED
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L2, q, 0)) == VG_ERR_INVALID
    assert len(c.scan_topk_after(dg.L2, q, 5, after=(1e300, 0))[0]) == 0
    c.close()


def test_tie_order_setting_does_not_change_the_answer(pkg):
    n, dim = 2531, 64
    rows = dg.corpus(dg.U8, n, dim, 71, low_entropy=True)
    q = dg.query(dg.U8, dim, 72, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    own = c.scan_distances(dg.L2, q)
    order = _order(own)
    rowids = np.arange(n, dtype=np.int64) + 1
    runs = _tie_runs(own, order)
    assert runs
    s, ln = runs[0]
    after = (float(own[order[s + 1]]), int(rowids[order[s + 1]]))
    ids, dd = _behind(own, order, rowids, after, 20)
    for mode in (pkg.TIE_REFERENCE, pkg.TIE_POSITION):
        c.set_tie_order(mode)
        _assert_same(c.scan_topk_after(dg.L2, q, 20, after=after), ids, dd, ctx=mode)
    c.close()


def test_lifecycle_cursor_from_before_the_edit(pkg):
    """after delete_rows, patch_rows and clone, a page taken with a cursor from before the edit equals the expected order of the rows
    as they are now - the cursor's own row deleted included"""
    n, dim = 2531, 100
    rows = dg.corpus(dg.F32, n, dim, 31)
    q = dg.query(dg.F32, dim, 32)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(dg.F32, dim)
    c.append(rows, rowids)
    gi, gd = c.scan_topk_after(dg.L2, q, 20)
    after = (float(gd[-1]), int(gi[-1]))
    own = c.scan_distances(dg.L2, q)
    cursor_pos = int(_order(own)[19])
    assert rowids[cursor_pos] == gi[-1]
    # delete the cursor's row and two rows of the next page
    nxt = _order(own)[20:22]
    gone = np.sort(np.array([cursor_pos, int(nxt[0]), int(nxt[1])], dtype=np.int64))
    c.delete_rows(gone)
    keep = np.ones(n, dtype=bool); keep[gone] = False
    rid2 = rowids[keep]
    own2 = c.scan_distances(dg.L2, q)
    assert len(own2) == n - 3
    ids, dd = _behind(own2, _order(own2), rid2, after, 20)
    got = c.scan_topk_after(dg.L2, q, 20, after=after)
    _assert_same(got, ids, dd, ctx="delete_rows")
    assert not set(got[0].tolist()) & set(rowids[gone].tolist()) and not set(got[0].tolist()) & set(gi.tolist())
    # patch a row of the coming page far away: it leaves the page
    victim = int(np.nonzero(rid2 == got[0][3])[0][0])
    c.patch_rows(np.array([victim], dtype=np.int64), np.full((1, dim), 1000.0, dtype=np.float32))
    own3 = c.scan_distances(dg.L2, q)
    ids, dd = _behind(own3, _order(own3), rid2, after, 20)
    got3 = c.scan_topk_after(dg.L2, q, 20, after=after)
    _assert_same(got3, ids, dd, ctx="patch_rows")
    assert rid2[victim] not in got3[0].tolist()
    # a clone answers the same cursor the same way
    d = c.clone()
    _assert_same(d.scan_topk_after(dg.L2, q, 20, after=after), ids, dd, ctx="clone")
    d.close()
    c.close()


def test_rowids_not_ascending(pkg):
    dim = 64
    rows = dg.corpus(dg.U8, 10, dim, 41, low_entropy=True)
    q = dg.query(dg.U8, dim, 42, low_entropy=True)
    c = pkg.Corpus(dg.U8, dim)
    ids = np.array([5, 4, 9, 1, 2, 3, 8, 7, 6, 10], dtype=np.int64)
    c.append(rows, ids)
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L1, q, 3)) == VG_ERR_UNSUPPORTED
    own = c.scan_distances(dg.L1, q)
    order = _order(own)
    keys = c.scan_topk_after_keys(dg.L1, q, 4)
    keys2 = c.scan_topk_after_keys(dg.L1, q, 64, after_key=int(keys[-1]))
    pos = (np.concatenate([keys, keys2]) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert pos.tolist() == order.tolist()
    c.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_logical_shards_equal_one_corpus(pkg, n_shards):
    n, dim = 2531, 100
    rows = dg.corpus(dg.U8, n, dim, 81, low_entropy=True)
    q = dg.query(dg.U8, dim, 82, low_entropy=True)
    rowids = np.arange(n, dtype=np.int64) * 3 + 11
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(dg.U8, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, n, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    allowed = np.random.default_rng(9).random(n) < 0.3
    for metric in (dg.L2, dg.DOT, dg.L1):
        own = c.scan_distances(metric, q)
        for masked in (False, True):
            if masked:
                assert c.set_mask(bits=allowed) == sh.set_mask(bits=allowed)
            order = _order(own, allowed if masked else None)
            scan = lambda after, k: sh.scan_topk_after(metric, q, k, after=after, masked=masked)
            cursors = _check_cursors(scan, own, order, rowids, ctx=(n_shards, metric, masked))
            assert "tie_middle" in cursors
            for name, after in cursors.items():
                a = c.scan_topk_after(metric, q, 20, after=after, masked=masked)
                b = sh.scan_topk_after(metric, q, 20, after=after, masked=masked)
                assert a[0].tolist() == b[0].tolist() and np.array_equal(a[1], b[1]), (name, masked)
            # keys over global positions chain like one corpus' keys
            key = None
            for _ in range(4):
                ka = c.scan_topk_after_keys(metric, q, 20, after_key=key, masked=masked)
                kb = sh.scan_topk_after_keys(metric, q, 20, after_key=key, masked=masked)
                assert ka.tolist() == kb.tolist()
                key = int(ka[-1])
            c.clear_mask(); sh.clear_mask()
    sh.close()
    c.close()


def test_shards_refuse_rowids_that_ascend_per_shard_only(pkg):
    """blocks are dealt out cyclically: rowids can ascend inside every shard and still not in global order.  One corpus holding these
    rows refuses the rowid form; the shards must too (a wrong page otherwise), while the key form works"""
    dim = 64
    rows = dg.corpus(dg.U8, 8, dim, 43, low_entropy=True)
    q = dg.query(dg.U8, dim, 44, low_entropy=True)
    ids = np.array([10, 11, 1, 2, 12, 13, 3, 4], dtype=np.int64)            # shard 0: 10 11 12 13, shard 1: 1 2 3 4
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows, ids)
    assert _error_code(pkg, lambda: c.scan_topk_after(dg.L1, q, 3)) == VG_ERR_UNSUPPORTED
    sh = pkg.Shards(dg.U8, dim, [0, 0], block_rows=2)
    sh.append(rows, ids)
    assert _error_code(pkg, lambda: sh.scan_topk_after(dg.L1, q, 3)) == VG_ERR_UNSUPPORTED
    assert _error_code(pkg, lambda: sh.scan_topk_batch_after(dg.L1, rows[:2], 3)) == VG_ERR_UNSUPPORTED
    assert sh.scan_topk_after_keys(dg.L1, q, 8).tolist() == c.scan_topk_after_keys(dg.L1, q, 8).tolist()
    sh.close()
    c.close()
