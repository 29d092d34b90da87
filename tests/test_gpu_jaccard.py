"""Jaccard / Tanimoto distance (VG_DIST_JACCARD, uint8 corpora: packed bit vectors) through every scan form, against numpy.

The expectation is jaccard_cases: d = float32(u - i) / float32(u) with i = popcount(q AND row), u = popcount(q OR row), 0 where
u == 0; order = stable argsort = (distance, scan position); rowids, order and distance bits compare with ==.  Shapes: one row length
per launch shape of the uint8 ladder, a ragged row, one long row; row counts with a partial last batch and more than one workgroup;
rows of mixed density with the query, its complement and an empty row planted across wavefront and workgroup boundaries, equal
rationals, zero queries and corpora whose rows all tie.  Refusals (another element type, tie_order = reference) through Python and
the raw C symbols, and the paths a Jaccard scan must not take (nibble filter, matrix-core batch)."""
import ctypes as C

import numpy as np
import pytest

import capped_cases as cc
import grouped_cases as gc
import jaccard_cases as jc
import labeled_cases as lc
import valued_cases as vc

pytestmark = pytest.mark.gpu

VG_OK, VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 0, 1, 5
JAC = jc.JACCARD
NEEDS_U8 = "Jaccard distance needs a uint8 corpus"


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


def _corpus(pkg, rows):
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


# ------------------------------------------------------------------------------------------------ plain forms

@pytest.mark.parametrize("dim,n", jc.PLAIN_CASES)
def test_topk_and_distances(pkg, dim, n):
    q = jc.query(dim, 7 * dim + 1)
    if n == 65:
        q = jc.query(dim, 7 * dim + 1, 0.5)                    # a dense query at one row count: fewer distances of exactly 1
    rows = jc.corpus(n, dim, q, 7 * dim + n)
    d = jc.distances(rows, q)
    assert np.array_equal(d.view(np.uint32), pkg.jaccard_reference(rows, q).view(np.uint32))
    assert np.isfinite(d).all() and d.min() >= 0 and d.max() <= 1
    c = _corpus(pkg, rows)
    lpr, u, lng = pkg.plan_scan_shape(pkg.U8, dim, JAC)
    name = c.kernel_name(JAC)
    assert name.startswith("scan_long_u8_jac_" if lng else "scan_u8_jac_u%d_lpr%d" % (u, lpr)), name
    got = c.scan_distances(JAC, q)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), d.view(np.uint32)), (dim, n)
    if n > 66 and q.any():
        assert d[0] == 0 and d[n - 1] == 0 and d[1] == 1 and d[n - 2] == 1 and d[2] == 1 and d[n - 3] == 1
    for k in (1, 20, 64):
        jc.check(c.scan_topk(JAC, q, k), jc.expected(d, k), (dim, n, k))
    c.close()


@pytest.mark.parametrize("weight", sorted(jc.EQUAL_RATIONALS))
def test_equal_rationals_tie_bit_for_bit_in_position_order(pkg, weight):
    """(1, 2), (2, 4), (3, 6), (16, 32), (24, 48), (32, 64): one float, 0x3F000000, and among themselves the order of their positions"""
    dim, n = 32, 2531
    q, rows, pos = jc.equal_rationals(n, dim, weight, 70 + weight)
    d = jc.distances(rows, q)
    c = _corpus(pkg, rows)
    got = c.scan_distances(JAC, q)
    assert (got[pos].view(np.uint32) == 0x3F000000).all() and np.array_equal(got.view(np.uint32), d.view(np.uint32))
    ids, dist = c.scan_topk(JAC, q, 64)
    jc.check((ids, dist), jc.expected(d, 64), weight)
    near, nd, matches = c.scan_within(JAC, q, 0.5)             # every row up to 1/2: the whole run, whatever its length
    jc.check((near, nd), jc.within(d, 0.5)[:2], weight)
    assert matches == jc.within(d, 0.5)[2] >= int((d < 0.5).sum()) + len(pos)
    halves = near[np.asarray(nd, dtype=np.float32).view(np.uint32) == 0x3F000000] - 1
    assert set(pos.tolist()) <= set(halves.tolist()) and halves.tolist() == sorted(halves.tolist())
    c.close()


def test_zero_query_and_identical_rows(pkg):
    for dim in (16, 100, 768):
        n = 2531
        zero = np.zeros(dim, dtype=np.uint8)
        rows = jc.zero_query_corpus(n, dim, dim)
        d = jc.distances(rows, zero)
        assert set(np.unique(d).tolist()) == {0.0, 1.0} and d[0] == 0 and (d[::3] == 0).all()
        c = _corpus(pkg, rows)
        assert np.array_equal(c.scan_distances(JAC, zero).view(np.uint32), d.view(np.uint32))
        for k in (1, 20, 64):
            jc.check(c.scan_topk(JAC, zero, k), jc.expected(d, k), (dim, k))
        q = jc.query(dim, dim + 3)                             # ... and a query over the same rows: its empty rows are at 1
        jc.check(c.scan_topk(JAC, q, 64), jc.expected(jc.distances(rows, q), 64), dim)
        c.close()
        rows = jc.identical(n, dim, dim)
        for q in (jc.query(dim, dim + 1), zero, rows[0].copy()):
            d = jc.distances(rows, q)
            assert (d == d[0]).all()
            c = _corpus(pkg, rows)
            for k in (1, 20, 64):
                ids, dist = c.scan_topk(JAC, q, k)
                assert ids.tolist() == list(range(1, k + 1)) and (dist == d[0]).all(), (dim, k)
            c.close()


@pytest.mark.parametrize("k", [65, 200])
def test_large_k(pkg, k):
    """k > 64: store mode, then radix select - on random rows, on identical rows (every row ties: the radix select sorts the whole
    corpus itself) and with exactly k - 1 rows below a distance that 5000 rows share"""
    dim = 32
    q = jc.weighted_query(dim, 64, 900 + k)
    for what, rows in (("random", jc.corpus(30001, dim, q, 901 + k)), ("identical", jc.identical(30001, dim, 902 + k)),
                       ("k - 1 below a value 5000 rows share", jc.shared_kth_value(k, dim, q, 903 + k))):
        d = jc.distances(rows, q)
        if what.startswith("k - 1"):
            kth = np.sort(d)[k - 1]
            assert kth == jc.HALF and int((d < kth).sum()) == k - 1 and int((d == kth).sum()) == 5000
        c = _corpus(pkg, rows)
        jc.check(c.scan_topk(JAC, q, k), jc.expected(d, k), (what, k))
        c.close()


@pytest.mark.parametrize("dim", jc.ROW_BYTES + jc.WIDE_ROW_BYTES + (jc.LONG_ROW_BYTES,))
def test_batch_equals_single_scans(pkg, dim):
    n = 2531
    q0 = jc.query(dim, 50 + dim)
    rows = jc.corpus(n, dim, q0, 51 + dim)
    c = _corpus(pkg, rows)
    per_pass, lpr, u = pkg.batch_masked_plan(c, JAC)           # the multi-query plan every batch form shares
    assert (per_pass, lpr, u) == pkg.batch_masked_plan(c, pkg.L1)
    lng = pkg.plan_scan_shape(pkg.U8, dim, JAC)[2]
    # 1 to 3 chunks per lane: 4 queries per pass; 4 or 6: 2; 8 chunks per lane and long rows: no multi-query form, nq single scans
    assert per_pass == (0 if lng or u == 8 else 4 if u <= 3 else 2) and (lng or u in (1, 2, 3, 4, 6, 8)), (dim, per_pass, u)
    rng = np.random.default_rng(52 + dim)
    for nq in (1, 4, 5, 9):
        qs = jc.random_rows(nq, dim, rng)
        qs[0] = q0
        if nq >= 5:
            qs[2] = 0                                          # a zero query in one batch slot
        for k in (1, 20, 64):
            ids, dist, cnt = c.scan_topk_batch(JAC, qs, k)
            path = c.last_batch_path()
            assert path == (5 if per_pass and nq >= 2 else 6), (dim, nq, path)      # never the matrix cores; long rows: the fallback
            for i in range(nq):
                si, sd = c.scan_topk(JAC, qs[i], k)
                assert cnt[i] == len(si) and ids[i, :cnt[i]].tolist() == si.tolist() and np.array_equal(dist[i, :cnt[i]], sd), (dim, nq, k, i)
            if k == 20:
                jc.check_batch((ids, dist, cnt), [jc.expected(jc.distances(rows, qs[i]), k) for i in range(nq)], k, (dim, nq))
    c.close()


# ------------------------------------------------------------------------------------------------ every other form

RUN = 40            # rows of the form corpus planted at distance exactly 1/2: a run of equal distances for the radii and limits to cut


@pytest.fixture(scope="module", params=jc.FORM_ROW_BYTES)
def form_case(request, pkg):
    """one corpus per row length, shared by the form tests: rows, five queries (the third all zero) and their numpy distances -
    computed once, left alone.  Query 0 has exactly `dim` set bits and RUN rows hold half of them and nothing else: distance 1/2"""
    dim, n = request.param, jc.FORM_ROWS
    q0 = jc.weighted_query(dim, dim, 300 + dim)
    rows = jc.corpus(n, dim, q0, 301 + dim)
    rng = np.random.default_rng(302 + dim)
    run = np.sort(rng.permutation(np.arange(70, n - 4))[:RUN])
    rows[run] = jc.rows_with_counts([dim // 2] * RUN, [0] * RUN, dim, q0, 303 + dim)
    qs = jc.random_rows(5, dim, rng)
    qs[0] = q0
    qs[2] = 0
    ds = [jc.distances(rows, q) for q in qs]
    for d in ds:
        d.setflags(write=False)
    assert int((ds[0] == jc.HALF).sum()) >= RUN and set(np.unique(ds[2]).tolist()) <= {0.0, 1.0}
    c = _corpus(pkg, rows)
    yield dim, n, c, qs, ds
    c.close()


def test_within(pkg, form_case):
    dim, n, c, qs, ds = form_case
    q, d = qs[0], ds[0]
    below_half = float(np.nextafter(jc.HALF, np.float32(0)))
    run = int((d == jc.HALF).sum())
    # 0: the planted copies of the query; 1/2 and the float below it: the whole run of equal distances or none of it; 1: every row
    for radius in (0.0, 0.5, below_half, 1.0, float(np.sort(d)[n // 3]), -1.0, float("inf")):
        want = jc.within(d, radius)
        got = c.scan_within(JAC, q, radius)
        jc.check(got, want, (dim, radius))
        assert got[2] == want[2], (dim, radius)
    assert jc.within(d, 0.0)[2] == 4 and jc.within(d, 1.0)[2] == n and jc.within(d, -1.0)[2] == 0
    assert jc.within(d, 0.5)[2] - jc.within(d, below_half)[2] == run >= RUN
    limit = jc.within(d, below_half)[2] + run // 2             # a limit that cuts inside the run
    want = jc.within(d, 0.5, limit=limit)
    got = c.scan_within(JAC, q, 0.5, limit=limit)
    jc.check(got, want, (dim, "limit"))
    assert got[2] == want[2] and len(got[0]) == limit and want[1][-1] == jc.HALF
    # the batch: a radius each (the zero query at 0: its empty rows)
    radii = [0.5, float(np.sort(ds[1])[50]), 0.0, 1.0, -1.0]
    for limit in (None, 11):
        got = c.scan_within_batch(JAC, qs, radii, limit=limit)
        for i in range(len(qs)):
            want = jc.within(ds[i], radii[i], limit=limit)
            jc.check(got[i], want, (dim, i, limit))
            assert got[i][2] == want[2], (dim, i, limit)
            if limit is None:
                single = c.scan_within(JAC, qs[i], radii[i])
                jc.check(got[i], single, (dim, i, "single"))
                assert got[i][2] == single[2]


def test_masked(pkg, form_case):
    dim, n, c, qs, ds = form_case
    allow = np.random.default_rng(310 + dim).random(n) < 0.3
    allow[0] = False                                           # a planted nearest row the mask hides
    c.set_mask(bits=allow)
    for k in (1, 20, 64):
        jc.check(c.scan_topk_masked(JAC, qs[0], k), jc.expected(ds[0], k, allow), (dim, k))
        got = c.scan_topk_batch_masked(JAC, qs, k)
        jc.check_batch(got, [jc.expected(d, k, allow) for d in ds], k, (dim, k))
        for i in range(len(qs)):
            jc.check((got[0][i, :got[-1][i]], got[1][i, :got[-1][i]]), c.scan_topk_masked(JAC, qs[i], k), (dim, k, i))
    for r, limit in ((0.5, None), (0.5, 13), (0.0, None), (1.0, None), (-1.0, None)):
        want = jc.within(ds[0], r, allow, limit)
        got = c.scan_within_masked(JAC, qs[0], r, limit=limit)
        jc.check(got, want, (dim, r))
        assert got[2] == want[2]
    c.clear_mask()


def test_paging_seven_rows_at_a_time(pkg, form_case):
    """the concatenated pages are the full order: page boundaries fall inside the runs at 1/2 and at 1"""
    dim, n, c, qs, ds = form_case
    full = jc.expected(ds[0], n)
    ids, dist, after = [], [], None
    while True:
        pi, pd = c.scan_topk_after(JAC, qs[0], 7, after)
        if len(pi) == 0:
            break
        ids += pi.tolist(); dist += pd.tolist()
        after = (pd[-1], pi[-1])
    jc.check((np.array(ids), np.array(dist)), full, dim)
    # the batch form: five queries page side by side
    fulls = [jc.expected(d, n) for d in ds]
    bids, bdist, cur = [[] for _ in qs], [[] for _ in qs], None
    for _ in range((n + 6) // 7 + 1):
        pi, pd, cnt = c.scan_topk_batch_after(JAC, qs, 7, cur)
        if not cnt.any():
            break
        cur = []
        for i in range(len(qs)):
            bids[i] += pi[i, :cnt[i]].tolist(); bdist[i] += pd[i, :cnt[i]].tolist()
            cur.append((bdist[i][-1], bids[i][-1]))
    for i in range(len(qs)):
        jc.check((np.array(bids[i]), np.array(bdist[i])), fulls[i], (dim, i))


def test_labeled_labelset_valued(pkg, form_case):
    dim, n, c, qs, ds = form_case
    labels, asked = lc.layouts(n)["uniform5"]
    c.set_labels(labels)
    q, d = qs[0], ds[0]
    for k in (1, 20, 64):
        for label in asked:
            lc.assert_same(c.scan_topk_labeled(JAC, q, k, label), *lc.expected(d, labels == label, k), ctx=(dim, k, label))
    qlab = np.array([0, 3, lc.ABSENT, 3, 1], dtype=np.uint32)
    got = c.scan_topk_batch_labeled(JAC, qs, qlab, 20)
    jc.check_batch(got, [lc.expected(ds[i], labels == qlab[i], 20) for i in range(5)], 20, dim)
    for i in range(5):
        jc.check((got[0][i, :got[-1][i]], got[1][i, :got[-1][i]]), c.scan_topk_labeled(JAC, qs[i], 20, int(qlab[i])), (dim, i))
    for lset, exclude in (([1, 3], False), ([0], True), ([lc.ABSENT], False)):
        allow = np.isin(labels, lset) ^ exclude
        lc.assert_same(c.scan_topk_labelset(JAC, q, 20, lset, exclude=exclude), *lc.expected(d, allow, 20), ctx=(dim, lset, exclude))
    sets = [[1, 3], [0], [2, 4], [0, 1], [3]]
    got = c.scan_topk_batch_labelset(JAC, qs, sets, 20, exclude=True)
    jc.check_batch(got, [lc.expected(ds[i], ~np.isin(labels, sets[i]), 20) for i in range(5)], 20, (dim, "label sets"))
    want = jc.within(d, 0.5, labels == 3, 50)
    got = c.scan_within_labeled(JAC, q, 0.5, 3, limit=50)
    jc.check(got, want, (dim, "within labeled"))
    assert got[2] == want[2]
    values = vc.layouts(n)["random"]
    c.set_values(values)
    lo, hi = vc.intervals(values)["on_present"]
    for k in (1, 20, 64):
        lc.assert_same(c.scan_topk_valued(JAC, q, k, lo, hi), *lc.expected(d, vc.allowed(values, lo, hi), k), ctx=(dim, k, "valued"))
    got = c.scan_topk_batch_valued(JAC, qs, [lo] * 5, [hi] * 5, 20)
    jc.check_batch(got, [lc.expected(ds[i], vc.allowed(values, lo, hi), 20) for i in range(5)], 20, (dim, "valued batch"))
    c.clear_values()
    c.clear_labels()


def test_grouped_and_capped(pkg, form_case):
    dim, n, c, qs, ds = form_case
    for lname in ("uniform5", "some_none", "pairs"):
        labels = gc.layouts(n, ds[0])[lname]
        c.set_labels(labels)
        for k in (1, 20, 64):
            gc.assert_same(c.scan_topk_grouped(JAC, qs[0], k), *gc.expected(ds[0], labels, None, k), ctx=(dim, lname, k))
            for m in (1, 3):
                gc.assert_same(c.scan_topk_capped(JAC, qs[0], k, m), *cc.expected(ds[0], labels, None, k, m), ctx=(dim, lname, k, m))
        ids, dist, lab, cnt = c.scan_topk_batch_grouped(JAC, qs, 20)
        for i in range(len(qs)):
            gc.assert_same((ids[i, :cnt[i]], dist[i, :cnt[i]], lab[i, :cnt[i]]), *gc.expected(ds[i], labels, None, 20), ctx=(dim, lname, i))
        for m in (1, 3):
            cids, cdist, clab, ccnt = c.scan_topk_batch_capped(JAC, qs, 20, m)
            for i in range(len(qs)):
                gc.assert_same((cids[i, :ccnt[i]], cdist[i, :ccnt[i]], clab[i, :ccnt[i]]), *cc.expected(ds[i], labels, None, 20, m),
                               ctx=(dim, lname, i, m))
    c.clear_labels()


@pytest.mark.parametrize("dim", jc.FORM_ROW_BYTES)
def test_three_shards(pkg, dim):
    n = jc.FORM_ROWS
    q0 = jc.query(dim, 400 + dim)
    rows = jc.corpus(n, dim, q0, 401 + dim)
    qs = jc.random_rows(5, dim, np.random.default_rng(402 + dim))
    qs[0] = q0
    qs[2] = 0
    ds = [jc.distances(rows, q) for q in qs]
    s = pkg.Shards(pkg.U8, dim, [0, 0, 0], block_rows=100)
    s.append(rows)
    assert min(s.shard_rows()) > 0
    for k in (1, 20, 64, 200):
        jc.check(s.scan_topk(JAC, q0, k), jc.expected(ds[0], k), (dim, k))
    jc.check_batch(s.scan_topk_batch(JAC, qs, 20), [jc.expected(d, 20) for d in ds], 20, dim)
    allow = np.random.default_rng(403 + dim).random(n) < 0.3
    s.set_mask(bits=allow)
    jc.check(s.scan_topk_masked(JAC, q0, 20), jc.expected(ds[0], 20, allow), (dim, "masked"))
    labels = gc.layouts(n, ds[0])["uniform5"]
    s.set_labels(labels)
    gc.assert_same(s.scan_topk_grouped(JAC, q0, 20), *gc.expected(ds[0], labels, None, 20), ctx=(dim, "grouped"))
    s.close()


# ------------------------------------------------------------------------------------------------ refusals

def _refused(pkg, fn, code, *texts):
    with pytest.raises(pkg.VectorGpuError) as ei:
        fn()
    msg = str(ei.value)
    assert msg.startswith("vectorgpu error %d:" % code), msg
    for t in texts:
        assert t in msg, msg


def _other_type_rows(pkg, vt, n, dim):
    rng = np.random.default_rng(5)
    return rng.standard_normal((n, dim), dtype=np.float32) if vt == pkg.F32 else rng.integers(-100, 100, (n, dim)).astype(np.int8)


@pytest.mark.parametrize("vt", ["F32", "I8"])
def test_other_element_types_are_refused(pkg, vt):
    vt = getattr(pkg, vt)
    n, dim = 300, 32
    rows = _other_type_rows(pkg, vt, n, dim)
    qs = rows[:3].copy()
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    c.set_mask(bits=np.ones(n, dtype=bool))
    c.set_profiling(True)                                      # the ring counts every scan launch
    L = pkg.lib()
    _refused(pkg, lambda: c.scan_topk(JAC, qs[0], 5), VG_ERR_UNSUPPORTED, "vg_scan_topk: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_topk(JAC, qs[0], 200), VG_ERR_UNSUPPORTED, "vg_scan_topk: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_distances(JAC, qs[0]), VG_ERR_UNSUPPORTED, "vg_scan_distances: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_topk_batch(JAC, qs, 5), VG_ERR_UNSUPPORTED, "vg_scan_topk_batch: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_within(JAC, qs[0], 0.5), VG_ERR_UNSUPPORTED, "vg_scan_within: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_within_batch(JAC, qs, 0.5), VG_ERR_UNSUPPORTED, "vg_scan_within_batch: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_topk_masked(JAC, qs[0], 5), VG_ERR_UNSUPPORTED, "vg_scan_topk_masked: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_topk_batch_masked(JAC, qs, 5), VG_ERR_UNSUPPORTED, "vg_scan_topk_batch_masked: " + NEEDS_U8)
    _refused(pkg, lambda: c.scan_topk_after(JAC, qs[0], 5), VG_ERR_UNSUPPORTED, NEEDS_U8)
    _refused(pkg, lambda: pkg.batch_masked_plan(c, JAC), VG_ERR_UNSUPPORTED, NEEDS_U8)
    assert c.kernel_name(JAC) == ""
    # the raw symbols: the code, the message, the counts zeroed, nothing launched
    q = np.ascontiguousarray(qs[0]); qb = np.ascontiguousarray(qs)
    ids = np.full(3 * 5, -7, dtype=np.int64); dist = np.zeros(3 * 5, dtype=np.float64)
    cnt = C.c_int(9)
    assert L.vg_scan_topk(c.h, JAC, pkg._ptr(q), 5, pkg._ptr(ids), pkg._ptr(dist), C.byref(cnt)) == VG_ERR_UNSUPPORTED
    assert cnt.value == 0 and L.vg_last_error().decode() == "vg_scan_topk: " + NEEDS_U8
    cnt = C.c_int(9)
    assert L.vg_scan_topk_masked(c.h, JAC, pkg._ptr(q), 5, pkg._ptr(ids), pkg._ptr(dist), C.byref(cnt)) == VG_ERR_UNSUPPORTED
    assert cnt.value == 0 and L.vg_last_error().decode() == "vg_scan_topk_masked: " + NEEDS_U8
    cnts = np.full(3, 9, dtype=np.int32)
    assert L.vg_scan_topk_batch(c.h, JAC, pkg._ptr(qb), 3, 5, pkg._ptr(ids), pkg._ptr(dist), pkg._ptr(cnts)) == VG_ERR_UNSUPPORTED
    assert cnts.tolist() == [0, 0, 0] and L.vg_last_error().decode() == "vg_scan_topk_batch: " + NEEDS_U8
    m, held = C.c_int64(9), C.c_int64(9)
    assert L.vg_scan_within(c.h, JAC, pkg._ptr(q), 0.5, 0, C.byref(m), C.byref(held)) == VG_ERR_UNSUPPORTED
    assert (m.value, held.value) == (0, 0) and L.vg_last_error().decode() == "vg_scan_within: " + NEEDS_U8
    assert c.within_last_launches() == 0 and c.within_batch_last_launches() == 0
    assert c.profile_mean_ms()[0] == 0                         # no scan was launched by any of the calls above
    # the argument checks that return VG_ERR_INVALID come first; an unknown metric keeps its code and text
    cnt = C.c_int(9)
    assert L.vg_scan_topk_masked(c.h, JAC, pkg._ptr(q), 0, pkg._ptr(ids), pkg._ptr(dist), C.byref(cnt)) == VG_ERR_INVALID
    c.clear_mask()
    _refused(pkg, lambda: c.scan_topk_masked(JAC, qs[0], 5), VG_ERR_INVALID, "no row mask set")
    _refused(pkg, lambda: c.scan_within(JAC, qs[0], float("nan")), VG_ERR_INVALID, "NaN")
    for call in (lambda: c.scan_topk(99, qs[0], 5), lambda: c.scan_topk_batch(99, qs, 5), lambda: c.scan_within(99, qs[0], 1.0),
                 lambda: c.scan_distances(99, qs[0])):
        _refused(pkg, call, VG_ERR_INVALID, "unknown distance metric 99")
    assert c.scan_topk(pkg.L2, qs[0], 1)[0].tolist() == [1]    # the handle still serves its own metrics
    c.close()
    # a shard set
    s = pkg.Shards(vt, dim, [0, 0, 0], block_rows=50)
    s.append(rows)
    s.set_mask(bits=np.ones(n, dtype=bool))
    _refused(pkg, lambda: s.scan_topk(JAC, qs[0], 5), VG_ERR_UNSUPPORTED, "vg_shards_scan_topk: " + NEEDS_U8)
    _refused(pkg, lambda: s.scan_topk_batch(JAC, qs, 5), VG_ERR_UNSUPPORTED, "vg_shards_scan_topk_batch: " + NEEDS_U8)
    _refused(pkg, lambda: s.scan_within(JAC, qs[0], 0.5), VG_ERR_UNSUPPORTED, NEEDS_U8)
    _refused(pkg, lambda: s.scan_topk_masked(JAC, qs[0], 5), VG_ERR_UNSUPPORTED, NEEDS_U8)
    cnt = C.c_int(9)
    assert L.vg_shards_scan_topk_masked(s.h, JAC, pkg._ptr(q), 5, pkg._ptr(ids), pkg._ptr(dist), C.byref(cnt)) == VG_ERR_UNSUPPORTED
    assert cnt.value == 0 and NEEDS_U8 in L.vg_last_error().decode()
    _refused(pkg, lambda: s.scan_topk(99, qs[0], 5), VG_ERR_INVALID, "unknown distance metric 99")
    s.close()


def test_reference_tie_order_is_refused(pkg):
    dim, n = 32, 300
    q = jc.query(dim, 1)
    rows = jc.corpus(n, dim, q, 2)
    qs = rows[:3].copy()
    what = "Jaccard distance is not served with tie_order = reference"
    c = _corpus(pkg, rows)
    c.set_tie_order(pkg.TIE_REFERENCE)
    _refused(pkg, lambda: c.scan_topk(JAC, q, 5), VG_ERR_UNSUPPORTED, "vg_scan_topk: " + what)
    _refused(pkg, lambda: c.scan_topk(JAC, q, 200), VG_ERR_UNSUPPORTED, "vg_scan_topk: " + what)
    _refused(pkg, lambda: c.scan_topk_batch(JAC, qs, 5), VG_ERR_UNSUPPORTED, "vg_scan_topk_batch: " + what)
    assert len(c.scan_topk(pkg.L1, q, 5)[0]) == 5              # the other metrics keep their reference order
    c.set_tie_order(pkg.TIE_POSITION)
    jc.check(c.scan_topk(JAC, q, 5), jc.expected(jc.distances(rows, q), 5))
    c.close()
    s = pkg.Shards(pkg.U8, dim, [0, 0, 0], block_rows=50)
    s.append(rows)
    s.set_tie_order(pkg.TIE_REFERENCE)
    _refused(pkg, lambda: s.scan_topk(JAC, q, 5), VG_ERR_UNSUPPORTED, "vg_shards_scan_topk: " + what)
    _refused(pkg, lambda: s.scan_topk_batch(JAC, qs, 5), VG_ERR_UNSUPPORTED, "vg_shards_scan_topk_batch: " + what)
    s.close()
    _refused(pkg, lambda: pkg.SlabScan(pkg.U8, dim, JAC, q, 5, 100, tie_order=pkg.TIE_REFERENCE), VG_ERR_UNSUPPORTED, "vg_slab_scan_begin: " + what)
    _refused(pkg, lambda: pkg.SlabScan(pkg.F32, dim, JAC, np.zeros(dim, dtype=np.float32), 5, 100), VG_ERR_UNSUPPORTED, "vg_slab_scan_begin: " + NEEDS_U8)
    _refused(pkg, lambda: pkg.SlabScan(pkg.U8, dim, 99, q, 5, 100), VG_ERR_INVALID, "unknown distance metric 99")


# ------------------------------------------------------------------------------------------------ paths not taken

def test_forced_nibble_filter_is_not_taken(pkg, monkeypatch):
    """With the size gate lifted (VG_SCAN_FILTER_MIN_MB=0, as the filter tests do) vg_corpus_set_scan_filter(c, 1) switches the nibble
    filter on for L2 / cosine / dot on this handle - the control: L2 names a filter kernel and its scan evaluates rows exactly.  A
    Jaccard scan on the same handle keeps the plain kernel, launches no filter and returns the exact answer; its batch takes the
    multi-query scan where an L2 batch takes the matrix cores"""
    monkeypatch.setenv("VG_SCAN_FILTER_MIN_MB", "0")
    dim, n = 768, 30001
    q = jc.query(dim, 11)
    rows = jc.corpus(n, dim, q, 12)
    d = jc.distances(rows, q)
    c = _corpus(pkg, rows)
    c.set_scan_filter(1)
    assert c.kernel_name(pkg.L2).startswith("scan_filter_u8_l2_n4"), c.kernel_name(pkg.L2)      # the control: the filter IS forced
    assert len(c.scan_topk(pkg.L2, q, 20)[0]) == 20
    assert c.filter_exact_evals() > 0                          # ... and ran (the read-out resets the count)
    name = c.kernel_name(JAC)
    assert name.startswith("scan_u8_jac_"), name
    for k in (1, 20, 64):
        jc.check(c.scan_topk(JAC, q, k), jc.expected(d, k), k)
    assert c.filter_exact_evals() == 0                         # no filter launch evaluated a row for Jaccard
    qs = rows[3:12].copy()
    c.scan_topk_batch(pkg.L2, qs, 20)
    assert c.last_batch_path() == 2                            # the control: an L2 batch takes the matrix cores
    ids, dist, cnt = c.scan_topk_batch(JAC, qs, 20)
    assert c.last_batch_path() == 5
    jc.check_batch((ids, dist, cnt), [jc.expected(jc.distances(rows, x), 20) for x in qs], 20)
    c.close()
