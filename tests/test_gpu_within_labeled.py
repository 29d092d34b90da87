"""Labeled range scans, single forms (vg_scan_within_labeled, vg_scan_within_labelset): every row of a label - or of a set of labels -
within a distance of the query, through the binding.

Contract (include/vectorgpu.h): a row matches when it carries an allowed label, its distance d - the float the plain scan computes -
satisfies (double)d <= radius and d is finite; a row without a label never matches; order is ascending (distance, scan position); with
a limit the first `limit` matches are held and the number of all matches is still reported; the row mask is neither read nor written.

  * uint8 / int8: rows, order, distance bits and count equal to the pinned CPU oracle's distances restricted to the label's rows here,
    for every label layout and every label worth asking for (the absent one included), radii ON a tied distance, below the minimum
    and +Inf included;
  * f32 / f16 / bf16 / long rows: equal to scan_within at the same radius restricted to the label's rows (the single forms share one
    launch shape, so bit for bit and count for count), and to the engine's own scan_distances restricted and filtered here;
  * limits around the match count, label sets (include, exclude, empty, duplicates, only absent labels), the row mask left alone, the
    held result, overflow of the device buffer, the contract's errors.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
from test_gpu_within import _assert_same, _expected, _own_radii, _radii_at_ranks

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1
N = lc.N
INT_SHAPES = [s for s in lc.SHAPES if s[0] in (dg.U8, dg.I8)]
FLOAT_SHAPES = [s for s in lc.SHAPES if s[0] not in (dg.U8, dg.I8)]
_ids = lambda shapes: ["%s-%d" % (dg.TYPE_NAMES[s[0]], s[1]) for s in shapes]


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


def _expected_allowed(dist, allowed, radius, rowids=None):
    """_expected over the allowed rows only: a row that is not allowed is given a distance that never matches"""
    d = np.where(np.asarray(allowed, dtype=bool), np.asarray(dist, dtype=np.float32), np.float32(np.nan))
    return _expected(d, radius, rowids)


def _radii_for(dist, allowed, pick):
    """radii at ranks of the ALLOWED rows' own distances; no allowed row: radii that would match every row of the corpus"""
    if not allowed.any():
        return [float(np.max(dist[np.isfinite(dist)])), float("inf")]
    return pick(dist[allowed])


def _allowed_by_set(labels, members, exclude):
    inside = np.isin(labels, np.asarray(members, dtype=np.uint32))
    return (labels != lc.NONE) & (~inside if exclude else inside)


# ------------------------------------------------------------------------------------------------- uint8 / int8 against the oracle

@pytest.mark.parametrize("vt,dim,per_pass,metrics", INT_SHAPES, ids=_ids(INT_SHAPES))
def test_int8_bit_exact_vs_oracle(pkg, orc, vt, dim, per_pass, metrics):
    rows = lc.data(vt, N, dim, 61 + dim)
    q = lc.data(vt, 1, dim, 62 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    tied = False
    for metric in metrics:
        want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
        for lname, (labels, asked) in lc.layouts(N).items():
            c.set_labels(labels)
            for label in asked:
                allowed = labels == label
                for radius in _radii_for(want, allowed, _radii_at_ranks):
                    ids, dist = _expected_allowed(want, allowed, radius)
                    tied = tied or (np.isfinite(radius) and int(np.sum(want[allowed] == np.float32(radius))) > 1)
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, label, radius)
                    _assert_same(c.scan_within_labeled(metric, q, radius, label), ids, dist, ctx=ctx)
                    assert (labels[ids - 1] == label).all(), ctx
            if lname == "some_none":                            # asking for every label there is still leaves the unlabeled rows out
                every = _allowed_by_set(labels, [], True)
                ids, dist = _expected_allowed(want, every, float("inf"))
                assert len(ids) == int(every.sum()) < N
                _assert_same(c.scan_within_labelset(metric, q, float("inf"), [], exclude=True), ids, dist, ctx=(lname, metric, "every label"))
    assert tied, "four-level data is there for radii on a tied distance"
    c.close()


# ------------------------------------------------------------------------------------------------- floats and long rows

@pytest.mark.parametrize("vt,dim,per_pass,metrics", FLOAT_SHAPES, ids=_ids(FLOAT_SHAPES))
def test_floats_equal_scan_within_restricted_to_the_label(pkg, vt, dim, per_pass, metrics):
    rows = lc.data(vt, N, dim, 63 + dim)
    q = lc.data(vt, 1, dim, 64 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    for metric in metrics:
        own = c.scan_distances(metric, q)
        for lname, (labels, asked) in lc.layouts(N).items():
            c.set_labels(labels)
            for label in asked:
                allowed = labels == label
                for radius in _radii_for(own, allowed, _own_radii):
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, label, radius)
                    got = c.scan_within_labeled(metric, q, radius, label)
                    ids, dist, _ = c.scan_within(metric, q, radius)             # every label's rows, then restricted here
                    keep = allowed[ids - 1]
                    _assert_same(got, ids[keep], dist[keep].astype(np.float32), ctx=ctx)
                    _assert_same(got, *_expected_allowed(own, allowed, radius), ctx=(ctx, "stream"))
    c.close()


# ------------------------------------------------------------------------------------------------- limits, sets, mask, held result

def _small(pkg, vt=dg.U8, dim=64, seed=70):
    rows = lc.data(vt, N, dim, seed)
    q = lc.data(vt, 1, dim, seed + 1)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    return c, q, c.scan_distances(dg.L2, q)


@pytest.mark.parametrize("vt,dim", [(dg.U8, 64), (dg.F32, 384), (dg.F32, 4100)])
def test_limits_around_the_match_count(pkg, vt, dim):
    c, q, own = _small(pkg, vt, dim, 70 + dim)
    labels, _ = lc.layouts(N)["uniform5"]
    c.set_labels(labels)
    allowed = labels == 3
    s = np.sort(own[allowed])
    for rank in (1, 40, len(s)):
        radius = float(s[rank - 1])
        ids, dist = _expected_allowed(own, allowed, radius)
        m = len(ids)
        assert m >= rank
        for limit in sorted(set([1, max(1, m - 1), m, m + 1])):
            ctx = (dg.TYPE_NAMES[vt], dim, rank, limit)
            _assert_same(c.scan_within_labeled(dg.L2, q, radius, 3, limit=limit), ids[:limit], dist[:limit], matches=m, ctx=ctx)
            _assert_same(c.scan_within_labelset(dg.L2, q, radius, [3], limit=limit), ids[:limit], dist[:limit], matches=m, ctx=ctx)
    c.close()


@pytest.mark.parametrize("vt,dim", [(dg.U8, 64), (dg.F32, 384), (dg.BF16, 384)])
def test_label_sets(pkg, vt, dim):
    c, q, own = _small(pkg, vt, dim, 80 + dim)
    for lname in ("uniform5", "some_none", "runs200"):
        labels, _ = lc.layouts(N)[lname]
        c.set_labels(labels)
        cases = [("include", [0, 3], False), ("exclude", [0, 3], True), ("empty", [], False), ("empty_exclude", [], True),
                 ("duplicates", [3, 0, 3, 3, 0], False), ("duplicates_exclude", [3, 0, 3, 3, 0], True),
                 ("absent_only", [lc.ABSENT, lc.ABSENT + 1], False), ("absent_only_exclude", [lc.ABSENT, lc.ABSENT + 1], True),
                 ("one", [2], False), ("unsorted", [4, lc.ABSENT, 1], False)]
        for cname, members, exclude in cases:
            allowed = _allowed_by_set(labels, members, exclude)
            for radius in _radii_for(own, allowed, _own_radii)[1::3] + [float("inf")]:
                ctx = (dg.TYPE_NAMES[vt], lname, cname, radius)
                got = c.scan_within_labelset(dg.L2, q, radius, members, exclude=exclude)
                _assert_same(got, *_expected_allowed(own, allowed, radius), ctx=ctx)
                if cname == "empty":
                    assert got[2] == 0 and c.within_last_launches() == 0, ctx          # allows nothing: no launch
                if cname == "one":
                    _assert_same(c.scan_within_labeled(dg.L2, q, radius, 2), got[0], got[1].astype(np.float32), ctx=(ctx, "single label"))
    c.close()


def test_the_row_mask_is_neither_read_nor_written(pkg):
    c, q, own = _small(pkg)
    labels, _ = lc.layouts(N)["uniform5"]
    c.set_labels(labels)
    allowed = labels == 0
    radius = float(np.sort(own[allowed])[50])
    before = (c.scan_within_labeled(dg.L2, q, radius, 0), c.scan_within_labelset(dg.L2, q, radius, [0, 3], exclude=True))
    assert c.mask_count() == -1
    assert c.set_mask(bits=np.zeros(N, dtype=bool)) == 0          # an all-clear mask: a masked scan would return nothing
    assert c.scan_within_masked(dg.L2, q, float("inf"))[2] == 0
    after = (c.scan_within_labeled(dg.L2, q, radius, 0), c.scan_within_labelset(dg.L2, q, radius, [0, 3], exclude=True))
    for b, a in zip(before, after):
        assert len(b[0]) > 0
        _assert_same(a, b[0], b[1].astype(np.float32), matches=b[2])
    assert c.mask_count() == 0
    keep = np.arange(N) % 7 == 0
    assert c.set_mask(bits=keep) == int(keep.sum())
    _assert_same(c.scan_within_labeled(dg.L2, q, radius, 0), before[0][0], before[0][1].astype(np.float32))
    assert c.mask_count() == int(keep.sum())
    ids, dist = _expected_allowed(own, keep, radius)             # ... and the masked scan still sees its own mask, not the label's bitmap
    _assert_same(c.scan_within_masked(dg.L2, q, radius), ids, dist)
    c.close()


def test_the_held_result_and_overflow(pkg):
    c, q, own = _small(pkg)
    qs = lc.data(dg.U8, 3, 64, 72)
    labels, _ = lc.layouts(N)["uniform5"]
    c.set_labels(labels)
    allowed = labels == 3
    radius = float(np.sort(own[allowed])[200])
    ids, dist = _expected_allowed(own, allowed, radius)
    got = c.scan_within_labeled(dg.L2, q, radius, 3)
    _assert_same(got, ids, dist)
    assert c.within_last_launches() == 1
    keys = c.within_keys(len(ids))
    assert ((keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == ids.tolist()
    assert lc.error_code(pkg, lambda: c.within_keys(len(ids) + 1)) == VG_ERR_INVALID
    # a batch call in between holds its results elsewhere
    c.scan_within_batch_labeled(dg.L2, qs, [0, 3, 1], float("inf"))
    c.scan_within_batch(dg.L2, qs, 1.0)
    assert c.within_keys(len(ids)).tolist() == keys.tolist()
    # the next single range scan of any form overwrites it
    c.scan_within(dg.L2, q, float("-inf"))
    assert lc.error_code(pkg, lambda: c.within_keys(1)) == VG_ERR_INVALID
    # a device buffer too small for the label's matches: the complete answer, one more launch; the label's matches decide, not all rows'
    c.set_within_initial_capacity(64)
    try:
        _assert_same(c.scan_within_labeled(dg.L2, q, radius, 3), ids, dist)
        assert c.within_last_launches() == 2
        _assert_same(c.scan_within_labeled(dg.L2, q, radius, 3, limit=5), ids[:5], dist[:5], matches=len(ids))
        # the largest radius on one of the label's distances at which its matches still fit 64 keys - several times as many rows overall
        fit = float(max(v for v in np.unique(own[allowed]) if int(np.sum(allowed & (own <= v))) <= 64))
        few = _expected_allowed(own, allowed, fit)
        assert 0 < len(few[0]) <= 64 < int(np.sum(own <= np.float32(fit)))
        c.set_within_initial_capacity(64)                      # (drops the buffer the overflow grew)
        _assert_same(c.scan_within_labeled(dg.L2, q, fit, 3), *few)
        assert c.within_last_launches() == 1
    finally:
        c.set_within_initial_capacity(0)
    c.close()


# ------------------------------------------------------------------------------------------------- contract

def test_contract(pkg):
    L = pkg.lib()
    dim = 16
    rows = lc.data(dg.U8, N, dim, 90)
    q = lc.data(dg.U8, 1, dim, 91)[0]
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    labels, _ = lc.layouts(N)["uniform5"]
    set3 = np.array([3], dtype=np.uint32)

    def raw_label(h, metric, query, radius, label):
        m, held = pkg.C.c_int64(7), pkg.C.c_int64(7)
        rc = L.vg_scan_within_labeled(h, metric, query, radius, 0, label, pkg.C.byref(m), pkg.C.byref(held))
        return rc, m.value, held.value

    def raw_set(h, metric, query, radius, members, n):
        m, held = pkg.C.c_int64(7), pkg.C.c_int64(7)
        rc = L.vg_scan_within_labelset(h, metric, query, radius, 0, members, n, 0, pkg.C.byref(m), pkg.C.byref(held))
        return rc, m.value, held.value

    bad = (VG_ERR_INVALID, 0, 0)
    assert raw_label(c.h, dg.L2, pkg._ptr(q), 5.0, 3) == bad                               # no labels set
    assert raw_set(c.h, dg.L2, pkg._ptr(q), 5.0, pkg._ptr(set3), 1) == bad
    c.set_labels(labels)
    assert raw_label(c.h, dg.L2, pkg._ptr(q), 5.0, lc.NONE) == bad                         # NONE names no row
    assert raw_label(c.h, dg.L2, pkg._ptr(q), float("nan"), 3) == bad
    assert raw_set(c.h, dg.L2, pkg._ptr(q), float("nan"), pkg._ptr(set3), 1) == bad
    assert c.within_last_launches() == 0                                                  # refused before any launch
    assert raw_label(c.h, 99, pkg._ptr(q), 5.0, 3) == bad
    assert raw_set(c.h, 99, pkg._ptr(q), 5.0, pkg._ptr(set3), 1) == bad
    assert raw_label(c.h, dg.L2, None, 5.0, 3) == bad
    assert raw_label(None, dg.L2, pkg._ptr(q), 5.0, 3) == bad
    assert raw_set(c.h, dg.L2, None, 5.0, pkg._ptr(set3), 1) == bad
    assert raw_set(None, dg.L2, pkg._ptr(q), 5.0, pkg._ptr(set3), 1) == bad
    assert raw_set(c.h, dg.L2, pkg._ptr(q), 5.0, None, 1) == bad                           # a set of one label and no pointer
    assert raw_set(c.h, dg.L2, pkg._ptr(q), 5.0, pkg._ptr(set3), -1) == bad
    with_none = np.array([1, lc.NONE], dtype=np.uint32)
    assert raw_set(c.h, dg.L2, pkg._ptr(q), 5.0, pkg._ptr(with_none), 2) == bad             # NONE in a set names no row
    # out_matches / out_held may be NULL
    assert L.vg_scan_within_labeled(c.h, dg.L2, pkg._ptr(q), 1e9, 0, 3, None, None) == 0
    assert c.within_last_launches() == 1
    own = c.scan_distances(dg.L2, q)
    ids, dist = _expected_allowed(own, labels == 3, 1e9)
    assert len(c.within_keys(len(ids))) == len(ids) == int(np.sum(labels == 3))
    # tie_order does not matter
    c.set_tie_order(pkg.TIE_REFERENCE)
    _assert_same(c.scan_within_labeled(dg.L2, q, 1e9, 3), ids, dist)
    c.set_tie_order(pkg.TIE_POSITION)
    # a failed call leaves nothing held
    assert raw_label(c.h, dg.L2, pkg._ptr(q), float("nan"), 3) == bad
    assert lc.error_code(pkg, lambda: c.within_keys(1)) == VG_ERR_INVALID
    # labels cleared after use
    c.clear_labels()
    assert raw_label(c.h, dg.L2, pkg._ptr(q), 5.0, 3) == bad
    assert lc.error_code(pkg, lambda: c.scan_within_labelset(dg.L2, q, 5.0, [3])) == VG_ERR_INVALID
    _assert_same(c.scan_within(dg.L2, q, 1e9), *_expected(own, 1e9))                       # the plain range scan is not affected
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: zero counts, no launch
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert e.scan_within_labeled(dg.L2, q, 1e9, 3)[2] == 0 and e.within_last_launches() == 0
    assert e.scan_within_labelset(dg.L2, q, 1e9, [], exclude=True)[2] == 0 and e.within_last_launches() == 0
    e.close()
