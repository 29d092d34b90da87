"""Value-range scans, single forms (vg_scan_topk_valued, _valued_labeled, _grouped_valued, _capped_valued, vg_scan_within_valued): an
int64 per row on the handle, a query names the closed interval [lo, hi] its rows' values must lie in.

Contract (include/vectorgpu.h): the masked scans' over the allowed rows.  Every answer is checked twice: against the handle's own
scan_distances filtered on the host by valued_cases.allowed (test_valued_cases.py pins that rule), and bit for bit against the masked
twin - the same kernels under a user mask holding exactly the allowed rows.  Layouts and intervals: valued_cases (unsigned, one-word
and signed-low-word compares all give wrong rows on one of them); 3001 rows, every shape of labeled_cases, k in (1, 20, 64).
"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
import valued_cases as vc

pytestmark = pytest.mark.gpu

VG_OK, VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 0, 1, 5
KS = (1, 20, 64)


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


def _same3(got, want, ctx):
    lc.assert_same(got[:2], *want[:2], ctx=ctx)
    assert got[2].tolist() == want[2].tolist(), ctx


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    rows = lc.data(vt, n, dim, 61 + dim)
    q = lc.data(vt, 1, dim, 62 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    assert not c.has_values()
    lay = vc.layouts(n)
    for mi, metric in enumerate(metrics):
        own = c.scan_distances(metric, q)
        # every layout x interval under the first metric; the others: the two layouts an unsigned / a one-word compare gets wrong
        for lname in (list(lay) if mi == 0 else ["extremes", "low_word_only"]):
            values = lay[lname]
            c.set_values(values)
            assert c.has_values()
            for iname, (lo, hi) in vc.intervals(values).items():
                allow = vc.allowed(values, lo, hi)
                c.set_mask(bits=allow)
                for k in (KS if iname in ("full", "on_present", "fewer_than_k") else (20,)):
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, iname, k)
                    got = c.scan_topk_valued(metric, q, k, lo, hi)
                    lc.assert_same(got, *lc.expected(own, allow, k), ctx=ctx)
                    lc.assert_same(got, *c.scan_topk_masked(metric, q, k), ctx=ctx + ("masked twin",))
            # None is the open end
            a = vc.intervals(values)["on_present"][0]
            lc.assert_same(c.scan_topk_valued(metric, q, 20, None, a), *lc.expected(own, vc.allowed(values, None, a), 20), ctx=(lname, "open lo"))
            lc.assert_same(c.scan_topk_valued(metric, q, 20, a, None), *lc.expected(own, vc.allowed(values, a, None), 20), ctx=(lname, "open hi"))
    c.close()


@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_conjunction_grouped_capped_and_within(pkg, vt, dim, per_pass, metrics):
    n = lc.N
    metric = metrics[0]
    rows = lc.data(vt, n, dim, 63 + dim)
    q = lc.data(vt, 1, dim, 64 + dim)[0]
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    own = c.scan_distances(metric, q)
    with np.errstate(invalid="ignore"):
        finite = own < np.inf                                    # (NaN and +Inf never match)
    radius = float(np.sort(own[finite])[n // 3])
    lay = vc.layouts(n)
    for lname, labname in (("random", "uniform5"), ("extremes", "some_none"), ("sorted", "runs200")):
        values = lay[lname]
        labels, asked = lc.layouts(n)[labname]
        c.set_values(values)
        c.set_labels(labels)
        iv = vc.intervals(values)
        for iname in ("full", "on_present", "on_present_shrunk", "none_inside", "lo_above_hi", "across_zero") + (("fewer_than_k",) if "fewer_than_k" in iv else ()):
            lo, hi = iv[iname]
            allow = vc.allowed(values, lo, hi)
            for k in (KS if iname == "on_present" else (20,)):
                ctx = (dg.TYPE_NAMES[vt], dim, lname, labname, iname, k)
                # the conjunction with one label
                for label in asked:
                    both = vc.allowed(values, lo, hi, labels, label)
                    got = c.scan_topk_valued(metric, q, k, lo, hi, label=label)
                    lc.assert_same(got, *lc.expected(own, both, k), ctx=ctx + (label,))
                    c.set_mask(bits=both)
                    lc.assert_same(got, *c.scan_topk_masked(metric, q, k), ctx=ctx + (label, "masked twin"))
                # filter by value, group by label: the masked grouped / capped scans under that bitmap; per_label = 1 is the grouped form
                c.set_mask(bits=allow)
                grouped = c.scan_topk_grouped_valued(metric, q, k, lo, hi)
                _same3(grouped, c.scan_topk_grouped(metric, q, k, masked=True), ctx + ("grouped",))
                _same3(c.scan_topk_capped_valued(metric, q, k, 1, lo, hi), grouped, ctx + ("capped 1",))
                for m in (2, 64):
                    _same3(c.scan_topk_capped_valued(metric, q, k, m, lo, hi), c.scan_topk_capped(metric, q, k, m, masked=True), ctx + ("capped", m))
                assert (labels[grouped[0] - 1] == grouped[2]).all() and allow[grouped[0] - 1].all(), ctx
            # the range form: the masked range scan under that bitmap, with and without a limit below the matches
            want = c.scan_within_masked(metric, q, radius)
            got = c.scan_within_valued(metric, q, radius, lo, hi)
            lc.assert_same(got[:2], *want[:2], ctx=(lname, iname, "within"))
            assert got[2] == want[2] == int((allow & finite & (own.astype(np.float64) <= radius)).sum()), (lname, iname)
            if want[2] > 3:
                lim = want[2] // 2
                cut = c.scan_within_valued(metric, q, radius, lo, hi, limit=lim)
                assert cut[2] == want[2] and len(cut[0]) == lim, (lname, iname)
                lc.assert_same(cut[:2], want[0][:lim], want[1][:lim], ctx=(lname, iname, "within limit"))
            everything = c.scan_within_valued(metric, q, np.inf, lo, hi)
            assert everything[2] == int((allow & finite).sum()), (lname, iname)            # closed ends: the count is the host rule's
    c.close()


def test_user_mask_and_labels_are_left_alone(pkg):
    n, dim = lc.N, 64
    rows = lc.data(dg.U8, n, dim, 71)
    q = lc.data(dg.U8, 1, dim, 72)[0]
    values = vc.layouts(n)["random"]
    labels = lc.layouts(n)["uniform5"][0]
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    c.set_values(values)
    c.set_labels(labels)
    mine = np.random.default_rng(7).random(n) < 0.2
    c.set_mask(bits=mine)
    before = c.scan_topk_masked(dg.L2, q, 20)
    lo, hi = vc.intervals(values)["across_zero"]
    c.scan_topk_valued(dg.L2, q, 20, lo, hi)
    c.scan_topk_valued(dg.L2, q, 20, lo, hi, label=3)
    c.scan_topk_grouped_valued(dg.L2, q, 20, lo, hi)
    c.scan_topk_capped_valued(dg.L2, q, 20, 2, lo, hi)
    c.scan_within_valued(dg.L2, q, 1e9, lo, hi)
    c.scan_topk_batch_valued(dg.L2, np.stack([q, q, q]), [lo, 1, lo], [hi, 0, hi], 20)
    assert c.mask_count() == int(mine.sum()) and c.has_labels() and c.has_values()
    lc.assert_same(c.scan_topk_masked(dg.L2, q, 20), *before)
    # values and mask do not combine: a valued scan answers over rows the mask leaves out
    own = c.scan_distances(dg.L2, q)
    lc.assert_same(c.scan_topk_valued(dg.L2, q, 20, lo, hi), *lc.expected(own, vc.allowed(values, lo, hi), 20))
    # clear_values: the values are gone, labels and mask are not
    c.clear_values()
    assert not c.has_values() and c.has_labels() and c.mask_count() == int(mine.sum())
    assert lc.error_code(pkg, lambda: c.scan_topk_valued(dg.L2, q, 20, lo, hi)) == VG_ERR_INVALID
    c.close()


def test_contract_and_error_codes(pkg):
    n, dim = 2001, 64
    rows = lc.data(dg.U8, n, dim, 81)
    q = lc.data(dg.U8, 1, dim, 82)[0]
    values = np.arange(n, dtype=np.int64) - 1000
    labels = (np.arange(n) % 3).astype(np.uint32)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    c.set_labels(labels)
    # no values set: every form refuses
    for call in (lambda: c.scan_topk_valued(dg.L2, q, 5, 0, 9), lambda: c.scan_topk_valued(dg.L2, q, 5, 0, 9, label=1),
                 lambda: c.scan_topk_grouped_valued(dg.L2, q, 5, 0, 9), lambda: c.scan_topk_capped_valued(dg.L2, q, 5, 2, 0, 9),
                 lambda: c.scan_within_valued(dg.L2, q, 1e9, 0, 9)):
        assert lc.error_code(pkg, call) == VG_ERR_INVALID
    with pytest.raises(pkg.VectorGpuError):
        c.set_values(values[:-1])                                # n must equal the rows held
    assert not c.has_values()
    c.set_values(values)
    c.clear_labels()
    # no labels: the plain and the range form answer, the labeled, grouped and capped forms refuse
    assert len(c.scan_topk_valued(dg.L2, q, 5, 0, 9)[0]) == 5 and c.scan_within_valued(dg.L2, q, 1e9, 0, 9)[2] == 10
    for call in (lambda: c.scan_topk_valued(dg.L2, q, 5, 0, 9, label=1), lambda: c.scan_topk_grouped_valued(dg.L2, q, 5, 0, 9),
                 lambda: c.scan_topk_capped_valued(dg.L2, q, 5, 2, 0, 9)):
        assert lc.error_code(pkg, call) == VG_ERR_INVALID
    c.set_labels(labels)
    for k, code in ((0, VG_ERR_INVALID), (-1, VG_ERR_INVALID), (65, VG_ERR_UNSUPPORTED)):
        assert lc.error_code(pkg, lambda: c.scan_topk_valued(dg.L2, q, k, 0, 9)) == code
        assert lc.error_code(pkg, lambda: c.scan_topk_valued(dg.L2, q, k, 0, 9, label=1)) == code
        assert lc.error_code(pkg, lambda: c.scan_topk_grouped_valued(dg.L2, q, k, 0, 9)) == code
        assert lc.error_code(pkg, lambda: c.scan_topk_capped_valued(dg.L2, q, k, 2, 0, 9)) == code
    assert lc.error_code(pkg, lambda: c.scan_topk_valued(dg.L2, q, 5, 0, 9, label=lc.NONE)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_capped_valued(dg.L2, q, 5, 0, 0, 9)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_topk_valued(99, q, 5, 0, 9)) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_within_valued(dg.L2, q, float("nan"), 0, 9)) == VG_ERR_INVALID
    with pytest.raises(ValueError):
        c.scan_topk_valued(dg.L2, q, 5, 0, 1 << 63)              # a bound is an int64
    # lo > hi: VG_OK, nothing; fewer than k rows inside: all of them; tie_order does not matter
    assert len(c.scan_topk_valued(dg.L2, q, 5, 1, 0)[0]) == 0 and c.scan_within_valued(dg.L2, q, 1e9, 1, 0)[2] == 0
    ids, dist = c.scan_topk_valued(dg.L2, q, 20, -3, 3)
    assert sorted(ids.tolist()) == list(range(998, 1005))
    c.set_tie_order(pkg.TIE_REFERENCE)
    lc.assert_same(c.scan_topk_valued(dg.L2, q, 20, -3, 3), ids, dist)
    c.set_tie_order(pkg.TIE_POSITION)
    # through the C symbols: NULLs are VG_ERR_INVALID and the count is zeroed first
    lib = pkg.lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    oi, od, ol, ok = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.float64), np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint64)
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_valued(c.h, dg.L2, None, 5, 0, 9, ptr(oi), ptr(od), C.byref(cnt)) == VG_ERR_INVALID      # (as vg_scan_topk_labelset: a NULL query is refused first)
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_valued(c.h, dg.L2, ptr(q), 5, 0, 9, None, ptr(od), C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    assert lib.vg_scan_topk_valued(c.h, dg.L2, ptr(q), 5, 0, 9, ptr(oi), ptr(od), None) == VG_ERR_INVALID
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_valued_keys(c.h, dg.L2, ptr(q), 5, 0, 9, None, C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_valued_labeled(c.h, dg.L2, ptr(q), 5, 0, 9, 1, ptr(oi), None, C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_grouped_valued(c.h, dg.L2, ptr(q), 5, 0, 9, ptr(oi), ptr(od), None, C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_capped_valued(c.h, dg.L2, ptr(q), 5, 0, 0, 9, ptr(oi), ptr(od), ptr(ol), C.byref(cnt)) == VG_ERR_INVALID and cnt.value == 0
    cnt = C.c_int(9)
    assert lib.vg_scan_topk_capped_valued_keys(c.h, dg.L2, ptr(q), 65, 2, 0, 9, ptr(ok), ptr(ol), C.byref(cnt)) == VG_ERR_UNSUPPORTED and cnt.value == 0
    m, h = C.c_int64(9), C.c_int64(9)
    assert lib.vg_scan_within_valued(c.h, dg.L2, None, 1e9, 0, 0, 9, C.byref(m), C.byref(h)) == VG_ERR_INVALID and m.value == 0 and h.value == 0
    assert lib.vg_corpus_set_values(c.h, None, n) == VG_ERR_INVALID and lib.vg_corpus_set_values(None, ptr(values), n) == VG_ERR_INVALID
    assert c.has_values()                                        # (a refused call before the upload leaves the values)
    # the _keys twins: the rows form's answer as packed keys over local positions
    cnt = C.c_int(0)
    assert lib.vg_scan_topk_valued_keys(c.h, dg.L2, ptr(q), 20, -3, 3, ptr(ok), C.byref(cnt)) == VG_OK and cnt.value == 7
    assert [int(x) & 0xFFFFFFFF for x in ok[:7]] == [int(i) - 1 for i in ids]
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: count 0
    e.set_values(np.zeros(0, dtype=np.int64))
    e.set_labels(np.zeros(0, dtype=np.uint32))
    assert len(e.scan_topk_valued(dg.L2, q, 5, None, None)[0]) == 0 and len(e.scan_topk_grouped_valued(dg.L2, q, 5, None, None)[0]) == 0
    assert e.scan_within_valued(dg.L2, q, 1e9, None, None)[2] == 0
    e.close()
