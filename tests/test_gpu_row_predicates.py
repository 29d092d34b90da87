"""Row predicates: the labeled, the label-set and the valued scans share one bitmap builder and one host path (csrc/vg_rowpred.hip).

1. the three predicates, asked for the same rows, and the masked scan under a numpy-built mask of those rows answer identically
   (rowids equal, distances bit-equal) around the edges of the 64-row bitmap word;
2. the bitmap grid's stride step: 2^20 + 65 rows is the smallest corpus whose words outnumber the capped grid's wavefronts and that
   ends in a partial word;
3. the scratch buffers the forms share on a handle (bitmap, uploaded set, group tables) hold nothing stale from the call in front;
4. every refusal of every entry point of the three families: return code, message, zeroed counts, and the order of the checks.  The
   expected texts were written down from the sources as they were before the host paths were folded into one.
"""
import ctypes as C

import numpy as np
import pytest

import datagen as dg

pytestmark = pytest.mark.gpu

VG_OK, VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 0, 1, 5
NONE = 0xFFFFFFFF
DIM, K = 8, 5


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


def _rows(n, seed):
    return np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)


def _same(got, want, ctx):
    assert got[0].tolist() == want[0].tolist(), ctx
    assert np.asarray(got[1]).tobytes() == np.asarray(want[1]).tobytes(), ctx
    for a, b in zip(got[2:], want[2:]):
        assert np.asarray(a).tolist() == np.asarray(b).tolist(), ctx


# ------------------------------------------------------------------------------------------------- 1. agreement

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_predicates_agree_with_each_other_and_the_mask(pkg, n):
    rng = np.random.default_rng(700 + n)
    L = 1
    labels = rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint32), size=n)
    labels[-1] = L                                            # the final, partial word holds an allowed row
    values = np.where(labels == NONE, -5, labels.astype(np.int64)).astype(np.int64)      # -5: outside every queried interval
    q = _rows(1, 800 + n)[0]
    c = pkg.Corpus(dg.F32, DIM)
    c.append(_rows(n, 900 + n))
    c.set_labels(labels)
    c.set_values(values)

    c.set_mask(bits=(labels == L))
    want = c.scan_topk_masked(dg.L2, q, K)
    assert len(want[0]) == min(K, int(np.sum(labels == L)))
    _same(c.scan_topk_labeled(dg.L2, q, K, L), want, "labeled")
    _same(c.scan_topk_labelset(dg.L2, q, K, [L]), want, "labelset")
    _same(c.scan_topk_valued(dg.L2, q, K, L, L), want, "valued")
    _same(c.scan_topk_valued(dg.L2, q, K, None, None, label=L), want, "valued, label only")
    want = c.scan_topk_grouped(dg.L2, q, K, masked=True)
    _same(c.scan_topk_grouped_labelset(dg.L2, q, K, [L]), want, "grouped labelset")
    _same(c.scan_topk_grouped_valued(dg.L2, q, K, L, L), want, "grouped valued")
    want = c.scan_topk_capped(dg.L2, q, K, 2, masked=True)
    _same(c.scan_topk_capped_labelset(dg.L2, q, K, 2, [L]), want, "capped labelset")
    _same(c.scan_topk_capped_valued(dg.L2, q, K, 2, L, L), want, "capped valued")
    want = c.scan_within_masked(dg.L2, q, 1e9)
    assert want[2] == int(np.sum(labels == L))
    _same(c.scan_within_labeled(dg.L2, q, 1e9, L), want, "within labeled")
    _same(c.scan_within_labelset(dg.L2, q, 1e9, [L]), want, "within labelset")
    _same(c.scan_within_valued(dg.L2, q, 1e9, L, L), want, "within valued")

    other = (labels != L) & (labels != NONE)
    c.set_mask(bits=other)
    _same(c.scan_topk_labelset(dg.L2, q, K, [L], exclude=True), c.scan_topk_masked(dg.L2, q, K), "exclude")
    _same(c.scan_topk_grouped_labelset(dg.L2, q, K, [L], exclude=True), c.scan_topk_grouped(dg.L2, q, K, masked=True), "grouped exclude")
    _same(c.scan_topk_capped_labelset(dg.L2, q, K, 2, [L], exclude=True), c.scan_topk_capped(dg.L2, q, K, 2, masked=True), "capped exclude")
    _same(c.scan_within_labelset(dg.L2, q, 1e9, [L], exclude=True), c.scan_within_masked(dg.L2, q, 1e9), "within exclude")
    c.close()


# ------------------------------------------------------------------------------------------------- 2. the grid's stride step

def test_bitmap_grid_stride_and_partial_last_word(pkg):
    n = (1 << 20) + 65                                         # 4096 workgroups x 4 wavefronts cover 2^20 rows per step
    marked = [(1 << 20) - 1, 1 << 20, (1 << 20) + 64]
    labels = np.zeros(n, dtype=np.uint32)
    labels[marked] = 7
    c = pkg.Corpus(dg.F32, DIM)
    c.append(_rows(n, 31))
    c.set_labels(labels)
    c.set_values(labels.astype(np.int64))
    q = _rows(1, 32)[0]
    want = sorted(p + 1 for p in marked)                       # implicit rowids: position + 1
    assert sorted(c.scan_topk_labeled(dg.L2, q, K, 7)[0].tolist()) == want
    assert sorted(c.scan_topk_labelset(dg.L2, q, K, [7])[0].tolist()) == want
    assert sorted(c.scan_topk_valued(dg.L2, q, K, 7, 7)[0].tolist()) == want
    ids, _, matches = c.scan_within_labeled(dg.L2, q, 1e9, 7)
    assert matches == 3 and sorted(ids.tolist()) == want
    c.close()


# ------------------------------------------------------------------------------------------------- 3. shared scratch

def test_shared_scratch_across_forms_back_to_back(pkg):
    n, nq = 200, 40
    rng = np.random.default_rng(41)
    labels = rng.integers(0, 12, size=n).astype(np.uint32)
    labels[::17] = NONE
    values = rng.integers(-50, 50, size=n).astype(np.int64)
    qs = _rows(nq, 42)
    c = pkg.Corpus(dg.F32, DIM)
    c.append(_rows(n, 43))
    c.set_labels(labels)
    c.set_values(values)
    lab_ok = labels != NONE

    def batch_masked(allow_of_query):                          # query i under the mask of its own condition, one batch per distinct mask
        ids, dist, cnt = [None] * nq, [None] * nq, [0] * nq
        for key in sorted(set(k for k, _ in allow_of_query)):
            allow = next(a for k, a in allow_of_query if k == key)
            c.set_mask(bits=allow)
            i_, d_, c_ = c.scan_topk_batch_masked(dg.L2, qs, K)
            for i, (k, _) in enumerate(allow_of_query):
                if k == key:
                    ids[i], dist[i], cnt[i] = i_[i, :c_[i]], d_[i, :c_[i]], int(c_[i])
        return ids, dist, cnt

    def check_batch(got, allow_of_query, ctx):
        ids, dist, cnt = batch_masked(allow_of_query)
        for i in range(nq):
            assert int(got[2][i]) == cnt[i], (ctx, i)
            _same((got[0][i, :cnt[i]], got[1][i, :cnt[i]]), (ids[i], dist[i]), (ctx, i))

    def check_single(got, allow, ctx, within=False):
        c.set_mask(bits=allow)
        _same(got, c.scan_within_masked(dg.L2, qs[0], 1e9) if within else c.scan_topk_masked(dg.L2, qs[0], K), ctx)

    sets3 = [[0, 1, 2], [3, 4], [5, 6, 7, 8]]
    qsets = [sets3[i % 3] for i in range(nq)]
    got = c.scan_topk_batch_labelset(dg.L2, qs, qsets, K)                              # 1: group tables into the set scratch
    check_batch(got, [(i % 3, np.isin(labels, sets3[i % 3])) for i in range(nq)], "batch labelset")
    s5 = [9, 10, 11, 0, 3]
    check_single(c.scan_topk_labelset(dg.L2, qs[0], K, s5), np.isin(labels, s5), "labelset")            # 2
    los = [(-40, -10), (0, 30)]
    got = c.scan_topk_batch_valued(dg.L2, qs, [los[i % 2][0] for i in range(nq)], [los[i % 2][1] for i in range(nq)], K)   # 3
    check_batch(got, [(i % 2, (values >= los[i % 2][0]) & (values <= los[i % 2][1])) for i in range(nq)], "batch valued")
    check_single(c.scan_topk_valued(dg.L2, qs[0], K, 31, 49), (values >= 31) & (values <= 49), "valued")   # 4
    check_single(c.scan_topk_labeled(dg.L2, qs[0], K, 6), lab_ok & (labels == 6), "labeled")               # 5
    check_single(c.scan_within_valued(dg.L2, qs[0], 1e9, -50, -41), (values >= -50) & (values <= -41), "within valued", within=True)   # 6
    c.close()


# ------------------------------------------------------------------------------------------------- 4. refusals

NQ = 3
_SET = np.array([1, 2], dtype=np.uint32)
_SET_NONE = np.array([1, NONE], dtype=np.uint32)
_DEFAULTS = dict(metric=dg.L2, k=K, label=1, set=_SET, nset=2, lo=0, hi=2, per_label=2, radius=1e9, qlabels=True)


def _entry_points(pkg):
    """name -> (who, noun, kind, features, call(h, p) -> (rc, counts))"""
    L = pkg.lib()
    q = _rows(1, 51)[0]
    qs = _rows(NQ, 52)

    def outs(kind):
        ids, dist = np.zeros(64 * NQ, dtype=np.int64), np.zeros(64 * NQ, dtype=np.float64)
        keys, labs = np.zeros(64 * NQ, dtype=np.uint64), np.zeros(64 * NQ, dtype=np.uint32)
        return {"r": [ids, dist], "rl": [ids, dist, labs], "k": [keys], "kl": [keys, labs]}[kind]

    def single(fn, kind, args):
        def call(h, p):
            cnt = C.c_int(7)
            rc = getattr(L, fn)(h, p["metric"], pkg._ptr(q), p["k"], *args(p), *[pkg._ptr(o) for o in outs(kind)], C.byref(cnt))
            return rc, [cnt.value]
        return call

    def within(fn, args):
        def call(h, p):
            m, held = C.c_int64(7), C.c_int64(7)
            rc = getattr(L, fn)(h, p["metric"], pkg._ptr(q), p["radius"], 0, *args(p), C.byref(m), C.byref(held))
            return rc, [m.value, held.value]
        return call

    setargs = lambda p: (pkg._ptr(p["set"]), p["nset"], 0)
    eps = {}
    for sfx, kr, kl in (("", "r", "rl"), ("_keys", "k", "kl")):
        def add(name, noun, feats, kind, args):
            eps[name + sfx] = (name, noun, "topk", feats, single(name + sfx, kind, args))
        add("vg_scan_topk_labeled", "labeled", {"labels", "label"}, kr, lambda p: (p["label"],))
        add("vg_scan_topk_labelset", "label-set", {"labels", "set"}, kr, setargs)
        add("vg_scan_topk_grouped_labelset", "label-set", {"labels", "set"}, kl, setargs)
        add("vg_scan_topk_capped_labelset", "label-set", {"labels", "set", "cap"}, kl, lambda p: (p["per_label"],) + setargs(p))
        add("vg_scan_topk_valued", "valued", {"values"}, kr, lambda p: (p["lo"], p["hi"]))
        add("vg_scan_topk_valued_labeled", "valued", {"values", "labels", "label"}, kr, lambda p: (p["lo"], p["hi"], p["label"]))
        add("vg_scan_topk_grouped_valued", "valued", {"values", "labels"}, kl, lambda p: (p["lo"], p["hi"]))
        add("vg_scan_topk_capped_valued", "valued", {"values", "labels", "cap"}, kl, lambda p: (p["per_label"], p["lo"], p["hi"]))
    eps["vg_scan_within_labeled"] = ("vg_scan_within_labeled", "labeled", "within", {"labels", "label"}, within("vg_scan_within_labeled", lambda p: (p["label"],)))
    eps["vg_scan_within_labelset"] = ("vg_scan_within_labelset", "label-set", "within", {"labels", "set"}, within("vg_scan_within_labelset", setargs))
    eps["vg_scan_within_valued"] = ("vg_scan_within_valued", "valued", "within", {"values"}, within("vg_scan_within_valued", lambda p: (p["lo"], p["hi"])))

    def batch(fn, mid):
        def call(h, p):
            cnt = np.full(NQ, 7, dtype=np.int32)
            ids, dist = outs("r")
            rc = getattr(L, fn)(h, p["metric"], pkg._ptr(qs), NQ, *mid(p), pkg._ptr(ids), pkg._ptr(dist), pkg._ptr(cnt))
            return rc, cnt.tolist()
        return call

    qlab = lambda p: np.full(NQ, p["label"], dtype=np.uint32)

    def bset(p):                                               # every query the same set; nset < 0: offsets that decrease
        n = p["nset"]
        return (p["k"], pkg._ptr(np.tile(p["set"], NQ)), pkg._ptr(np.arange(NQ + 1, dtype=np.int64) * n), 0)

    def bval(p):
        lab = qlab(p) if p["qlabels"] else None
        return (p["k"], pkg._ptr(np.full(NQ, p["lo"], dtype=np.int64)), pkg._ptr(np.full(NQ, p["hi"], dtype=np.int64)), None if lab is None else pkg._ptr(lab))

    eps["vg_scan_topk_batch_labeled"] = ("vg_scan_topk_batch_labeled", "labeled", "topk", {"labels", "qlabel"}, batch("vg_scan_topk_batch_labeled", lambda p: (pkg._ptr(qlab(p)), p["k"])))
    eps["vg_scan_topk_batch_labelset"] = ("vg_scan_topk_batch_labelset", "label-set", "topk", {"labels", "set", "offsets"}, batch("vg_scan_topk_batch_labelset", bset))
    eps["vg_scan_topk_batch_valued"] = ("vg_scan_topk_batch_valued", "valued", "topk", {"values", "labels", "qlabel"}, batch("vg_scan_topk_batch_valued", bval))

    def wbatch(h, p):
        m, held = np.full(NQ, 7, dtype=np.int64), np.full(NQ, 7, dtype=np.int64)
        rc = L.vg_scan_within_batch_labeled(h, p["metric"], pkg._ptr(qs), NQ, pkg._ptr(qlab(p)), pkg._ptr(np.full(NQ, p["radius"], dtype=np.float64)), 0,
                                            pkg._ptr(m), pkg._ptr(held))
        return rc, m.tolist() + held.tolist()
    eps["vg_scan_within_batch_labeled"] = ("vg_scan_within_batch_labeled", "labeled", "wbatch", {"labels", "wlabel"}, wbatch)
    return eps


# (case, which entry points, overrides, handle, rc, message) - `w`: the name messages carry, `n`: the noun
_NAN = float("nan")
_CASES = [
    ("k = 0", lambda k, f: k == "topk", dict(k=0), "full", VG_ERR_INVALID, lambda w, n, f: "%s: k must be at least 1" % w),
    ("k = 65", lambda k, f: k == "topk", dict(k=65), "full", VG_ERR_UNSUPPORTED, lambda w, n, f: "%s: k must be in 1..64 (%s scans use the fused list only)" % (w, n)),
    ("k = 65, unknown metric", lambda k, f: k == "topk", dict(k=65, metric=99), "full", VG_ERR_UNSUPPORTED,
     lambda w, n, f: "%s: k must be in 1..64 (%s scans use the fused list only)" % (w, n)),
    ("unknown metric", lambda k, f: True, dict(metric=99), "full", VG_ERR_INVALID, lambda w, n, f: "unknown distance metric 99"),
    ("unknown metric, no labels", lambda k, f: "labels" in f, dict(metric=99), "nolabels", VG_ERR_INVALID, lambda w, n, f: "unknown distance metric 99"),
    ("no labels", lambda k, f: "labels" in f, dict(), "nolabels", VG_ERR_INVALID, lambda w, n, f: "%s: no labels set" % w),
    ("no values", lambda k, f: "values" in f, dict(), "novalues", VG_ERR_INVALID, lambda w, n, f: "%s: no values set" % w),
    ("no values, no labels", lambda k, f: "values" in f and "labels" in f, dict(), "neither", VG_ERR_INVALID, lambda w, n, f: "%s: no values set" % w),
    ("LABEL_NONE", lambda k, f: "label" in f, dict(label=NONE), "full", VG_ERR_INVALID, lambda w, n, f: "%s: VG_LABEL_NONE names no row" % w),
    ("LABEL_NONE, a query's", lambda k, f: "qlabel" in f, dict(label=NONE), "full", VG_ERR_INVALID, lambda w, n, f: "%s: query 0: VG_LABEL_NONE names no row" % w),
    ("LABEL_NONE, a range query's", lambda k, f: "wlabel" in f, dict(label=NONE), "full", VG_ERR_INVALID,
     lambda w, n, f: "%s: a query's label is VG_LABEL_NONE, which names no row" % w),
    ("LABEL_NONE in a set", lambda k, f: "set" in f, dict(set=_SET_NONE), "full", VG_ERR_INVALID, lambda w, n, f: "%s: VG_LABEL_NONE names no row" % w),
    ("a negative set count", lambda k, f: "set" in f, dict(nset=-1), "full", VG_ERR_INVALID,
     lambda w, n, f: ("%s: set_offsets decrease at query 0" if "offsets" in f else "%s: bad label-set pointer / count") % w),
    ("per_label = 0", lambda k, f: "cap" in f, dict(per_label=0), "full", VG_ERR_INVALID, lambda w, n, f: "%s: per_label must be at least 1" % w),
    ("a NaN radius", lambda k, f: k == "within", dict(radius=_NAN), "full", VG_ERR_INVALID, lambda w, n, f: "%s: the radius is NaN" % w),
    ("a NaN radius, batch", lambda k, f: k == "wbatch", dict(radius=_NAN), "full", VG_ERR_INVALID, lambda w, n, f: "%s: radius 0 is NaN" % w),
    ("lo > hi", lambda k, f: "values" in f, dict(lo=3, hi=2), "full", VG_OK, None),
    ("an empty set", lambda k, f: "set" in f, dict(nset=0), "full", VG_OK, None),
]


def test_refusals(pkg):
    n = 65
    rng = np.random.default_rng(61)
    labels = rng.integers(0, 3, size=n).astype(np.uint32)
    handles = {}
    for name, lab, val in (("full", True, True), ("nolabels", False, True), ("novalues", True, False), ("neither", False, False)):
        c = pkg.Corpus(dg.F32, DIM)
        c.append(_rows(n, 62))
        if lab:
            c.set_labels(labels)
        if val:
            c.set_values(labels.astype(np.int64))
        handles[name] = c
    L = pkg.lib()
    eps = _entry_points(pkg)
    assert len(eps) == 23
    ran = 0
    for case, applies, over, handle, want_rc, message in _CASES:
        for name, (who, noun, kind, feats, call) in eps.items():
            if not applies(kind, feats):
                continue
            c = handles[handle]
            if kind == "within":
                c.scan_within(dg.L2, _rows(1, 63)[0], 1e9)            # something held, a launch counted: the call must drop both
                assert c.within_last_launches() == 1
            rc, counts = call(c.h, dict(_DEFAULTS, **over))
            ctx = (case, name)
            assert rc == want_rc, ctx + (L.vg_last_error().decode(),)
            assert all(x == 0 for x in counts), ctx + (counts,)
            if message is not None:
                assert L.vg_last_error().decode() == message(who, noun, feats), ctx
            if kind == "within":
                assert c.within_last_launches() == 0, ctx
                ids, dist = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float64)
                assert L.vg_scan_within_fetch(c.h, 0, 1, pkg._ptr(ids), pkg._ptr(dist)) == VG_ERR_INVALID, ctx
            ran += 1
    assert ran > 150
    # the entry points answer a well-formed call
    for name, (who, noun, kind, feats, call) in eps.items():
        rc, counts = call(handles["full"].h, dict(_DEFAULTS))
        assert rc == VG_OK and counts[0] > 0, (name, rc, counts)
    for c in handles.values():
        c.close()
