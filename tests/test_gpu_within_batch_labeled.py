"""Labeled batch range scans (vg_scan_within_batch_labeled): many queries, each its own label and its own radius, through the binding.

Contract (include/vectorgpu.h): query i's answer is what scan_within_labeled is contracted to return for (q_i, radii[i], labels[i]),
at the caller's index i; a query whose label is LABEL_NONE refuses the whole call, as in scan_topk_batch_labeled.

  * every shape of labeled_cases.SHAPES: the plan's queries per pass (no instance of the labeled range form is left out: DESIGN.md
    3.21), every query equal to scan_within_labeled for it alone - bit for bit and count for count, where the batch runs the single
    scan's lane decomposition (uint8 / int8 sums are integers: always; the fallback shapes ARE the single scans) - and, uint8 / int8,
    to the pinned CPU oracle's distances restricted to the label's rows here.  An f32 shape whose batch runs another lane decomposition
    than the single scan is held to scan_within_batch with the same radii restricted to the label's rows instead: the same floats;
  * nine queries (ragged against 4 and 2 per pass) whose labels mix inside a pass, one naming an absent label; radii rotated over the
    queries, -Inf and +Inf side by side; the launch count; overflow (only the overflowed pass runs again; which queries share a pass
    follows from the label order); a batch larger than a staging slice in random label order; rows without a label; logical shards
    == one corpus for the three labeled range forms; the contract's errors.
"""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
from test_gpu_within import _assert_same, _expected, _own_radii, _radii_at_ranks

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1
N, NQ = lc.N, 9                                                # 9 queries: ragged against 4 and against 2 per pass


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


def _passes(nq, per_pass):
    return (nq + per_pass - 1) // per_pass


def _expected_allowed(dist, allowed, radius, rowids=None):
    d = np.where(np.asarray(allowed, dtype=bool), np.asarray(dist, dtype=np.float32), np.float32(np.nan))
    return _expected(d, radius, rowids)


def _radii_for(dist, allowed, pick):
    if not allowed.any():
        return [float(np.max(dist[np.isfinite(dist)])), float("inf")]
    return pick(dist[allowed])


def _query_labels(asked):
    """nine labels in no order: 5 + 3 (or 3 + 3 + 2) of the layout's labels and the absent one, so that cut into passes of 4 and of 2
    BY LABEL some pass holds two labels"""
    a = [x for x in asked if x != lc.ABSENT]
    pat = [0, 1, 0, 1, None, 0, 1, 0, 0] if len(a) == 2 else [2, 1, 0, 1, None, 0, 2, 1, 0]
    return np.array([lc.ABSENT if j is None else a[j] for j in pat], dtype=np.uint32)


def _label_order(ql):
    return np.argsort(ql, kind="stable")


def _some_pass_mixes(ql, per_pass):
    s = ql[_label_order(ql)]
    return any(len(set(s[g:g + per_pass].tolist())) > 1 for g in range(0, len(s), per_pass))


# ------------------------------------------------------------------------------------------------- every shape

@pytest.mark.parametrize("vt,dim,per_pass,metrics", lc.SHAPES, ids=lc.SHAPE_IDS)
def test_every_shape(pkg, orc, vt, dim, per_pass, metrics):
    rows = lc.data(vt, N, dim, 131 + dim)
    qs = lc.data(vt, NQ, dim, 132 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    ints = vt in (dg.U8, dg.I8)
    for metric in metrics:
        plan = c.within_batch_labeled_plan(metric)
        assert plan == pkg.within_batch_labeled_plan(c, metric)
        assert plan[0] == per_pass, (dim, metric)                  # no instance left out
        assert plan == pkg.within_batch_plan(c, metric), (dim, metric)      # one launch shape with the other batch range scans
        # the single scan's lane decomposition: its floats are the batch's
        exact = ints or per_pass == 0 or plan[1:] == pkg.plan_scan_shape(vt, dim, metric)[:2]
        base = [orc.scan_distances(orc.AVX2, metric, vt, qs[i], rows) if ints else c.scan_distances(metric, qs[i]) for i in range(NQ)]
        for lname, (labels, asked) in lc.layouts(N).items():
            c.set_labels(labels)
            ql = _query_labels(asked)
            assert lc.ABSENT in ql and (lname != "last_row_only" or 9 in ql)
            assert per_pass == 0 or _some_pass_mixes(ql, per_pass), (lname, per_pass)
            allowed = [labels == ql[i] for i in range(NQ)]
            per_query = [_radii_for(base[i], allowed[i], _radii_at_ranks if ints else _own_radii) for i in range(NQ)]
            rounds = [[per_query[i][(i + rnd) % len(per_query[i])] for i in range(NQ)] for rnd in (0, 1, 4)]
            side_by_side = np.zeros(NQ)                          # -Inf and +Inf next to each other in every pass
            side_by_side[_label_order(ql)] = [float("-inf") if j % 2 == 0 else float("inf") for j in range(NQ)]
            rounds.append(side_by_side.tolist())
            for rnd, radii in enumerate(rounds):
                res = c.scan_within_batch_labeled(metric, qs, ql, radii)
                assert len(res) == NQ
                if per_pass:
                    assert c.within_batch_last_launches() == _passes(NQ, per_pass)
                unlabeled = None if exact else c.scan_within_batch(metric, qs, radii)
                for i in range(NQ):
                    ctx = (dg.TYPE_NAMES[vt], dim, dg.METRIC_NAMES[metric], lname, rnd, i, int(ql[i]), radii[i])
                    assert (labels[res[i][0] - 1] == ql[i]).all(), ctx          # (a row without a label never appears)
                    if ints:
                        _assert_same(res[i], *_expected_allowed(base[i], allowed[i], radii[i]), ctx=(ctx, "oracle"))
                    if exact:
                        single = c.scan_within_labeled(metric, qs[i], radii[i], int(ql[i]))
                        _assert_same(res[i], single[0], single[1].astype(np.float32), matches=single[2], ctx=(ctx, "single"))
                    else:
                        keep = allowed[i][unlabeled[i][0] - 1]
                        _assert_same(res[i], unlabeled[i][0][keep], unlabeled[i][1][keep].astype(np.float32), ctx=(ctx, "batch, restricted"))
                    if rnd == 3:
                        assert res[i][2] == (0 if radii[i] < 0 else int(allowed[i].sum())), ctx
            if lname == "uniform5":                              # a limit cuts the held result, the count stays
                radii = rounds[1]
                full = c.scan_within_batch_labeled(metric, qs, ql, radii)
                for limit in (1, 7):
                    res = c.scan_within_batch_labeled(metric, qs, ql, radii, limit=limit)
                    for i in range(NQ):
                        _assert_same(res[i], full[i][0][:limit], full[i][1][:limit].astype(np.float32), matches=full[i][2], ctx=(dim, metric, i, "limit", limit))
    c.close()


def test_a_fallback_batch_keeps_the_single_scans_held_result(pkg):
    vt, dim = dg.F16, 384
    rows = lc.data(vt, N, dim, 141)
    qs = lc.data(vt, NQ, dim, 142)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    labels, asked = lc.layouts(N)["uniform5"]
    c.set_labels(labels)
    assert c.within_batch_labeled_plan(dg.L2)[0] == 0
    single = c.scan_within_labeled(dg.L2, qs[0], float("inf"), 3)
    keys = c.within_keys(len(single[0]))
    launches = c.within_last_launches()
    res = c.scan_within_batch_labeled(dg.L2, qs, _query_labels(asked), float("inf"))
    assert sum(r[2] for r in res) > 0
    assert c.within_keys(len(single[0])).tolist() == keys.tolist() and c.within_last_launches() == launches
    c.close()


# ------------------------------------------------------------------------------------------------- overflow

@pytest.mark.parametrize("vt,dim", [(dg.U8, 64), (dg.F32, 384), (dg.F32, 1536)])
def test_only_the_overflowed_pass_runs_again(pkg, vt, dim):
    rows = lc.data(vt, N, dim, 151 + dim)
    qs = lc.data(vt, NQ, dim, 152 + dim)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    metric = dg.L2
    per_pass, lpr, u = c.within_batch_labeled_plan(metric)
    assert per_pass in (2, 4)
    if vt == dg.F32 and (lpr, u) != pkg.plan_scan_shape(vt, dim, metric)[:2]:
        own = None                                               # another lane decomposition than the stream's: the unlabeled batch is the reference
    else:
        own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
    labels = (np.arange(N) % 3).astype(np.uint32)                # 1000 rows a label
    c.set_labels(labels)
    ql = np.array([2, 0, 1, 0, 2, 1, 0, 2, 1], dtype=np.uint32)
    pos = np.empty(NQ, dtype=np.int64)
    pos[_label_order(ql)] = np.arange(NQ)                        # where a query sits once the batch is ordered by label
    big = 5
    mates = [i for i in range(NQ) if i != big and pos[i] // per_pass == pos[big] // per_pass]
    inf_q = mates[-1]                                            # every row of its label, in the pass of `big`
    last = int(_label_order(ql)[-1])                             # the query alone in the ragged last pass
    assert pos[last] // per_pass != pos[big] // per_pass and last not in (big, inf_q, 0)
    ranked = own if own is not None else [c.scan_distances(metric, qs[i]) for i in range(NQ)]
    radii = []
    for i in range(NQ):
        s = np.sort(ranked[i][labels == ql[i]])
        rank = 600 if i == big else 3 + i
        radii.append(0.5 * (float(s[rank - 1]) + float(s[rank])) if s[rank - 1] < s[rank] else float(s[rank - 1]))
    radii[0] = float("-inf")
    radii[inf_q] = float("inf")

    def expected(rr):
        if own is not None:
            return [_expected_allowed(own[i], labels == ql[i], rr[i]) for i in range(NQ)]
        un = c.scan_within_batch(metric, qs, rr)
        return [(un[i][0][(labels == ql[i])[un[i][0] - 1]], un[i][1][(labels == ql[i])[un[i][0] - 1]].astype(np.float32)) for i in range(NQ)]

    exp = expected(radii)
    assert len(exp[0][0]) == 0 and 590 <= len(exp[big][0]) <= 700 and len(exp[inf_q][0]) == int(np.sum(labels == ql[inf_q]))
    assert all(0 < len(exp[i][0]) <= 40 for i in range(1, NQ) if i not in (big, inf_q))
    pkg.set_within_batch_initial_capacity(c, 64)
    try:
        for limit in (None, 17):
            res = c.scan_within_batch_labeled(metric, qs, ql, radii, limit=limit)
            assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 1         # only the pass that overflowed ran again
            for i in range(NQ):
                ids, dist = exp[i]
                cut = len(ids) if limit is None else limit
                _assert_same(res[i], ids[:cut], dist[:cut], matches=len(ids), ctx=(dim, i, limit))
        radii2 = list(radii)
        radii2[last] = float("inf")                              # the ragged last pass overflows too
        exp2 = expected(radii2)
        res = c.scan_within_batch_labeled(metric, qs, ql, radii2)
        assert c.within_batch_last_launches() == _passes(NQ, per_pass) + 2
        for i in range(NQ):
            _assert_same(res[i], exp2[i][0], exp2[i][1], ctx=(dim, i, "two passes"))
        # 1000 rows within the radius, none of them of the query's label: nothing takes room, no pass runs again
        absent = ql.copy()
        absent[big] = lc.ABSENT
        res = c.scan_within_batch_labeled(metric, qs, absent, [float("inf") if i == big else float("-inf") for i in range(NQ)])
        assert c.within_batch_last_launches() == _passes(NQ, per_pass)
        assert all(r[2] == 0 and len(r[0]) == 0 for r in res)
    finally:
        pkg.set_within_batch_initial_capacity(c, 0)
    c.close()


# ------------------------------------------------------------------------------------------------- more queries than a staging slice

def test_a_batch_larger_than_a_staging_slice_in_random_label_order(pkg):
    dim, nq = 64, 300
    rows = lc.data(dg.U8, N, dim, 161)
    qs = lc.data(dg.U8, nq, dim, 162)
    c = pkg.Corpus(dg.U8, dim)
    c.append(rows)
    labels, _ = lc.layouts(N)["some_none"]
    c.set_labels(labels)
    rng = np.random.default_rng(163)
    ql = rng.choice(np.array([0, 1, 2, 3, 4, lc.ABSENT], dtype=np.uint32), nq)
    assert len(set(ql.tolist())) == 6 and (np.diff(ql.astype(np.int64)) < 0).any()
    per_pass = c.within_batch_labeled_plan(dg.L2)[0]
    assert per_pass in (2, 4)
    ranks = rng.integers(0, 60, nq)
    radii, exp = [], []
    for i in range(nq):
        own = c.scan_distances(dg.L2, qs[i])
        allowed = labels == ql[i]
        radii.append(float(np.sort(own[allowed])[ranks[i]]) if allowed.any() else float("inf"))
        exp.append(_expected_allowed(own, allowed, radii[i]))
    res = c.scan_within_batch_labeled(dg.L2, qs, ql, radii)
    assert c.within_batch_last_launches() == _passes(nq, per_pass)
    for i in range(nq):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=(i, int(ql[i])))
        assert (labels[res[i][0] - 1] != lc.NONE).all()
    keys = c.within_batch_keys(nq - 1, len(exp[nq - 1][0]))      # held at the caller's indices
    assert ((keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == exp[nq - 1][0].tolist()
    c.close()


# ------------------------------------------------------------------------------------------------- shards

@pytest.mark.parametrize("n_shards", [3, 8])
@pytest.mark.parametrize("vt,dim", [(dg.U8, 100), (dg.F32, 384)])
def test_shards_equal_one_corpus(pkg, n_shards, vt, dim):
    rows = lc.data(vt, N, dim, 171 + dim)
    qs = lc.data(vt, NQ, dim, 172 + dim)
    rowids = np.arange(N, dtype=np.int64) * 2 + 5
    c = pkg.Corpus(vt, dim)
    c.append(rows, rowids)
    sh = pkg.Shards(vt, dim, [0] * n_shards, block_rows=40)
    for r0 in range(0, N, 1000):
        sh.append(rows[r0:r0 + 1000], rowids[r0:r0 + 1000])
    assert sh.within_batch_labeled_plan(dg.L2) == c.within_batch_labeled_plan(dg.L2)
    assert lc.error_code(pkg, lambda: sh.scan_within_labeled(dg.L2, qs[0], 1.0, 0)) == VG_ERR_INVALID          # no labels
    assert lc.error_code(pkg, lambda: sh.scan_within_labelset(dg.L2, qs[0], 1.0, [0])) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: sh.scan_within_batch_labeled(dg.L2, qs, np.zeros(NQ, dtype=np.uint32), 1.0)) == VG_ERR_INVALID
    same = lambda many, one, ctx: _assert_same(many, one[0], one[1].astype(np.float32), matches=one[2], ctx=ctx)
    for lname in ("uniform5", "last_row_only", "some_none"):
        labels, asked = lc.layouts(N)[lname]
        c.set_labels(labels)
        sh.set_labels(labels)
        ql = _query_labels(asked)
        for metric in (dg.L2, dg.DOT):
            own = [c.scan_distances(metric, qs[i]) for i in range(NQ)]
            ranks = [0, 40, 700, N // 2, N - 1, 3, 12, 100, 1]
            radii = [float(np.sort(own[i])[ranks[i]]) for i in range(NQ)]
            radii[4] = float("inf")
            for limit in (None, 1, 33):
                for label in asked:
                    for r in (radii[1], radii[3], float("inf")):
                        one = c.scan_within_labeled(metric, qs[0], r, label, limit=limit)
                        if limit is None:
                            ids, dist = _expected_allowed(own[0], labels == label, r, rowids)
                            _assert_same(one, ids, dist, ctx=("corpus", lname, metric, label, r))
                        same(sh.scan_within_labeled(metric, qs[0], r, label, limit=limit), one, ("labeled", n_shards, lname, metric, label, r, limit))
                for members, exclude in (([asked[0], lc.ABSENT], False), ([asked[0]], True), ([], True), ([], False)):
                    one = c.scan_within_labelset(metric, qs[1], radii[3], members, exclude=exclude, limit=limit)
                    same(sh.scan_within_labelset(metric, qs[1], radii[3], members, exclude=exclude, limit=limit), one,
                         ("labelset", n_shards, lname, metric, members, exclude, limit))
                one = c.scan_within_batch_labeled(metric, qs, ql, radii, limit=limit)
                many = sh.scan_within_batch_labeled(metric, qs, ql, radii, limit=limit)
                assert sum(r[2] for r in one) > 0
                for i in range(NQ):
                    same(many[i], one[i], ("batch", n_shards, lname, metric, i, limit))
    sh.close()
    c.close()


# ------------------------------------------------------------------------------------------------- contract

def test_contract(pkg):
    L = pkg.lib()
    dim = 16
    c = pkg.Corpus(dg.U8, dim)
    qs = lc.data(dg.U8, 3, dim, 181)
    rows = lc.data(dg.U8, N, dim, 182)
    c.append(rows)
    labels, _ = lc.layouts(N)["uniform5"]
    ql = np.array([3, 0, 3], dtype=np.uint32)
    good = np.array([1.0, 5.0, 2.0])
    bad = np.array([1.0, float("nan"), 2.0])
    none = np.array([3, lc.NONE, 0], dtype=np.uint32)

    def raw(h, metric, queries, nq, qlabels, radii):
        m, held = np.full(3, 7, dtype=np.int64), np.full(3, 7, dtype=np.int64)
        rc = L.vg_scan_within_batch_labeled(h, metric, queries, nq, qlabels, radii, 0, pkg._ptr(m), pkg._ptr(held))
        return rc, m.tolist(), held.tolist()

    zero = [0, 0, 0]
    refused = (VG_ERR_INVALID, zero, zero)
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(ql), pkg._ptr(good)) == refused               # no labels set
    c.set_labels(labels)
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(ql), pkg._ptr(bad)) == refused
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(none), pkg._ptr(good)) == refused             # the rule of scan_topk_batch_labeled
    assert c.within_batch_last_launches() == 0                                                    # refused before any launch
    assert lc.error_code(pkg, lambda: c.scan_within_batch_labeled(dg.L2, qs, none, 1.0)) == VG_ERR_INVALID
    assert raw(c.h, 99, pkg._ptr(qs), 3, pkg._ptr(ql), pkg._ptr(good)) == refused
    assert raw(c.h, dg.L2, None, 3, pkg._ptr(ql), pkg._ptr(good)) == refused
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, None, pkg._ptr(good)) == refused
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(ql), None) == refused
    assert raw(None, dg.L2, pkg._ptr(qs), 3, pkg._ptr(ql), pkg._ptr(good)) == refused
    assert raw(c.h, dg.L2, pkg._ptr(qs), 0, pkg._ptr(ql), pkg._ptr(good))[0] == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: c.scan_within_batch_labeled(dg.L2, qs[:0], ql[:0], [])) == VG_ERR_INVALID
    with pytest.raises(ValueError):
        c.scan_within_batch_labeled(dg.L2, qs, ql[:2], 1.0)                                        # one label per query

    own = [c.scan_distances(dg.L2, qs[i]) for i in range(3)]
    allowed = [labels == ql[i] for i in range(3)]
    radii = [float(np.sort(own[i][allowed[i]])[10 * (i + 1)]) for i in range(3)]
    exp = [_expected_allowed(own[i], allowed[i], radii[i]) for i in range(3)]
    res = c.scan_within_batch_labeled(dg.L2, qs, ql, radii)
    for i in range(3):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=i)                                          # caller order, not label order
    same = c.scan_within_batch_labeled(dg.L2, qs, ql, radii[1])                                    # a scalar radius is broadcast
    for i in range(3):
        _assert_same(same[i], *_expected_allowed(own[i], allowed[i], radii[1]), ctx=("scalar", i))
    res = c.scan_within_batch_labeled(dg.L2, qs, ql, radii)
    n0 = len(exp[0][0])
    keys = c.within_batch_keys(0, n0)
    assert ((keys & np.uint64(0xFFFFFFFF)).astype(np.int64) + 1).tolist() == exp[0][0].tolist()
    assert lc.error_code(pkg, lambda: c.within_batch_keys(0, n0 + 1)) == VG_ERR_INVALID
    # the single forms' held result and the batch form's stay apart
    single = c.scan_within_labeled(dg.L2, qs[2], radii[2], 3)
    _assert_same(single, exp[2][0], exp[2][1])
    assert c.within_batch_keys(0, n0).tolist() == keys.tolist()
    # the unlabeled batch overwrites the labeled batch's held result, and does not read the labels
    un = c.scan_within_batch(dg.L2, qs, radii)
    assert len(c.within_batch_keys(0, len(un[0][0]))) == len(un[0][0]) > n0
    # a refused call leaves nothing held
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(none), pkg._ptr(good)) == refused
    assert lc.error_code(pkg, lambda: c.within_batch_keys(0, 1)) == VG_ERR_INVALID
    # the row mask: neither read nor written
    assert c.set_mask(bits=np.zeros(N, dtype=bool)) == 0
    res = c.scan_within_batch_labeled(dg.L2, qs, ql, radii)
    for i in range(3):
        _assert_same(res[i], exp[i][0], exp[i][1], ctx=("all-clear mask", i))
    assert c.mask_count() == 0
    # labels cleared after use
    c.clear_labels()
    assert raw(c.h, dg.L2, pkg._ptr(qs), 3, pkg._ptr(ql), pkg._ptr(good)) == refused
    c.close()
    e = pkg.Corpus(dg.U8, dim)                                  # an empty corpus: every count 0, no launch
    e.set_labels(np.zeros(0, dtype=np.uint32))
    res = e.scan_within_batch_labeled(dg.L2, qs, ql, 1e9)
    assert [(len(r[0]), r[2]) for r in res] == [(0, 0)] * 3 and e.within_batch_last_launches() == 0
    e.close()
