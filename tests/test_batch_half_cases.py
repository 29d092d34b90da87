"""The worlds of tests/batch_half_cases.py against the float64 reference alone - no device.  For every world, metric, k and batch size that
tests/test_gpu_batch_half_forms.py runs: the share of queries left to the weaker band check stays within batch_reference.BAND_SHARE_CAP
(seeds that exceed it are moved on in batch_half_cases.SEED_STEP, never the cap), every planted query's plant - and its named second copy -
are the decided first entries, and check_batch REJECTS an answer with a near-bound row lost, two slots exchanged or a second copy ahead of
its first: what makes the device file worth trusting."""
import numpy as np
import pytest

import datagen as dg
import batch_reference as br
import batch_half_cases as bh


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    bh.close_worlds()


def _ids(worlds):
    return ["-".join(dg.TYPE_NAMES[x] if j == 0 else str(x) for j, x in enumerate(v)) for v in worlds]


def check_shares(w, refs, cases, judged=None):
    worst = 0.0
    for nq, metric, k in sorted(set(cases)):
        mask = None if judged is None else judged[:nq]
        share = refs[metric].band_share(k, nq, mask)
        worst = max(worst, share)
        assert share <= br.BAND_SHARE_CAP, (dg.TYPE_NAMES[w.vt], w.dim, w.n, nq, dg.METRIC_NAMES[metric], k, share)
    print("worst band share %.4f  (%s dim %d n %d, %d cases)" % (worst, dg.TYPE_NAMES[w.vt], w.dim, w.n, len(set(cases))))


def check_plants(w, refs, nq=None):
    """under every metric but dot: the plant first, a named second copy second at the same distance; decided (a float64 gap to every row
    left out, or a named pair) except for the queries HalfWorld.weak_first names.  The duplicate ladder: its first entries, in order."""
    nq = w.nq if nq is None else nq
    for metric, ref in refs.items():
        weak = w.weak_first(metric)
        for i in range(nq):
            if i in weak:
                continue
            assert ref.pos[i, 0] == w.plant[i], (dg.METRIC_NAMES[metric], i, ref.pos[i, :3], w.plant[i])
            if w.ladder and i == bh.LADDER_Q:                      # (more copies than the checker looks at past a boundary: their ORDER is what is held)
                m = min(ref.kmax, len(w.ladder))
                assert ref.pos[i, :m].tolist() == w.ladder[:m] and (ref.d[i, :m] == ref.d[i, 0]).all()
                continue
            assert ref.clear_boundary(i, 1), (dg.METRIC_NAMES[metric], i, ref.d[i, :3])
            if i in w.second:
                assert ref.pos[i, 1] == w.second[i] and ref.d[i, 1] == ref.d[i, 0] and ref.clear_boundary(i, 2), (dg.METRIC_NAMES[metric], i)
        for t, at in w.slack_rows.items():                         # the rows aimed at the slack are among the target's nearest, in the order of their units
            if metric in (dg.L2, dg.SQUARED_L2) and t < nq:
                assert ref.pos[t, 1:4].tolist() == at[::-1], (t, ref.pos[t, :5], at)


@pytest.mark.parametrize("vt,dim", bh.small_worlds(), ids=_ids(bh.small_worlds()))
def test_small_worlds(orc, vt, dim):
    w = bh.world(vt, dim)
    refs = bh.references(w, orc, br)
    check_shares(w, refs, bh.bucket_cases(vt, dim) + [c[1:] for c in bh.form_cases(vt, dim)])
    check_plants(w, refs)
    if (vt, dim) in bh.UNJUDGED_WORLDS:
        qs = bh.unjudgeable_queries(w)
        urefs = bh.references(w, orc, br, qs, "unjudgeable", (dg.DOT, dg.COSINE, dg.L2))
        judged = np.ones(129, dtype=bool)
        judged[list(bh.UNJUDGED_SLOTS)] = False
        check_shares(w, urefs, [(129, m, 20) for m in urefs], judged)
    if (vt, dim) in bh.DOT1_WORLDS:                                # dot at k = 1: more than a wavefront of queries with no row at -Inf, all decided
        sel = bh.dot1_queries(w)
        drefs = bh.references(w, orc, br, w.queries[sel], "dot1", (dg.DOT,))
        assert len(sel) > 32 and np.isfinite(drefs[dg.DOT].d[:, 0]).all() and drefs[dg.DOT].band_share(1) == 0.0
    if (vt, dim) in bh.APPEND_WORLDS:
        rows, dup = bh.appended(w)
        arefs = br.batch_references(vt, (dg.DOT, dg.COSINE, dg.L2), w.queries[:bh.APPEND_NQ], rows, orc, kmax=20, duplicates=dup)
        check_shares(w, arefs, [(bh.APPEND_NQ, m, 20) for m in arefs])
        d = arefs[dg.DOT]                                          # (ahead of it only rows of huge magnitude and rows at -Inf: one Inf element)
        assert w.n + 123 in d.pos[bh.APPEND_BEST, :12].tolist() and d.clear_boundary(bh.APPEND_BEST, 20)
        assert arefs[dg.L2].pos[bh.APPEND_COPY, :2].tolist() == [w.plant[bh.APPEND_COPY], w.n + 377]


@pytest.mark.parametrize("vt,dim,n", bh.TINY_WORLDS, ids=_ids(bh.TINY_WORLDS))
def test_tiny_worlds(orc, vt, dim, n):
    """less than one tile, and one row more than a tile: fewer rows can enter a list than k = 20 / 32 asks for"""
    w = bh.world(vt, dim, n)
    refs = bh.references(w, orc, br)
    check_shares(w, refs, [(bh.TINY_NQ, m, k) for m in bh.ALL_METRICS for k in (1, 20, 32) if (m, k) != (dg.DOT, 1)])
    check_plants(w, refs)
    e = refs[dg.L2].enter                                          # (an Inf element: an L2 distance of +Inf, which never enters a list)
    assert (e < n).all() and (e < (20 if n == 20 else 32)).all() and (e >= n - 3).all()


@pytest.mark.parametrize("vt,dim", bh.small_worlds(), ids=_ids(bh.small_worlds()))
def test_sparse_worlds(orc, vt, dim):
    """every type and k-step bucket: the split form's cases; three of them also under the fused kernel"""
    w = bh.world(vt, dim, bh.N_SPARSE)
    refs = bh.references(w, orc, br)
    cases = bh.split_cases(vt, dim)
    if (vt, dim) in bh.SPARSE_WORLDS:
        cases = cases + [(nq, m, k) for nq in (129, 257) for m in bh.ALL_METRICS for k in (20, 32)]
    check_shares(w, refs, cases)
    check_plants(w, refs)


def test_staged_world(orc):
    vt, dim, n = bh.STAGED
    w = bh.world(vt, dim, n)
    assert len(w.ladder) == 35 and len(w.ladder) > 20 and (n + 31) // 32 >= 65536
    refs = bh.references(w, orc, br, metrics=(dg.L2, dg.DOT), kmax=20)
    check_shares(w, refs, [(nq, m, 20) for nq in (40, 160) for m in refs])
    check_plants(w, refs)


def _answer(orc, vt, metric, rows, qs, k):
    ids = np.zeros((len(qs), k), dtype=np.int64)
    dist = np.zeros((len(qs), k), dtype=np.float64)
    cnt = np.zeros(len(qs), dtype=np.int32)
    for i, q in enumerate(qs):
        oi, od, _ = orc.topk_ordered(orc.scan_distances(orc.AVX2, metric, vt, q, rows), None, k)
        ids[i, :len(oi)], dist[i, :len(oi)], cnt[i] = oi, od, len(oi)
    return ids, dist, cnt


@pytest.mark.parametrize("metric", (dg.L2, dg.COSINE), ids=lambda m: dg.METRIC_NAMES[m])
def test_checker_rejects_what_a_wrong_filter_would_answer(orc, metric):
    """on the bf16 small world of 100 elements, 64 queries, k = 20: the right answer passes; each corruption is rejected, and each differs
    from the right answer in an entry the reference DECIDES (a clear boundary: the set comparison, not the band check)"""
    vt, dim, nq, k = dg.BF16, 100, 64, 20
    w = bh.world(vt, dim)
    ref = bh.references(w, orc, br)[metric]
    qs = w.queries[:nq]
    ids, dist, cnt = _answer(orc, vt, metric, w.rows, qs, k)
    ids1, _, _ = _answer(orc, vt, metric, w.rows, qs, k + 1)

    def check(i2, d2, c2):
        return br.check_batch(vt, metric, k, qs, w.rows, i2, d2, c2, orc, reference=ref)

    assert check(ids, dist, cnt) <= br.BAND_SHARE_CAP * nq
    t, other, dup = 5, 40, 2
    near = w.slack_rows[t][-1] + 1                                  # the row one unit of cerr |q| |x| behind the plant
    assert ref.clear_boundary(t, k) and ref.clear_boundary(other, k) and ref.clear_boundary(dup, k)
    assert near in ids[t].tolist() and ids1[t, k] - 1 not in ref.pos[t, :k].tolist()

    def lost_near_bound_row(i2, d2, c2):                            # ... swapped for the next-best row: sorted, distances right
        keep = [r for r in ids[t].tolist() if r != near] + [int(ids1[t, k])]
        i2[t] = keep
        d2[t] = [float(orc.distance(orc.AVX2, metric, vt, qs[t], w.rows[r - 1])) for r in keep]
        assert set(i2[t].tolist()) != set((ref.pos[t, :k] + 1).tolist())

    def slots_exchanged(i2, d2, c2):
        i2[[t, other]], d2[[t, other]] = ids[[other, t]], dist[[other, t]]
        assert i2[t, 0] - 1 == w.plant[other] != ref.pos[t, 0]

    def second_copy_first(i2, d2, c2):
        assert ids[dup, :2].tolist() == [w.plant[dup] + 1, w.second[dup] + 1] and dist[dup, 0] == dist[dup, 1]
        assert ref.group[w.plant[dup]] == ref.group[w.second[dup]] >= 0 and ref.clear_boundary(dup, 1)
        i2[dup, :2] = ids[dup, 1::-1]

    for fn in (lost_near_bound_row, slots_exchanged, second_copy_first):
        i2, d2, c2 = ids.copy(), dist.copy(), cnt.copy()
        fn(i2, d2, c2)
        with pytest.raises(AssertionError):
            check(i2, d2, c2)
