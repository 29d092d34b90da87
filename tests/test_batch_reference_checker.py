"""The batch reference checker (tests/batch_reference.py) must be able to FAIL: a correct answer built with numpy and the oracle is
accepted, and every corruption a batched kernel can plausibly produce - a lost candidate, a permutation that is not undone, a list out
of order, a distance slightly off, a short count, a tie in the wrong order - raises AssertionError.  No GPU."""
import numpy as np
import pytest

import datagen as dg
import batch_reference as br

N, DIM, NQ, K = 3000, 48, 40, 10
DUP = [5, 77]                                                  # two identical rows, and query 0 is that row: a tie at distance 0


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(4801)
    rows = rng.standard_normal((N, DIM), dtype=np.float32)
    qs = rng.standard_normal((NQ, DIM), dtype=np.float32)
    rows[DUP[1]] = rows[DUP[0]]
    qs[0] = rows[DUP[0]]
    return rows, qs


def _answer(orc, metric, rows, qs, k):
    ids = np.zeros((len(qs), k), dtype=np.int64)
    dist = np.zeros((len(qs), k), dtype=np.float64)
    cnt = np.zeros(len(qs), dtype=np.int32)
    for i, q in enumerate(qs):
        d = orc.scan_distances(orc.AVX2, metric, dg.F32, q, rows)
        oi, od, _ = orc.topk_ordered(d, None, k)
        ids[i, :len(oi)], dist[i, :len(oi)], cnt[i] = oi, od, len(oi)
    return ids, dist, cnt


@pytest.mark.parametrize("metric", (dg.L2, dg.SQUARED_L2, dg.COSINE, dg.DOT))
def test_checker_accepts_the_right_answer_and_rejects_every_corruption(orc, world, metric):
    rows, qs = world
    ref = br.batch_references(dg.F32, (metric,), qs, rows, orc, kmax=K, duplicates=[DUP])[metric]
    assert ref.band_share(K) <= br.BAND_SHARE_CAP
    ids, dist, cnt = _answer(orc, metric, rows, qs, K)
    # the answer's own (k + 1)-th rows, for the first corruption
    ids1, _, _ = _answer(orc, metric, rows, qs, K + 1)

    def check(ids_, dist_, cnt_):
        return br.check_batch(dg.F32, metric, K, qs, rows, ids_, dist_, cnt_, orc, duplicates=[DUP], reference=ref)

    assert check(ids, dist, cnt) <= br.BAND_SHARE_CAP * NQ
    clear = [i for i in range(1, NQ) if ref.clear_boundary(i, K)]
    a, b = clear[0], clear[1]

    def corrupt(fn):
        i2, d2, c2 = ids.copy(), dist.copy(), cnt.copy()
        fn(i2, d2, c2)
        with pytest.raises(AssertionError):
            check(i2, d2, c2)

    def lost_best(i2, d2, c2):                                 # the best row replaced by the (k + 1)-th: the list stays sorted, its distances right
        i2[a, :K] = ids1[a, 1:K + 1]
        d2[a, :K] = [float(orc.distance(orc.AVX2, metric, dg.F32, qs[a], rows[r - 1])) for r in i2[a, :K]]

    def swapped(i2, d2, c2):
        i2[[a, b]], d2[[a, b]] = ids[[b, a]], dist[[b, a]]

    def rotated(i2, d2, c2):
        i2[a], d2[a] = np.roll(ids[a], 1), np.roll(dist[a], 1)

    def off(i2, d2, c2):
        d2[a, K // 2] *= 1.0 + 1e-4

    def short(i2, d2, c2):
        c2[b] -= 1

    def tie_descending(i2, d2, c2):
        assert ids[0, :2].tolist() == [DUP[0] + 1, DUP[1] + 1] and dist[0, 0] == dist[0, 1]
        i2[0, :2] = ids[0, 1::-1]

    for fn in (lost_best, swapped, rotated, off, short, tie_descending):
        corrupt(fn)


def test_checker_names_the_duplicate_pair_at_the_boundary(orc, world):
    """k = 1 on the query with two identical best rows: a float64 gap of 0 at the boundary - clear only because the pair is named, and then
    the lower position is the one expected"""
    rows, qs = world
    named = br.batch_references(dg.F32, (dg.L2,), qs[:1], rows, orc, kmax=1, duplicates=[DUP])[dg.L2]
    unnamed = br.batch_references(dg.F32, (dg.L2,), qs[:1], rows, orc, kmax=1)[dg.L2]
    assert named.clear_boundary(0, 1) and not unnamed.clear_boundary(0, 1)
    ids = np.array([[DUP[1] + 1]], dtype=np.int64)
    with pytest.raises(AssertionError):
        br.check_batch(dg.F32, dg.L2, 1, qs[:1], rows, ids, np.zeros((1, 1)), np.array([1]), orc, reference=named)
    ids[0, 0] = DUP[0] + 1
    assert br.check_batch(dg.F32, dg.L2, 1, qs[:1], rows, ids, np.zeros((1, 1)), np.array([1]), orc, reference=named) == 0


def test_checker_takes_the_oracle_for_rows_and_queries_float64_does_not_speak_for(orc):
    """NaN / Inf rows never enter, a row whose norm underflows float32 is the reference's zero norm (cosine 1.0), a query whose squares
    overflow float32 has no L2 neighbours at all: the counts and lists follow the oracle there"""
    rng = np.random.default_rng(4802)
    rows = rng.standard_normal((500, 16), dtype=np.float32)
    rows[3, 2] = np.nan
    rows[4] = np.inf
    rows[6] = rng.standard_normal(16).astype(np.float32) * np.float32(1e-38)
    qs = rng.standard_normal((3, 16), dtype=np.float32)
    qs[1] *= np.float32(1e25)
    qs[2] = 0.0
    for metric in (dg.L2, dg.COSINE, dg.DOT):
        ref = br.batch_references(dg.F32, (metric,), qs, rows, orc, kmax=5)[metric]
        ids, dist, cnt = _answer(orc, metric, rows, qs, 5)
        br.check_batch(dg.F32, metric, 5, qs, rows, ids, dist, cnt, orc, reference=ref)
        if metric == dg.L2:
            assert ref.enter.tolist() == [498, 0, 498] and cnt.tolist() == [5, 0, 5]
        if metric == dg.COSINE:
            assert ref.d[0][ref.pos[0] == 6].tolist() in ([], [1.0])
