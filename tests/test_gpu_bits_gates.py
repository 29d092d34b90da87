"""The integer gates of the Hamming / Jaccard matrix-core batches (vg_batch_bits.hip, vg_batch_bitsl.hip and their _within forms) met on
purpose, against numpy.

tests/bits_batch_cases.py builds the data: a LADDER - for a query of w set bits a row for every class (i common bits, e extra bits), twice,
so that a row sits at every distance next to any threshold a list or a radius can take, the 64 tightest Jaccard pairs of the row length
among them - in a random order, in runs of falling distance (every row of a new distance beats all rows before it) and in runs of
rising distance (only the first rows of a run can pass); and batches of pairwise DIFFERENT queries, so that an answer in another
query's slot never compares equal.  A top-k batch is cut into up to 256 partitions with lists of their own, and a workgroup's gate
holds the `list not full` sentinel until its own lists are full: the top-k cases take the DENSE ladders (1024 tiles or more, among the
allowed rows too) and assert it, so that every partition is four tiles or more and the later ones are judged under real thresholds -
falling runs then refresh them with every tile, rising runs close the gate after a partition's first tile.  tests/test_bits_batch_cases.py proves the gate claim itself on
the host; here the kernels' answers are compared: rowids, order, distance bits and counts with ==.

Every case sets VG_BATCH_BITS_MIN_QUERIES=2 and asserts after each call that the form under test answered (path 8)."""
import numpy as np
import pytest

import bits_batch_cases as bb

pytestmark = pytest.mark.gpu

NAMES = ("hamming", "jaccard")
SHORT, LONG = (16, 100, 128), (200, 512)


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


def _qpb(dim):
    """queries per workgroup; the long range form needs one workgroup of queries"""
    return 256 if dim <= 128 else 128 if (dim + 15) // 16 * 16 <= 256 else 64


def _corpus(pkg, monkeypatch, rows):
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


def _metric(pkg, name):
    return getattr(pkg, name.upper())


# ---------------------------------------------------------------------------------------------------- range forms

def _range_batch(name, dim, nq, seed):
    """(rows, copy, queries, slot -> distinct query, distances of the distinct queries): the ladder's own query (0) in three slots of
    four, a different other query in every fourth slot"""
    n_other = max(1, nq // 4)
    rows, qs, copy = bb.ladder_corpus(name, dim, "random", n_other + 1, seed)
    which = np.zeros(nq, dtype=np.int64)
    which[3::4] = 1 + np.arange(len(which[3::4]))
    if nq == 2:
        which[1] = 1
    return rows, copy, qs[which], which, bb.batch_distances(name, rows, qs)


def _ladder_radii(name, dim, d0, count):
    """edge radii of the ladder query, the most telling first: (Jaccard) the distances of the tightest pairs - as a radius the threshold
    is the very next float - then `count` ranks over all distinct distances, the float below each, Hamming +- 0.5, the five fixed ones"""
    out = []
    if name == "jaccard":
        for i, u, i2, u2, _ in bb.jaccard_tight(8 * dim, bb.LADDER_WEIGHT[dim])[:16]:
            v = bb.jaccard_f32(i, u)
            out += [float(v), float(np.nextafter(v, np.float32(-1)))]
    ndist = len(np.unique(d0))
    ranks = np.unique(np.r_[np.arange(4), np.linspace(0, ndist - 1, count).astype(np.int64)])
    edge = bb.edge_radii(name, d0, ranks)
    return out + edge[5:] + edge[:5]


def _range_check(name, c, metric, masked, qs, which, d, radii, allowed, limit, ctx):
    got = (c.scan_within_batch_masked if masked else c.scan_within_batch)(metric, qs, radii, limit=limit)
    assert c.within_batch_last_path() == 8, ctx
    pos = {}
    wants = []
    for w, r in zip(which, radii):
        if w not in pos:
            pos[w] = bb.order(d[w], allowed)
        wants.append(bb.within(d[w], r, limit=limit, pos=pos[w]))
    bb.check_within(name, got, wants, ctx)
    return got


def _slot_radii(name, which, d, ladder_radii, shift, allowed=None):
    """the ladder query's slots walk through its edge radii from `shift` on; another query takes 0 (its planted row) or its own 3rd distance"""
    out, j = [], shift
    for s, w in enumerate(which):
        if w == 0:
            out.append(ladder_radii[j % len(ladder_radii)])
            j += 1
        else:
            dw = d[w] if allowed is None else d[w][allowed]
            out.append(0.0 if s % 8 == 3 else float(np.sort(dw)[2]))
    return out


@pytest.mark.parametrize("nq_kind", ["least", "padding", "257"])
@pytest.mark.parametrize("dim", SHORT + LONG)
@pytest.mark.parametrize("name", NAMES)
def test_range_ladder(pkg, monkeypatch, name, dim, nq_kind):
    """nq: the fewest queries the form takes (2; long rows: one workgroup), one more than a query group of the long forms holds (65, 129:
    the second group is padding but for one slot), 257"""
    least = 2 if dim <= 128 else _qpb(dim)
    nq = {"least": least, "padding": 65 if dim <= 128 else _qpb(dim) + 1, "257": 257}[nq_kind]
    rows, copy, qs, which, d = _range_batch(name, dim, nq, 7 * dim + nq)
    lr = _ladder_radii(name, dim, d[0], 24)
    c = _corpus(pkg, monkeypatch, rows)
    slots = int((which == 0).sum())
    shifts = range(0, len(lr), max(slots, len(lr) // 6 + 1))    # (two queries: six calls pick six of the radii)
    matched = 0
    for shift in shifts:
        radii = _slot_radii(name, which, d, lr, shift)
        for limit in (None, 5):
            got = _range_check(name, c, _metric(pkg, name), False, qs, which, d, radii, None, limit, (name, dim, nq, shift, limit))
        matched += sum(g[2] for g in got)
    assert 0 < matched < 4_000_000
    c.close()


@pytest.mark.parametrize("dim", [128, 200])
@pytest.mark.parametrize("name", NAMES)
def test_range_every_query_overflows_by_another_amount(pkg, monkeypatch, name, dim):
    """regions of 8 keys; slot s matches at least 9 + s rows: one more launch into regions of the counted sizes"""
    nq = 65 if dim <= 128 else _qpb(dim)
    rows, copy, qs, which, d = _range_batch(name, dim, nq, 11 * dim)
    radii = [float(np.sort(d[w])[8 + s]) for s, w in enumerate(which)]
    c = _corpus(pkg, monkeypatch, rows)
    c.set_within_batch_initial_capacity(8)
    got = _range_check(name, c, _metric(pkg, name), False, qs, which, d, radii, None, None, (name, dim))
    assert c.within_batch_last_launches() == 2
    assert all(g[2] >= 9 + s for s, g in enumerate(got)) and len({g[2] for g in got}) > 8      # (equal distances: fewer amounts than slots)
    c.close()


@pytest.mark.parametrize("nq", [128, 257])
@pytest.mark.parametrize("dim", SHORT)
@pytest.mark.parametrize("name", NAMES)
def test_masked_range_ladder(pkg, monkeypatch, name, dim, nq):
    """the mask drops every class's first copy: the allowed row of a distance is never the first one at it"""
    rows, copy, qs, which, d = _range_batch(name, dim, nq, 13 * dim + nq)
    allowed = copy == 1
    lr = _ladder_radii(name, dim, d[0][allowed], 24)
    c = _corpus(pkg, monkeypatch, rows)
    assert c.set_mask(bits=allowed) == int(allowed.sum())
    radii = _slot_radii(name, which, d, lr, 0, allowed)
    for limit in (None, 5):
        _range_check(name, c, _metric(pkg, name), True, qs, which, d, radii, allowed, limit, (name, dim, nq, limit))
    c.close()


# ---------------------------------------------------------------------------------------------------- top-k forms

TOPK_FORMS = [("plain", 16), ("plain", 100), ("plain", 128), ("plain", 200), ("plain", 512), ("masked", 128), ("masked", 200),
              ("masked", 272), ("labeled", 100), ("labeled", 128)]


def _ks(kind, dim):
    """lists of 1, 20 and 32 keys - the longest; rows of 193 - 256 bytes serve 29 keys plain, 28 masked"""
    return (1, 20, 29 if kind == "plain" else 28) if 192 < dim <= 256 else (1, 20, 32)


@pytest.mark.parametrize("ordering", ["random", "descending", "ascending"])
@pytest.mark.parametrize("kind,dim", TOPK_FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_topk_ladder(pkg, monkeypatch, name, kind, dim, ordering):
    """70 queries: the ladder's own (labeled: twice, once per label) and 69 different others, over the dense ladder: 1024 tiles or
    more in at most 256 partitions.  masked: every class's first copy is dropped.  labeled: the rows alternate between two labels -
    the next-better row of the other label must never enter"""
    metric, nq = _metric(pkg, name), 70
    rows, qs, copy = bb.ladder_corpus(name, dim, ordering, nq, 17 * dim + len(ordering), dense=True)
    n = len(rows)
    assert (n if kind != "masked" else int((copy != 0).sum())) // bb.TILE >= 4 * bb.PARTITIONS      # four tiles or more per partition
    d = bb.batch_distances(name, rows, qs)
    lad = bb.ladder(name, dim, ordering, True)
    assert np.array_equal(d[0, :len(lad.rows)].view(np.uint32), bb.ladder_distances(name, dim, lad).view(np.uint32))
    c = _corpus(pkg, monkeypatch, rows)
    which = np.arange(nq)
    if kind == "masked":
        allowed = [copy != 0] * nq
        c.set_mask(bits=allowed[0])
    elif kind == "labeled":
        lab = (np.arange(n) % 2).astype(np.uint32)
        which = np.r_[0, np.arange(nq)]
        ql = np.r_[1, np.arange(nq) % 2].astype(np.uint32)
        allowed = [lab == l for l in ql]
        c.set_labels(lab)
    else:
        allowed = [None] * nq
    pos = [bb.order(d[w], al) for w, al in zip(which, allowed)]
    for k in _ks(kind, dim):
        ctx = (name, kind, dim, ordering, k)
        if kind == "plain":
            got, path = c.scan_topk_batch(metric, qs[which], k), c.last_batch_path()
        elif kind == "masked":
            got, path = c.scan_topk_batch_masked(metric, qs[which], k), c.batch_masked_last_path()
        else:
            got, path = c.scan_topk_batch_labeled(metric, qs[which], ql, k), c.batch_labeled_last_path()
        assert path == 8, (ctx, path)
        bb.CASES[name].check_batch(got, [bb.expected(d[w], k, pos=p) for w, p in zip(which, pos)], k, ctx)
    c.close()


@pytest.mark.parametrize("dim", [100, 200])
@pytest.mark.parametrize("name", NAMES)
def test_one_tile_holds_the_answer(pkg, monkeypatch, name, dim):
    """n = 1024 tiles + 1 row: 256 partitions would be 5 tiles each, so 205 hold rows and the last one holds tiles 1020 .. 1024.  All 20
    best rows of query j (1 .. 5) lie in tile 1023 - j, in a shuffled order - for j <= 3 a tile of the last partition, behind tiles
    that filled its lists with worse rows; query 0 has 19 of them in the last whole tile and the best one in the partial tile, the
    corpus' last row.  Row r of a query's 20 is the query with r of its set bits cleared: Hamming r, Jaccard r / |q| - no other row
    comes near"""
    last = 4 * bb.PARTITIONS - 1                                 # the last whole tile
    metric, n, k, nq = _metric(pkg, name), (last + 1) * 32 + 1, 20, 6
    rng = np.random.default_rng(300 + dim)
    qs = bb.distinct_queries(dim, nq + 2, 301 + dim)[2:]
    rows = bb.jc.random_rows(n, dim, rng)
    for j, q in enumerate(qs):
        on = np.flatnonzero(np.unpackbits(q))
        assert on.size > 2 * k
        near = np.repeat(np.unpackbits(q)[None, :], k, axis=0)
        for r in range(k):
            near[r, rng.permutation(on)[:r]] = 0
        at = (last - j) * 32 + rng.permutation(32)[:k]
        if j == 0:
            at[0] = n - 1
        rows[at] = np.packbits(near, axis=1)
    d = bb.batch_distances(name, rows, qs)
    for j in range(nq):
        best = bb.order(d[j])[:k]
        assert set((best[1:] // 32).tolist()) == {last - j} and (best[0] == n - 1 if j == 0 else best[0] // 32 == last - j)
    c = _corpus(pkg, monkeypatch, rows)
    for kk in (1, k):
        got = c.scan_topk_batch(metric, qs, kk)
        assert c.last_batch_path() == 8
        bb.CASES[name].check_batch(got, [bb.expected(d[j], kk) for j in range(nq)], kk, (name, dim, kk))
    c.close()


@pytest.mark.parametrize("name", NAMES)
def test_all_4096_bits(pkg, monkeypatch, name):
    """512-byte rows, a query of all 4096 bits against rows of all bits, none and half of them: under a radius that matches nothing that
    query stands in the Jaccard gate as |q| = 4096 with gt = 0, and its pair with a full row is the one pair that passes the gate - the
    exact test has to reject it (vg_batch_bitsl_within.hip).  64 queries: the full one under every radius, the empty one, 55 others"""
    metric, dim, n, nq = _metric(pkg, name), 512, 2531, 64
    rows, others, pos = bb.planted(dim, n, 57, 400)
    half = np.zeros(dim, dtype=np.uint8)
    half[::2] = 255
    rows[[3, 40, 2530]], rows[[4, 41, 2000]], rows[[6, 63, 64]] = 255, 0, half
    full = np.full(dim, 255, dtype=np.uint8)
    qs = np.concatenate([np.repeat(full[None, :], 8, axis=0), others[:1], others[2:]])      # (others[1] is the full query again)
    which = np.r_[np.zeros(8, dtype=np.int64), 1 + np.arange(56)]
    distinct = np.concatenate([full[None, :], others[:1], others[2:]])
    d = bb.batch_distances(name, rows, distinct)
    dh = float(d[0, 6])
    radii = [-1.0, -1.0e-30, -bb.FLT_MAX, -0.0, 0.0, dh, float(np.nextafter(np.float32(dh), np.float32(-1))), bb.FLT_MAX]
    radii += [-1.0 if s % 2 else 0.0 for s in range(56)]
    c = _corpus(pkg, monkeypatch, rows)
    for limit in (None, 5):
        got = _range_check(name, c, metric, False, qs, which, d, radii, None, limit, (name, limit))
    assert [g[2] for g in got[:3]] == [0, 0, 0] and got[3][2] == got[4][2] >= 3          # nothing; the full rows at -0.0 and at 0
    for k in (1, 20):
        ans = c.scan_topk_batch(metric, distinct, k)
        assert c.last_batch_path() == 8
        bb.CASES[name].check_batch(ans, [bb.expected(d[j], k) for j in range(len(distinct))], k, (name, k))
    c.close()
