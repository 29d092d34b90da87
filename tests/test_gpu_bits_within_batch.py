"""Hamming / Jaccard batch range scans on the integer matrix cores (vg_batch_bits_within.hip, within_batch_last_path() == 8).

The expectation is hamming_cases / jaccard_cases (numpy: exact popcounts, one float32 division; `within` over `distances`) or scan_within
on the same handle; ids, order, distance bits and `matches` compare with ==.  VG_BATCH_BITS_MIN_QUERIES=2 unless a case is about the
default.  Row bytes: 16 runs as 8 k-steps with half of them zero, 48 as 16, 100 (stride 112, ragged) and 128 as 32."""
import numpy as np
import pytest

import hamming_cases as hc
import jaccard_cases as jc

pytestmark = pytest.mark.gpu

CASES = {"hamming": hc, "jaccard": jc}
DEFAULT_MIN_QUERIES = 256               # the shipped threshold of the range form
FLT_MAX = float(np.finfo(np.float32).max)


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


def _corpus(pkg, monkeypatch, rows, min_queries="2"):
    monkeypatch.delenv("VG_BATCH_BITS_MIN_QUERIES", raising=False)
    if min_queries is not None:
        monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", min_queries)
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


def _planted(m, n, dim, nq, seed):
    """(rows, queries, index of each query among the distinct ones, the distinct ones): the helper module's corpus with the query also
    at both sides of the first tile boundary; nq queries over at most 7 distinct ones - the planted one, an all-zero one, random ones"""
    q0 = m.query(dim, seed)
    rows = m.corpus(n, dim, q0, seed + 1)
    rows[31] = rows[32] = q0
    base = np.stack([m.query(dim, seed + 2 + i) for i in range(min(nq, 7))])
    base[0], base[1] = q0, 0
    which = np.arange(nq) % len(base)
    return rows, base[which], which, base


def _radii(name, d):
    """the edge radii of one query with distances d: below zero, -0.0, 0, the 40th smallest distance (ties at the radius are all in),
    Jaccard: the float just below it / Hamming: a non-integer radius above it, +Inf, 1 (Jaccard: everything), FLT_MAX"""
    d40 = np.float32(np.sort(d)[min(39, d.size - 1)])
    other = float(np.nextafter(d40, np.float32(-np.inf))) if name == "jaccard" else float(d40) + 0.5
    return [-1.0, -0.0, 0.0, float(d40), other, float("inf"), 1.0, FLT_MAX]


def _check(m, got, ds, which, radii, limit, ctx):
    for i, (w, r) in enumerate(zip(which, radii)):
        wi, wd, wm = m.within(ds[w], r, limit=limit)
        assert got[i][2] == wm, (ctx, i, r)
        m.check(got[i], (wi, wd), (ctx, i, r))


@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("n", [33, 30001])
@pytest.mark.parametrize("dim", [16, 48, 100, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_batch_against_numpy(pkg, monkeypatch, name, dim, n, nq):
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, n, dim, nq, 11 * dim + n + nq)
    ds = [m.distances(rows, q) for q in base]
    kinds = [_radii(name, d) for d in ds]
    c = _corpus(pkg, monkeypatch, rows)
    for shift in range(0, 8, nq):                              # (two queries: four calls take them through the eight radii)
        radii = [kinds[w][(i + shift) % 8] for i, w in enumerate(which)]
        for limit in (None, 5):
            got = c.scan_within_batch(metric, qs, radii, limit=limit)
            assert c.within_batch_last_path() == 8, (name, dim, n, nq)
            _check(m, got, ds, which, radii, limit, (name, dim, n, nq, shift, limit))
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_overflow_runs_the_launch_once_more(pkg, monkeypatch, name):
    """regions of 8 keys: one query matches 40 rows or more, the others their planted rows or none"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, 2531, 128, 5, 61)
    ds = [m.distances(rows, q) for q in base]
    radii = [_radii(name, ds[0])[3], -0.0, 0.0, 0.0, -1.0]
    c = _corpus(pkg, monkeypatch, rows)
    c.set_within_batch_initial_capacity(8)
    got = c.scan_within_batch(metric, qs, radii)
    assert c.within_batch_last_path() == 8 and c.within_batch_last_launches() == 2
    assert got[0][2] >= 40 and all(g[2] <= 8 for g in got[1:])
    _check(m, got, ds, which, radii, None, name)
    c.close()


@pytest.mark.parametrize("dim", [48, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name, dim):
    """every distance of a query ties: all rows or none; and the batch equals one scan_within per query"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    qs = _planted(m, 40, dim, 6, 6)[1]
    rows = m.identical(2531, dim, 5)
    radii = [_radii(name, m.distances(rows[:1], q))[3 + i % 2] for i, q in enumerate(qs)]       # at the distance / beside it
    c = _corpus(pkg, monkeypatch, rows)
    got = c.scan_within_batch(metric, qs, radii)
    assert c.within_batch_last_path() == 8
    for i, q in enumerate(qs):
        si, sd, sm = c.scan_within(metric, q, radii[i])
        assert got[i][2] == sm and sm in (0, 2531), i
        m.check(got[i], (si, sd), (name, dim, i))
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, 30001, 128, 5, 31)
    ds = [m.distances(rows, q) for q in base]
    radii = [_radii(name, d)[3 + i] for i, d in enumerate(ds)]
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 128, [0, 0, 0], block_rows=100)
    s.append(rows)
    assert min(s.shard_rows()) > 0
    _check(m, s.scan_within_batch(metric, qs, radii), ds, which, radii, None, name)
    s.close()


@pytest.mark.parametrize("dim,nq,switch,masked,path", [(144, 64, "2", False, 5), (128, DEFAULT_MIN_QUERIES - 1, None, False, 5),
                                                       (128, DEFAULT_MIN_QUERIES, None, False, 8), (128, 64, "2", True, 5)])
def test_routing(pkg, monkeypatch, dim, nq, switch, masked, path):
    """a stride of 144 keeps the multi-query range scan; the switch unset: one query fewer than the default threshold keeps it, a batch of
    the threshold does not; the masked batch keeps it on an eligible corpus"""
    rows, qs, which, base = _planted(hc, 2531, dim, nq, 41)
    ds = [hc.distances(rows, q) for q in base]
    radii = [_radii("hamming", ds[w])[3] for w in which]
    c = _corpus(pkg, monkeypatch, rows, switch)
    allowed = np.arange(2531) % 3 != 0 if masked else None
    if masked:
        c.set_mask(bits=allowed)
    got = (c.scan_within_batch_masked if masked else c.scan_within_batch)(pkg.HAMMING, qs, radii)
    assert c.within_batch_last_path() == path, (dim, nq, c.within_batch_last_path())
    for i, w in enumerate(which):
        wi, wd, wm = hc.within(ds[w], radii[i], allowed=allowed)
        assert got[i][2] == wm
        hc.check(got[i], (wi, wd), (dim, nq, i))
    c.close()
