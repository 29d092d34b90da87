"""Hamming / Jaccard batches on the integer matrix cores (vg_batch_bits.hip, last_batch_path() == 8) against numpy.

The expectation is hamming_cases / jaccard_cases: exact integer popcounts and, for Jaccard, one float32 division; ids, counts and
distance bits compare with ==.  Every case lowers VG_BATCH_BITS_MIN_QUERIES to 2 before it creates its corpus.  Shapes: a padded
ladder step (16 bytes), 48, a ragged row (100: stride 112) and the longest (128); 33 rows (a full tile and a 1-row tile) and 30001
(several tiles per partition, a partial last one); 2 queries (254 padding slots) and 257 (two query groups)."""
import numpy as np
import pytest

import hamming_cases as hc
import jaccard_cases as jc

pytestmark = pytest.mark.gpu

CASES = {"hamming": hc, "jaccard": jc}
DEFAULT_MIN_QUERIES = 64                # the shipped threshold (measured: DESIGN.md 3.25) - the path ships switched ON


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


def _metric(pkg, name):
    return pkg.HAMMING if name == "hamming" else pkg.JACCARD


def _queries(m, nq, dim, q0, seed):
    """nq queries over at most 7 distinct ones (a period that shares no factor with the 32 queries of a wavefront): the planted one,
    an all-zero one (Jaccard: u = |x|, distance 0 against the all-zero rows), random ones.  Returns (queries, index of each in base, base)"""
    base = np.stack([m.query(dim, seed + i) for i in range(min(nq, 7))])
    base[0] = q0
    base[1] = 0
    which = np.arange(nq) % len(base)
    return base[which], which, base


def _planted(m, n, dim, q0, seed):
    """the helper module's corpus plus rows equal to the query on both sides of the first tile boundary"""
    rows = m.corpus(n, dim, q0, seed)
    rows[31] = q0
    rows[32] = q0
    return rows


def _corpus(pkg, monkeypatch, rows, min_queries="2"):
    if min_queries is None:
        monkeypatch.delenv("VG_BATCH_BITS_MIN_QUERIES", raising=False)
    else:
        monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", min_queries)
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


def _check(m, got, rows, queries, k, ctx, ds=None):
    """the batch answer against numpy; ds: the base queries' distances, computed once by the caller and shared over its k values"""
    qs, which, base = queries
    ds = ds if ds is not None else [m.distances(rows, q) for q in base]
    want = [m.expected(d, k) for d in ds]
    m.check_batch(got, [want[w] for w in which], k, ctx)
    return ds


@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("n", [33, 30001])
@pytest.mark.parametrize("dim", [16, 48, 100, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_batch_against_numpy(pkg, monkeypatch, name, dim, n, nq):
    m, metric = CASES[name], _metric(pkg, name)
    q0 = m.query(dim, 11 * dim + n)
    rows = _planted(m, n, dim, q0, 12 * dim + n)
    qs = _queries(m, nq, dim, q0, 13 * dim + nq)
    c = _corpus(pkg, monkeypatch, rows)
    ds = None
    for k in (1, 20, 32):
        got = c.scan_topk_batch(metric, qs[0], k)
        assert c.last_batch_path() == 8, (name, dim, n, nq, k)
        ds = _check(m, got, rows, qs, k, (name, dim, n, nq, k), ds)
    got = c.scan_topk_batch(metric, qs[0], 33)                 # lists of more than 32 keys keep the multi-query scan
    assert c.last_batch_path() != 8
    _check(m, got, rows, qs, 33, (name, dim, n, nq, 33), ds)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name):
    """every distance ties: the first k positions; and the batch equals one scan_topk per query"""
    m, metric = CASES[name], _metric(pkg, name)
    dim, n, k = 100, 2531, 20
    rows = m.identical(n, dim, 5)
    qs = _queries(m, 5, dim, m.query(dim, 6), 7)
    c = _corpus(pkg, monkeypatch, rows)
    ids, dist, cnt = c.scan_topk_batch(metric, qs[0], k)
    assert c.last_batch_path() == 8
    _check(m, (ids, dist, cnt), rows, qs, k, name)
    for i in range(len(qs[0])):
        assert ids[i].tolist() == list(range(1, k + 1))
        si, sd = c.scan_topk(metric, qs[0][i], k)
        assert cnt[i] == len(si) and ids[i].tolist() == si.tolist() and np.array_equal(dist[i].astype(np.float32).view(np.uint32), sd.astype(np.float32).view(np.uint32))
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_staged_form(pkg, monkeypatch, name):
    """more than 65 536 tiles: the pre-pass and several stages"""
    m, metric = CASES[name], _metric(pkg, name)
    dim, n, k = 16, 2_100_000, 20
    q0 = m.query(dim, 21)
    rows = _planted(m, n, dim, q0, 22)
    qs = _queries(m, 3, dim, q0, 23)
    c = _corpus(pkg, monkeypatch, rows)
    got = c.scan_topk_batch(metric, qs[0], k)
    assert c.last_batch_path() == 8
    _check(m, got, rows, qs, k, name)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric = CASES[name], _metric(pkg, name)
    dim, n, k = 48, 30001, 20
    q0 = m.query(dim, 31)
    rows = _planted(m, n, dim, q0, 32)
    qs = _queries(m, 5, dim, q0, 33)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, dim, [0, 0, 0], block_rows=100)
    s.append(rows)
    assert min(s.shard_rows()) > 0
    _check(m, s.scan_topk_batch(metric, qs[0], k), rows, qs, k, name)        # (a shard handle does not expose its batch path)
    s.close()


def test_default_routing(pkg, monkeypatch):
    """the switch unset: 9 queries keep the multi-query scan, a batch of the default threshold takes the matrix cores (the path ships on)"""
    dim, n, k = 32, 2531, 20
    q0 = hc.query(dim, 41)
    rows = hc.corpus(n, dim, q0, 42)
    qs = _queries(hc, DEFAULT_MIN_QUERIES, dim, q0, 43)
    c = _corpus(pkg, monkeypatch, rows, min_queries=None)
    ds = None
    for nq, path in ((9, 5), (DEFAULT_MIN_QUERIES - 1, 5), (DEFAULT_MIN_QUERIES, 8)):
        got = c.scan_topk_batch(pkg.HAMMING, qs[0][:nq], k)
        assert c.last_batch_path() == path, (nq, c.last_batch_path())
        ds = _check(hc, got, rows, (qs[0][:nq], qs[1][:nq], qs[2]), k, nq, ds)
    c.close()
