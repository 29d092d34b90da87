"""Hamming / Jaccard batches over rows of 129 to 512 bytes on the integer matrix cores (vg_batch_bitsl.hip, last_batch_path() == 8).

The expectation is hamming_cases / jaccard_cases (numpy: exact popcounts, one float32 division) or scan_topk on the same handle; ids,
counts and distance bits compare with ==.  VG_BATCH_BITS_MIN_QUERIES=2 unless a case is about the default.  Row bytes: 144 and 200
(stride 208, ragged) run as 2 K-slices x 24 / 32 k-steps, 256 fills that step, 272 is the first of 4 K-slices, 384 and 512 fill those."""
import numpy as np
import pytest

import hamming_cases as hc
import jaccard_cases as jc

pytestmark = pytest.mark.gpu

CASES = {"hamming": hc, "jaccard": jc}
DEFAULT_MIN_QUERIES = 32                # the shipped threshold of rows beyond 128 bytes, every ladder step (measured: DESIGN.md 3.26)


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


def _same_as_scans(c, metric, qs, k, got):
    for i, q in enumerate(qs):
        si, sd = c.scan_topk(metric, q, k)
        assert got[2][i] == len(si) and got[0][i].tolist() == si.tolist(), i
        assert np.array_equal(got[1][i].astype(np.float32).view(np.uint32), sd.astype(np.float32).view(np.uint32)), i


@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("n", [33, 30001])
@pytest.mark.parametrize("dim", [144, 200, 256, 272, 384, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_batch_against_numpy(pkg, monkeypatch, name, dim, n, nq):
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, n, dim, nq, 11 * dim + n + nq)
    ds = [m.distances(rows, q) for q in base]
    c = _corpus(pkg, monkeypatch, rows)
    for k in (1, 20, 32, 33):
        got = c.scan_topk_batch(metric, qs, k)
        assert k == 32 or (c.last_batch_path() == 8) == (k < 32), (name, dim, n, nq, k, c.last_batch_path())
        m.check_batch(got, [m.expected(ds[w], k) for w in which], k, (name, dim, n, nq, k))
    c.close()


@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_one_k_slice_at_a_time(pkg, monkeypatch, name, dim):
    """queries whose set bits lie in one quarter of the row, rows equal to them, and all ones against all ones (|q| = |x| = i = 8 dim)"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    qs = np.zeros((5, dim), dtype=np.uint8)
    for s in range(4):
        qs[s, s * dim // 4:(s + 1) * dim // 4] = hc.query(dim // 4, 50 + s) | 1
    qs[4] = 255
    rows = m.corpus(70, dim, qs[0], 55)
    rows[[7, 30, 31, 32, 69]] = qs
    rows[40] = 255
    c = _corpus(pkg, monkeypatch, rows)
    ds = [m.distances(rows, q) for q in qs]
    for k in (5, 29):                                          # (29: the longest lists beside two 64 KiB tiles - all of the LDS)
        got = c.scan_topk_batch(metric, qs, k)
        assert c.last_batch_path() == 8
        m.check_batch(got, [m.expected(d, k) for d in ds], k, (name, dim, k))
    c.close()


@pytest.mark.parametrize("dim", [200, 384])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name, dim):
    """every distance ties: the first k positions; and the batch equals one scan_topk per query"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    qs = _planted(m, 40, dim, 5, 6)[1]
    c = _corpus(pkg, monkeypatch, m.identical(2531, dim, 5))
    got = c.scan_topk_batch(metric, qs, 20)
    assert c.last_batch_path() == 8
    assert all(ids.tolist() == list(range(1, 21)) for ids in got[0])
    _same_as_scans(c, metric, qs, 20, got)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_staged_form(pkg, monkeypatch, name):
    """more than 65 536 tiles: the pre-pass and several stages, against scan_topk per query on the same handle"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    q0 = m.query(144, 21)
    rows = hc.corpus(2_100_000, 144, q0, 22)
    rows[31] = rows[32] = q0
    qs = np.stack([q0, np.zeros_like(q0), m.query(144, 23)])
    c = _corpus(pkg, monkeypatch, rows)
    got = c.scan_topk_batch(metric, qs, 20)
    assert c.last_batch_path() == 8
    _same_as_scans(c, metric, qs, 20, got)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, 30001, 272, 5, 31)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 272, [0, 0, 0], block_rows=100)
    s.append(rows)
    assert min(s.shard_rows()) > 0
    m.check_batch(s.scan_topk_batch(metric, qs, 20), [m.expected(m.distances(rows, q), 20) for q in base], 20, name)
    s.close()


@pytest.mark.parametrize("dim,nq,switch,path", [(528, 64, "2", 5), (256, 9, None, 5), (256, DEFAULT_MIN_QUERIES - 1, None, 5), (256, DEFAULT_MIN_QUERIES, None, 8)])
def test_routing(pkg, monkeypatch, dim, nq, switch, path):
    """a stride of 528 keeps the multi-query scan; the switch unset: 9 queries and one fewer than the default threshold keep it too, a batch of the threshold does not"""
    rows, qs, which, base = _planted(hc, 2531, dim, nq, 41)
    c = _corpus(pkg, monkeypatch, rows, switch)
    got = c.scan_topk_batch(pkg.HAMMING, qs, 20)
    assert c.last_batch_path() == path, (dim, nq, c.last_batch_path())
    ds = [hc.distances(rows, q) for q in base]
    hc.check_batch(got, [hc.expected(ds[w], 20) for w in which], 20, (dim, nq))
    c.close()
