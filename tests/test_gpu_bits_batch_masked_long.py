"""Masked Hamming / Jaccard batches over rows of 129 to 512 bytes on the integer matrix cores (vg_batch_bitsl.hip, the gathering form:
batch_masked_last_path() == 8) against numpy.

The expectation is hamming_cases / jaccard_cases with allowed=: exact popcounts, one float32 division for Jaccard; ids, counts and
distance bits compare with ==.  VG_BATCH_BITS_MIN_QUERIES=2 unless a case is about the default.  Row bytes as in
test_gpu_bits_batch_long.py; rows of 193 .. 256 bytes serve k <= 28 (the positions take the LDS the 29th key had).  Copies of the
planted query sit at allowed positions (32, 1000) and directly in front of them at disallowed ones (31, 999); its complement at 1500."""
import numpy as np
import pytest

import hamming_cases as hc
import jaccard_cases as jc

pytestmark = pytest.mark.gpu

CASES = {"hamming": hc, "jaccard": jc}
DEFAULT_MIN_QUERIES = {192: 32, 256: 32, 384: 32, 512: 16}    # row bytes: the shipped threshold of its ladder step (measured: DESIGN.md 3.30)
ON, OFF = [32, 1000, 1500], [0, 31, 999]


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


def _data(m, n, dim, nq, seed):
    """(rows, queries, index of each query in base, base): the helper module's corpus + the plants above; nq queries over 7 distinct"""
    q0 = m.query(dim, seed)
    rows = m.corpus(n, dim, q0, seed + 1)
    rows[[31, 32, 999, 1000]] = q0
    rows[1500] = ~q0
    base = np.stack([m.query(dim, seed + 2 + i) for i in range(min(nq, 7))])
    base[0], base[1] = q0, 0
    which = np.arange(nq) % len(base)
    return rows, base[which], which, base


def _mask(kind, n, seed):
    a = np.zeros(n, dtype=bool)
    if kind == "all":
        a[:] = True
    elif kind == "one":
        a[32] = True
    elif kind == "block":
        a[1000:2000] = True
        a[[0, n - 1]] = True
    else:
        count = {"n32": 32, "n33": 33, "sparse": (3 * n) // 100, "dense": (9 * n) // 10}[kind]
        free = np.setdiff1d(np.arange(n), ON + OFF)
        a[np.random.default_rng(seed).choice(free, count - len(ON), replace=False)] = True
        a[ON] = True
    return a


def _corpus(pkg, monkeypatch, rows, min_queries="2"):
    monkeypatch.delenv("VG_BATCH_BITS_MIN_QUERIES", raising=False)
    if min_queries is not None:
        monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", min_queries)
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


def _same_as_single_scans(c, metric, qs, k, got):
    for i, q in enumerate(qs):
        si, sd = c.scan_topk_masked(metric, q, k)
        assert got[2][i] == len(si) and got[0][i].tolist() == si.tolist(), i
        assert np.array_equal(got[1][i].astype(np.float32).view(np.uint32), sd.astype(np.float32).view(np.uint32)), i


def _batch(m, c, metric, ds, which, allowed, k, ctx, path=8):
    """one masked batch on `c` against numpy (ds: the distances of the distinct queries); returns the answer"""
    got = c.scan_topk_batch_masked(metric, ds[1][which], k)
    if path is not None:
        assert c.batch_masked_last_path() == path, (ctx, k, c.batch_masked_last_path())
    want = [m.expected(d, k, allowed=allowed) for d in ds[0]]
    m.check_batch(got, [want[w] for w in which], k, (ctx, k))
    return got


@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("dim", [144, 200, 256, 272, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_masked_batch_against_numpy(pkg, monkeypatch, name, dim, nq):
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 30001
    rows, qs, which, base = _data(m, n, dim, nq, 17 * dim + nq)
    ds = ([m.distances(rows, q) for q in base], base)          # computed once, shared by every mask and k
    kmax = 28 if 192 < dim <= 256 else 32
    c = _corpus(pkg, monkeypatch, rows)
    for kind in ("all", "one", "n32", "n33", "sparse", "dense", "block"):
        allowed = _mask(kind, n, dim + nq)
        assert c.set_mask(bits=allowed) == int(allowed.sum())
        for k in (1, 20, kmax):
            ids, dist, cnt = _batch(m, c, metric, ds, which, allowed, k, (name, dim, nq, kind))
            if kind == "one":
                assert cnt.tolist() == [1] * nq and ids[:, 0].tolist() == [33] * nq
            if kind == "all":
                pi, pd, pc = c.scan_topk_batch(metric, qs, k)
                assert np.array_equal(ids, pi) and dist.tobytes() == pd.tobytes() and np.array_equal(cnt, pc)
        _batch(m, c, metric, ds, which, allowed, kmax + 1, (name, dim, nq, kind), path=5)   # lists that do not fit keep the multi-query scan
    c.close()


@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_one_k_slice_at_a_time(pkg, monkeypatch, name, dim):
    """queries whose set bits lie in one quarter of the row; the even positions are allowed, so entries 31 | 32 of the list are rows
    62 | 64: rows equal to the queries there, and copies at the disallowed rows in between"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    qs = np.zeros((5, dim), dtype=np.uint8)
    for s in range(4):
        qs[s, s * dim // 4:(s + 1) * dim // 4] = hc.query(dim // 4, 50 + s) | 1
    qs[4] = 255
    rows = m.corpus(200, dim, qs[0], 55)
    rows[[14, 60, 62, 64, 138]] = qs
    rows[[61, 63, 65]] = qs[1:4]
    allowed = np.arange(200) % 2 == 0
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=allowed)
    ds = ([m.distances(rows, q) for q in qs], qs)
    for k in (5, 28 if dim == 256 else 32):
        _batch(m, c, metric, ds, np.arange(5), allowed, k, (name, dim))
    c.close()


@pytest.mark.parametrize("dim", [200, 384])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name, dim):
    """every distance ties: the first k allowed positions; and the batch equals one scan_topk_masked per query"""
    m, metric, n, k = CASES[name], getattr(pkg, name.upper()), 2531, 20
    rows = m.identical(n, dim, 5)
    qs = np.stack([m.query(dim, 6 + i) for i in range(5)])
    allowed = _mask("sparse", n, 8)
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=allowed)
    got = _batch(m, c, metric, ([m.distances(rows, q) for q in qs], qs), np.arange(5), allowed, k, (name, dim))
    assert all(ids.tolist() == (np.flatnonzero(allowed)[:k] + 1).tolist() for ids in got[0])
    _same_as_single_scans(c, metric, qs, k, got)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_staged_form(pkg, monkeypatch, name):
    """2.1M allowed rows: 65 625 virtual tiles, the pre-pass and several stages, against scan_topk_masked per query on the same handle"""
    m, metric, n, k = CASES[name], getattr(pkg, name.upper()), 2_400_000, 20
    q0 = m.query(144, 21)
    rows = hc.corpus(n, 144, q0, 22)
    rows[[31, 32, 999, 1000]] = q0                             # (31 and 999 are disallowed, 32 and 1000 allowed)
    qs = np.stack([q0, np.zeros_like(q0), m.query(144, 23)])
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=np.arange(n) % 8 != 7)
    got = c.scan_topk_batch_masked(metric, qs, k)
    assert c.batch_masked_last_path() == 8 and got[0][0, :4].tolist() == [1, 33, 65, 1001]   # (the corpus' own copies at 63 and n - 1 are disallowed too)
    _same_as_single_scans(c, metric, qs, k, got)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 30001
    rows, qs, which, base = _data(m, n, 272, 5, 31)
    allowed = _mask("sparse", n, 32)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 272, [0, 0, 0], block_rows=100)
    s.append(rows)
    s.set_mask(bits=allowed)
    assert min(s.shard_rows()) > 0
    _batch(m, s, metric, ([m.distances(rows, q) for q in base], base), which, allowed, 20, name, path=None)   # (a shard handle does not expose its batch path)
    s.close()


@pytest.mark.parametrize("dim", sorted(DEFAULT_MIN_QUERIES))
def test_default_routing(pkg, monkeypatch, dim):
    """the switch unset: one query fewer than the step's shipped threshold keeps the multi-query scan, the threshold takes the matrix cores"""
    n, min_q = 2531, DEFAULT_MIN_QUERIES[dim]
    rows, qs, which, base = _data(hc, n, dim, min_q, 41)
    allowed = _mask("sparse", n, 42)
    c = _corpus(pkg, monkeypatch, rows, min_queries=None)
    c.set_mask(bits=allowed)
    ds = ([hc.distances(rows, q) for q in base], base)
    for nq, path in ((min_q - 1, 5), (min_q, 8)):
        _batch(hc, c, pkg.HAMMING, ds, which[:nq], allowed, 20, nq, path=path)
    c.close()
