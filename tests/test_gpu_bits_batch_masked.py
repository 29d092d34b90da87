"""Masked Hamming / Jaccard batches on the integer matrix cores (vg_batch_bits.hip, the gathering form: batch_masked_last_path() == 8)
against numpy.

The expectation is hamming_cases / jaccard_cases with allowed=: exact integer popcounts and, for Jaccard, one float32 division; ids,
counts and distance bits compare with ==.  Every case lowers VG_BATCH_BITS_MIN_QUERIES to 2 before it creates its corpus.  Copies of
the planted query sit at allowed positions (32, 1000) and directly in front of them at disallowed ones (31, 999); its complement at an
allowed one (1500)."""
import numpy as np
import pytest

import hamming_cases as hc
import jaccard_cases as jc

pytestmark = pytest.mark.gpu

CASES = {"hamming": hc, "jaccard": jc}
DEFAULT_MIN_QUERIES = 64                # the shipped threshold of the masked form (measured: DESIGN.md 3.29)
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


def _metric(pkg, name):
    return pkg.HAMMING if name == "hamming" else pkg.JACCARD


def _data(m, n, dim, nq, seed):
    """(rows, queries, index of each query in base, base): the helper module's corpus + the plants above; nq queries over 7 distinct"""
    q0 = m.query(dim, seed)
    rows = m.corpus(n, dim, q0, seed + 1)
    rows[[31, 32, 999, 1000]] = q0
    rows[1500] = ~q0
    base = np.stack([m.query(dim, seed + 2 + i) for i in range(min(nq, 7))])
    base[0] = q0
    base[1] = 0
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
        count = {"n32": 32, "n33": 33, "sparse": (3 * n) // 100}[kind]
        free = np.setdiff1d(np.arange(n), ON + OFF)
        a[np.random.default_rng(seed).choice(free, count - len(ON), replace=False)] = True
        a[ON] = True
    return a


def _corpus(pkg, monkeypatch, rows, min_queries="2"):
    if min_queries is None:
        monkeypatch.delenv("VG_BATCH_BITS_MIN_QUERIES", raising=False)
    else:
        monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", min_queries)
    c = pkg.Corpus(pkg.U8, rows.shape[1])
    c.append(rows)
    return c


def _batch(m, c, metric, rows, qs, which, base, allowed, k, ctx, path=8):
    """one masked batch on `c` against numpy; returns the answer"""
    got = c.scan_topk_batch_masked(metric, qs, k)
    if path is not None:
        assert c.batch_masked_last_path() == path, (ctx, c.batch_masked_last_path())
    want = [m.expected(m.distances(rows, q), k, allowed=allowed) for q in base]
    m.check_batch(got, [want[w] for w in which], k, ctx)
    return got


@pytest.mark.parametrize("kind", ["all", "one", "n32", "n33", "sparse", "block"])
@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("dim", [16, 100, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_masked_batch_against_numpy(pkg, monkeypatch, name, dim, nq, kind):
    m, metric, n = CASES[name], _metric(pkg, name), 30001
    rows, qs, which, base = _data(m, n, dim, nq, 17 * dim + nq)
    allowed = _mask(kind, n, dim + nq)
    c = _corpus(pkg, monkeypatch, rows)
    assert c.set_mask(bits=allowed) == int(allowed.sum())
    for k in (1, 20, 32):
        ids, dist, cnt = _batch(m, c, metric, rows, qs, which, base, allowed, k, (name, dim, nq, kind, k))
        if kind == "one":
            assert cnt.tolist() == [1] * nq and ids[:, 0].tolist() == [33] * nq
        if kind == "all":
            pi, pd, pc = c.scan_topk_batch(metric, qs, k)
            assert np.array_equal(ids, pi) and dist.tobytes() == pd.tobytes() and np.array_equal(cnt, pc)
    _batch(m, c, metric, rows, qs, which, base, allowed, 33, (name, dim, nq, kind, 33), path=5)   # lists of more than 32 keys keep the multi-query scan
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_staged_form(pkg, monkeypatch, name):
    """2.1M allowed rows: more than 65 536 virtual tiles, the pre-pass and several stages"""
    m, metric, n = CASES[name], _metric(pkg, name), 2_400_000
    rows, qs, which, base = _data(m, n, 16, 3, 21)
    allowed = np.arange(n) % 8 != 7                             # (31 and 999 are disallowed, 32 and 1000 allowed)
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=allowed)
    _batch(m, c, metric, rows, qs, which, base, allowed, 20, name)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_lifecycle(pkg, monkeypatch, name):
    """the position list follows the mask: a second mask, a cleared one, appended rows, a clone"""
    m, metric, n, k = CASES[name], _metric(pkg, name), 5000, 20
    rows, qs, which, base = _data(m, n + 1000, 32, 5, 51)
    c = _corpus(pkg, monkeypatch, rows[:n])
    for kind in ("sparse", "block"):                            # mask A, mask B
        allowed = _mask(kind, n, 52)
        c.set_mask(bits=allowed)
        _batch(m, c, metric, rows[:n], qs, which, base, allowed, k, (name, kind))
    for drop in (c.clear_mask, lambda: (c.set_mask(bits=allowed), c.append(rows[n:]))):    # (appending rows drops the mask)
        drop()
        with pytest.raises(pkg.VectorGpuError, match="no row mask set"):
            c.scan_topk_batch_masked(metric, qs, k)
    allowed = _mask("sparse", n + 1000, 53)
    allowed[n + 7] = True
    c.set_mask(bits=allowed)
    _batch(m, c, metric, rows, qs, which, base, allowed, k, (name, "appended"))
    c2 = c.clone()
    _batch(m, c2, metric, rows, qs, which, base, allowed, k, (name, "clone"))
    c2.close()
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric, n, k = CASES[name], _metric(pkg, name), 30001, 20
    rows, qs, which, base = _data(m, n, 48, 5, 31)
    allowed = _mask("sparse", n, 32)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 48, [0, 0, 0], block_rows=100)
    s.append(rows)
    s.set_mask(bits=allowed)
    assert min(s.shard_rows()) > 0
    _batch(m, s, metric, rows, qs, which, base, allowed, k, name, path=None)   # (a shard handle does not expose its batch path)
    s.close()


def test_default_routing(pkg, monkeypatch):
    """the switch unset: one query fewer than the shipped threshold keeps the multi-query scan, the threshold takes the matrix cores"""
    n, k = 2531, 20
    rows, qs, which, base = _data(hc, n, 32, DEFAULT_MIN_QUERIES, 41)
    allowed = _mask("sparse", n, 42)
    c = _corpus(pkg, monkeypatch, rows, min_queries=None)
    c.set_mask(bits=allowed)
    for nq, path in ((DEFAULT_MIN_QUERIES - 1, 5), (DEFAULT_MIN_QUERIES, 8)):
        _batch(hc, c, pkg.HAMMING, rows, qs[:nq], which[:nq], base, allowed, k, nq, path=path)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name):
    """every distance ties: the first k allowed positions; and the batch equals one scan_topk_masked per query"""
    m, metric, n, k = CASES[name], _metric(pkg, name), 2531, 20
    rows = m.identical(n, 100, 5)
    qs = np.stack([m.query(100, 6 + i) for i in range(5)])
    allowed = _mask("sparse", n, 8)
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=allowed)
    ids, dist, cnt = _batch(m, c, metric, rows, qs, np.arange(5), qs, allowed, k, name)
    for i in range(5):
        assert ids[i].tolist() == (np.flatnonzero(allowed)[:k] + 1).tolist()
        si, sd = c.scan_topk_masked(metric, qs[i], k)
        assert cnt[i] == len(si) and ids[i].tolist() == si.tolist() and np.array_equal(dist[i].astype(np.float32).view(np.uint32), sd.astype(np.float32).view(np.uint32))
    c.close()
