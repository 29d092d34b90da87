"""Labeled Hamming / Jaccard batches on the integer matrix cores (vg_batch_bits.hip, the labeled form: batch_labeled_last_path() == 8)
against numpy.

The expectation is hamming_cases / jaccard_cases with allowed = (row labels == the query's label): exact integer popcounts and, for
Jaccard, one float32 division; ids, counts and distance bits compare with ==.  Every case lowers VG_BATCH_BITS_MIN_QUERIES to 2 before
it creates its corpus unless it is about routing.  Copies of the planted query (query 0) sit at positions 32 and 1000 under its own
label and directly in front of them (31, 999) under another."""
import numpy as np
import pytest

from test_gpu_bits_batch_masked import CASES, _corpus, _data, _metric, pkg   # noqa: F401  (pkg: the module's fixture)

pytestmark = pytest.mark.gpu

DEFAULT_MIN_QUERIES = 256               # the shipped threshold of the labeled form (measured: DESIGN.md 3.32); 0: through the switch only
NONE = 0xFFFFFFFF


def _labels(kind, n, nq, seed):
    """(row labels, query labels) of a layout; query 0 is the planted one"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 3, n).astype(np.uint32)
    ql = (np.arange(nq) % 3).astype(np.uint32)
    if kind == "one":
        return np.full(n, 7, np.uint32), np.full(nq, 7, np.uint32)
    if kind == "own":                                           # label 5: no row, label 6: 3 rows (fewer than k)
        lab = rng.integers(0, 257, n).astype(np.uint32)
        ql = ((np.arange(nq) + 4) % 257).astype(np.uint32)
    if kind == "none":
        lab[rng.random(n) < 0.1] = NONE
        ql[1] = 77                                              # (no row carries it)
    if kind == "n32_33":
        ql[np.arange(nq) % 4 == 0], ql[np.arange(nq) % 4 == 1] = 100, 101
    lab[[32, 1000]], lab[[31, 999]] = ql[0], {"none": NONE, "n32_33": 2}.get(kind, ql[0] + 1)
    if kind == "own":
        lab[lab == 5] = 7
        lab[np.flatnonzero(lab == 6)[3:]] = 7
    if kind == "n32_33":
        free = rng.permutation(np.setdiff1d(np.arange(n), [31, 32, 999, 1000]))
        lab[free[:30]], lab[free[30:63]] = 100, 101             # (+ the two plants: 32 rows of label 100, 33 of 101)
    return lab, ql


def _batch(m, c, metric, rows, qs, which, base, lab, ql, ks, ctx, path=8):
    """labeled batches on `c` for every k of `ks` against numpy (one sort per query, cut to each k); returns the last answer"""
    d = [m.distances(rows, q) for q in base]
    full = [m.expected(d[w], max(ks), allowed=lab == l) for w, l in zip(which, ql)]
    for k in ks:
        got = c.scan_topk_batch_labeled(metric, qs, ql, k)
        if path is not None:
            assert (c.batch_labeled_last_path() == 8) == (path == 8), (ctx, k, c.batch_labeled_last_path())
        m.check_batch(got, [(i[:k], dd[:k]) for i, dd in full], k, (ctx, k))
    return got


@pytest.mark.parametrize("kind", ["one", "three", "own", "none", "n32_33"])
@pytest.mark.parametrize("nq", [2, 257])
@pytest.mark.parametrize("dim", [16, 100, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_labeled_batch_against_numpy(pkg, monkeypatch, name, dim, nq, kind):
    m, metric, n = CASES[name], _metric(pkg, name), 30001
    rows, qs, which, base = _data(m, n, dim, nq, 17 * dim + nq)
    lab, ql = _labels(kind, n, nq, dim + nq)
    if kind == "n32_33":
        assert (int((lab == 100).sum()), int((lab == 101).sum())) == (32, 33)
    c = _corpus(pkg, monkeypatch, rows)
    c.set_labels(lab)
    ids, _, cnt = _batch(m, c, metric, rows, qs, which, base, lab, ql, (1, 32, 20), (name, dim, nq, kind))
    if kind != "one":                                           # the plants of query 0: its own label's copies, not the ones in front
        first = set(ids[0, :cnt[0]].tolist())
        assert {33, 1001} <= first and not {32, 1000} & first
    if kind == "own":
        assert cnt[1] == 0 and (nq == 2 or cnt[2] == 3)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name):
    """every distance ties: the batch equals one scan_topk_labeled per query and the multi-query scan (the switch at 0)"""
    m, metric, n, k = CASES[name], _metric(pkg, name), 2531, 20
    rows = m.identical(n, 100, 5)
    qs = np.stack([m.query(100, 6 + i) for i in range(5)])
    lab, ql = _labels("three", n, 5, 8)
    c = _corpus(pkg, monkeypatch, rows)
    c.set_labels(lab)
    ids, dist, cnt = _batch(m, c, metric, rows, qs, np.arange(5), qs, lab, ql, (k,), name)
    for i in range(5):
        si, sd = c.scan_topk_labeled(metric, qs[i], k, ql[i])
        assert cnt[i] == len(si) and ids[i, :cnt[i]].tolist() == si.tolist() and dist[i, :cnt[i]].tobytes() == sd.tobytes()
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "0")
    mi, md, mc = c.scan_topk_batch_labeled(metric, qs, ql, k)
    assert c.batch_labeled_last_path() == 5
    assert np.array_equal(ids, mi) and dist.tobytes() == md.tobytes() and np.array_equal(cnt, mc)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_staged_form(pkg, monkeypatch, name):
    """2.4M rows: 75 000 tiles, the pre-pass and several stages; label 63 sits behind the pre-pass range only - that list is seeded empty"""
    m, metric, n = CASES[name], _metric(pkg, name), 2_400_000
    rows, qs, which, base = _data(m, n, 16, 3, 21)
    lab = np.random.default_rng(22).integers(0, 63, n).astype(np.uint32)
    lab[n // 2::50] = 63
    ql = np.array([1, 63, 5], np.uint32)
    lab[[32, 1000]], lab[[31, 999]] = 1, 2
    c = _corpus(pkg, monkeypatch, rows)
    c.set_labels(lab)
    _batch(m, c, metric, rows, qs, which, base, lab, ql, (20,), name)
    c.close()


def test_switch_routing(pkg, monkeypatch):
    """one query keeps the scans, two take the matrix cores; longer rows, longer lists and a corpus without labels keep what they had"""
    n = 2531
    for dim, nq, k, path in ((32, 1, 20, 5), (32, 2, 20, 8), (144, 2, 20, 5), (32, 2, 33, 5)):
        rows, qs, which, base = _data(CASES["hamming"], n, dim, 2, 41)
        (lab, ql), qs, which = _labels("three", n, nq, 42), qs[:nq], which[:nq]
        c = _corpus(pkg, monkeypatch, rows)
        with pytest.raises(pkg.VectorGpuError, match="no labels set"):
            c.scan_topk_batch_labeled(pkg.HAMMING, qs, ql, k)
        assert c.batch_labeled_last_path() == 0
        c.set_labels(lab)
        _batch(CASES["hamming"], c, pkg.HAMMING, rows, qs, which, base, lab, ql, (k,), (dim, nq, k), path=path)
        c.close()


@pytest.mark.skipif(DEFAULT_MIN_QUERIES == 0, reason="the labeled form ships switched off: it is reached through the switch alone")
def test_default_routing(pkg, monkeypatch):
    """the switch unset: one query fewer than the shipped threshold keeps the multi-query scan, the threshold takes the matrix cores"""
    n, m = 2531, CASES["hamming"]
    rows, qs, which, base = _data(m, n, 32, DEFAULT_MIN_QUERIES, 41)
    lab, ql = _labels("three", n, DEFAULT_MIN_QUERIES, 42)
    c = _corpus(pkg, monkeypatch, rows, min_queries=None)
    c.set_labels(lab)
    for nq, path in ((DEFAULT_MIN_QUERIES - 1, 5), (DEFAULT_MIN_QUERIES, 8)):
        _batch(m, c, pkg.HAMMING, rows, qs[:nq], which[:nq], base, lab, ql[:nq], (20,), nq, path=path)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric, n = CASES[name], _metric(pkg, name), 30001
    rows, qs, which, base = _data(m, n, 128, 5, 31)
    lab, ql = _labels("three", n, 5, 32)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 128, [0, 0, 0], block_rows=100)
    s.append(rows)
    s.set_labels(lab)
    assert min(s.shard_rows()) > 0
    _batch(m, s, metric, rows, qs, which, base, lab, ql, (20,), name, path=None)   # (a shard handle does not expose its batch path)
    s.close()
