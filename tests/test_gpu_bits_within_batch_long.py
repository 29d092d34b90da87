"""Hamming / Jaccard batch range scans over rows of 129 to 512 bytes on the integer matrix cores (vg_batch_bitsl_within.hip,
within_batch_last_path() == 8).

The expectation is hamming_cases / jaccard_cases (numpy: exact popcounts, one float32 division; `within` over `distances`) or scan_within
on the same handle; ids, order, distance bits and `matches` compare with ==.  VG_BATCH_BITS_MIN_QUERIES=2 unless a case is about
routing.  Row bytes: 144 and 200 (stride 208, ragged) run as 2 K-slices x 24 / 32 k-steps with 128 queries per workgroup, 256 fills that
step, 272 is the first of 4 K-slices with 64 queries per workgroup, 384 and 512 fill those.  A batch needs one workgroup of queries."""
import numpy as np
import pytest

import hamming_cases as hc
from test_gpu_bits_within_batch import CASES, _check, _corpus, _planted, _radii, pkg  # noqa: F401 (pkg: the module's fixture)

pytestmark = pytest.mark.gpu

DEFAULT_MIN_QUERIES = {256: 256, 512: 64}      # the shipped thresholds of the two K-splits (measured: DESIGN.md 3.28); 0: switched off


def _qpb(dim):
    """queries per workgroup"""
    return 128 if (dim + 15) // 16 * 16 <= 256 else 64


@pytest.mark.parametrize("full_slice", [False, True])
@pytest.mark.parametrize("n", [33, 30001])
@pytest.mark.parametrize("dim", [144, 200, 256, 272, 384, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_batch_against_numpy(pkg, monkeypatch, name, dim, n, full_slice):
    """one workgroup of queries, or 257: a full slice of 2 / 4 query groups and a slice of one real query.  7 distinct queries and 8
    radii cycle over the batch: every query meets every radius, in every accumulator quad and both lane halves"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    nq = 257 if full_slice else _qpb(dim)
    rows, qs, which, base = _planted(m, n, dim, nq, 11 * dim + n + nq)
    ds = [m.distances(rows, q) for q in base]
    kinds = [_radii(name, d) for d in ds]
    radii = [kinds[w][i % 8] for i, w in enumerate(which)]
    c = _corpus(pkg, monkeypatch, rows)
    for limit in (None, 5):
        got = c.scan_within_batch(metric, qs, radii, limit=limit)
        assert c.within_batch_last_path() == 8, (name, dim, n, nq)
        _check(m, got, ds, which, radii, limit, (name, dim, n, nq, limit))
    c.close()


@pytest.mark.parametrize("dim", [256, 512])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_one_k_slice_at_a_time(pkg, monkeypatch, name, dim):
    """queries whose set bits lie in one quarter of the row, rows equal to them, and all ones against all ones (|q| = |x| = i = 8 dim)
    at the radii 0, -0.0 and -1 (Jaccard, 512 bytes: the pair that passes the gate's stand-in for `matches nothing`)"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    base = np.zeros((5, dim), dtype=np.uint8)
    for s in range(4):
        base[s, s * dim // 4:(s + 1) * dim // 4] = hc.query(dim // 4, 50 + s) | 1
    base[4] = 255
    rows = m.corpus(70, dim, base[0], 55)
    rows[[7, 30, 31, 32, 69]] = base
    rows[40] = 255
    which = np.arange(_qpb(dim)) % 5
    ds = [m.distances(rows, q) for q in base]
    radii = [[0.0, -0.0, -1.0][i // 5 % 3] if w == 4 else [0.0, float(np.sort(ds[w])[2])][i // 5 % 2] for i, w in enumerate(which)]
    c = _corpus(pkg, monkeypatch, rows)
    got = c.scan_within_batch(metric, base[which], radii)
    assert c.within_batch_last_path() == 8
    assert (got[4][2], got[9][2], got[14][2]) == (2, 2, 0)         # all ones: rows 40 and 69 at 0 and -0.0, nothing below zero
    _check(m, got, ds, which, radii, None, (name, dim))
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_overflow_runs_the_launch_once_more(pkg, monkeypatch, name):
    """regions of 8 keys: one query matches 40 rows or more, the others their planted rows or none"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    rows, qs, which, base = _planted(m, 2531, 256, 128, 61)
    ds = [m.distances(rows, q) for q in base]
    radii = [_radii(name, ds[0])[3]] + [[-0.0, 0.0, 0.0, -1.0][i % 4] for i in range(1, 128)]
    c = _corpus(pkg, monkeypatch, rows)
    c.set_within_batch_initial_capacity(8)
    got = c.scan_within_batch(metric, qs, radii)
    assert c.within_batch_last_path() == 8 and c.within_batch_last_launches() == 2
    assert got[0][2] >= 40 and all(g[2] <= 8 for g in got[1:])
    _check(m, got, ds, which, radii, None, name)
    c.close()


@pytest.mark.parametrize("dim", [200, 384])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_identical_rows_and_single_scans(pkg, monkeypatch, name, dim):
    """every distance of a query ties: all rows or none; and the batch equals one scan_within per query"""
    m, metric = CASES[name], getattr(pkg, name.upper())
    qs = _planted(m, 40, dim, _qpb(dim), 6)[1]
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
    rows, qs, which, base = _planted(m, 30001, 272, 64, 31)
    ds = [m.distances(rows, q) for q in base]
    radii = [_radii(name, ds[w])[3 + i % 5] for i, w in enumerate(which)]
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 272, [0, 0, 0], block_rows=100)
    s.append(rows)
    assert min(s.shard_rows()) > 0
    _check(m, s.scan_within_batch(metric, qs, radii), ds, which, radii, None, name)
    s.close()


def _default_cases():
    """the switch unset: one query below the shipped default keeps path 5, a batch of it takes path 8; a default of 0: nothing does"""
    for dim, d in DEFAULT_MIN_QUERIES.items():
        yield from [(dim, d - 1, None, False, 5), (dim, d, None, False, 8)] if d else [(dim, 257, None, False, 5)]


@pytest.mark.parametrize("dim,nq,switch,masked,path", [(528, 128, "2", False, 5), (256, 127, "2", False, 5), (256, 128, "2", False, 8),
                                                       (512, 63, "2", False, 5), (512, 64, "2", False, 8), (256, 128, "2", True, 5)]
                         + list(_default_cases()))
def test_routing(pkg, monkeypatch, dim, nq, switch, masked, path):
    """a stride of 528 keeps the multi-query range scan; below one workgroup of queries the switch cannot take a batch off it; the masked
    batch keeps it on an eligible corpus; the switch unset: the shipped defaults"""
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
