"""Masked Hamming / Jaccard batch range scans on the integer matrix cores (vg_batch_bits_within.hip, the gathering form:
within_batch_last_path() == 8) against numpy.

The expectation is hamming_cases / jaccard_cases `within(distances, r, limit=, allowed=)`: exact popcounts and one float32 division; ids,
order, distance bits and `matches` compare with ==.  VG_BATCH_BITS_MIN_QUERIES=2 unless a case is about the default; the form takes 128
queries or more whatever the switch says.  The planted query sits at an allowed position (32) and directly in front of it at a
disallowed one (31).  Row bytes: 16 runs as 8 k-steps with half of them zero, 100 (stride 112, ragged) and 128 as 32."""
import numpy as np
import pytest

import hamming_cases as hc
from test_gpu_bits_batch_masked import _mask
from test_gpu_bits_within_batch import CASES, _corpus, _planted, _radii, pkg  # noqa: F401 (pkg: the module's fixture)

pytestmark = pytest.mark.gpu

FLOOR = 128                             # queries the form needs whatever the switch says: half a workgroup's slots
DEFAULT_MIN_QUERIES = 128               # the shipped threshold (measured: DESIGN.md 3.31) - the floor itself


def _case(m, name, n, dim, nq, allowed, seed):
    """(rows, queries, which, per distinct query its distances, per query its radius): the 7 distinct queries and the 8 edge radii -
    taken over the ALLOWED rows' distances - cycle over the batch, so that every query meets every radius"""
    rows, qs, which, base = _planted(m, n, dim, nq, seed)
    ds = [m.distances(rows, q) for q in base]
    kinds = [_radii(name, d[allowed]) for d in ds]
    return rows, qs, which, ds, [kinds[w][i % 8] for i, w in enumerate(which)]


def _check(m, got, ds, which, radii, limit, allowed, ctx):
    want = {}
    for i, (w, r) in enumerate(zip(which, radii)):
        key = (w, np.float64(r).tobytes())                     # (-0.0 and 0.0 apart)
        if key not in want:
            want[key] = m.within(ds[w], r, limit=limit, allowed=allowed)
        wi, wd, wm = want[key]
        assert got[i][2] == wm, (ctx, i, r)
        m.check(got[i], (wi, wd), (ctx, i, r))


@pytest.mark.parametrize("kind", ["all", "one", "n32", "n33", "sparse", "block"])
@pytest.mark.parametrize("nq", [FLOOR, 257])
@pytest.mark.parametrize("dim", [16, 100, 128])
@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_masked_batch_against_numpy(pkg, monkeypatch, name, dim, nq, kind):
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 30001
    allowed = _mask(kind, n, dim + nq)
    rows, qs, which, ds, radii = _case(m, name, n, dim, nq, allowed, 13 * dim + nq)
    c = _corpus(pkg, monkeypatch, rows)
    assert c.set_mask(bits=allowed) == int(allowed.sum())
    for limit in (None, 5):
        got = c.scan_within_batch_masked(metric, qs, radii, limit=limit)
        assert c.within_batch_last_path() == 8, (name, dim, nq, kind)
        _check(m, got, ds, which, radii, limit, allowed, (name, dim, nq, kind, limit))
        if allowed[32] and not allowed[31]:                     # query 42: the planted one at radius 0 - position 32, never 31
            assert (which[42], radii[42]) == (0, 0.0) and 33 in got[42][0] and 32 not in got[42][0]
        if kind == "all":
            for a, b in zip(got, c.scan_within_batch(metric, qs, radii, limit=limit)):
                assert a[2] == b[2] and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_overflow_runs_the_launch_once_more(pkg, monkeypatch, name):
    """regions of 8 keys: one query matches 40 allowed rows or more, the others their planted row or none"""
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 2531
    allowed = _mask("sparse", n, 62) | (np.arange(n) % 5 == 2)
    rows, qs, which, ds, _ = _case(m, name, n, 128, FLOOR, allowed, 61)
    radii = [_radii(name, ds[0][allowed])[3]] + [[-0.0, 0.0, 0.0, -1.0][i % 4] for i in range(1, FLOOR)]
    c = _corpus(pkg, monkeypatch, rows)
    c.set_mask(bits=allowed)
    c.set_within_batch_initial_capacity(8)
    got = c.scan_within_batch_masked(metric, qs, radii)
    assert c.within_batch_last_path() == 8 and c.within_batch_last_launches() == 2
    assert got[0][2] >= 40 and all(g[2] <= 8 for g in got[1:])
    _check(m, got, ds, which, radii, None, allowed, name)
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_mask_lifecycle(pkg, monkeypatch, name):
    """the position list follows the mask: shared with the masked top-k batch, rebuilt behind a second mask and behind a cleared one"""
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 5000
    rows, qs, which, ds, _ = _case(m, name, n, 32, FLOOR, np.ones(n, dtype=bool), 51)
    c = _corpus(pkg, monkeypatch, rows)
    for step, kind in enumerate(("sparse", "block", "n33")):
        allowed = _mask(kind, n, 52 + step)
        if step == 2:
            c.clear_mask()
        c.set_mask(bits=allowed)
        if step == 0:                                           # the top-k batch builds the list, the range batch finds it
            ids, dist, cnt = c.scan_topk_batch_masked(metric, qs, 20)
            assert c.batch_masked_last_path() == 8
            m.check_batch((ids, dist, cnt), [m.expected(ds[w], 20, allowed=allowed) for w in which], 20, name)
        radii = [_radii(name, ds[w][allowed])[3 + i % 3] for i, w in enumerate(which)]
        got = c.scan_within_batch_masked(metric, qs, radii)
        assert c.within_batch_last_path() == 8, kind
        _check(m, got, ds, which, radii, None, allowed, (name, kind))
    c.close()


@pytest.mark.parametrize("dim,nq,switch,path", [(128, FLOOR - 1, "2", 5), (128, FLOOR, "2", 8), (128, DEFAULT_MIN_QUERIES - 1, None, 5),
                                                (128, DEFAULT_MIN_QUERIES, None, 8), (144, 256, "2", 5)])
def test_routing(pkg, monkeypatch, dim, nq, switch, path):
    """below the floor the switch cannot take a batch off the multi-query range scan; the switch unset: the shipped default; a stride of
    144 keeps the multi-query range scan"""
    n = 2531
    allowed = np.arange(n) % 3 != 0
    rows, qs, which, ds, _ = _case(hc, "hamming", n, dim, nq, allowed, 41)
    radii = [_radii("hamming", ds[w][allowed])[3] for w in which]
    c = _corpus(pkg, monkeypatch, rows, switch)
    c.set_mask(bits=allowed)
    got = c.scan_within_batch_masked(pkg.HAMMING, qs, radii)
    assert c.within_batch_last_path() == path, (dim, nq, c.within_batch_last_path())
    _check(hc, got, ds, which, radii, None, allowed, (dim, nq))
    c.close()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
def test_three_shards(pkg, monkeypatch, name):
    m, metric, n = CASES[name], getattr(pkg, name.upper()), 30001
    allowed = _mask("sparse", n, 32)
    rows, qs, which, ds, radii = _case(m, name, n, 128, FLOOR, allowed, 31)
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    s = pkg.Shards(pkg.U8, 128, [0, 0, 0], block_rows=100)
    s.append(rows)
    s.set_mask(bits=allowed)
    assert min(s.shard_rows()) > 0
    _check(m, s.scan_within_batch_masked(metric, qs, radii), ds, which, radii, None, allowed, name)
    s.close()
