"""A reference checker for batched top-k answers: every query of a batch against float64 distances over ALL rows - no sampling, no GPU.

The ranking reference is plain numpy over the stored values widened to float64 (datagen.storage_to_f64):

  * one matmul Q X^T ranks every row; the rows that can matter to a list of up to `kmax` entries (the kmax + SHORTLIST_EXTRA best by that
    pass) are then evaluated again element by element: squared L2 as the sum of (q - x)**2 (not qq + nn - 2 q.x, which cancels for the
    near-duplicates the tests plant), L2 as its square root, dot as -q.x, cosine as 1 - q.x / (|q| |x|) with the reference's 1.0 for a
    zero norm.  Bit-identical rows get bit-identical values that way, whatever their position.  A row outside the short list keeps the
    matmul pass' value, off by ~dim 2^-52 (qq + nn); the short list is only trusted while its last entries stay clear of that (otherwise
    the query's whole column is evaluated element by element);
  * pairs the reference's own special-casing DEFINES have no float64 meaning: a row or a query holding an Inf / NaN element (f16 / bf16
    kernels skip NaN lanes, f32 ones propagate them), or whose sum of squares leaves the float32 range (a norm that underflows is the
    reference's zero norm, one that overflows its Inf).  Those few rows (all queries) and queries (all rows) take the oracle's value
    (orc.scan_distances), widened.  Everything else is ranked without the oracle.

check_batch() then holds a batch answer (rowids = position + 1) against it with the bars the suite already uses; see there."""
import numpy as np

import datagen as dg
from test_gpu_scan import _check_float_distances

SHORTLIST_EXTRA = 16          # rows kept beyond kmax per query
NEAR_ROWS = 8                 # left-out rows looked at for the boundary gap; more near ties than that: the band check
BAND_SHARE_CAP = 0.1          # at most 1 judged query in 10 of a case may fall back to the band check
_F32_SQ_HI, _F32_SQ_LO = 1.0e37, 1.0e-37
_CHUNK_BYTES = 1 << 29        # (no intermediate beyond ~1 GB: a chunk of the distance matrix and one derived copy)


def completeness_tol(metric, q_l1, kth):
    """the slack of the suite's "nothing better was left behind" assertions (tests/test_gpu_batch_q8.py), taken over unchanged"""
    return 1e-5 * (abs(float(kth)) + (float(q_l1) * 4.0 if metric == dg.DOT else (1.0 if metric == dg.COSINE else 0.0)))


def _metric_of(metric, G, qq, nn):
    """distances of one chunk from the matmul pass (ranking only)"""
    with np.errstate(all="ignore"):
        if metric == dg.DOT:
            return -G
        if metric == dg.COSINE:
            den = np.sqrt(qq)[:, None] * np.sqrt(nn)[None, :]
            return np.where(den > 0.0, 1.0 - G / np.where(den > 0.0, den, 1.0), 1.0)
        d = np.maximum(qq[:, None] + nn[None, :] - 2.0 * G, 0.0)
        return np.sqrt(d) if metric == dg.L2 else d


def _elementwise(metric, q, x):
    """q (dim,), x (m, dim) float64 -> the m distances, element by element"""
    with np.errstate(all="ignore"):
        if metric in (dg.L2, dg.SQUARED_L2):
            d = ((q[None, :] - x) ** 2).sum(axis=1)
            return np.sqrt(d) if metric == dg.L2 else d
        dot = (q[None, :] * x).sum(axis=1)
        if metric == dg.DOT:
            return -dot
        den = np.sqrt((q * q).sum()) * np.sqrt((x * x).sum(axis=1))
        return np.where(den > 0.0, 1.0 - dot / np.where(den > 0.0, den, 1.0), 1.0)


def _out_of_range(v64):
    """vectors the float64 reference does not speak for: a non-finite element, or a sum of squares outside the float32 range"""
    with np.errstate(all="ignore"):
        ss = (v64 * v64).sum(axis=1)
    return ~np.isfinite(v64).all(axis=1) | ~(ss <= _F32_SQ_HI) | ((ss > 0.0) & (ss < _F32_SQ_LO))


class BatchReference:
    """per query the `width` best rows by (float64 distance, position): pos[i], d[i] (+Inf past the rows that can enter a list);
    enter[i] = rows whose distance is below +Inf (NaN and +Inf never enter a list, -Inf does); group[p] = the named set of bit-identical
    rows position p belongs to, or -1"""

    def __init__(self, vt, metric, kmax, pos, d, enter, q_l1, group):
        self.vt, self.metric, self.kmax = vt, metric, kmax
        self.pos, self.d, self.enter, self.q_l1, self.group = pos, d, enter, q_l1, group

    def clear_boundary(self, i, k):
        """does query i's top-k SET follow from the float64 distances alone?  Every row inside against every near row outside: a gap above
        2 tol, or a named pair of identical rows (the lower position wins: no gap to ask for)"""
        kk = int(min(k, self.enter[i]))
        if kk == 0 or self.enter[i] <= kk:
            return True
        # (a k-th best of -Inf: every row inside is at -Inf - any row above -Inf outside is clear of them, one at -Inf is a tie)
        slack = 2.0 * completeness_tol(self.metric, self.q_l1[i], self.d[i, kk - 1]) if np.isfinite(self.d[i, kk - 1]) else 0.0
        d_in, d_out = self.d[i, :kk], self.d[i, kk:kk + NEAR_ROWS]
        g_in, g_out = self.group[self.pos[i, :kk]], self.group[self.pos[i, kk:kk + NEAR_ROWS]]
        with np.errstate(invalid="ignore"):
            near = ~((d_out[None, :] - d_in[:, None]) > slack)                     # (-Inf against -Inf: NaN, a tie)
        same = (g_in[:, None] == g_out[None, :]) & (g_in[:, None] >= 0)
        if len(d_out) == NEAR_ROWS and near[kk - 1, NEAR_ROWS - 1]:
            return False                                                           # more near rows than were looked at
        return not (near & ~same).any()

    def band_share(self, k, nq=None, judged=None):
        """share of the (judged) queries whose boundary is not clear - from the reference alone"""
        nq = self.pos.shape[0] if nq is None else nq
        which = [i for i in range(nq) if judged is None or judged[i]]
        if not which:
            return 0.0
        return sum(0 if self.clear_boundary(i, k) else 1 for i in which) / len(which)


def batch_references(vt, metrics, queries, rows, orc, kmax=64, duplicates=()):
    """{metric: BatchReference} of one batch over one corpus (one matmul serves every metric).  duplicates: lists of positions that hold
    bit-identical rows, named by whoever planted them."""
    n, dim = rows.shape
    nq = queries.shape[0]
    X, Q = dg.storage_to_f64(vt, rows), dg.storage_to_f64(vt, queries)
    row_sp, q_sp = _out_of_range(X), _out_of_range(Q)
    sp_rows = np.nonzero(row_sp)[0]
    Xm, Qm = X.copy(), Q.copy()
    Xm[row_sp] = 0.0                                                               # (kept out of the matmul: their columns are patched)
    Qm[q_sp] = 0.0
    nn, qq = (Xm * Xm).sum(axis=1), (Qm * Qm).sum(axis=1)
    nn_mid = float(np.median(nn))                                                  # (the matmul pass' error scale for an ordinary row)
    group = np.full(n, -1, dtype=np.int64)
    for gi, members in enumerate(duplicates):
        members = np.asarray(members, dtype=np.int64)
        bits = np.ascontiguousarray(rows[members]).view(np.uint8)
        assert (bits == bits[0]).all(), "named duplicates must be identical rows"
        group[members] = gi
    width = min(n, kmax + SHORTLIST_EXTRA)
    out = {m: (np.zeros((nq, width), dtype=np.int64), np.full((nq, width), np.inf), np.zeros(nq, dtype=np.int64)) for m in metrics}
    step = max(1, int(_CHUNK_BYTES // (8 * n)))
    sp_block = rows[sp_rows]
    for c0 in range(0, nq, step):
        c1 = min(nq, c0 + step)
        G = Qm[c0:c1] @ Xm.T
        for metric in metrics:
            pos_o, d_o, enter_o = out[metric]
            D = _metric_of(metric, G, qq[c0:c1], nn)
            for i in range(c0, c1):
                if q_sp[i]:
                    D[i - c0] = orc.scan_distances(orc.AVX2, metric, vt, queries[i], rows).astype(np.float64)
                elif len(sp_rows):
                    D[i - c0, sp_rows] = orc.scan_distances(orc.AVX2, metric, vt, queries[i], sp_block).astype(np.float64)
            D[np.isnan(D)] = np.inf
            enter_o[c0:c1] = (D < np.inf).sum(axis=1)
            short = np.argpartition(D, width - 1, axis=1)[:, :width] if width < n else np.tile(np.arange(n), (c1 - c0, 1))
            for i in range(c0, c1):
                p = np.sort(short[i - c0])
                coarse = D[i - c0, p]
                fine = _elementwise(metric, Q[i], X[p]) if not q_sp[i] else coarse.copy()
                keep = row_sp[p] | ~(coarse < np.inf)                              # (patched pairs keep the oracle's value)
                fine[keep] = coarse[keep]
                order = np.lexsort((p, fine))
                p, fine = p[order], fine[order]
                # the short list was chosen by the matmul pass: trust it only while the entries that decide anything stay clear of that pass' error
                decide = min(width, kmax + NEAR_ROWS) - 1
                eps = 1e-9 if metric == dg.COSINE else 1e-9 * (qq[i] + nn_mid if metric != dg.DOT else np.sqrt(qq[i] * nn_mid))
                if width < n and np.isfinite(fine[decide]) and not (fine[decide] <= coarse.max() - eps) and not q_sp[i]:
                    full = _elementwise(metric, Q[i], X)
                    full[row_sp] = D[i - c0, row_sp]
                    full[np.isnan(full)] = np.inf
                    order = np.lexsort((np.arange(n), full))[:width]
                    p, fine = order, full[order]
                pos_o[i], d_o[i] = p, fine
    q_l1 = np.abs(np.where(np.isfinite(Q), Q, 0.0)).sum(axis=1)
    return {m: BatchReference(vt, m, kmax, out[m][0], out[m][1], out[m][2], q_l1, group) for m in metrics}


def check_batch(vt, metric, k, queries, rows, ids, dist, cnt, orc, duplicates=(), reference=None):
    """every query of the batch answer (ids = position + 1, dist, cnt as Corpus.scan_topk_batch returns them):

      count      cnt[i] == min(k, rows that can enter a list)
      distances  the k returned ones against orc.scan_distances over the returned rows, the suite's own bar (_check_float_distances)
      order      non-decreasing; equal distances in ascending rowid order
      complete   clear boundary (float64 gap between the k-th and the (k+1)-th best row above 2 tol): the returned SET is the float64
                 top-k set; otherwise the band check of the existing tests: no row left out is better than the k-th returned distance - tol

    Returns the number of queries that took the band check."""
    ref = reference if reference is not None else batch_references(vt, (metric,), queries, rows, orc, max(k, 1), duplicates)[metric]
    assert ref.metric == metric and ref.kmax >= k and ref.pos.shape[0] >= queries.shape[0]
    n = rows.shape[0]
    banded = 0
    for i in range(queries.shape[0]):
        m = int(cnt[i])
        kk = int(min(k, ref.enter[i]))
        assert m == kk, ("count", i, m, kk)
        if m == 0:
            continue
        got_ids = np.asarray(ids[i][:m], dtype=np.int64)
        pos = got_ids - 1
        assert pos.min() >= 0 and pos.max() < n and len(set(pos.tolist())) == m, ("rowids", i, got_ids)
        d32 = np.asarray(dist[i][:m]).astype(np.float32)
        want = orc.scan_distances(orc.AVX2, metric, vt, queries[i], rows[pos])
        try:
            _check_float_distances(d32, want, vt, metric, queries[i], rows[pos])
        except AssertionError as e:
            raise AssertionError(("distances", i) + e.args)
        assert not np.isnan(d32).any() and (d32[1:] >= d32[:-1]).all(), ("order", i, d32)
        tie = d32[1:] == d32[:-1]
        assert (got_ids[1:][tie] > got_ids[:-1][tie]).all(), ("tie order", i, got_ids, d32)
        if ref.clear_boundary(i, k):
            assert set(pos.tolist()) == set(ref.pos[i, :kk].tolist()), \
                ("top-k set", i, sorted(set(ref.pos[i, :kk].tolist()) - set(pos.tolist())), sorted(set(pos.tolist()) - set(ref.pos[i, :kk].tolist())))
        else:
            banded += 1
            left = ~np.isin(ref.pos[i], pos) & (ref.d[i] < np.inf)
            tol = completeness_tol(metric, ref.q_l1[i], d32[m - 1])
            assert not left.any() or ref.d[i][left].min() >= float(d32[m - 1]) - tol, ("left behind", i, ref.pos[i][left][:3], ref.d[i][left][:3], d32[m - 1])
    return banded
