"""What the capped-scan tests share: the host-side expectation and a model of the host merge (no test in here).

The contract (include/vectorgpu.h, capped scans): take every row with a finite distance and a label other than NONE (masked form:
whose mask bit is set), order them by the 64-bit scan key = (distance, scan position), walk that order and keep a row iff fewer than m
rows of its label have been kept, return the first k rows kept.  `expected` is those four steps in numpy over the distances
scan_distances returns on the same handle: grouped_cases.expected with the cap."""
import numpy as np

import grouped_cases as gc

NONE = gc.NONE


def expected(dist, labels, allowed, k, m, rowids=None):
    """(rowids, distances, labels) of the first k rows kept under the cap m; allowed: None or a bool per row"""
    d = np.asarray(dist, dtype=np.float32)
    lab = np.asarray(labels, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        ok = (d < np.inf) & (lab != NONE)                       # 1. finite and labeled
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    pos = np.nonzero(ok)[0]
    pos = pos[np.lexsort((pos, d[pos]))]                        # 2. (distance, position) order
    by_label = np.argsort(lab[pos], kind="stable")              # 3. a row's rank among the rows of its label, in that order ...
    sl = lab[pos][by_label]
    start = np.r_[0, np.nonzero(sl[1:] != sl[:-1])[0] + 1] if sl.size else np.zeros(0, dtype=np.int64)
    rank = np.empty(pos.size, dtype=np.int64)
    rank[by_label] = np.arange(pos.size) - np.repeat(start, np.diff(np.r_[start, pos.size]))
    pos = pos[rank < m][:k]                                     # ... below m: kept; 4. the first k
    ids = pos + 1 if rowids is None else np.asarray(rowids)[pos]
    return ids, d[pos], lab[pos]


def merge_model(keys, labels, pos_offsets, k, m):
    """python model of vg_merge_keys_capped: (keys with global positions, labels)"""
    ents = []
    for l in range(keys.shape[0]):
        for j in range(keys.shape[1]):
            kk = int(keys[l, j])
            if kk == 0xFFFFFFFFFFFFFFFF:
                break
            if int(labels[l, j]) == NONE:
                continue
            g = (0 if pos_offsets is None else int(pos_offsets[l])) + (kk & 0xFFFFFFFF)
            ents.append((kk >> 32, g, int(labels[l, j])))
    ents.sort()
    kept, ok, ol = {}, [], []
    for img, g, lab in ents:
        if kept.get(lab, 0) >= m:
            continue
        kept[lab] = kept.get(lab, 0) + 1
        ok.append((img << 32) | g); ol.append(lab)
        if len(ok) == k:
            break
    return ok, ol


def _judge_f64(got, ref, labels, metric, q, k, m, ctx, allowed=None):
    """one f32 answer against float64 distances of every row: the cap, the count, per-row value, order, and no row left behind that
    is better than what was returned in its place - each within 1e-5 relative (batch_reference.completeness_tol)"""
    from batch_reference import completeness_tol          # (imports the GPU suite's distance bar: only where a test judges)
    gi, gd, gl = got
    if allowed is not None:                                     # masked form: a row whose bit is clear is a row without a label
        labels = np.where(np.asarray(allowed, dtype=bool), labels, NONE).astype(np.uint32)
    _, per = np.unique(labels[labels != NONE], return_counts=True)
    assert len(gi) == min(k, int(np.minimum(per, m).sum())), ctx
    pos = gi - 1
    assert (labels[pos] == gl).all() and len(set(pos.tolist())) == len(pos), ctx
    kept = dict(zip(*np.unique(gl, return_counts=True)))
    assert max(kept.values()) <= m, ctx
    q_l1 = float(np.abs(q.astype(np.float64)).sum())
    for p, d in zip(pos, gd):
        assert abs(d - ref[p]) <= completeness_tol(metric, q_l1, ref[p]), (ctx, p, d, ref[p])
    assert np.all(np.diff(gd) >= 0), ctx
    out = np.ones(len(labels), dtype=bool)
    out[pos] = False
    out &= labels != NONE
    for l in np.unique(labels[out]):
        best_left = float(ref[out & (labels == l)].min())
        if kept.get(l, 0) == m:                                 # a full label: its rows left out are no better than its worst kept row
            worst = float(gd[gl == l].max())
            assert best_left >= worst - completeness_tol(metric, q_l1, worst), (ctx, "a full label left a better row out", l)
        else:                                                   # room under the cap: only a full answer may leave a row out
            assert len(gi) == k, (ctx, l)
            assert best_left >= float(gd[-1]) - completeness_tol(metric, q_l1, gd[-1]), (ctx, "a better row left out", l)
