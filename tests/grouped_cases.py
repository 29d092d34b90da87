"""What the grouped-scan tests share: label layouts and the host-side expectation (no test in here).

The contract (include/vectorgpu.h, grouped scans): take every row with a finite distance and a label other than NONE (masked form:
whose mask bit is set), order them by the 64-bit scan key = (distance, scan position), keep the first row of each label, return the
first k rows kept.  `expected` is those three steps in numpy over the distances scan_distances returns on the same handle."""
import numpy as np

import labeled_cases as lc

N = lc.N
NONE = lc.NONE


def expected(dist, labels, allowed, k, rowids=None):
    """(rowids, distances, labels) of the first k group representatives; allowed: None or a bool per row"""
    d = np.asarray(dist, dtype=np.float32)
    lab = np.asarray(labels, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        ok = (d < np.inf) & (lab != NONE)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    pos = np.nonzero(ok)[0]
    pos = pos[np.lexsort((pos, d[pos]))]                        # 1. (distance, position) order
    _, first = np.unique(lab[pos], return_index=True)           # 2. the first row of each label ...
    pos = pos[np.sort(first)][:k]                               # ... in that order; 3. the first k
    ids = pos + 1 if rowids is None else np.asarray(rowids)[pos]
    return ids, d[pos], lab[pos]


def assert_same(got, ids, dist, labels, ctx=None):
    gi, gd, gl = got
    assert gi.tolist() == np.asarray(ids).tolist(), ctx
    assert gl.tolist() == np.asarray(labels).tolist(), ctx
    assert np.array_equal(np.asarray(gd).astype(np.float32).view(np.uint32), np.asarray(dist, dtype=np.float32).view(np.uint32)), ctx


def hot(dist, n_hot):
    """the nearest n_hot rows (by (distance, position)) get label 1, every other row a label of its own (>= 2)"""
    d = np.asarray(dist, dtype=np.float32)
    n = d.size
    order = np.lexsort((np.arange(n), d))
    lab = (np.arange(n) + 2).astype(np.uint32)
    lab[order[:n_hot]] = 1
    return lab


def layouts(n, dist, seed=0):
    """name -> labels per row; `dist`: the distances of the query the `hot` layout is built around"""
    rng = np.random.default_rng(2000 + seed)
    out = {}
    out["uniform5"] = rng.integers(0, 5, n).astype(np.uint32)
    out["runs200"] = (np.arange(n) // 200).astype(np.uint32)
    out["all_one"] = np.full(n, 7, dtype=np.uint32)
    out["unique"] = np.arange(n).astype(np.uint32)
    lab = rng.integers(0, 40, n).astype(np.uint32); lab[rng.random(n) < 0.3] = NONE
    out["some_none"] = lab
    out["pairs"] = (np.arange(n) // 2).astype(np.uint32)
    out["hot"] = hot(dist, 500)
    return out


def key(d, pos):
    """the 64-bit scan key of (float distance, position)"""
    b = int(np.float32(d).view(np.uint32))
    s = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
    return (s << 32) | int(pos)


def merge_model(keys, labels, pos_offsets, k):
    """numpy / python model of vg_merge_keys_grouped: (keys with global positions, labels)"""
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
    seen, ok, ol = set(), [], []
    for img, g, lab in ents:
        if lab in seen:
            continue
        seen.add(lab)
        ok.append((img << 32) | g); ol.append(lab)
        if len(ok) == k:
            break
    return ok, ol
