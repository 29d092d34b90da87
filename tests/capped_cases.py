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
