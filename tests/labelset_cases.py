"""What the label-set tests share: layouts, the sets asked for, the host-side "allowed" rule and the mixes of a batch (no test in here).

Shapes, row count and data are the labeled scans' (labeled_cases): 3001 rows is no multiple of 64 or of any rows-per-batch."""
import numpy as np

import labeled_cases as lc

NONE = lc.NONE
ABSENT = lc.ABSENT
NQS = (1, 4, 5, 9, 33, 37)         # 33 and 37 cross the 32-query membership group, ragged against 4 and 2 per pass
MAXQ = 37


def layouts(n, seed=0):
    """labeled_cases.layouts plus `unique`: every row its own label, a permutation of 0 .. n-1.  name -> labels per row"""
    out = {name: lab for name, (lab, _) in lc.layouts(n, seed).items()}
    out["unique"] = np.random.default_rng(2000 + seed).permutation(n).astype(np.uint32)
    return out


def present(labels):
    return np.unique(labels[labels != NONE])


def sets_for(labels, seed=0):
    """name -> one set (int64 array, as a caller would write it: unsorted, with duplicates where the name says so)"""
    rng = np.random.default_rng(3000 + seed)
    have = present(labels)
    some = rng.permutation(have)[:min(70, max(1, len(have) // 2))]
    filler = 200000 + np.arange(70 - len(some))                  # labels no layout hands out
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "one": have[-1:].astype(np.int64),
        "three_one_absent": np.array([have[0], ABSENT, have[len(have) // 2]], dtype=np.int64),
        "seventy": rng.permutation(np.concatenate([some.astype(np.int64), filler])),       # more than a wavefront of labels
        "all_present": rng.permutation(have).astype(np.int64),
        "dups_descending": np.sort(np.concatenate([have[:3], have[:3], [ABSENT, ABSENT]]).astype(np.int64))[::-1].copy(),
    }


def allowed(labels, s, exclude):
    """the contract: a row is allowed iff it carries a label and that label is in the set (exclude: is not in it)"""
    inside = np.isin(labels, np.asarray(s, dtype=np.int64).astype(np.uint32)) if len(s) else np.zeros(len(labels), dtype=bool)
    return (labels != NONE) & (inside != bool(exclude))


def mixes(labels, qs, seed=0):
    """name -> (queries [MAXQ, dim], a set per query), cut to nq by the caller.  `qs`: MAXQ queries"""
    assert len(qs) == MAXQ
    rng = np.random.default_rng(4000 + seed)
    base = list(sets_for(labels, seed).values())
    have = present(labels)
    own = []
    for i in range(MAXQ):                                        # every query its own set: the six named ones, then random subsets
        if i < len(base):
            own.append(base[(i * 5 + 3) % len(base)])            # (not in their listed order)
        else:
            m = int(rng.integers(1, min(len(have), 40) + 1))
            own.append(np.concatenate([rng.permutation(have)[:m].astype(np.int64), [300000 + i]]))
    dup = np.ascontiguousarray(np.repeat(qs[:1], MAXQ, axis=0))
    apart = [own[i % 3] for i in range(MAXQ)]                    # three sets, equal ones never neighbours in caller order
    # every present label but one: on `unique` 3000 labels a set, all distinct - a group of more than two is searched in global memory
    large = [rng.permutation(np.delete(have, i % len(have))).astype(np.int64) for i in range(MAXQ)]
    return {"own": (qs, own), "all_one_set": (qs, [base[2]] * MAXQ), "one_query_many_sets": (dup, own), "equal_sets_apart": (qs, apart),
            "all_but_one": (qs, large)}


def grouped_order(dist, labels, allow):
    """positions of the grouped contract over the allowed rows, all of them: finite distance, (distance, position) order, first row of each label"""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pos = np.nonzero(np.asarray(allow, dtype=bool) & (d < np.inf) & (labels != NONE))[0]
    pos = pos[np.lexsort((pos, d[pos]))]
    _, first = np.unique(labels[pos], return_index=True)
    return pos[np.sort(first)]
