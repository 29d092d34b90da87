"""What the value-range tests share: value layouts, the intervals asked for, the host-side "allowed" rule and the mixes of a batch (no
test in here).

Shapes, row count and data are the labeled scans' (labeled_cases): 3001 rows is no multiple of 64 or of any rows-per-batch.  The
layouts are the ones where a comparison of int64 values can go wrong: an unsigned compare, a compare of one 32-bit half only, a signed
compare of the low half."""
import numpy as np

import labeled_cases as lc
import labelset_cases as ls

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NQS = ls.NQS                       # 33 and 37 cross the 32-query membership group, ragged against 4 and 2 per pass
MAXQ = ls.MAXQ


def layouts(n, seed=0):
    """name -> an int64 value per row"""
    rng = np.random.default_rng(5000 + seed)
    out = {}
    out["sorted"] = (np.arange(n, dtype=np.int64) // 7) * 10 + 1000                      # ascending with repeats: whole batches outside
    out["random"] = rng.integers(-(1 << 45), 1 << 45, n).astype(np.int64)
    out["all_equal"] = np.full(n, 42, dtype=np.int64)
    v = rng.integers(-1000, 1001, n).astype(np.int64)                                    # an unsigned or a 32-bit compare orders these wrongly
    for j, special in enumerate((I64_MIN, I64_MAX, -1, 0, 1)):
        v[rng.permutation(n)[:9] if j else [0, n // 2, n - 1]] = special
    v[1] = I64_MAX
    out["extremes"] = v
    out["high_word_only"] = (rng.integers(-4, 4, n).astype(np.int64) << 32) + 0x1234      # equal low words
    low = rng.integers(0, 1 << 32, n).astype(np.int64)                                    # equal high words, bit 31 set in about half
    low[:4] = (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0)
    out["low_word_only"] = (np.int64(5) << 32) | low
    return out


def allowed(values, lo, hi, labels=None, label=None):
    """the contract: a row is allowed iff lo <= values[p] <= hi, signed and closed at both ends (None: the open end) - and, with
    `labels` and `label`, iff it also carries that label"""
    lo = I64_MIN if lo is None else int(lo)
    hi = I64_MAX if hi is None else int(hi)
    v = np.asarray(values, dtype=np.int64)
    ok = (v >= np.int64(lo)) & (v <= np.int64(hi)) if lo <= hi else np.zeros(len(v), dtype=bool)
    if label is not None:
        ok = ok & (np.asarray(labels) == np.uint32(label))
    return ok


def intervals(values, k=20):
    """name -> (lo, hi) as Python ints, for one layout.  `on_present_shrunk` is `on_present` with one taken off each end: what the
    two allow differs by exactly the rows that sit on the ends - the interval is closed"""
    u = [int(x) for x in np.unique(values)]
    mid = u[len(u) // 2]
    out = {"full": (I64_MIN, I64_MAX), "lo_above_hi": (1, 0), "ends_swapped": (I64_MAX, I64_MIN), "one_value": (mid, mid),
           "min_min": (I64_MIN, I64_MIN), "max_max": (I64_MAX, I64_MAX), "across_zero": (-(1 << 40), 1 << 40)}
    a, b = u[len(u) // 3], u[(2 * len(u)) // 3]
    out["on_present"] = (a, b)
    out["on_present_shrunk"] = (a + 1, b - 1)
    gaps = [(x + 1, y - 1) for x, y in zip(u, u[1:]) if y - x > 1]
    out["none_inside"] = gaps[len(gaps) // 2] if gaps else (u[-1] + 1, u[-1] + 10)
    v = np.asarray(values, dtype=np.int64)
    few = [x for x in u if 0 < int((v <= x).sum()) < k]
    if few:
        out["fewer_than_k"] = (u[0], few[-1])
    return out


def mixes(values, qs, labels=None, seed=0):
    """name -> (queries [MAXQ, dim], los, his, a label per query or None), cut to nq by the caller.  `qs`: MAXQ queries.  With
    `labels` (a uint32 per row) every mix comes with per-query labels, drawn from the labels present"""
    assert len(qs) == MAXQ
    rng = np.random.default_rng(6000 + seed)
    base = list(intervals(values).values())
    u = np.unique(values)
    own = []
    for i in range(MAXQ):                                        # every query its own interval: the named ones, then random ones
        if i < len(base):
            own.append(base[(i * 5 + 3) % len(base)])            # (not in their listed order)
        else:
            x, y = sorted(int(t) for t in u[rng.integers(0, len(u), 2)])
            own.append((x, y))
    dup = np.ascontiguousarray(np.repeat(qs[:1], MAXQ, axis=0))
    apart = [own[(i % 3) * 2 + 1] for i in range(MAXQ)]          # three intervals, equal ones never neighbours in caller order
    qlab, qlab3 = None, None
    if labels is not None:
        have = ls.present(labels)
        qlab = np.array([have[(i * 3 + 1) % len(have)] for i in range(MAXQ)], dtype=np.uint32)
        qlab3 = np.array([have[(i % 3) % len(have)] for i in range(MAXQ)], dtype=np.uint32)
    sp = lambda ivs: ([t[0] for t in ivs], [t[1] for t in ivs])
    return {"own": (qs,) + sp(own) + (qlab,), "all_one_interval": (qs,) + sp([base[7]] * MAXQ) + (qlab,),
            "one_query_many_intervals": (dup,) + sp(own) + (qlab,), "equal_conditions_apart": (qs,) + sp(apart) + (qlab3,)}
