"""The host rule the value-range GPU tests lean on (valued_cases.allowed), pinned against a literal table of hand-written cases - and the
properties of the layouts, intervals and mixes those tests assume.  No device."""
import numpy as np

import valued_cases as vc

MIN, MAX = vc.I64_MIN, vc.I64_MAX
VALUES = np.array([MIN, -(1 << 32) - 1, -(1 << 32), -(1 << 31), -1, 0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, MAX], dtype=np.int64)
LABELS = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, vc.lc.NONE], dtype=np.uint32)

# (lo, hi, label or None) -> the positions allowed, written out by hand
TABLE = [
    ((MIN, MAX, None), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]),
    ((None, None, None), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]),
    ((1, 0, None), []),
    ((MAX, MIN, None), []),
    ((MIN, MIN, None), [0]),
    ((MAX, MAX, None), [11]),
    ((0, 0, None), [5]),
    ((-1, 1, None), [4, 5, 6]),                                          # across zero, closed at both ends
    ((0, 1, None), [5, 6]),
    ((-1, 0, None), [4, 5]),
    ((2, (1 << 31) - 2, None), []),                                      # between two present values
    ((None, -1, None), [0, 1, 2, 3, 4]),                                 # an unsigned compare would put these at the top
    ((0, None, None), [5, 6, 7, 8, 9, 10, 11]),
    (((1 << 31) - 1, 1 << 31, None), [7, 8]),                            # bit 31 of the low word is no sign
    ((1 << 31, (1 << 32) - 1, None), [8, 9]),
    (((1 << 32) - 1, 1 << 32, None), [9, 10]),                           # differ in both words
    ((-(1 << 32) - 1, -(1 << 32), None), [1, 2]),
    ((-(1 << 32), -(1 << 31), None), [2, 3]),
    ((1, (1 << 32) - 1, None), [6, 7, 8, 9]),                            # equal high words: the low words decide, unsigned
    ((MIN, MAX, 0), [0, 3, 6, 9]),
    ((MIN, MAX, 2), [2, 5, 8]),                                          # (the last row carries no label)
    ((-1, 1 << 31, 1), [4, 7]),
    ((0, 0, 1), []),
    ((1, 0, 0), []),
]


def test_allowed_against_the_table():
    for (lo, hi, label), want in TABLE:
        got = vc.allowed(VALUES, lo, hi, LABELS if label is not None else None, label)
        assert np.nonzero(got)[0].tolist() == want, (lo, hi, label)


def test_layouts_hold_what_their_names_say():
    n = vc.lc.N
    lay = vc.layouts(n)
    assert set(lay) == {"sorted", "random", "all_equal", "extremes", "high_word_only", "low_word_only"}
    for name, v in lay.items():
        assert v.dtype == np.int64 and v.shape == (n,), name
    s = lay["sorted"]
    assert (np.diff(s) >= 0).all() and len(np.unique(s)) < n
    assert len(np.unique(lay["all_equal"])) == 1
    assert all((lay["extremes"] == x).any() for x in (MIN, MAX, -1, 0, 1))
    h = lay["high_word_only"]
    assert len(np.unique(h & 0xFFFFFFFF)) == 1 and len(np.unique(h >> 32)) > 2 and (h < 0).any() and (h > 0).any()
    w = lay["low_word_only"]
    assert len(np.unique(w >> 32)) == 1 and ((w & 0x80000000) != 0).any() and ((w & 0x80000000) == 0).any()


def test_intervals_do_what_their_names_say():
    n = vc.lc.N
    for name, v in vc.layouts(n).items():
        iv = vc.intervals(v)
        count = lambda key: int(vc.allowed(v, *iv[key]).sum())
        assert count("full") == n and count("lo_above_hi") == 0 and count("ends_swapped") == 0, name
        assert count("one_value") >= 1 and iv["one_value"][0] == iv["one_value"][1], name
        assert count("min_min") == int((v == MIN).sum()) and count("max_max") == int((v == MAX).sum()), name
        assert count("none_inside") == 0 and iv["none_inside"][0] <= iv["none_inside"][1], name
        lo, hi = iv["on_present"]
        assert (v == lo).any() and (v == hi).any(), name
        on_ends = int(((v == lo) | (v == hi)).sum())
        assert count("on_present") - count("on_present_shrunk") == on_ends and on_ends >= 1, name      # closed at both ends
        if "fewer_than_k" in iv:
            assert 0 < count("fewer_than_k") < 20, name
    assert "fewer_than_k" in vc.intervals(vc.layouts(n)["sorted"]) and "fewer_than_k" in vc.intervals(vc.layouts(n)["extremes"])
    assert 0 < int(vc.allowed(vc.layouts(n)["random"], *vc.intervals(vc.layouts(n)["random"])["across_zero"]).sum()) < n


def test_mixes_cover_the_batch_cases():
    n = vc.lc.N
    v = vc.layouts(n)["random"]
    labels = vc.lc.layouts(n)["some_none"][0]
    qs = np.arange(vc.MAXQ * 4, dtype=np.float32).reshape(vc.MAXQ, 4)
    for lab in (None, labels):
        m = vc.mixes(v, qs, lab)
        assert set(m) == {"own", "all_one_interval", "one_query_many_intervals", "equal_conditions_apart"}
        for name, (mq, los, his, ql) in m.items():
            assert len(mq) == len(los) == len(his) == vc.MAXQ, name
            assert (ql is None) == (lab is None), name
            if ql is not None:
                assert len(ql) == vc.MAXQ and (ql != vc.lc.NONE).all() and np.isin(ql, labels).all(), name
        conds = lambda name: [(m[name][1][i], m[name][2][i], None if lab is None else int(m[name][3][i])) for i in range(vc.MAXQ)]
        assert len(set(conds("own"))) > 32                                          # more distinct conditions than one group holds
        assert len(set(c[:2] for c in conds("all_one_interval"))) == 1
        assert (m["one_query_many_intervals"][0] == qs[0]).all()
        apart = conds("equal_conditions_apart")
        assert len(set(apart)) == 3 and all(apart[i] != apart[i + 1] and apart[i] == apart[i + 3] for i in range(vc.MAXQ - 3))
        assert any(lo > hi for lo, hi, _ in conds("own"))                          # an empty interval rides in a batch
