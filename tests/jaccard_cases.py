"""What the Jaccard-distance tests share: shapes, data with planted rows and the host-side expectation (no test in here).

The expected answer everywhere is numpy: with i = np.unpackbits(rows & q, axis=1).sum(1) and u = np.unpackbits(rows | q, axis=1).sum(1)
the distance is np.float32(u - i) / np.float32(u), 0 where u == 0, and the order is np.argsort(d, kind="stable") = (distance, scan
position).  Rowids, order and distance bits are compared with ==: both sides convert two integers below 2^24 exactly and divide once
in IEEE single precision, so nothing in the contract rounds differently on the two sides and there is nothing to tolerate.

Uniform random bytes would put every distance near 2/3 and test little, so a random row draws its own bit density from 1/64, 1/8
and 1/2: sparse rows against a sparse query share no bit at all (distance exactly 1: long runs of ties), dense ones spread out."""
import numpy as np

JACCARD, HAMMING, COSINE, L1 = 7, 6, 3, 5
F32, F16, BF16, U8, I8 = 1, 2, 3, 4, 5

# the uint8 ladder's launch shapes as in hamming_cases: up to 1024 bytes 1 to 4 chunks per lane; 6 and 8 chunks per lane are first
# reached by rows of 6144 and 8192 bytes, which - like the long row - run with 65 and 2531 rows only
ROW_BYTES = (1, 16, 17, 32, 64, 100, 128, 192, 256, 384, 768, 1024)
WIDE_ROW_BYTES = (6144, 8192)
LONG_ROW_BYTES = 9000                                                  # the long-row kernel
ROW_COUNTS = (1, 63, 64, 65, 2531, 30001)                              # a partial last batch of rows; more than one workgroup
WIDE_ROW_COUNTS = (65, 2531)
PLAIN_CASES = [(dim, n) for dim in ROW_BYTES for n in ROW_COUNTS] + \
              [(dim, n) for dim in WIDE_ROW_BYTES + (LONG_ROW_BYTES,) for n in WIDE_ROW_COUNTS]
FORM_ROW_BYTES = (32, 128, 768)
FORM_ROWS = 2531
DENSITIES = (1.0 / 64, 1.0 / 8, 1.0 / 2)
HALF = np.float32(0.5)


def counts(rows, q):
    """(i, u) int64 [n] each: popcount(q AND row) and popcount(q OR row), the rows taken in slices so that the unpacked bits of a
    long-row corpus stay small"""
    rows = np.asarray(rows)
    i = np.empty(rows.shape[0], dtype=np.int64)
    u = np.empty(rows.shape[0], dtype=np.int64)
    step = max(1, (1 << 25) // max(1, rows.shape[1]))
    for r0 in range(0, rows.shape[0], step):
        i[r0:r0 + step] = np.unpackbits(rows[r0:r0 + step] & q[None, :], axis=1).sum(1)
        u[r0:r0 + step] = np.unpackbits(rows[r0:r0 + step] | q[None, :], axis=1).sum(1)
    return i, u


def distances(rows, q):
    """float32 [n]: (u - i) / u as one float32 division, 0 where the union is empty"""
    i, u = counts(rows, q)
    out = np.zeros(i.size, dtype=np.float32)
    np.divide((u - i).astype(np.float32), u.astype(np.float32), out=out, where=u > 0)
    return out


def random_rows(n, dim, rng, densities=DENSITIES):
    """n rows of `dim` bytes, each row with a bit density of its own drawn from `densities` (1/2, 1/8, 1/64: one, three and six
    random bytes ANDed together)"""
    rows = rng.integers(0, 256, (n, dim)).astype(np.uint8)
    dens = rng.choice(np.asarray(densities), n)
    for bound, rounds in ((1.0 / 8, 2), (1.0 / 64, 3)):
        sel = np.flatnonzero(dens <= bound)
        for _ in range(rounds):
            rows[sel] &= rng.integers(0, 256, (sel.size, dim)).astype(np.uint8)
    return rows


def query(dim, seed, density=1.0 / 8):
    return random_rows(1, dim, np.random.default_rng(seed), (density,))[0]


def weighted_query(dim, weight, seed):
    """a query with exactly `weight` set bits"""
    bits = np.zeros(8 * dim, dtype=bool)
    bits[np.random.default_rng(seed).permutation(8 * dim)[:weight]] = True
    return np.packbits(bits)


def corpus(n, dim, q, seed):
    """rows of mixed density with the planted rows around positions 0, 63, 64 and n - 1 (ties across wavefront and workgroup
    boundaries), each where the corpus has such a position to spare: the query itself at these four (distance 0), its complement next
    to each (distance 1) and an all-zero row next to that (distance 1, or 0 for a zero query)"""
    rows = random_rows(n, dim, np.random.default_rng(seed))
    taken = set()
    for plant, where in ((q, (0, 63, 64, n - 1)), (~q, (1, 62, 65, n - 2)), (np.zeros_like(q), (2, 61, 66, n - 3))):
        for p in where:
            if 0 <= p < n and p not in taken:
                rows[p] = plant
                taken.add(p)
    return rows


def identical(n, dim, seed):
    """every row the same: everything ties and the answer is the first k positions"""
    return np.repeat(random_rows(1, dim, np.random.default_rng(seed), (1.0 / 8,)), n, axis=0)


def rows_with_counts(common, extra, dim, q, seed):
    """a row per entry: `common[j]` of the query's set bits and `extra[j]` of its unset bits, chosen at random - so that
    i = common[j] and u = |q| + extra[j]"""
    rng = np.random.default_rng(seed)
    common, extra = np.asarray(common, dtype=np.int64), np.asarray(extra, dtype=np.int64)
    qbits = np.unpackbits(q).astype(bool)
    on, off = np.flatnonzero(qbits), np.flatnonzero(~qbits)
    assert common.max(initial=0) <= on.size and extra.max(initial=0) <= off.size
    bits = np.zeros((common.size, 8 * dim), dtype=bool)
    for idx, want in ((on, common), (off, extra)):
        if idx.size:
            rank = np.argsort(np.argsort(rng.random((want.size, idx.size)), axis=1), axis=1)
            bits[:, idx] = rank < want[:, None]
    return np.packbits(bits, axis=1)


# Equal rationals.  A row's (i, u) obey i <= |q| <= u, so one query cannot meet (1, 2) and (32, 64) both: the pairs go with a query
# weight each, (i, u) = (1, 2), (2, 4) under a query of 2 bits, (2, 4), (3, 6) under 3 bits, (16, 32), (24, 48), (32, 64) under 32 -
# every one of them 1/2, and the float of every one of them the same 0x3F000000.
EQUAL_RATIONALS = {2: ((1, 2), (2, 4)), 3: ((2, 4), (3, 6)), 32: ((16, 32), (24, 48), (32, 64))}
EQUAL_POSITIONS = (5, 62, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2500)      # wavefront (64) and workgroup (1024) boundaries


def equal_rationals(n, dim, weight, seed):
    """(query, rows, planted positions): mixed-density rows with a row of distance 1/2 at every EQUAL_POSITIONS entry below n, the
    (i, u) pairs of EQUAL_RATIONALS[weight] in turn"""
    q = weighted_query(dim, weight, seed)
    rows = random_rows(n, dim, np.random.default_rng(seed + 1))
    pos = [p for p in EQUAL_POSITIONS if p < n]
    pairs = [EQUAL_RATIONALS[weight][j % len(EQUAL_RATIONALS[weight])] for j in range(len(pos))]
    rows[pos] = rows_with_counts([i for i, u in pairs], [u - weight for i, u in pairs], dim, q, seed + 2)
    return q, rows, np.asarray(pos)


def zero_query_corpus(n, dim, seed):
    """rows for an all-zero query: every third row all zero (distance 0: the union is empty), the others mixed (distance 1 unless
    they happen to be empty too)"""
    rows = random_rows(n, dim, np.random.default_rng(seed))
    rows[::3] = 0
    return rows


def shared_kth_value(k, dim, q, seed, n_shared=5000, n_above=1000):
    """exactly k - 1 rows strictly below a distance (1/2) that n_shared rows share, the rest above it, in a random row order; q must
    have an even number w >= 4 of set bits: i = w / 2 of them and nothing else is 1/2, more of them is below, fewer plus extra bits above"""
    rng = np.random.default_rng(seed)
    w = int(np.unpackbits(q).sum())
    assert w >= 4 and w % 2 == 0
    common = np.concatenate([rng.integers(w // 2 + 1, w + 1, k - 1), np.full(n_shared, w // 2), rng.integers(0, w // 2, n_above)])
    extra = np.concatenate([np.zeros(k - 1 + n_shared, dtype=np.int64), rng.integers(0, 8 * dim - w + 1, n_above)])
    order = rng.permutation(common.size)
    return rows_with_counts(common[order], extra[order], dim, q, seed + 1)


def expected(d, k, allowed=None, rowids=None):
    """(rowids, distances) of the first k rows in (distance, scan position) order; allowed: None or a bool per row"""
    d = np.asarray(d, dtype=np.float32)
    pos = np.argsort(d, kind="stable")
    if allowed is not None:
        pos = pos[np.asarray(allowed, dtype=bool)[pos]]
    pos = pos[:k]
    return (pos + 1 if rowids is None else np.asarray(rowids)[pos]), d[pos]


def within(d, radius, allowed=None, limit=None):
    """(rowids, distances, matches) of the rows with d <= radius in that order, cut to `limit`; `matches` counts all of them"""
    d = np.asarray(d, dtype=np.float32)
    ok = d.astype(np.float64) <= radius
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    pos = np.argsort(d, kind="stable")
    pos = pos[ok[pos]]
    m = int(pos.size)
    if limit is not None:
        pos = pos[:limit]
    return pos + 1, d[pos], m


def check(got, want, ctx=None):
    """rowids, order and distance bits, =="""
    gi, gd = got[0], got[1]
    wi, wd = want[0], want[1]
    assert np.asarray(gi).tolist() == np.asarray(wi).tolist(), ctx
    assert np.array_equal(np.asarray(gd).astype(np.float32).view(np.uint32), np.asarray(wd, dtype=np.float32).view(np.uint32)), ctx


def check_batch(got, wants, k, ctx=None):
    """a batch answer (rowids [nq, k], distances [nq, k], counts [nq]) against one expectation per query"""
    ids, dist, cnt = got[0], got[1], got[-1]
    for i, want in enumerate(wants):
        assert int(cnt[i]) == len(want[0]), (ctx, i)
        check((ids[i, :cnt[i]], dist[i, :cnt[i]]), want, (ctx, i))
