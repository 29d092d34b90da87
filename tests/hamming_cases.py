"""What the Hamming-distance tests share: shapes, data with planted rows and the host-side expectation (no test in here).

The expected answer everywhere is numpy: d = np.unpackbits(rows ^ q, axis=1).sum(1).astype(np.float32), and the order is
np.argsort(d, kind="stable") = (distance, scan position).  Rowids, order and distance bits are compared with ==: the distance is
an integer below 2^24, there is nothing to tolerate.  Hamming distances are small integers, so nearly every list here is decided by
ties."""
import numpy as np

HAMMING, L1 = 6, 5
F32, F16, BF16, U8, I8 = 1, 2, 3, 4, 5

# one per launch shape of the uint8 ladder and a ragged row (100).  Up to 1024 bytes the ladder takes 1 to 4 chunks per lane; 6 and 8
# chunks per lane are first reached by rows of 6144 and 8192 bytes (64 lanes x 6 / x 8), so these two are in the list as well
ROW_BYTES = (1, 16, 17, 32, 64, 100, 128, 192, 256, 384, 768, 1024, 6144, 8192)
LONG_ROW_BYTES = 9000                                                  # the long-row kernel
ROW_COUNTS = (1, 63, 64, 65, 2531, 30001)                              # a partial last batch of rows; more than one workgroup
FORM_ROW_BYTES = (32, 128, 768)
FORM_ROWS = 2531


def distances(rows, q):
    """float32 [n]: popcount(q XOR row), the rows taken in slices so that the unpacked bits of a long-row corpus stay small"""
    rows = np.asarray(rows)
    out = np.empty(rows.shape[0], dtype=np.float32)
    step = max(1, (1 << 25) // max(1, rows.shape[1]))
    for r0 in range(0, rows.shape[0], step):
        out[r0:r0 + step] = np.unpackbits(rows[r0:r0 + step] ^ q[None, :], axis=1).sum(1).astype(np.float32)
    return out


def query(dim, seed):
    return np.random.default_rng(seed).integers(0, 256, dim).astype(np.uint8)


def corpus(n, dim, q, seed):
    """random bytes with the planted rows: the query itself at positions 0, 63, 64 and n - 1 (distance 0; ties across wavefront and
    workgroup boundaries) and its complement in the middle (distance 8 * dim), each where the corpus has such a position to spare"""
    rows = np.random.default_rng(seed).integers(0, 256, (n, dim)).astype(np.uint8)
    for p in (0, 63, 64, n - 1):
        if 0 <= p < n and n > 1:
            rows[p] = q
    if n > 2:
        rows[n // 2] = ~q
    return rows


def identical(n, dim, seed):
    """every row the same: everything ties and the answer is the first k positions"""
    return np.repeat(np.random.default_rng(seed).integers(0, 256, (1, dim)).astype(np.uint8), n, axis=0)


def rows_at_distance(weights, dim, q, seed):
    """a row per entry of `weights`, exactly that many bits away from q"""
    rng = np.random.default_rng(seed)
    w = np.asarray(weights, dtype=np.int64)
    rank = np.argsort(rng.random((w.size, 8 * dim)), axis=1)
    return np.packbits(rank < w[:, None], axis=1) ^ q[None, :]


def shared_kth_value(k, dim, q, seed, n_shared=5000, n_above=1000):
    """exactly k - 1 rows strictly below a distance that n_shared rows share, the rest above it, in a random row order"""
    rng = np.random.default_rng(seed)
    at = 4 * dim                                               # half the bits
    w = np.concatenate([rng.integers(0, at, k - 1), np.full(n_shared, at), rng.integers(at + 1, 8 * dim + 1, n_above)])
    return rows_at_distance(rng.permutation(w), dim, q, seed + 1)


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
