"""What the labeled-scan tests share: shapes, data, label layouts and the host-side expectation (no test in here).

Shapes are the smallest at which the labeled paths differ: 3001 rows is no multiple of 64 or of any rows-per-batch and gives every
wavefront of the grid a batch on the narrow shapes.  uint8 / int8 values come from four levels, so that equal distances are routine and
the (distance, position) order is exercised."""
import numpy as np

import datagen as dg

N = 3001
NONE = 0xFFFFFFFF
ABSENT = 123456                 # a label no layout hands out

# (type, dim, queries per pass of the batch form - 0: the fallback, metrics)
L2_COS = (dg.L2, dg.COSINE)
SHAPES = [
    (dg.F32, 384, 4, dg.ALL_METRICS),          # U = 3, NQ = 4
    (dg.F32, 768, 4, L2_COS),                  # 192 chunks = 64 lanes x 3: still 4 queries per pass
    (dg.F32, 1536, 2, L2_COS),                 # U = 6, NQ = 2 (no shape of <= 3 chunks per lane covers 384 chunks)
    (dg.U8, 64, 4, L2_COS),                    # U = 1, 16 rows per batch
    (dg.U8, 768, 4, dg.ALL_METRICS),           # register-resident
    (dg.I8, 100, 4, L2_COS),                   # a padding chunk
    (dg.F16, 384, 0, L2_COS),                  # fallback
    (dg.BF16, 384, 0, L2_COS),                 # fallback
    (dg.F32, 4100, 0, L2_COS),                 # long rows: fallback
]
SHAPE_IDS = ["%s-%d" % (dg.TYPE_NAMES[s[0]], s[1]) for s in SHAPES]


def data(vt, n, dim, seed):
    rng = np.random.default_rng(seed)
    if vt == dg.U8:
        return rng.integers(0, 4, (n, dim)).astype(np.uint8)
    if vt == dg.I8:
        return rng.integers(-2, 2, (n, dim)).astype(np.int8)
    return np.ascontiguousarray(dg.corpus(vt, n, dim, seed))


def layouts(n, seed=0):
    """name -> (labels per row, the labels worth asking for)"""
    rng = np.random.default_rng(1000 + seed)
    out = {}
    out["uniform5"] = (rng.integers(0, 5, n).astype(np.uint32), [0, 3, ABSENT])
    out["runs200"] = ((np.arange(n) // 200).astype(np.uint32), [0, 7, (n - 1) // 200])          # whole batches skipped
    out["all_one"] = (np.full(n, 7, dtype=np.uint32), [7, 8])
    lab = np.full(n, 1, dtype=np.uint32); lab[n - 1] = 9
    out["last_row_only"] = (lab, [9, 1])
    lab = rng.integers(0, 5, n).astype(np.uint32); lab[rng.random(n) < 0.3] = NONE
    out["some_none"] = (lab, [2, 4])
    return out


def expected(dist, allowed, k, rowids=None):
    """rowids and distances of the k first allowed rows with a finite distance (NaN / +Inf never) in (distance, position) order"""
    d = np.asarray(dist, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pos = np.nonzero(np.asarray(allowed, dtype=bool) & (d < np.inf))[0]
    pos = pos[np.lexsort((pos, d[pos]))][:k]
    ids = pos + 1 if rowids is None else np.asarray(rowids)[pos]
    return ids, d[pos]


def assert_same(got, ids, dist, ctx=None):
    gi, gd = got
    assert gi.tolist() == np.asarray(ids).tolist(), ctx
    assert np.array_equal(np.asarray(gd).astype(np.float32).view(np.uint32), np.asarray(dist, dtype=np.float32).view(np.uint32)), ctx


def error_code(pkg, fn):
    import pytest
    with pytest.raises(pkg.VectorGpuError) as ei:
        fn()
    return int(str(ei.value).split("error ")[1].split(":")[0])


def f64_distances(metric, q, x):
    """float64 numpy reference: q (dim,), x (m, dim) -> m distances"""
    q = q.astype(np.float64); x = x.astype(np.float64)
    if metric in (dg.L2, dg.SQUARED_L2):
        d = ((q[None, :] - x) ** 2).sum(axis=1)
        return np.sqrt(d) if metric == dg.L2 else d
    if metric == dg.L1:
        return np.abs(q[None, :] - x).sum(axis=1)
    dot = (q[None, :] * x).sum(axis=1)
    if metric == dg.DOT:
        return -dot
    den = np.sqrt((q * q).sum()) * np.sqrt((x * x).sum(axis=1))
    return np.where(den > 0.0, 1.0 - dot / np.where(den > 0.0, den, 1.0), 1.0)
