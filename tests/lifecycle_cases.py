"""Case builder of tests/test_gpu_lifecycle.py: the paths that read a derived per-row copy of a corpus, and the lifecycle scripts
(patch / delete / append, clear + smaller append, clone, reserve / trim) as plain numpy bookkeeping - no device.

A script is a list of Steps.  A step names one call on the handle (op, args) and, when `rows` is not None, the state to compare the
handle against afterwards: the surviving rows, their rowids and the named sets of bit-identical rows among them.  A step with
warm = True asks the runner to build the path's derived data in that state (a small run) without comparing anything: what such a
state holds - 70 rows of NaN / Inf / 1e18 at the very end - is there to be left behind the corpus' new end by the next deletion.

tests/test_lifecycle_cases.py checks the bookkeeping and the float64 reference's band share of every batch state without a device."""
import collections
import functools

import numpy as np

import datagen as dg

K, NQ = 20, 40
N_Q8, N_SMALL, N_LONG = 70_003, 9_003, 3_003      # the forced int8 batch filter refuses corpora below 65 536 rows
Q8_FLOOR = 1 << 16
FLOATS = (dg.F32, dg.F16, dg.BF16)

Path = collections.namedtuple("Path", "name vt dim n kind metric env scan_filter proof")
_FILTER = {"VG_SCAN_FILTER_MIN_MB": "0", "VG_SCAN_FILTER_NO_GUARD": "1"}       # (small corpora: every list's warm-up would trip the guard)
PATHS = (
    Path("scan_q8_f32", dg.F32, 100, N_SMALL, "scan", dg.L2, dict(_FILTER, VG_SCAN_FILTER_SHADOW="int8"), 1, "filter"),
    Path("scan_q8_f16", dg.F16, 33, N_SMALL, "scan", dg.COSINE, dict(_FILTER, VG_SCAN_FILTER_SHADOW="int8"), 1, "filter"),
    Path("scan_bf16_f32", dg.F32, 384, N_SMALL, "scan", dg.DOT, dict(_FILTER, VG_SCAN_FILTER_SHADOW="bf16"), 1, "filter"),
    Path("scan_n4_u8", dg.U8, 100, N_SMALL, "scan", dg.L2, dict(_FILTER, VG_SCAN_FILTER_N4="1"), 1, "n4"),
    Path("scan_n4_i8", dg.I8, 33, N_SMALL, "scan", dg.DOT, dict(_FILTER, VG_SCAN_FILTER_N4="1"), 1, "n4"),
    Path("batch_q8_f32", dg.F32, 33, N_Q8, "batch", dg.DOT, {"VG_BATCH_Q8": "1"}, None, 7),
    Path("batch_q8_bf16", dg.BF16, 100, N_Q8, "batch", dg.L2, {"VG_BATCH_Q8": "1"}, None, 7),
    Path("batch_bf16_f32", dg.F32, 100, N_SMALL, "batch", dg.L2, {"VG_F32_FILTER": "1", "VG_BATCH_Q8": "0"}, None, 3),
    Path("batch_bf16_f32_520", dg.F32, 520, N_SMALL, "batch", dg.COSINE, {"VG_F32_FILTER": "1", "VG_BATCH_Q8": "0"}, None, 3),
    Path("batch_tm_f16", dg.F16, 384, N_SMALL, "batch", dg.SQUARED_L2, {"VG_BATCH_Q8": "0"}, None, 3),
    Path("batch_long_bf16", dg.BF16, 1032, N_LONG, "batch", dg.L2, {"VG_BATCH_Q8": "0"}, None, 4),
    Path("batch_i8_u8", dg.U8, 384, N_SMALL, "batch", dg.L2, {}, None, 2),
    Path("batch_i8_i8", dg.I8, 33, N_SMALL, "batch", dg.L2, {}, None, 2),
    Path("batch_f32_xnorm", dg.F32, 100, N_SMALL, "batch", dg.L2, {"VG_F32_FILTER": "0", "VG_BATCH_Q8": "0"}, None, 1),
)
PATH_BY_NAME = {p.name: p for p in PATHS}
SWITCHES = sorted({k for p in PATHS for k in p.env} | {"VG_BATCH_MFMA", "VG_SCAN_FILTER", "VG_BATCH_TILE_MAJOR", "VG_BATCH_LONG", "VG_MULTI_SCAN"})

Step = collections.namedtuple("Step", "op args rows ids dups warm")
World = collections.namedtuple("World", "rows ids qs")


def _seed(p):
    return 5100 + 97 * PATHS.index(p)


def make_ids(n, first=10, step=3):
    """explicit rowids: ascending, not contiguous"""
    return np.arange(first, first + step * n, step, dtype=np.int64)


@functools.lru_cache(maxsize=4)
def world(name):
    p = PATH_BY_NAME[name]
    rows = dg.corpus(p.vt, p.n, p.dim, _seed(p))
    qs = dg.corpus(p.vt, NQ, p.dim, _seed(p) + 1)
    return World(rows, make_ids(p.n), qs)


def special_rows(vt, dim, n, seed):
    """n rows cycling NaN / Inf / huge magnitude (floats; f16: its largest magnitudes); for the integer types the extreme values"""
    base = dg.corpus(vt, n, dim, seed)
    if vt not in FLOATS:
        info = np.iinfo(dg.NP_DTYPE[vt])
        base[0::3] = info.max
        base[1::3] = info.min
        return base
    x = dg.storage_to_f64(vt, base).astype(np.float32)
    x[0::3, dim // 3] = np.nan
    x[1::3, dim - 1] = np.inf
    x[2::3] *= np.float32(6.0e4 if vt == dg.F16 else 1.0e18)
    return dg.to_storage(vt, x)


def best_row(vt, metric, q):
    """a row no other row of a random corpus beats for query q"""
    if metric != dg.DOT:
        return q.copy()                                          # distance 0
    if vt in FLOATS:
        return dg.to_storage(vt, (dg.storage_to_f64(vt, q) * 3.0).astype(np.float32))
    info = np.iinfo(dg.NP_DTYPE[vt])
    return np.where(q.astype(np.int64) > 0, info.max, info.min).astype(dg.NP_DTYPE[vt])


class Model:
    """the rows a handle should hold, kept next to it"""

    def __init__(self, rows, ids):
        self.rows, self.ids = rows.copy(), ids.copy()
        self.tag = np.zeros(len(ids), dtype=np.int64)            # 1: a copy of query 0

    def dups(self):
        g = np.nonzero(self.tag == 1)[0]
        return (tuple(int(x) for x in g),) if len(g) > 1 else ()

    def snap(self, op, args, warm=False, check=True):
        if not check:
            return Step(op, args, None, None, None, warm)
        return Step(op, args, self.rows.copy(), self.ids.copy(), self.dups(), warm)

    def patch(self, pos, new, tag=None, **kw):
        self.rows[pos] = new
        self.tag[pos] = 0 if tag is None else tag
        return self.snap("patch", (np.asarray(pos, dtype=np.int64), new), **kw)

    def delete(self, pos):
        keep = np.ones(len(self.ids), bool)
        keep[pos] = False
        self.rows, self.ids, self.tag = self.rows[keep], self.ids[keep], self.tag[keep]
        return self.snap("delete", (np.asarray(pos, dtype=np.int64),))

    def append(self, new, ids):
        self.rows, self.ids = np.concatenate([self.rows, new]), np.concatenate([self.ids, ids])
        self.tag = np.concatenate([self.tag, np.zeros(len(ids), dtype=np.int64)])
        return self.snap("append", (new, ids))


def _patch_step(p, w, m, rng):
    """300 scattered rows: position 0, the last row, five copies of query 0, fresh random rows; floats: a NaN row, an Inf row, a zero row"""
    n = len(m.ids)
    pos = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)[:298]]).astype(np.int64)
    new = dg.corpus(p.vt, 300, p.dim, _seed(p) + 2)
    tag = np.zeros(300, dtype=np.int64)
    new[2:7], tag[2:7] = w.qs[0], 1
    if p.vt in FLOATS:
        _, edge = dg.edge_rows(p.vt, p.dim, _seed(p) + 3)
        new[7] = edge[13 if p.vt == dg.F32 else 12]              # NaN
        new[8] = edge[14 if p.vt == dg.F32 else 10]              # Inf
        new[9] = edge[1]                                         # all zero
        assert np.isnan(dg.storage_to_f64(p.vt, new[7])).any() and np.isinf(dg.storage_to_f64(p.vt, new[8])).any() and not new[9].any()
    return m.patch(pos, new, tag)


def _delete_positions(m_now, end_min, target_mod, rng):
    """a run of 7 at the front, 200 singles, a run at the very end of at least end_min rows - the smallest that leaves
    (rows mod 32) == target_mod"""
    e = end_min
    while (m_now - 207 - e) % 32 != target_mod:
        e += 1
    singles = 7 + rng.permutation(m_now - 7 - e)[:200]
    dele = np.sort(np.concatenate([np.arange(7), singles, np.arange(m_now - e, m_now)])).astype(np.int64)
    assert len(np.unique(dele)) == 207 + e
    return dele, e


@functools.lru_cache(maxsize=2)
def edit_script(name):
    """patch, three deletions (rows mod 32 -> 0, 1, 31; the first one drops more than two whole tiles from the end, planted with
    NaN / Inf / huge rows beforehand), then an append with a new best row of query 1"""
    p, w = PATH_BY_NAME[name], world(name)
    m, rng = Model(w.rows, w.ids), np.random.default_rng(_seed(p) + 4)
    steps = [_patch_step(p, w, m, rng)]
    for i, target in enumerate((0, 1, 31)):
        n = len(m.ids)
        if i == 0:
            steps.append(m.patch(np.arange(n - 70, n), special_rows(p.vt, p.dim, 70, _seed(p) + 5), warm=True, check=False))
        dele, _ = _delete_positions(n, 70 if i == 0 else 3, target, rng)
        steps.append(m.delete(dele))
    more = dg.corpus(p.vt, 100, p.dim, _seed(p) + 6)
    more[37] = best_row(p.vt, p.metric, w.qs[1])
    steps.append(m.append(more, np.arange(10**7, 10**7 + 100, dtype=np.int64)))
    return tuple(steps)


def clear_sizes(p):
    """(rows before the clear, rows appended after it): about half, not a multiple of 32, at or above the int8 batch filter's floor"""
    return (2 * p.n - 1, p.n) if p.proof == 7 else (p.n, p.n // 2 + 2)


@functools.lru_cache(maxsize=2)
def clear_script(name):
    """first content (with NaN / Inf / huge rows right behind where the second content will end), clear, then fewer, different rows"""
    p, w = PATH_BY_NAME[name], world(name)
    n1, n2 = clear_sizes(p)
    first = w.rows if n1 == p.n else dg.corpus(p.vt, n1, p.dim, _seed(p) + 7)
    first = first.copy()
    first[n2:n2 + 70] = special_rows(p.vt, p.dim, 70, _seed(p) + 5)
    m = Model(first, make_ids(n1))
    steps = [m.snap("create", (m.rows, m.ids), warm=True, check=False)]
    second = dg.corpus(p.vt, n2, p.dim, _seed(p) + 8)
    second[n2 - 1] = best_row(p.vt, p.metric, w.qs[1])
    m = Model(second, make_ids(n2, 5, 2))
    steps.append(m.snap("clear_append", (second, m.ids.copy())))
    return tuple(steps)


def within_radius(d, want=50):
    """a radius that about `want` rows of the distances d match, in the middle of the widest nearby gap: (radius, gap)"""
    s = np.sort(d[np.isfinite(d)].astype(np.float64))
    j = max(range(want - 5, want + 6), key=lambda i: s[i] - s[i - 1])
    return 0.5 * (s[j] + s[j - 1]), s[j] - s[j - 1]
