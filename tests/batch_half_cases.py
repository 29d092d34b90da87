"""Corpora for the f64 anchor of the f16 / bf16 / f32-behind-bf16 batch filter (vg_batch_h.hip): rows, master queries, what was planted
where, and the named groups of identical rows.  No device is needed: tests/test_batch_half_cases.py holds every world against the reference
alone (band share, plants, and that the checker can fail on them), tests/test_gpu_batch_half_forms.py runs the kernel over them.

Rows are N(0, 1) elements with the decaying spectrum and per-row magnitudes 1 / 2 / 8 of tests/test_gpu_batch_q8_forms.py (iid rows put
a query's k-th and (k + 1)-th neighbour closer than the suite's own slack too often, see its docstring).  Planted in every world:

  * an exact copy of EVERY query at a position of its own: the first tile, rows 31 / 32 / 33, the last ragged tile, the first and last row
    of a partition, the rest spread out.  Under every metric but dot a query's first rowid is its plant: a swapped slot cannot pass;
  * second copies of a few plants further down (`duplicates`): ties must go by position;
  * rows aimed at the filter's slack.  The filter passes a pair when its matrix-core score, widened by E = cerr |q| |x|, can beat the
    query's current k-th best; cerr = (dim + 64) 2^-21, + 2^-7 + 2^-16 for f32 rows behind their bf16 shadow copy (vg_batch_h_launch).
    For a target query q and u in SLACK_UNITS the row x = (1 - u cerr) (q + r), r orthogonal to q with |r|^2 = 2 u cerr |q|^2, is worse
    than the plant by u E under dot, by u cerr under cosine and by 2 u E in the squared L2 distance: u units of the error term of each
    inequality - in float64, BEFORE the row is rounded to its storage type.  An f32 row keeps these offsets under every metric.  A
    half-precision row is rounded by up to 2^-11 (f16) / 2^-8 (bf16) per element, which moves its dot product and its cosine by about as
    much as the offset (f16) or by more (bf16: ~2^-9 against u cerr ~ 8e-5 at dim 100); in the squared L2 distance the rounding enters
    through 2 e.r with |r| ~ sqrt(2 u cerr) |q| only and the offsets survive.  So "1 / 2 / 4 units behind the plant, in that order" holds
    - and is asserted (test_batch_half_cases.check_plants) - under L2 and squared L2; under dot and cosine the half-precision rows are
    rows within a few units of the plant, on either side of it, no more.  They sit in the tiles ahead of the plant in descending u, so
    that at k = 1 each of them has to pass a threshold it beats by a few units only.
    f32 worlds also hold rows that differ from a query below bf16 precision (low mantissa bits only: the shadow copy of each IS the
    query's, asserted) - only the exact evaluation orders them;
  * what the filter cannot judge: rows with norms outside [1e-15, 1e15] (and just inside) where the type holds them, a zero row, the
    Inf / NaN / largest-value / subnormal rows of datagen.edge_rows.  batch_reference hands exactly these to the oracle;
  * corpora of more than 7040 rows: the _adversarial rows of tests/test_gpu_batch_q8.py."""
import numpy as np

import datagen as dg
from test_gpu_batch_q8 import _adversarial
from test_gpu_batch_q8_forms import spectrum

MASTER_NQ = 257
ADV_Q0 = 20                                    # _adversarial's rows are made of queries 20 .. 24
SECOND_COPIES = (2, 33, 130)                   # queries whose plant has a second copy further down
SLACK_TARGETS = (5, 40, 200)                   # queries with rows aimed at the filter's slack
SLACK_UNITS = (4, 2, 1)                        # units of cerr |q| |x| behind the plant, in the order of their positions
SUBBF_TARGET = 6                               # f32 worlds: the query with near-copies below bf16 precision
SUBBF_MASKS = (0xFFF, 0x3FF, 0xFF)             # mantissa bits replaced in each of them
LADDER_Q = 7                                   # staged world: the query whose best row is copied up the stage ladder
ALL_METRICS = (dg.DOT, dg.COSINE, dg.L2, dg.SQUARED_L2)
N_SMALL, N_SPARSE, N_STAGED = 20_003, 8_259, 2_097_187
TINY_NQ = 8


def cerr(vt, dim):
    """a.cerr of vg_batch_h_launch"""
    return (dim + 64) * 2.0 ** -21 + (2.0 ** -7 + 2.0 ** -16 if vt == dg.F32 else 0.0)


def slack_row(vt, dim, q64, units, rng):
    """(1 - c) (q + r): r orthogonal to q, |r|^2 = 2 c |q|^2, c = units * cerr - float32 values, not yet in storage"""
    c = units * cerr(vt, dim)
    r = rng.standard_normal(dim) * spectrum(dim)
    r -= q64 * (r @ q64) / (q64 @ q64)
    r *= np.sqrt(2.0 * c * (q64 @ q64) / (r @ r))
    return ((1.0 - c) * (q64 + r)).astype(np.float32)


def subbf_row(q32, mask, rng):
    """the query with the mantissa bits of `mask` replaced by random ones; elements whose bf16 rounding would change keep the query's"""
    b = q32.view(np.uint32)
    x = ((b & np.uint32(0xFFFFFFFF ^ mask)) | rng.integers(0, mask + 1, b.shape, dtype=np.uint32)).view(np.float32)
    same = dg.f32_to_bf16_bits(x) == dg.f32_to_bf16_bits(q32)
    return np.where(same, x, q32).astype(np.float32)


class HalfWorld:
    def __init__(self, vt, dim, n, seed, nq=MASTER_NQ, ladder=False):
        self.vt, self.dim, self.n, self.nq = vt, dim, n, nq
        rng = np.random.default_rng(seed)
        w = spectrum(dim)
        rows = rng.standard_normal((n, dim), dtype=np.float32) * w * rng.choice(np.array([1, 1, 1, 2, 8], dtype=np.float32), (n, 1))
        qs = rng.standard_normal((nq, dim), dtype=np.float32) * w
        self._used = set()
        self.plant, self.second, self.duplicates = {}, {}, []
        self.slack_rows, self.subbf_rows, self.window_rows, self.ladder = {}, [], {}, []
        self.unjudged_rows = []                                    # zero / Inf / NaN / out-of-window rows (positions)
        late = {}                                                  # position -> row in storage, written after the conversion
        tiny = n < 7041
        if tiny:
            assert nq == TINY_NQ and n >= 20
            zero_at, edge_at = self.take(4)[0], self.take([6, 9])
            rows[zero_at] = 0.0
            _, edge = dg.edge_rows(vt, dim, seed + 1)
            bad = [r for r in edge if not np.isfinite(dg.storage_to_f64(vt, r)).all()]
            late[edge_at[0]], late[edge_at[1]] = bad[0], bad[-1]   # (f32: a NaN and an Inf element; halves: +Inf and +Inf / -Inf)
            self.unjudged_rows += [zero_at] + edge_at
            plant_at = iter([0, 1, 2, 3, 5, n - 1, n - 2, 7])
            slack_at = {5: [10, 11, 12]}                           # (target 5's plant: row n - 1, behind them)
            second_at = {2: 13}
            targets = (5,)
        else:
            self.take([11, n - 1, 5000, 5001] + list(range(6000, 6009)) + list(range(7000, 7040)))
            rows = _adversarial(rows, qs[ADV_Q0:], rng)
            if vt == dg.F16:                                       # (the largest / smallest norms the type holds)
                rows[6005] = rng.standard_normal(dim).astype(np.float32) * np.float32(1e3)
                rows[6004] = rng.standard_normal(dim).astype(np.float32) * np.float32(1e-4)
            self.unjudged_rows += [6000, 6004, 6005, 6006, 6007, 6008]
            self.plant[ADV_Q0], self.plant[ADV_Q0 + 1] = 11, n - 1
            self.plant[ADV_Q0 + 2] = self.take(40)[0]              # ahead of row 5000 = 3 x this query: the cosine tie goes by position
            _, edge = dg.edge_rows(vt, dim, seed + 1)
            for at, r in zip(self.take(range(3000, 3000 + len(edge))), edge):
                late[at] = r
                self.unjudged_rows.append(at)
            if vt != dg.F16:                                       # unit rows scaled to both sides of both ends of [1e-15, 1e15]; f16 holds neither
                for at, scale in zip(self.take(range(6100, 6106)), (1e-20, 5e-16, 2e-15, 5e14, 2e15, 1e20)):
                    u = rng.standard_normal(dim)
                    rows[at] = (u / np.linalg.norm(u) * scale).astype(np.float32)
                    self.window_rows[at] = scale
                    self.unjudged_rows.append(at)
            if ladder:
                # Copies of one query's best row at rows 32 2^j - 1 and 32 2^j, j = 0 .. 16, and in the last tile: more of them than k.  With
                # a power-of-two partition count the pre-pass and every stage of vgb_stage_bounds end at such a row - an assumption about
                # where the bounds fall, not about the answer: the reference decides the answer either way.
                self.ladder = self.take([p for j in range(17) for p in (32 * 2 ** j - 1, 32 * 2 ** j)] + [n - 3])
                self.plant[LADDER_Q] = self.ladder[0]
            # the slack targets: plant in the last row of a 96-row partition (3 tiles; 256 partitions over the small world), its slack rows
            # in the tiles before it - 480 p .. 480 p + 95 is also inside one 160-row partition (128 partitions)
            slack_at, targets = {}, tuple(t for t in SLACK_TARGETS if t < nq)
            for ti, t in enumerate(targets):
                base = 480 * (ti + 1)
                slack_at[t] = self.take([base + 5, base + 40, base + 70])
                self.plant[t] = self.take(base + 95)[0]
            # first tile, rows 31 / 32 / 33, first and last rows of partitions (96 p, 96 p + 95; 160 p + 159), the last ragged tile
            edges = [0, 1, 2, 4, 31, 32, 33, 96, 191, 192, 287, 159, 160, 319, 9600, 9695, n - 2, n - 4, n - 5, n - 33, n - 34]
            step = max(7, (n - 200) // (nq + 64)) | 1
            plant_at = iter(edges + [97 + step * j for j in range(nq + 64)])
            second_at = {i: 1000 * (si + 1) + n // 2 for si, i in enumerate(c for c in SECOND_COPIES if c < nq)}
        for i in range(nq):
            if i in self.plant:
                continue
            p = next(plant_at)
            while p in self._used or p >= n:
                p = next(plant_at)
            self.plant[i] = self.take(p)[0]
        for i, p in second_at.items():
            self.second[i] = self.take(p)[0]
        subbf_at = []
        if vt == dg.F32 and not tiny and SUBBF_TARGET < nq:
            subbf_at = self.take([self.plant[SUBBF_TARGET] + 3 + 64 * j for j in range(len(SUBBF_MASKS))])
        self.rows = dg.to_storage(vt, rows)
        self.queries = dg.to_storage(vt, qs)
        for at, r in late.items():
            self.rows[at] = r
        for i, p in self.plant.items():
            self.rows[p] = self.queries[i]
        for i, p in self.second.items():
            assert p > self.plant[i]
            self.rows[p] = self.queries[i]
            self.duplicates.append([self.plant[i], p])
        if self.ladder:
            self.rows[self.ladder] = self.queries[LADDER_Q]
            self.duplicates.append(list(self.ladder))
        for t in targets:                                          # (from the STORED query: what the kernel is given)
            q64 = dg.storage_to_f64(vt, self.queries[t])
            assert max(slack_at[t]) < self.plant[t]
            for at, units in zip(slack_at[t], SLACK_UNITS):
                self.rows[at] = dg.to_storage(vt, slack_row(vt, dim, q64, units, rng))
            self.slack_rows[t] = list(slack_at[t])
        for at, mask in zip(subbf_at, SUBBF_MASKS):
            x = subbf_row(self.queries[SUBBF_TARGET], mask, rng)
            assert np.array_equal(dg.f32_to_bf16_bits(x), dg.f32_to_bf16_bits(self.queries[SUBBF_TARGET])) and not np.array_equal(x, self.queries[SUBBF_TARGET])
            self.rows[at] = x
            self.subbf_rows.append(at)
        self._check_window_rows()

    def take(self, positions):
        positions = [int(p) for p in np.atleast_1d(positions)]
        assert not self._used.intersection(positions) and max(positions) < self.n and min(positions) >= 0, positions
        self._used.update(positions)
        return positions

    def _check_window_rows(self):
        """each scaled row's norm lands on the intended side of [1e-15, 1e15]"""
        for at, scale in self.window_rows.items():
            nrm = float(np.linalg.norm(dg.storage_to_f64(self.vt, self.rows[at])))
            assert abs(nrm / scale - 1.0) < 0.05 and (1e-15 <= nrm <= 1e15) == (scale in (2e-15, 5e14)), (at, scale, nrm)

    def weak_first(self, metric):
        """queries whose plant is not ahead of every other row by a float64 gap under `metric` - by construction: dot has no plants at all;
        under cosine the 3 x copy of query ADV_Q0 + 2 and the 1e-3 cluster around ADV_Q0 + 4 are at 0 too, and so are near-copies below bf16
        precision.  Everything else must be decided."""
        if metric == dg.DOT:
            return set(range(self.nq))
        if metric == dg.COSINE:
            return {ADV_Q0 + 2, ADV_Q0 + 4} | ({SUBBF_TARGET} if self.subbf_rows else set())
        return set()


# One world at a time is kept (the cases of one corpus follow each other).  Seeds moved on where the first one left more than
# batch_reference.BAND_SHARE_CAP of some case to the band check (tried without a device, reference alone: test_batch_half_cases.py).
SEED_STEP = {(dg.F16, 384, N_SMALL): 1, (dg.BF16, 384, N_SMALL): 1, (dg.F32, 192, N_SMALL): 1, (dg.F32, 384, N_SMALL): 1, (dg.F32, 1000, N_SMALL): 1,
             (dg.F16, 100, 33): 5, (dg.BF16, 100, 33): 13, (dg.BF16, 384, N_SPARSE): 1}
_CURRENT = {}


def world_seed(vt, dim, n):
    return 9700 + dim + 7 * vt + (n % 1000) + 10_000 * SEED_STEP.get((vt, dim, n), 0)


def world(vt, dim, n=N_SMALL, nq=None):
    nq = (TINY_NQ if n < 7041 else (160 if n == N_STAGED else MASTER_NQ)) if nq is None else nq
    key = (vt, dim, n, nq)
    if key not in _CURRENT:
        close_worlds()
        _CURRENT[key] = HalfWorld(vt, dim, n, world_seed(vt, dim, n), nq, ladder=(n == N_STAGED))
    return _CURRENT[key]


def close_worlds():
    for w in _CURRENT.values():
        for attr in ("_refs", "_corpus"):
            v = getattr(w, attr, None)
            if attr == "_corpus" and v is not None:
                v.close()
            if v is not None:
                setattr(w, attr, None)
    _CURRENT.clear()


def references(w, orc, br, queries=None, tag="master", metrics=ALL_METRICS, kmax=32):
    """{metric: BatchReference} of world w, computed once per (tag, metrics) and kept with the world"""
    if getattr(w, "_refs", None) is None:
        w._refs = {}
    key = (tag, tuple(metrics))
    if key not in w._refs:
        w._refs[key] = br.batch_references(w.vt, tuple(metrics), w.queries if queries is None else queries, w.rows, orc, kmax=kmax,
                                           duplicates=w.duplicates)
    return w._refs[key]


# ---- the matrix both test files walk: (type, dim) of the small world, and per world the (metric, k, nq) combinations the device file runs
HALF_DIMS = (100, 256, 384, 500, 768, 1000)                         # NTB 8, 16, 24, 32, 48, 64 at 2 bytes per element
F32_DIMS = (100, 192, 384, 500, 600, 1000)                          # the same buckets through the bf16 shadow copy (600, 1000: if path 3 serves)
BATCH_SIZES = (1, 31, 32, 33, 128, 129, 257)
KS = (1, 20, 27, 32)
# (no dot at k = 1: the rows with one +-Inf element - datagen.edge_rows, _adversarial - are at -Inf for every query whose element there has
#  the right sign, several of them for most queries: a tie at -Inf that no float64 gap decides.  At k >= 20 they are all inside the list.
#  The k = 1 dot inequality is anchored on the queries that meet no such row: dot1_queries, f32 worlds only.)
K_PAIRS = {1: ((dg.L2, dg.COSINE), (dg.SQUARED_L2, dg.COSINE)), 32: ((dg.COSINE, dg.DOT), (dg.L2, dg.DOT)), 27: ((dg.L2,), (dg.DOT,))}


# VG_BATCH_H_WAVES=8 / =4, VG_BATCH_TILE_MAJOR=0 on the small world.  VG_BATCH_H_SPLIT=1 has cases of its own (split_cases): the filter kernel
# of the split form keeps no lists, so its thresholds are those of the pre-pass and the earlier stages.  A corpus below 2^16 tiles has
# neither: every real pair passes, and a wavefront's region of 2048 pairs (32 queries x 64 rows) runs over once its 32 queries meet a THIRD
# tile in one partition - the fused kernel then answers (vg_batch_h_split_off).  The small world has 3 tiles in most partitions, so the split
# form answers there only for batches of a few queries; it answers every batch of one query group over the sparse world (259 tiles over
# 256 partitions: at most 2 each), over the tiny worlds, and behind the pre-pass of the staged world.
FORMS = ("waves8", "waves4", "rowmajor")
SPLIT_NQ = {8: 129, 16: 129, 24: 129, 32: 129, 48: 128, 64: 128}    # k-steps -> the largest batch size of BATCH_SIZES that is ONE query group there
TINY_WORLDS = [(vt, 100, n) for vt in (dg.F16, dg.BF16, dg.F32) for n in (20, 33)]
SPARSE_WORLDS = [(dg.BF16, 256), (dg.F16, 384), (dg.F32, 192)]
APPEND_WORLDS = [(dg.BF16, 256), (dg.F32, 192)]
UNJUDGED_WORLDS = [(dg.F16, 100), (dg.BF16, 384), (dg.F32, 192)]
UNJUDGED_SLOTS = (1, 31, 32)                                        # zero, one NaN element, one Inf element
STAGED = (dg.BF16, 16, N_STAGED)
APPEND_NQ, APPEND_BEST, APPEND_COPY = 129, 9, 10                    # queries whose new best row (dot) / second copy arrives with the appended rows


def form_cases(vt, dim):
    """(form, nq, metric, k): the full cross at dim 384; elsewhere one metric and k per form.  257 queries: two query groups and the
    4-wavefront form by itself; the forced 4-wavefront form also on a batch too small to choose it (33)"""
    one = [("split", 1, m, k) for d, m, k in SPLIT_ONE_QUERY if d == dim]
    if dim == 384:
        return [(f, 33 if (f == "waves4" and k == 1) else 257, m, k) for f in FORMS for m in ALL_METRICS for k in KS if (m, k) != (dg.DOT, 1)] + one
    out = [(f, 33 if f == "waves4" else 257, ALL_METRICS[(i + dim) % 4], KS[(i + dim // 4) % 4]) for i, f in enumerate(FORMS)]
    return [(f, nq, dg.L2 if (m, k) == (dg.DOT, 1) else m, k) for f, nq, m, k in out] + one


def filter_stride(dim):
    """bytes of a row as the matrix core reads it: 2-byte elements, zero padded to 16 bytes (an f32 corpus: its bf16 shadow copy)"""
    return (2 * dim + 15) // 16 * 16


def ntb_of(dim):
    """vgb_ntb64 of that row: k-steps of 32 bytes"""
    return [b for b in (8, 16, 24, 32, 48, 64) if (filter_stride(dim) + 31) // 32 <= b][0]


# the split form outside dim 384: one metric and k per k-step bucket (2 KiB rows: k <= 29, or no form of this kernel serves)
SPLIT_ONE = {8: (dg.L2, 20), 16: (dg.COSINE, 1), 32: (dg.DOT, 32), 48: (dg.SQUARED_L2, 27), 64: (dg.COSINE, 20)}
SPLIT_TINY = ((dg.L2, 20), (dg.COSINE, 20), (dg.DOT, 32))          # (metric, k) over every tiny world
# (dim, metric, k) of ONE query over the small world (every type): 626 tiles over 256 partitions are three tiles each, which one query's
# 96 pairs a region can afford - they ride with the other forms' cases (form_cases)
SPLIT_ONE_QUERY = ((384, dg.L2, 20), (384, dg.COSINE, 1), (1000, dg.DOT, 20))


def split_cases(vt, dim):
    """(nq, metric, k) of VG_BATCH_H_SPLIT=1 over the SPARSE world of (vt, dim): every type and k-step bucket, the full cross at dim 384.
    One query group (SPLIT_NQ), so that 256 partitions hold at most 2 tiles each and no pair region runs over: wavefronts of 32 queries
    fill theirs to the last pair (2 tiles x 32 rows x 32 queries = 2048), the ragged last wavefront of 129 holds one query."""
    nq = SPLIT_NQ[ntb_of(dim)]
    if dim == 384:
        return [(nq, m, k) for m in ALL_METRICS for k in KS if (m, k) != (dg.DOT, 1)]
    return [(nq,) + SPLIT_ONE[ntb_of(dim)]]


DOT1_WORLDS = [(dg.F32, 100), (dg.F32, 384)]


def dot1_queries(w):
    """the master queries that have NO row at -Inf under dot (no Inf element of a row meets an element of theirs of the same sign): for
    these dot at k = 1 is decided by a float64 gap.  About a quarter of the queries of an f32 world; none of an f16 / bf16 world (counted: every
    query meets such a row there) - dot at k = 1 stays out for the half-precision types."""
    X, Q = dg.storage_to_f64(w.vt, w.rows[w.unjudged_rows]), dg.storage_to_f64(w.vt, w.queries)
    with np.errstate(all="ignore"):
        return np.nonzero(~((Q @ X.T) == np.inf).any(axis=1))[0]


def unjudgeable_queries(w):
    """the first 129 master queries with a zero query, one NaN element and one Inf element in slots 1, 31 and 32"""
    qs = w.queries[:129].copy()
    nan, inf = {dg.F32: (np.float32(np.nan), np.float32(np.inf)), dg.F16: (dg.F16_NAN, dg.F16_INF), dg.BF16: (dg.BF_NAN, dg.BF_INF)}[w.vt]
    qs[UNJUDGED_SLOTS[0]] = 0
    qs[UNJUDGED_SLOTS[1], w.dim // 3] = nan
    qs[UNJUDGED_SLOTS[2], w.dim - 1] = inf
    return qs


def appended(w):
    """500 rows appended behind the world's ragged last tile: (all rows, their named duplicates).  Among them 30 x query APPEND_BEST (its new
    best ordinary row under dot) and a copy of query APPEND_COPY (ties with its plant across the boundary: second by position)"""
    rng = np.random.default_rng(world_seed(w.vt, w.dim, w.n) + 5)
    extra = rng.standard_normal((500, w.dim), dtype=np.float32) * spectrum(w.dim) * rng.choice(np.array([1, 2, 8], dtype=np.float32), (500, 1))
    extra[123] = dg.storage_to_f64(w.vt, w.queries[APPEND_BEST]).astype(np.float32) * np.float32(30.0)
    extra = dg.to_storage(w.vt, extra)
    extra[377] = w.queries[APPEND_COPY]
    assert APPEND_COPY not in w.second
    return np.concatenate([w.rows, extra]), w.duplicates + [[w.plant[APPEND_COPY], w.n + 377]]


def small_worlds():
    return [(vt, dim) for vt in (dg.F16, dg.BF16) for dim in HALF_DIMS] + [(dg.F32, dim) for dim in F32_DIMS]


def bucket_cases(vt, dim):
    """(nq, metric, k) on one small world: all four metrics at k = 20, k = 1 / 27 / 32 under their metrics, every batch size.  The batch
    size walks with the case (every size meets every world; the full cross is taken at dim 384 only)."""
    out = []
    sizes = BATCH_SIZES if dim == 384 else (BATCH_SIZES[(dim // 4 + vt) % 7], 129, 257)
    for j, nq in enumerate(sizes):
        for metric in (ALL_METRICS if (dim == 384 or j == 0) else (ALL_METRICS[(j + dim) % 4],)):
            out.append((nq, metric, 20))
        for k in (1, 27, 32):
            for metric in K_PAIRS[k][j % 2]:
                if dim == 384 or (j + k) % 3 == 0:
                    out.append((nq, metric, k))
    return out
