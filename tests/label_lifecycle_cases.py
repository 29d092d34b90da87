"""Case builder of tests/test_gpu_label_lifecycle.py: labels and the row mask of a handle across its lifecycle (patch / delete /
append, clear + a smaller or a larger re-append, clone, trim / reserve) as plain numpy bookkeeping - no device, no test in here.

Paths are the smallest shapes at which the label-aware code differs (labeled_cases.SHAPES): f32 x 384 (multi kernel, 4 queries per
pass), f32 x 1536 (2 per pass; the masked grouped / capped batch falls back to single scans), uint8 x 64 under L2 and cosine (four-level
values: equal distances are routine), f16 x 384 cosine (fallback forms, cached row norms) and bf16 x 384 L2 (fallback).

Float paths: random N(0,1) rows cannot be judged exactly, so every query i gets a LADDER of its own: rows equal to the query except in
one coordinate c_i where the query holds 0 and rung j holds t_j = (j + 1) * step - exactly representable in bf16 / f16 / f32, so the
float64 distances of a ladder to its query are strictly increasing, spaced far above 2 * batch_reference.completeness_tol, and far
below every other row (L2: <= 9 against ~ sqrt(2 dim); cosine: <= 0.53 against ~ 1 - 3.5 / sqrt(dim)).  Ladder rows sit at scattered
positions - position 0, the last one and both sides of every 64-row block boundary (the 3-shard map's) among them - and rank in the
ladder is independent of position.  Labels and mask follow the RANK (rung_label / rung_allowed): a label filling its cap on the first
rungs, a label whose better row comes later in scan order, LABEL_NONE rows among the nearest, a label only masked-out rows carry, a
label that the patch leaves on NaN / +Inf rows only, a block of labels with ~3 rows each, then labels of one rung each - enough
distinct ones that a 64-label grouped answer ends inside the ladder.  tests/test_label_lifecycle_cases.py proves, from float64 alone,
that every compared answer is decided; integer paths need none of this (the oracle is bit-exact there).

A script is a list of Steps: one call on the handle (op, args) and the state to compare afterwards (rows, rowids, labels, allowed).
The Model follows the code's rules: patch keeps labels and mask; delete, append and clear drop both (Step.dropped) and the step's
labels / allowed are what the script sets again; clone, trim and reserve keep both.  Step.prev_labels / prev_allowed: what the handle
held before the call, fitted to the new length - the stale state a wrong implementation would answer from."""
import collections
import functools

import numpy as np

import batch_reference as br
import datagen as dg
import labeled_cases as lab
import lifecycle_cases as lc

N, N_HALF = 3001, 1503                  # 3001 % 64 = 57; 1503 % 64 = 31, about half
NQ, NQ_GROUP = 9, 5                     # labeled batch: 9 queries; grouped / capped: 5 (one full pass of 4 and a ragged one)
KMS = ((20, 3), (64, 5), (20, 1))
NONE, ABSENT = lab.NONE, lab.ABSENT
FLOATS = lc.FLOATS
BLOCK = 64
R_BIG, R_SMALL = 144, 32                # rungs of the ladders of queries 0..4 / 5..8 (the latter only answer labeled scans)
L_POOL, L_SINGLE, L_MASKED, L_SPECIAL, L_U, L_V = 100, 200, 500, 999, 1000, 2000
NEAR = 8                                # eligible rows behind an answer's last row that must be clear of it too

Path = collections.namedtuple("Path", "name vt dim metric")
PATHS = (
    Path("f32_384_l2", dg.F32, 384, dg.L2),
    Path("f32_1536_l2", dg.F32, 1536, dg.L2),
    Path("u8_64_l2", dg.U8, 64, dg.L2),
    Path("u8_64_cosine", dg.U8, 64, dg.COSINE),
    Path("f16_384_cosine", dg.F16, 384, dg.COSINE),
    Path("bf16_384_l2", dg.BF16, 384, dg.L2),
)
PATH_BY_NAME = {p.name: p for p in PATHS}

World = collections.namedtuple("World", "rows ids labels allowed ladder")       # ladder[i][rank] = rowid of query i's rung (floats)
Step = collections.namedtuple("Step", "op args rows ids labels allowed dropped prev_labels prev_allowed")


def _seed(p):
    return 7100 + 131 * PATHS.index(p)


def is_float(p):
    return p.vt in FLOATS


def coord(i):
    """the coordinate query i's ladder climbs along (the query holds 0 there)"""
    return 5 + 7 * i


@functools.lru_cache(maxsize=None)
def queries(name):
    p = PATH_BY_NAME[name]
    qs = lab.data(p.vt, NQ, p.dim, _seed(p) + 1)
    if is_float(p):
        for i in range(NQ):
            qs[i, coord(i)] = 0                                    # (+0.0 in every float format)
            if p.vt == dg.F32:                                     # the lane the patch's +Inf element sits in: under DOT the row is at
                qs[i, p.dim - 1] = abs(qs[i, p.dim - 1]) * (1.0 if i % 2 == 0 else -1.0)      # -Inf for even queries, +Inf for odd ones
    return qs


def rung_t(p, j):
    """offset of rung j (fractions: between rungs) - multiples of 1/32 (L2) or 1/8 (cosine) below 2^8 of them: exact in bf16"""
    return (j + 1) * (0.25 if p.metric == dg.COSINE else 1.0 / 16.0)


def ladder_row(p, q, i, j):
    x = dg.storage_to_f64(p.vt, q[None, :]).astype(np.float32)
    x[0, coord(i)] = rung_t(p, j)
    return dg.to_storage(p.vt, x)[0]


def rung_label(i, j):
    if j in (0, 1, 2, 3, 4, 5, 30):
        return L_U + i                                             # fills a cap of 3 / 5 on the first rungs; only ladder i carries it
    if j in (8, 12):
        return L_V + i                                             # rung 8 sits BEHIND rung 12 in scan order
    if j in (6, 9, 40):
        return NONE
    if j in (7, 15):
        return L_MASKED                                            # every row of this label is masked out
    if i == 0 and j in (10, 11):
        return L_SPECIAL                                           # the patch turns both rows into NaN / +Inf rows
    if 16 <= j < 54:
        return L_POOL + (j - 16) % 13                              # ~3 rungs each
    return L_SINGLE + j                                            # one rung each


def rung_allowed(j):
    return not (j in (7, 15) or (j >= 54 and j % 5 == 0))


def _ladder_positions(n, rng):
    """per query the positions of its rungs: [0, n-1] (query 0), both sides of the 64-row boundaries dealt out in turn, the rest
    scattered over the rows in front of the last 450 (the deletions' end runs take few rungs that way)"""
    sizes = [R_BIG] * NQ_GROUP + [R_SMALL] * (NQ - NQ_GROUP)
    pos = [[] for _ in range(NQ)]
    pos[0] += [0, n - 1]
    for b in range(1, (n - 2) // BLOCK + 1):
        pos[b % NQ] += [BLOCK * b - 1, BLOCK * b]
    used = set(x for l in pos for x in l)
    free = [int(x) for x in 1 + rng.permutation(n - 451) if int(x) not in used]
    for i in range(NQ):
        assert len(pos[i]) <= sizes[i]
        take = sizes[i] - len(pos[i])
        pos[i] += free[:take]
        free = free[take:]
    return [np.array(l, dtype=np.int64) for l in pos]


def _build(p, n, seed, ids):
    rng = np.random.default_rng(seed)
    rows = lab.data(p.vt, n, p.dim, seed + 1)
    labels = np.where(rng.random(n) < 0.5, L_POOL + rng.integers(0, 13, n), L_SINGLE + rng.integers(0, R_BIG, n)).astype(np.uint32)
    labels[rng.random(n) < 0.1] = NONE
    allowed = rng.random(n) < 0.75
    hidden = rng.permutation(n)[:30]
    labels[hidden], allowed[hidden] = L_MASKED, False
    ladder = None
    if is_float(p):
        qs, ladder = queries(p.name), []
        for i, at in enumerate(_ladder_positions(n, rng)):
            order = at[rng.permutation(len(at))]                   # rank -> position
            if i == 0:                                             # position 0 and the last one among the nearest rungs
                for want, rank in ((0, 2), (n - 1, 4)):
                    j = int(np.nonzero(order == want)[0][0])
                    order[j], order[rank] = order[rank], order[j]
            if order[8] < order[12]:
                order[8], order[12] = order[12], order[8]
            for j, pos in enumerate(order):
                rows[pos] = ladder_row(p, qs[i], i, j)
                labels[pos] = rung_label(i, j)
                allowed[pos] = rung_allowed(j)
            ladder.append(ids[order].copy())
    else:                                                          # integers: labels worth asking for, one of them on few rows
        labels[rng.permutation(n)[:12]] = L_U
        labels[rng.permutation(n)[:5]] = L_V
    return World(rows, ids, labels, allowed, ladder)


@functools.lru_cache(maxsize=None)
def world(name, small=False):
    p = PATH_BY_NAME[name]
    if small:
        return _build(p, N_HALF, _seed(p) + 40, lc.make_ids(N_HALF, 5, 2))
    return _build(p, N, _seed(p) + 20, lc.make_ids(N))


def ask_labels(name, i):
    """the three labels query i asks the labeled scans for, one of them absent"""
    if is_float(PATH_BY_NAME[name]):
        return (L_U + i, L_V + i, ABSENT)                           # (labels whose rows all sit in the query's own ladder)
    return (L_U, L_V, ABSENT)


def batch_labels(name):
    """labeled batch: a label per query, mixed"""
    return np.array([ask_labels(name, i)[(0, 1, 0, 2, 1, 0, 0, 1, 2)[i]] for i in range(NQ)], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------- the reference

def distances(p, orc, rows, metric=None):
    """[NQ, rows] float64 reference distances of every query (metric: the path's unless given): floats element by element in float64, rows the float64 reference does not
    speak for (a NaN / Inf element, a norm outside the float32 range) take the oracle's value, as batch_reference has it; uint8: the
    oracle's float32, which is exact there"""
    qs = queries(p.name)
    metric = p.metric if metric is None else metric
    if not is_float(p):
        return np.stack([orc.scan_distances(orc.AVX2, metric, p.vt, q, rows).astype(np.float64) for q in qs])
    X, Q = dg.storage_to_f64(p.vt, rows), dg.storage_to_f64(p.vt, qs)
    sp = np.nonzero(br._out_of_range(X))[0]
    out = np.stack([br._elementwise(metric, Q[i], X) for i in range(NQ)])
    for i in range(NQ):
        if len(sp):
            out[i, sp] = orc.scan_distances(orc.AVX2, metric, p.vt, qs[i], rows[sp]).astype(np.float64)
    return out


def eligible(kind, d, labels, allowed, label=None):
    """positions a scan of this kind may return, in (distance, position) order - float64, nothing is cast"""
    with np.errstate(invalid="ignore"):
        ok = np.asarray(d, dtype=np.float64) < np.inf
    ok &= (labels == label) if kind == "labeled" else (labels != NONE)
    if allowed is not None:
        ok &= np.asarray(allowed, dtype=bool)
    pos = np.nonzero(ok)[0]
    return pos[np.lexsort((pos, np.asarray(d, dtype=np.float64)[pos]))]


def answer(kind, d, labels, allowed, k, m=None, label=None):
    """the contract over float64 distances: positions, in order.  kind: labeled (rows of `label`), grouped (first row of each label),
    capped (at most m of a label)"""
    order = eligible(kind, d, labels, allowed, label)
    if kind == "labeled":
        return order[:k]
    cap, kept, have = (1 if kind == "grouped" else m), [], {}
    for pos in order:
        l = int(labels[pos])
        if have.get(l, 0) < cap:
            have[l] = have.get(l, 0) + 1
            kept.append(pos)
            if len(kept) == k:
                break
    return np.array(kept, dtype=np.int64)


def plan(name):
    """every call of one `ask`: (kind, masked, k, m, query, label); grouped does not read m, so it runs once per k"""
    out = []
    for k, m in KMS:
        for i in range(NQ_GROUP):
            for l in ask_labels(name, i):
                out.append(("labeled", False, k, None, i, int(l)))
        for masked in (False, True):
            for i in range(NQ_GROUP):
                out.append(("capped", masked, k, m, i, None))
    for k in sorted(set(k for k, _ in KMS)):
        for masked in (False, True):
            for i in range(NQ_GROUP):
                out.append(("grouped", masked, k, None, i, None))
        bl = batch_labels(name)
        for i in range(NQ):
            out.append(("batch_labeled", False, k, None, i, int(bl[i])))
    return out


def family(call):
    kind, masked = call[0], call[1]
    return ("labeled" if kind == "batch_labeled" else kind) + ("_masked" if masked else "")


FAMILIES = ("labeled", "grouped", "grouped_masked", "capped", "capped_masked")


def expect(call, D, labels, allowed):
    kind, masked, k, m, i, label = call
    return answer("labeled" if kind == "batch_labeled" else kind, D[i], labels, allowed if masked else None, k, m, label)


def fit(a, n, fill):
    """an array of the previous state read at the new length: cut, or continued by `fill`"""
    a = np.asarray(a)
    return a[:n].copy() if len(a) >= n else np.concatenate([a, np.full(n - len(a), fill, dtype=a.dtype)])


# ---------------------------------------------------------------------------------------------------- model and scripts

class Model(lc.Model):
    """lifecycle_cases.Model with the labels and the mask the handle should hold (None: dropped)"""

    def __init__(self, w):
        super().__init__(w.rows, w.ids)
        self.labels, self.allowed = w.labels.copy(), w.allowed.copy()

    def _step(self, op, args, dropped, prev):
        return Step(op, args, self.rows.copy(), self.ids.copy(), self.labels.copy(), self.allowed.copy(), dropped,
                    fit(prev[0], len(self.ids), NONE), fit(prev[1], len(self.ids), False))

    def patch(self, pos, new):
        prev = (self.labels, self.allowed)
        super().patch(pos, new)
        return self._step("patch", (np.asarray(pos, dtype=np.int64), new), False, prev)      # labels and mask stay

    def delete(self, pos):
        prev = (self.labels, self.allowed)
        keep = np.ones(len(self.ids), bool)
        keep[pos] = False
        super().delete(pos)
        self.labels, self.allowed = self.labels[keep], self.allowed[keep]                   # (what the script sets again: they follow the rows)
        return self._step("delete", (np.asarray(pos, dtype=np.int64),), True, prev)

    def append(self, new, ids, labels, allowed):
        prev = (self.labels, self.allowed)
        super().append(new, ids)
        self.labels = np.concatenate([self.labels, np.asarray(labels, dtype=np.uint32)])
        self.allowed = np.concatenate([self.allowed, np.asarray(allowed, dtype=bool)])
        return self._step("append", (new, ids), True, prev)


def _where(m, rowids):
    """current positions of the rowids still held"""
    at = np.searchsorted(m.ids, rowids)
    at = at[at < len(m.ids)]
    return at[np.isin(m.ids[at], rowids)]


def _patch_step(p, w, m, rng):
    """300 rows: fresh random ones at scattered positions; floats: per big ladder rung 20 moved down to between rungs 1 and 2, rung 3
    moved up to between rungs 25 and 26, rung 18 moved out (a random row), and ladder 0's two L_SPECIAL rungs become a row with a NaN
    and a row with a +Inf element (its last lane; f32: under DOT that row is at -Inf for the even queries, whose last element is
    positive, and at +Inf for the odd ones) - their labels stay where they are"""
    n = len(m.ids)
    new = lab.data(p.vt, 300, p.dim, _seed(p) + 2)
    if not is_float(p):
        pos = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)[:298]]).astype(np.int64)
        return m.patch(pos, new)
    qs = queries(p.name)
    on_ladder = np.concatenate([_where(m, l) for l in w.ladder])
    plain = np.setdiff1d(np.arange(n), on_ladder)
    pos, j = [], 0
    for i in range(NQ_GROUP):
        at = np.searchsorted(m.ids, w.ladder[i][[20, 3, 18]])
        new[j], new[j + 1] = ladder_row(p, qs[i], i, 1.5), ladder_row(p, qs[i], i, 25.5)
        pos += at.tolist()
        j += 3
    at = np.searchsorted(m.ids, w.ladder[0][[10, 11]])
    x = dg.storage_to_f64(p.vt, new[j:j + 2]).astype(np.float32)
    x[0, p.dim // 3], x[1, p.dim - 1] = np.nan, np.inf
    new[j:j + 2] = dg.to_storage(p.vt, x)
    pos += at.tolist()
    pos += plain[rng.permutation(len(plain))[:300 - len(pos)]].tolist()
    return m.patch(np.array(pos, dtype=np.int64), new)


def _delete_positions(p, w, m, end_min, target_mod, d, rng):
    """a run of 7 at the front, 200 singles - three rungs of every big ladder among them -, a run at the very end of at least end_min
    rows: the smallest that leaves (rows mod 64) == target_mod"""
    n = len(m.ids)
    e = end_min
    while (n - 207 - e) % BLOCK != target_mod:
        e += 1
    body = np.arange(7, n - e)
    singles = []
    if is_float(p):
        rungs = np.concatenate([_where(m, w.ladder[i][[16 + d, 60 + d, 64 + d]]) for i in range(NQ_GROUP)])
        singles = rungs[(rungs >= 7) & (rungs < n - e)].tolist()
        body = np.setdiff1d(body, np.concatenate([_where(m, l) for l in w.ladder]))
    singles += body[rng.permutation(len(body))[:200 - len(singles)]].tolist()
    dele = np.sort(np.concatenate([np.arange(7), singles, np.arange(n - e, n)])).astype(np.int64)
    assert len(np.unique(dele)) == 207 + e
    return dele


@functools.lru_cache(maxsize=None)
def edit_script(name):
    """patch, three deletions (rows mod 64 -> 0, 1, 63; the first cuts more than two whole 64-row blocks off the end), then an append
    of 100 rows with a new ladder top for query 1 (a new best row of it on the integer paths)"""
    p, w = PATH_BY_NAME[name], world(name)
    m, rng = Model(w), np.random.default_rng(_seed(p) + 4)
    steps = [_patch_step(p, w, m, rng)]
    for d, target in enumerate((0, 1, 63)):
        steps.append(m.delete(_delete_positions(p, w, m, 130 if d == 0 else 3, target, d, rng)))
    more = lab.data(p.vt, 100, p.dim, _seed(p) + 6)
    labels = (L_POOL + rng.integers(0, 13, 100)).astype(np.uint32)
    allowed = rng.random(100) < 0.75
    more[37] = ladder_row(p, queries(name)[1], 1, -0.5) if is_float(p) else lc.best_row(p.vt, p.metric, queries(name)[1])
    labels[37], allowed[37] = ask_labels(name, 1)[0], True
    steps.append(m.append(more, np.arange(10**7, 10**7 + 100, dtype=np.int64), labels, allowed))
    return tuple(steps)


def _content_step(op, w, prev):
    return Step(op, (w.rows, w.ids), w.rows.copy(), w.ids.copy(), w.labels.copy(), w.allowed.copy(), True,
                fit(prev.labels, len(w.ids), NONE), fit(prev.allowed, len(w.ids), False))


@functools.lru_cache(maxsize=None)
def clear_smaller_script(name):
    """(first content, the step): the first content's 70 labels right behind where the second content will end all equal the label
    query 0 asks the labeled scans for, and their mask bits are set; then clear and about half as many rows (no multiple of 64)"""
    first, second = world(name), world(name, small=True)
    labels, allowed = first.labels.copy(), first.allowed.copy()
    labels[N_HALF:N_HALF + 70], allowed[N_HALF:N_HALF + 70] = ask_labels(name, 0)[0], True
    first = first._replace(labels=labels, allowed=allowed)
    return first, _content_step("clear_append", second, first)


@functools.lru_cache(maxsize=None)
def clear_larger_script(name):
    """(first content, the step): the second content holds more labels than max(rows, 1024) of the first and more bitmap words - both
    allocations are made again"""
    first, second = world(name, small=True), world(name)
    return first, _content_step("clear_append", second, first)


def compared_states(name):
    """every state an answer is compared in: (what, Step)"""
    out = [("start", _content_step("create", world(name), world(name, small=True)))]
    out += [("edit %d %s" % (i, s.op), s) for i, s in enumerate(edit_script(name))]
    out.append(("clear_smaller", clear_smaller_script(name)[1]))
    out.append(("clear_larger", clear_larger_script(name)[1]))
    return out
