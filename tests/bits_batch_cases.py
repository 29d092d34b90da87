"""What tests/test_gpu_bits_gates.py and tests/test_gpu_bits_lifecycle.py share (no test in here; tests/test_bits_batch_cases.py checks
this module without a device): the Hamming / Jaccard distances of a whole batch at once, batches of pairwise DIFFERENT queries with a
planted row each, ladders of rows that put a row at every distance next to a list's threshold, the edge radii of such a ladder, a numpy
transcription of the kernels' integer gates, and the lifecycle script of the bit-vector forms as plain numpy bookkeeping.

Everything is exact integer arithmetic plus - for Jaccard - one float32 division: every comparison the tests make is ==."""
import collections
import functools

import numpy as np

import hamming_cases as hc
import jaccard_cases as jc
from lifecycle_cases import Model, make_ids

CASES = {"hamming": hc, "jaccard": jc}
TILE = 32
FLT_MAX = float(np.finfo(np.float32).max)
NO_LABEL = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- the reference of a whole batch

def _bits(a):
    return np.unpackbits(np.ascontiguousarray(a), axis=1).astype(np.float32)


def batch_distances(name, rows, qs):
    """float32 [nq, n].  I = Qbits @ Xbits.T is exact in float32 (every count is <= 4096 < 2^24); Hamming = |q| + |x| - 2 I, Jaccard =
    float32(u - I) / float32(u) with u = |q| + |x| - I, 0 where u == 0.  The rows go in slices so that their unpacked bits stay small"""
    rows, qs = np.asarray(rows), np.asarray(qs)
    Q = _bits(qs)
    qc = Q.sum(1)
    out = np.zeros((qs.shape[0], rows.shape[0]), dtype=np.float32)
    step = max(1, (1 << 21) // max(1, rows.shape[1]))
    for r0 in range(0, rows.shape[0], step):
        X = _bits(rows[r0:r0 + step])
        I = Q @ X.T
        S = qc[:, None] + X.sum(1)[None, :]
        if name == "hamming":
            out[:, r0:r0 + step] = S - 2.0 * I
        else:
            u = S - I
            np.divide(u - I, u, out=out[:, r0:r0 + step], where=u > 0)
    return out


def order(d, allowed=None):
    """scan positions in (distance, position) order, the allowed ones only"""
    pos = np.argsort(np.asarray(d, dtype=np.float32), kind="stable")
    return pos if allowed is None else pos[np.asarray(allowed, dtype=bool)[pos]]


def expected(d, k, allowed=None, rowids=None, pos=None):
    """hamming_cases.expected; `pos`: order(d, allowed) computed before, shared by every k"""
    d = np.asarray(d, dtype=np.float32)
    pos = (order(d, allowed) if pos is None else pos)[:k]
    return (pos + 1 if rowids is None else np.asarray(rowids)[pos]), d[pos]


def within(d, radius, allowed=None, limit=None, rowids=None, pos=None):
    """hamming_cases.within, with explicit rowids; `pos`: order(d, allowed) computed before - a radius takes a prefix of it"""
    d = np.asarray(d, dtype=np.float32)
    pos = order(d, allowed) if pos is None else pos
    m = int(np.searchsorted(d[pos].astype(np.float64), radius, side="right")) if radius == radius else 0
    pos = pos[:m] if limit is None else pos[:min(m, limit)]
    return (pos + 1 if rowids is None else np.asarray(rowids)[pos]), d[pos], m


def check_within(name, got, wants, ctx):
    m = CASES[name]
    assert len(got) == len(wants), ctx
    for i, ((wi, wd, wm), g) in enumerate(zip(wants, got)):
        assert g[2] == wm, (ctx, i, g[2], wm)
        m.check(g, (wi, wd), (ctx, i))


# ---------------------------------------------------------------------------------------------------- distinct queries

def distinct_queries(dim, nq, seed):
    """nq pairwise different queries: query 0 all zero, query 1 all ones, the others of bit density 1/8 or 1/2"""
    rng = np.random.default_rng(seed)
    qs = jc.random_rows(nq, dim, rng, (1.0 / 8, 1.0 / 2))
    qs[:, 0] |= 1                                               # (none of them empty)
    qs[0] = 0
    if nq > 1:
        qs[1] = 255
    assert len(np.unique(qs, axis=0)) == nq
    return qs


def plant_positions(n, nq, seed, forced=()):
    """a position per query, all different: the forced ones, the first tile, both sides of tile boundaries, the last - partial - tile,
    the rest anywhere"""
    last = (n - 1) // TILE * TILE                               # first row of the last tile
    special = [p for p in (5, 31, 32, 0, n - 1, last, last - 1, 63, 64, 1023, 1024, n // 2 // TILE * TILE - 1) if 0 <= p < n]
    pos = list(dict.fromkeys(list(forced) + special))[:nq]
    rest = np.setdiff1d(np.arange(n), pos)
    pos += np.random.default_rng(seed).choice(rest, nq - len(pos), replace=False).tolist()
    assert len(set(pos)) == nq
    return np.asarray(pos, dtype=np.int64)


def planted(dim, n, nq, seed, forced=()):
    """(rows, queries, positions): mixed-density rows with query i at positions[i] - its first answer is a row no other query has"""
    qs = distinct_queries(dim, nq, seed)
    rows = jc.random_rows(n, dim, np.random.default_rng(seed + 1))
    pos = plant_positions(n, nq, seed + 2, forced)
    rows[pos] = qs
    return rows, qs, pos


# ---------------------------------------------------------------------------------------------------- the gates, transcribed

def gate_ham(qc, thr):
    """vgbb_gate_ham: ng of `2 i + ng - |x| >= 0`"""
    thr = np.float32(thr)
    if thr == -np.inf:
        return -(1 << 30)
    if not thr < np.float32(1.0e9):
        return 1 << 30
    return int(np.ceil(thr)) - 1 - int(qc)


def gate_jac(thr):
    """vgbb_gate_jac: gt of `(S - 2 i) << 18 <= umul24(gt, S - i)`"""
    thr = np.float32(thr)
    if thr == -np.inf:
        return 0
    if not thr < np.float32(2.0):
        return 1 << 19
    return int(np.ceil(np.float32(thr * np.float32(262144.0))))


def passes_ham(i, ng, xx):
    return 2 * np.asarray(i, dtype=np.int64) + ng - xx >= 0


def passes_jac(i, qc, gt, xx):
    """the kernels' expression in uint32 arithmetic: the shift wraps at 2^32, the product takes the low 24 bits of both factors"""
    i, qc, gt, xx = (np.asarray(a, dtype=np.int64) for a in (i, qc, gt, xx))
    S = qc + xx
    lhs = ((S - 2 * i) << 18) & 0xFFFFFFFF
    rhs = ((gt & 0xFFFFFF) * ((S - i) & 0xFFFFFF)) & 0xFFFFFFFF
    return lhs <= rhs


def jaccard_f32(i, u):
    """fl((u - i) / u), 0 where u == 0"""
    i, u = np.asarray(i, dtype=np.int64), np.asarray(u, dtype=np.int64)
    out = np.zeros(np.broadcast(i, u).shape, dtype=np.float32)
    np.divide((u - i).astype(np.float32), u.astype(np.float32), out=out, where=u > 0)
    return out


def gate_jac_many(thr):
    """gate_jac over an array of finite thresholds below 2"""
    return np.ceil(np.asarray(thr, dtype=np.float32) * np.float32(262144.0)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def jaccard_tight(nbits, w, count=64):
    """the `count` (i, u, i2, u2, slack) of a query of w set bits in rows of nbits bits with the smallest slack gt u - ((u - i) << 18),
    gt = gate_jac(thr), thr = fl((u2 - i2) / u2) the next distinct distance above the pair's own among the pairs such a query can meet"""
    i, u = np.meshgrid(np.arange(w + 1), np.arange(max(w, 1), nbits + 1), indexing="ij")
    i, u = i.ravel(), u.ravel()
    d = jaccard_f32(i, u)
    srt = np.argsort(d, kind="stable")
    ds = d[srt]
    first = np.flatnonzero(np.r_[True, ds[1:] != ds[:-1]])     # start of every run of equal distances
    run = np.cumsum(np.r_[True, ds[1:] != ds[:-1]]) - 1
    has_next = run < len(first) - 1
    nxt = srt[first[np.minimum(run + 1, len(first) - 1)]]      # a pair of the next distinct distance
    thr = d[nxt]
    slack = gate_jac_many(thr) * u[srt] - ((u[srt] - i[srt]) << 18)
    slack = np.where(has_next, slack, np.iinfo(np.int64).max)
    best = np.argsort(slack, kind="stable")[:count]
    return tuple((int(i[srt[b]]), int(u[srt[b]]), int(i[nxt[b]]), int(u[nxt[b]]), int(slack[b])) for b in best)


# ---------------------------------------------------------------------------------------------------- gate ladders

LADDER_WEIGHT = {16: 40, 100: 150, 128: 200, 200: 200, 256: 200, 272: 200, 512: 200}
Ladder = collections.namedtuple("Ladder", "q rows common extra copy")
PARTITIONS = 256                                    # the most partitions a batch is cut into (vg_batch_api.hip: one per CU, at most 256)
DENSE_TILES = 4 * PARTITIONS                        # tiles a dense ladder holds at least - among its ALLOWED rows too: a workgroup then
#                                                     owns four tiles or more and meets the gate under thresholds its own lists made


def _extras(free, count=0):
    """unset bits of the query a class takes: 0, 1, a few small ones, half and all of them; count > 0: at least so many - the
    smallest ones and as many spread evenly over the rest"""
    out = {e for e in (0, 1, 2, 3, 5, 8, 13, 21, 34, free // 2, free - 1, free) if 0 <= e <= free}
    if count:
        out |= set(range(min(free + 1, count // 2))) | set(np.linspace(0, free, count - count // 2).astype(np.int64).tolist())
    return sorted(out)


def _rows_with_counts(common, extra, q, seed):
    """jaccard_cases.rows_with_counts for tens of thousands of rows: the query's set bits (and its unset ones) stand in ONE random order,
    a row takes a run of that order - `common` (`extra`) long, from an offset of its own, cyclic"""
    rng = np.random.default_rng(seed)
    qbits = np.unpackbits(q).astype(bool)
    bits = np.zeros((common.size, qbits.size), dtype=bool)
    for idx, want in ((np.flatnonzero(qbits), common), (np.flatnonzero(~qbits), extra)):
        if idx.size:
            assert want.max(initial=0) <= idx.size
            idx = rng.permutation(idx)
            off = rng.integers(0, idx.size, want.size)
            for r0 in range(0, want.size, 8192):
                sl = slice(r0, r0 + 8192)
                run = (np.arange(idx.size)[None, :] - off[sl, None]) % idx.size < want[sl, None]
                part = bits[sl]
                part[:, idx] = run
    return np.packbits(bits, axis=1)


@functools.lru_cache(maxsize=8)
def _ladder_classes(dim, dense):
    """(query, rows, common, extra, copies) - one row per class (i, e) and copy, in class order, copy after copy: i over 0 .. w, e over
    _extras, plus the 64 tightest Jaccard pairs of this row length and the pairs whose distance is their threshold.  Two copies; a dense
    ladder takes more e and as many copies (three or more) as it needs for DENSE_TILES tiles without its first copy"""
    w, nbits = LADDER_WEIGHT[dim], 8 * dim
    q = jc.weighted_query(dim, w, 9000 + dim)
    cls = {(i, e) for i in range(w + 1) for e in _extras(nbits - w, (DENSE_TILES * TILE // 2) // (w + 1) + 4 if dense else 0)}
    for i, u, i2, u2, _ in jaccard_tight(nbits, w):
        cls |= {(i, u - w), (i2, u2 - w)}
    cls = np.asarray(sorted(cls), dtype=np.int64)
    copies = max(3, -(-DENSE_TILES * TILE // len(cls)) + 1) if dense else 2
    common, extra = np.tile(cls[:, 0], copies), np.tile(cls[:, 1], copies)
    assert common.size <= 70_000
    if dense:
        assert (copies - 1) * len(cls) >= DENSE_TILES * TILE
        return q, _rows_with_counts(common, extra, q, 9100 + dim), common, extra, copies
    return q, jc.rows_with_counts(common, extra, dim, q, 9100 + dim), common, extra, copies


@functools.lru_cache(maxsize=4)
def ladder(name, dim, ordering, dense=False):
    """the ladder of one row length in one ordering.  Every class stands at two (dense: three or more) positions far apart - its copies.
      random      a permutation
      descending  copy 0 as a run of falling distance (equal ones side by side), then every other copy as another: inside a run every
                  row of a new distance beats all rows before it
      ascending   every copy as a run of rising distance: only the first rows of a run can pass the gate, and in a later run these
                  tie with what the lists hold
    dense: DENSE_TILES tiles or more, so that each of the at most 256 partitions of a top-k batch is several tiles long and its
    workgroup judges tiles under thresholds that its own lists produced - a small ladder is one tile per partition on a 256-CU device,
    where only the `list not full` sentinel ever stands in the gate.  The range forms' gate is the radius: they take the small one"""
    q, rows, common, extra, copies = _ladder_classes(dim, dense)
    per = common.size // copies
    copy = np.repeat(np.arange(copies), per)
    w = LADDER_WEIGHT[dim]
    d = (w - common + extra).astype(np.float32) if name == "hamming" else jaccard_f32(common, w + extra)
    if ordering == "random":
        perm = np.random.default_rng(9200 + dim).permutation(common.size)
    else:
        sign = -1.0 if ordering == "descending" else 1.0
        perm = np.concatenate([c * per + np.argsort(sign * d[c * per:(c + 1) * per], kind="stable") for c in range(copies)])
    return Ladder(q, rows[perm], common[perm], extra[perm], copy[perm])


def ladder_distances(name, dim, lad):
    """the ladder query's distances from the classes alone (the tests compare them with batch_distances over the rows)"""
    w = LADDER_WEIGHT[dim]
    return (w - lad.common + lad.extra).astype(np.float32) if name == "hamming" else jaccard_f32(lad.common, w + lad.extra)


def ladder_corpus(name, dim, ordering, nq, seed, dense=False):
    """(rows, queries, copy): the ladder with a planted row of every other query behind it, shuffled; query 0 is the ladder's own, the
    others are distinct_queries (one all zero, one all ones).  copy: the copy's number for ladder rows, 1 for the planted ones"""
    lad = ladder(name, dim, ordering, dense)
    others = distinct_queries(dim, nq - 1, seed)
    perm = np.random.default_rng(seed + 1).permutation(nq - 1)
    rows = np.concatenate([lad.rows, others[perm]])
    qs = np.concatenate([lad.q[None, :], others])
    assert len(np.unique(qs, axis=0)) == nq
    return rows, qs, np.concatenate([lad.copy, np.ones(nq - 1, dtype=np.int64)])


def edge_radii(name, d, ranks):
    """the edge radii of a query with distances d: every distinct distance at the `ranks` of the sorted distinct ones, the float just
    below each, Hamming d - 0.5 and d + 0.5 too, and -1, -0.0, 0, +Inf, FLT_MAX"""
    distinct = np.unique(np.asarray(d, dtype=np.float32))
    out = [-1.0, -0.0, 0.0, float("inf"), FLT_MAX]
    for r in ranks:
        v = distinct[min(r, distinct.size - 1)]
        out += [float(v), float(np.nextafter(v, np.float32(-np.inf)))]
        if name == "hamming":
            out += [float(v) - 0.5, float(v) + 0.5]
    return out


# ---------------------------------------------------------------------------------------------------- the lifecycle of the bit forms

N0, N_CLEAR, NQ_LIFE, K_LIFE = 3001, 1503, 130, 20
N_DELETED = 12                                      # 3001 -> 2989 rows (2989 % 32 = 13): the deleted rows lie inside the new last tile
CAPACITY = 3200                                     # the handle's reservation: the append of step 5 crosses it
# planted positions of queries 0 .. 9: queries 0 and 2 .. 5 inside the block that step 3 deletes, 6 and 7 in the same tile in front of it,
# 8 in the second tile, 9 at the row right behind the end of step 4's smaller content (1503)
FORCED = (3000, 5, 2989, 2990, 2995, 2999, 2976, 2988, 40, N_CLEAR)
Q_PATCH_A, Q_PATCH_B, Q_CLONE = 12, 16, 21           # queries whose planted rows the patches move: allowed and of their query's label there
State = collections.namedtuple("State", "op args rows ids allowed labels dropped")


def query_labels(nq=NQ_LIFE):
    return (np.arange(nq) % 5).astype(np.uint32)


def _mask_and_labels(rows, qs, pos_of, seed, flip):
    """a mask of about 70 % and labels 0 .. 4 over `rows`; the planted row of query i (pos_of: {query: position}) is allowed unless
    i % 4 == 2 and carries its query's label unless i % 4 == 3 - `flip` swaps the two exceptions' roles with those of i % 4 == 0"""
    rng = np.random.default_rng(seed)
    n = len(rows)
    allowed = rng.random(n) < 0.7
    labels = rng.integers(0, 5, n).astype(np.uint32)
    labels[rng.random(n) < 0.05] = NO_LABEL
    ql = query_labels()
    for i, p in pos_of.items():
        off_mask, off_label = (i % 4 == 0, i % 4 == 0) if flip else (i % 4 == 2, i % 4 == 3)
        allowed[p] = not off_mask
        labels[p] = (ql[i] + 1) % 5 if off_label else ql[i]
    return allowed, labels


def _positions(rows, qs):
    """{query: first position of a row equal to it}"""
    out = {}
    for i, q in enumerate(qs):
        at = np.flatnonzero((rows == q[None, :]).all(1))
        if at.size:
            out[i] = int(at[0])
    return out


@functools.lru_cache(maxsize=4)
def lifecycle(dim):
    """(queries, states) of one row length.  states[0] is the fresh content (appended in two halves by the runner); every later state
    names one call (op, args) and what the handle holds afterwards.  dropped: the call dropped mask and labels, the runner sets the
    state's own - which differ from the previous ones at planted rows.  trim / reserve / clone change no row: their states repeat the
    rows of the state in front.
      1 create   2 patch   3 delete (a block at the end)   4 clear_append (1503 rows)   5 append (across the reservation)
      6 trim   7 reserve   8 clone   9 patch (the original, the clone keeps state 8)"""
    seed = 9300 + dim
    rows, qs, pos = planted(dim, N0, NQ_LIFE, seed, FORCED)
    m = Model(rows, make_ids(N0))
    states = []

    def snap(op, args, dropped, flip=False, keep=None):
        if keep is not None:
            allowed, labels = keep.allowed, keep.labels
        else:
            allowed, labels = _mask_and_labels(m.rows, qs, _positions(m.rows, qs), seed + 10 + len(states), flip)
        states.append(State(op, args, m.rows.copy(), m.ids.copy(), allowed, labels, dropped))

    snap("create", (m.rows.copy(), m.ids.copy()), True)
    # 2 patch: query A's planted row becomes its complement; a copy of query B lands below B's planted row, at an allowed row of B's
    # label - the tie at distance 0 now resolves to it
    s0, ql = states[0], query_labels()
    below = [p for p in range(int(pos[Q_PATCH_B])) if s0.allowed[p] and s0.labels[p] == ql[Q_PATCH_B] and p not in set(pos.tolist())]
    assert below
    at = np.asarray([pos[Q_PATCH_A], below[len(below) // 2]], dtype=np.int64)
    new = np.stack([~qs[Q_PATCH_A], qs[Q_PATCH_B]])
    m.patch(at, new)
    snap("patch", (at, new), False, keep=s0)
    # 3 delete the last 12 rows: four of them equal queries
    dele = np.arange(N0 - N_DELETED, N0, dtype=np.int64)
    m.delete(dele)
    snap("delete", (dele,), True, flip=True)
    # 4 clear, then 1503 other rows: the old row 1503 - right behind the new end, inside its last tile - equals query 9, which the new
    # content does not hold; the queries from 30 on get a planted row at new positions
    fresh = jc.random_rows(N_CLEAR, dim, np.random.default_rng(seed + 3))
    newpos = plant_positions(N_CLEAR, NQ_LIFE - 30, seed + 4)
    fresh[newpos] = qs[30:]
    m = Model(fresh, make_ids(N_CLEAR, 5, 2))
    snap("clear_append", (fresh.copy(), m.ids.copy()), True)
    # 5 append 2000 rows (3503 > the reservation): planted rows of queries 2 .. 29
    more = jc.random_rows(2000, dim, np.random.default_rng(seed + 5))
    more[plant_positions(2000, 28, seed + 6)] = qs[2:30]
    more_ids = np.arange(10**7, 10**7 + 2000, dtype=np.int64)
    m.append(more, more_ids)
    snap("append", (more, more_ids), True, flip=True)
    for op in ("trim", "reserve", "clone"):
        snap(op, (), False, keep=states[-1])
    # 9 patch the original: the planted rows of query C and of the query behind it become their complements
    where = _positions(m.rows, qs)
    at, new = np.asarray([where[Q_CLONE], where[Q_CLONE + 1]], dtype=np.int64), np.stack([~qs[Q_CLONE], ~qs[Q_CLONE + 1]])
    m.patch(at, new)
    snap("patch", (at, new), False, keep=states[-1])
    return qs, tuple(states)


def lifecycle_radii(d, allowed=None):
    """a radius per query of a state with distances d [nq, n]: 0 (the planted row), the query's 5th smallest (allowed) distance, the float
    below that - in turn"""
    out = []
    for i in range(d.shape[0]):
        di = d[i] if allowed is None else d[i][allowed]
        d5 = np.float32(np.sort(di)[4])
        out.append([0.0, float(d5), float(np.nextafter(d5, np.float32(-np.inf)))][i % 3])
    return out


def answers(name, kind, qs, rows, ids, allowed, labels, radii=None):
    """the expected answer of one form over a state, a list per query: top-k forms (rowids, distances), range forms
    (rowids, distances, matches).  kind: plain / masked / labeled / within / within_masked"""
    d = batch_distances(name, rows, qs)
    ql = query_labels(len(qs))
    out = []
    for i in range(len(qs)):
        if kind in ("within", "within_masked"):
            out.append(within(d[i], radii[i], allowed=allowed if kind == "within_masked" else None, rowids=ids))
        else:
            al = allowed if kind == "masked" else (labels == ql[i]) if kind == "labeled" else None
            out.append(expected(d[i], K_LIFE, allowed=al, rowids=ids))
    return out


def stale_states(states, j):
    """what a handle that missed part of call j would answer from: {what: (rows, ids, allowed, labels)}
      before  the call did not happen at all
      behind  the new rows plus what the buffer holds behind the new end up to the next multiple of 32 (the previous content's rows, with
              its mask bits and labels) - where the call left such rows
      kept    the new rows under the previous mask and labels fitted to the new length - where the call dropped them"""
    old, new = states[j - 1], states[j]
    out = {"before": (old.rows, old.ids, old.allowed, old.labels)}
    n = len(new.ids)
    end = min(len(old.ids), (n + TILE - 1) // TILE * TILE)
    if new.op in ("delete", "clear_append") and end > n:
        out["behind"] = (np.concatenate([new.rows, old.rows[n:end]]), np.concatenate([new.ids, -1 - np.arange(end - n)]),
                         np.concatenate([new.allowed, old.allowed[n:end]]), np.concatenate([new.labels, old.labels[n:end]]))
    if new.dropped:
        out["kept"] = (new.rows, new.ids, np.resize(old.allowed, n), np.resize(old.labels, n))
    return out
