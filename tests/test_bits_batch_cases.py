"""tests/bits_batch_cases.py without a device: the batch reference against hamming_cases / jaccard_cases bit for bit, the claim the
kernels' integer gates rest on (a pair whose distance is below the threshold passes) over every pair of counts a row of
up to 4096 bits can have, the ladders' make-up, and that every step of the lifecycle script is decided by what the step changed: an
answer computed from the rows before the call, from the rows the buffer still holds behind the new end, or under the previous mask and
labels differs from the true one."""
import numpy as np
import pytest

import bits_batch_cases as bb

NAMES = ("hamming", "jaccard")


# ---------------------------------------------------------------------------------------------------- the batch reference

@pytest.mark.parametrize("dim", [16, 100, 128, 200, 512])
@pytest.mark.parametrize("name", NAMES)
def test_batch_reference_is_the_single_query_reference(name, dim):
    m = bb.CASES[name]
    rows, qs, pos = bb.planted(dim, 700, 9, 100 + dim)
    rows[7], rows[8] = 0, 255
    assert not qs[0].any() and (qs[1] == 255).all()
    d = bb.batch_distances(name, rows, qs)
    assert d.dtype == np.float32
    ids = bb.make_ids(700)
    allowed = np.arange(700) % 3 != 1
    for i, q in enumerate(qs):
        one = m.distances(rows, q)
        assert np.array_equal(d[i].view(np.uint32), one.view(np.uint32)), (name, dim, i)
        for al in (None, allowed):
            wi, wd = m.expected(one, 20, allowed=al, rowids=ids)
            gi, gd = bb.expected(d[i], 20, allowed=al, rowids=ids)
            assert gi.tolist() == wi.tolist() and gd.tobytes() == wd.tobytes()
            for r in bb.edge_radii(name, one, (0, 3, 40)):
                for limit in (None, 5):
                    wi, wd, wm = m.within(one, r, allowed=al, limit=limit)
                    gi, gd, gm = bb.within(d[i], r, allowed=al, limit=limit)
                    assert gm == wm and gi.tolist() == wi.tolist() and gd.tobytes() == wd.tobytes(), (name, dim, i, r, limit)
    assert d[0, 7] == 0 and (name == "hamming" or d[0, 8] == 1)     # the zero query: against a zero row, against all ones


def test_distinct_queries_have_an_answer_of_their_own():
    for name in NAMES:
        rows, qs, pos = bb.planted(100, 3001, 257, 5)
        assert len(np.unique(qs, axis=0)) == 257 and len(set(pos.tolist())) == 257
        assert {0, 5, 31, 32, 63, 64, 2976, 2975, 3000} <= set(pos.tolist())      # first tile, tile boundaries, the partial tile
        d = bb.batch_distances(name, rows, qs)
        first = [int(bb.order(d[i])[0]) for i in range(257)]
        assert first == pos.tolist()


# ---------------------------------------------------------------------------------------------------- the gate claim

def _jaccard_gate_sweep(us):
    """every 0 <= i <= u for u in us against thr = the float above fl((u - i) / u): (pairs, rejected, largest product)"""
    pairs = rejected = top = 0
    for u in us:
        i = np.arange(u + 1, dtype=np.int64)
        thr = np.nextafter(bb.jaccard_f32(i, u), np.float32(np.inf))
        gt = bb.gate_jac_many(thr)
        assert (gt <= 1 << 19).all()
        # the kernel sees |q| and |x| with |q| + |x| = S = u + i; the expression depends on S and i only
        ok = bb.passes_jac(i, u, gt, i)
        lhs, rhs = (u - i) << 18, gt * u
        assert (lhs < 1 << 32).all() and (rhs < 1 << 32).all()     # neither side wraps: the transcription's masks change nothing
        assert np.array_equal(ok, lhs <= rhs)
        pairs, rejected, top = pairs + i.size, rejected + int((~ok).sum()), max(top, int(rhs.max()))
    return pairs, rejected, top


def test_jaccard_gate_never_rejects_a_pair_below_the_threshold():
    """DESIGN.md 3.25, all 8 394 752 pairs of counts 0 <= i <= u, 1 <= u <= 4096, and the empty union (u = 0: distance 0, the threshold
    the smallest denormal, gt = 1) against the tightest threshold a float32 can be"""
    pairs, rejected, top = _jaccard_gate_sweep(range(0, 4097))
    assert pairs == 8_394_752 + 1 and rejected == 0
    assert top == 1_073_745_920 < 1 << 32


def test_jaccard_gate_scalar_form_and_sentinels():
    assert bb.gate_jac(-np.inf) == 0 and bb.gate_jac(np.inf) == 1 << 19 and bb.gate_jac(2.0) == 1 << 19 and bb.gate_jac(1.0) == 1 << 18
    for thr in (1.0e-45, 0.5, 0.33333334, 1.0):
        assert bb.gate_jac(thr) == int(bb.gate_jac_many(np.float32(thr)))
    # the open gate passes every pair a row can form; the query that matches nothing (|q| = 4096, gt = 0) passes none but the pair of
    # all 4096 bits on both sides, which the exact test then rejects (vg_batch_bitsl_within.hip)
    i, x = np.meshgrid(np.arange(0, 4097, 7), np.arange(0, 4097, 7))
    keep = i <= x
    assert not bb.passes_jac(i[keep], 4096, 0, x[keep]).any()
    assert bb.passes_jac(4096, 4096, 0, 4096)
    for qc in (0, 1, 200, 4096):
        ii, xx = i[keep & (i <= qc)], x[keep & (i <= qc)]
        assert bb.passes_jac(ii, qc, 1 << 19, xx).all()


def test_jaccard_tight_triples_pass_with_their_slack():
    for dim in (16, 100, 128, 200, 512):
        w = bb.LADDER_WEIGHT[dim]
        tight = bb.jaccard_tight(8 * dim, w)
        assert len(tight) == 64
        lad = bb.ladder("jaccard", dim, "random")
        have = set(zip(lad.common.tolist(), lad.extra.tolist()))
        for i, u, i2, u2, slack in tight:
            d, thr = bb.jaccard_f32(i, u), bb.jaccard_f32(i2, u2)
            assert d < thr and slack == bb.gate_jac(thr) * u - ((u - i) << 18) and slack >= 0
            assert bb.passes_jac(i, w, bb.gate_jac(thr), u + i - w)
            assert (i, u - w) in have and (i2, u2 - w) in have      # both planted: the row and the one whose distance is its threshold
        assert tight[0][4] <= tight[-1][4] < 1 << 18


def test_hamming_gate_passes_exactly_the_pairs_below_the_threshold():
    """the gate passes iff d < thr, for thr in d, d + 0.5, d + 1 - over a SAMPLE of the counts |q|, |x|, i <= 4096: every 61st value, all
    of 0 .. 69 and all of 4030 .. 4096 (about 200 values each, every combination of them a row can form), not the full range"""
    counts = np.unique(np.r_[np.arange(0, 4097, 61), np.arange(0, 70), np.arange(4030, 4097)])
    for qc in counts:
        x, i = np.meshgrid(counts, counts, indexing="ij")
        keep = (i <= x) & (i <= qc) & (qc + x - i <= 4096)
        x, i = x[keep], i[keep]
        d = qc + x - 2 * i
        for add, want in ((0.0, False), (0.5, True), (1.0, True)):
            ng = np.ceil((d + add).astype(np.float32)).astype(np.int64) - 1 - qc
            assert (bb.passes_ham(i, ng, x) == want).all(), (qc, add)
    assert bb.gate_ham(7, 12.5) == 13 - 1 - 7 and bb.gate_ham(7, 12.0) == 12 - 1 - 7
    assert bb.gate_ham(7, -np.inf) == -(1 << 30) and bb.gate_ham(7, np.inf) == 1 << 30 and bb.gate_ham(7, 3.0e38) == 1 << 30
    assert not bb.passes_ham(4096, -(1 << 30), 0) and bb.passes_ham(0, 1 << 30, 4096)


# ---------------------------------------------------------------------------------------------------- the ladders

@pytest.mark.parametrize("dim,dense", [(16, False), (100, False), (128, False), (200, False), (512, False),
                                       (16, True), (100, True), (128, True), (272, True)])
@pytest.mark.parametrize("name", NAMES)
def test_ladders(name, dim, dense):
    w, nbits = bb.LADDER_WEIGHT[dim], 8 * dim
    for ordering in ("random", "descending", "ascending"):
        lad = bb.ladder(name, dim, ordering, dense)
        n, copies = len(lad.rows), int(lad.copy.max()) + 1
        per = n // copies
        assert n <= 70_000 and int(np.unpackbits(lad.q).sum()) == w and copies == (2 if not dense else max(copies, 3))
        if dense:                                               # four tiles or more per partition, under a mask without copy 0 too
            assert (lad.copy != 0).sum() // bb.TILE >= bb.DENSE_TILES == 4 * 256
        d = bb.ladder_distances(name, dim, lad)
        if ordering == "random":                                # the rows are what their classes say
            assert np.array_equal(bb.batch_distances(name, lad.rows, lad.q[None, :])[0].view(np.uint32), d.view(np.uint32))
            assert set(range(w + 1)) == set(lad.common.tolist()) and {0, 1, nbits - w} <= set(lad.extra.tolist())
            cls = lad.common * 10_000 + lad.extra
            for c in range(copies):                             # every class once per copy
                assert len(np.unique(cls[lad.copy == c])) == per == int((lad.copy == c).sum())
            first, second = (np.flatnonzero(lad.copy == c)[np.argsort(cls[lad.copy == c])] for c in (0, 1))
            assert np.median(np.abs(first - second)) > n // 8   # ... and the copies of a class far apart
        else:
            sign = -1 if ordering == "descending" else 1
            for c in range(copies):                             # a run per copy
                run = slice(c * per, (c + 1) * per)
                assert (lad.copy[run] == c).all() and (sign * np.diff(d[run]) >= 0).all()
                assert d[run][0 if sign > 0 else -1] == 0 and d[run][-1 if sign > 0 else 0] == d.max()


# ---------------------------------------------------------------------------------------------------- the lifecycle script

def test_lifecycle_script_shape():
    qs, states = bb.lifecycle(100)
    assert [s.op for s in states] == ["create", "patch", "delete", "clear_append", "append", "trim", "reserve", "clone", "patch"]
    assert [len(s.ids) for s in states] == [3001, 3001, 2989, 1503, 3503, 3503, 3503, 3503, 3503]
    assert 2989 % 32 == 13 and 1503 % 32 == 31 and 1503 + 2000 > bb.CAPACITY > 3001
    assert [s.dropped for s in states] == [True, False, True, True, True, False, False, False, False]
    for s in states:
        assert len(s.rows) == len(s.ids) == len(s.allowed) == len(s.labels) and len(np.unique(s.ids)) == len(s.ids)
    deleted = states[1].rows[2989:]
    assert sum(bool((deleted == q[None, :]).all(1).any()) for q in qs) >= 5        # rows equal to queries leave with the block
    assert (states[2].rows[1503] == qs[9]).all() and not (states[3].rows == qs[9][None, :]).all(1).any()


@pytest.mark.parametrize("dim", [100, 128, 200, 272, 512])
@pytest.mark.parametrize("name", NAMES)
def test_every_lifecycle_step_discriminates(name, dim):
    """the device-free stand-in for mutation testing: per step that changes rows, mask or labels, and per form, the answer of a
    handle that missed (part of) the call differs from the true one for at least one query"""
    qs, states = bb.lifecycle(dim)
    kinds = {100: ("plain", "labeled"), 128: ("masked", "within", "within_masked"), 200: ("plain",), 272: ("masked",), 512: ("within",)}[dim]

    def ask(kind, rows, ids, allowed, labels, radii):
        return [tuple(np.asarray(a).tolist() for a in ans[:2]) for ans in bb.answers(name, kind, qs, rows, ids, allowed, labels, radii)]

    for j in range(1, len(states)):
        s = states[j]
        if s.op in ("trim", "reserve", "clone"):                # no row, mask bit or label changes: the state in front again
            assert s.rows is not states[j - 1].rows and np.array_equal(s.rows, states[j - 1].rows) and s.allowed is states[j - 1].allowed
            continue
        stale = bb.stale_states(states, j)
        assert set(stale) == {"before"} | ({"behind"} if s.op in ("delete", "clear_append") else set()) | ({"kept"} if s.dropped else set())
        for kind in kinds:
            d = bb.batch_distances(name, s.rows, qs)
            radii = bb.lifecycle_radii(d, s.allowed if kind == "within_masked" else None)
            true = ask(kind, s.rows, s.ids, s.allowed, s.labels, radii)
            for what, (rows, ids, allowed, labels) in stale.items():
                if what == "kept" and kind in ("plain", "within"):
                    continue                                    # (forms that read neither mask nor labels)
                assert ask(kind, rows, ids, allowed, labels, radii) != true, (name, dim, j, s.op, kind, what)
