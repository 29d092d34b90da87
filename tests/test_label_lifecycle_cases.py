"""The case builder of the label lifecycle tests (tests/label_lifecycle_cases.py) without a device.

  * bookkeeping: every script is replayed independently on a list of (rowid, row bytes, label, allowed) and the shapes the scripts
    promise are there (rows mod 64 reaches 0, 1 and 63, more than two whole 64-row blocks leave from the end, the clear scripts'
    sizes force / avoid the label and bitmap reallocations, stale labels and mask bits lie right behind the smaller content's end);
  * every float case is DECIDED by float64 alone - a condition, the share of undecided cases allowed is zero: the contract's answer
    lies wholly in the query's ladder, and every two neighbours among the eligible rows up to 8 behind the answer's last row differ by
    more than 2 * batch_reference.completeness_tol (an evaluation within tol of float64 then orders all of them the same way, so it
    keeps the same rows in the same order);
  * the float64 contract of label_lifecycle_cases.answer is labeled_cases / grouped_cases / capped_cases.expected, which cast to float32;
  * the tests can see: with the previous state's labels or mask at the new length (= labels shifted by the deletion), and for the
    patch - which keeps labels - with the previous rows, every family's answers differ from the right ones; one stale label or bitmap
    bit behind the smaller content's end changes the labeled answer's count."""
import numpy as np
import pytest

import batch_reference as br
import capped_cases as cc
import datagen as dg
import grouped_cases as gc
import label_lifecycle_cases as ll
import labeled_cases as lab

ALL = [p.name for p in ll.PATHS]
FLOAT = [p.name for p in ll.PATHS if ll.is_float(p)]


def _replay(w, steps):
    cur = [(int(i), r.tobytes(), int(l), bool(a)) for i, r, l, a in zip(w.ids, w.rows, w.labels, w.allowed)]
    out = []
    for s in steps:
        if s.op == "patch":
            for pos, new in zip(s.args[0], s.args[1]):
                e = cur[int(pos)]
                cur[int(pos)] = (e[0], new.tobytes(), e[2], e[3])                 # labels and mask stay with the position
        elif s.op == "delete":
            gone = set(int(x) for x in s.args[0])
            assert len(gone) == len(s.args[0]) and (np.diff(s.args[0]) > 0).all()
            cur = [e for i, e in enumerate(cur) if i not in gone]
        elif s.op == "append":
            n_new = len(s.args[1])
            cur += [(int(i), r.tobytes(), int(l), bool(a)) for i, r, l, a in zip(s.args[1], s.args[0], s.labels[-n_new:], s.allowed[-n_new:])]
        out.append(list(cur))
    return out


@pytest.mark.parametrize("name", ALL)
def test_edit_script_bookkeeping(name):
    p, w, steps = ll.PATH_BY_NAME[name], ll.world(name), ll.edit_script(name)
    assert [s.op for s in steps] == ["patch", "delete", "delete", "delete", "append"]
    assert [s.dropped for s in steps] == [False, True, True, True, True]
    assert (np.diff(w.ids) > 1).all() and len(w.ids) == ll.N
    for s, want in zip(steps, _replay(w, steps)):
        assert s.ids.tolist() == [e[0] for e in want] and (np.diff(s.ids) > 0).all()
        assert all(r.tobytes() == e[1] for r, e in zip(s.rows, want))
        assert s.labels.tolist() == [e[2] for e in want] and s.allowed.tolist() == [e[3] for e in want]
        assert len(s.prev_labels) == len(s.prev_allowed) == len(s.ids) and s.labels.dtype == np.uint32
    pos = steps[0].args[0]
    assert len(pos) == len(set(pos.tolist())) == 300
    assert np.array_equal(steps[0].labels, w.labels) and np.array_equal(steps[0].allowed, w.allowed)
    first = steps[1].args[0]
    assert int((first >= ll.N - 128).sum()) >= 128 and first[-1] == ll.N - 1 and set(range(7)) <= set(first.tolist())
    assert [len(s.ids) % 64 for s in steps[1:4]] == [0, 1, 63]
    assert all(len(s.args[0]) >= 210 for s in steps[1:4])
    assert len(steps[4].args[1]) == 100 and steps[4].ids[-100:].tolist() == steps[4].args[1].tolist()
    if ll.is_float(p):
        x = dg.storage_to_f64(p.vt, steps[0].rows[np.searchsorted(w.ids, w.ladder[0][[10, 11]])])
        assert np.isnan(x[0]).any() and np.isinf(x[1]).any()
        assert (steps[0].labels == ll.L_SPECIAL).sum() == 2                        # nobody else carries that label


@pytest.mark.parametrize("name", FLOAT)
def test_ladders_are_where_they_should_be(name):
    p = ll.PATH_BY_NAME[name]
    for w in (ll.world(name), ll.world(name, small=True)):
        n = len(w.ids)
        at = [np.searchsorted(w.ids, l) for l in w.ladder]
        every = np.concatenate(at)
        assert len(set(every.tolist())) == len(every) == 5 * ll.R_BIG + 4 * ll.R_SMALL
        assert 0 in at[0][:6] and n - 1 in at[0][:6]
        for b in range(1, (n - 2) // 64 + 1):                                    # both sides of every block boundary of the 3-shard map
            assert 64 * b - 1 in every and 64 * b in every, b
        for i in range(ll.NQ):
            assert at[i][8] > at[i][12]                                          # the better row of L_V comes later in scan order
            assert w.labels[at[i][:6]].tolist() == [ll.L_U + i] * 6 and (w.labels == ll.L_U + i).sum() == 7
            assert w.labels[at[i][[6, 9]]].tolist() == [ll.NONE] * 2
            assert not w.allowed[w.labels == ll.L_MASKED].any() and w.labels[at[i][7]] == ll.L_MASKED
        D = ll.distances(p, None, w.rows)                                         # (no special rows: the oracle is not asked)
        for i in range(ll.NQ):
            d = D[i, at[i]]
            assert (np.diff(d) > 0).all() and d[0] > 0
            rest = np.delete(D[i], at[i])
            assert rest.min() > 1.5 * d[-1], (i, rest.min(), d[-1])               # far below every other row


@pytest.mark.parametrize("name", ALL)
def test_clear_scripts_bookkeeping(name):
    first, step = ll.clear_smaller_script(name)
    n1, n2 = len(first.ids), len(step.ids)
    assert (n1, n2) == (ll.N, ll.N_HALF) and n2 % 64 not in (0,) and 0.45 < n2 / n1 < 0.55
    assert (first.labels[n2:n2 + 70] == ll.ask_labels(name, 0)[0]).all() and first.allowed[n2:n2 + 70].all()
    assert step.rows.tobytes() != first.rows[:n2].tobytes() and (np.diff(step.ids) > 1).all()
    assert (n2 + 63) // 64 < (n1 + 63) // 64 and n2 <= max(n1, 1024)            # both buffers are reused
    first, step = ll.clear_larger_script(name)
    n1, n2 = len(first.ids), len(step.ids)
    assert n2 > max(n1, 1024) and (n2 + 63) // 64 > (n1 + 63) // 64               # both are allocated again


def test_the_patch_plants_a_row_at_minus_inf_under_dot(orc):
    """f32 x 384: the patch's +Inf element sits in the last lane, where the even queries are positive and the odd ones negative - under
    DOT the row (label L_SPECIAL, allowed) is at -Inf for queries 0, 2, 4 and at +Inf for 1, 3; it outlives the first deletion"""
    name = "f32_384_l2"
    p, w, steps = ll.PATH_BY_NAME[name], ll.world(name), ll.edit_script(name)
    rowid = int(w.ladder[0][11])
    for s in steps[:2]:
        at = int(np.searchsorted(s.ids, rowid))
        assert s.ids[at] == rowid and s.labels[at] == ll.L_SPECIAL and s.allowed[at]
        assert np.isinf(s.rows[at, p.dim - 1]) and np.isfinite(s.rows[at, :p.dim - 1]).all()
        D = ll.distances(p, orc, s.rows, metric=dg.DOT)
        assert D[[0, 2, 4], at].tolist() == [-np.inf] * 3 and D[[1, 3], at].tolist() == [np.inf] * 2
        assert np.isfinite(np.delete(D[:5], [at, int(np.searchsorted(s.ids, int(w.ladder[0][10])))], axis=1)).all()


def _d32(D):
    return D.astype(np.float32)


@pytest.mark.parametrize("name", ALL)
def test_the_float64_contract_is_the_float32_one(orc, name):
    p = ll.PATH_BY_NAME[name]
    for what, s in ll.compared_states(name):
        D = ll.distances(p, orc, s.rows)
        for call in ll.plan(name):
            kind, masked, k, m, i, label = call
            pos = ll.expect(call, D, s.labels, s.allowed)
            al = s.allowed if masked else None
            if kind in ("labeled", "batch_labeled"):
                ids = lab.expected(_d32(D[i]), s.labels == label, k, rowids=s.ids)[0]
            elif kind == "grouped":
                ids = gc.expected(_d32(D[i]), s.labels, al, k, rowids=s.ids)[0]
            else:
                ids = cc.expected(_d32(D[i]), s.labels, al, k, m, rowids=s.ids)[0]
            assert s.ids[pos].tolist() == ids.tolist(), (what, call)


@pytest.mark.parametrize("name", FLOAT)
def test_every_float_case_is_decided(orc, name):
    p = ll.PATH_BY_NAME[name]
    qs = ll.queries(name)
    q_l1 = np.abs(dg.storage_to_f64(p.vt, qs)).sum(axis=1)
    for what, s in ll.compared_states(name):
        D = ll.distances(p, orc, s.rows)
        on_ladder = [(s.rows == qs[i][None, :]).sum(axis=1) >= p.dim - 1 for i in range(ll.NQ)]
        full = 0
        for call in ll.plan(name):
            kind, masked, k, m, i, label = call
            pos = ll.expect(call, D, s.labels, s.allowed)
            if not len(pos):
                assert label == ll.ABSENT, (what, call)
                continue
            full += len(pos) == k
            assert on_ladder[i][pos].all(), (what, call, "the answer leaves the ladder")
            order = ll.eligible("labeled" if kind == "batch_labeled" else kind, D[i], s.labels, s.allowed if masked else None, label)
            last = int(np.nonzero(order == pos[-1])[0][0])
            d = D[i, order[:last + 1 + ll.NEAR]]
            tol = br.completeness_tol(p.metric, q_l1[i], d.max())
            assert (np.diff(d) > 2 * tol).all(), (what, call, np.diff(d).min(), tol)
        assert full >= 40, (what, full)                                           # (most grouped / capped lists are full ones)


def _differs(name, fam, right, wrong):
    return any(r.tolist() != w.tolist() for c, r, w in zip(ll.plan(name), right, wrong) if ll.family(c) == fam)


@pytest.mark.parametrize("name", ALL)
def test_the_tests_can_see(orc, name):
    p = ll.PATH_BY_NAME[name]
    plan = ll.plan(name)
    prev_rows = ll.world(name).rows
    for what, s in ll.compared_states(name):
        D = ll.distances(p, orc, s.rows)
        right = [s.ids[ll.expect(c, D, s.labels, s.allowed)] for c in plan]
        if s.op == "patch":                                                      # labels and mask stay: the previous ROWS are the stale state
            D0 = ll.distances(p, orc, prev_rows)
            stale = [s.ids[ll.expect(c, D0, s.labels, s.allowed)] for c in plan]
            for fam in ll.FAMILIES:
                assert _differs(name, fam, right, stale), (what, fam, "the previous rows")
            continue
        stale = [s.ids[ll.expect(c, D, s.prev_labels, s.allowed)] for c in plan]
        for fam in ll.FAMILIES:
            assert _differs(name, fam, right, stale), (what, fam, "the previous labels")
        stale = [s.ids[ll.expect(c, D, s.labels, s.prev_allowed)] for c in plan]
        for fam in ("grouped_masked", "capped_masked"):
            assert _differs(name, fam, right, stale), (what, fam, "the previous mask")


@pytest.mark.parametrize("name", ALL)
def test_one_stale_label_or_bit_behind_the_smaller_content_shows(orc, name):
    """clear_smaller on the numpy model: the second content read one row too far - the first content's row, label and mask bit at
    position n2 - changes the count of query 0's labeled answer"""
    p = ll.PATH_BY_NAME[name]
    first, s = ll.clear_smaller_script(name)
    n2 = len(s.ids)
    label = ll.ask_labels(name, 0)[0]
    rows = np.concatenate([s.rows, first.rows[n2:n2 + 1]])
    labels, allowed = np.append(s.labels, first.labels[n2]), np.append(s.allowed, first.allowed[n2])
    D, D1 = ll.distances(p, orc, s.rows), ll.distances(p, orc, rows)
    assert labels[n2] == label and allowed[n2] and np.isfinite(D1[0, n2])
    for k in (20, 64):
        right = ll.answer("labeled", D[0], s.labels, None, k, label=label)
        wrong = ll.answer("labeled", D1[0], labels, None, k, label=label)
        assert len(right) < k and len(wrong) == len(right) + 1 and n2 in wrong, (k, len(right), len(wrong))
