"""The case builder of the lifecycle tests (tests/lifecycle_cases.py) without a device: every script's bookkeeping is replayed
independently (a dict keyed by rowid), the shapes the scripts promise are there (rows mod 32 reaches 0, 1 and 31, more than two
whole tiles leave from the end with NaN / Inf / huge rows planted in them, the int8 batch filter's corpora stay at or above its
floor), and for every state a batch is compared in, the float64 reference alone decides at least nine queries in ten by set
equality (batch_reference.BAND_SHARE_CAP)."""
import numpy as np
import pytest

import batch_reference as br
import datagen as dg
import lifecycle_cases as lc

BATCH = [p.name for p in lc.PATHS if p.kind == "batch"]
ALL = [p.name for p in lc.PATHS]


def _replay(w_rows, w_ids, steps):
    """the same operations on a list of (rowid, row bytes): what survives after every step"""
    cur = [(int(i), r.tobytes()) for i, r in zip(w_ids, w_rows)]
    out = []
    for s in steps:
        if s.op == "patch":
            for pos, new in zip(s.args[0], s.args[1]):
                cur[int(pos)] = (cur[int(pos)][0], new.tobytes())
        elif s.op == "delete":
            gone = set(int(x) for x in s.args[0])
            assert len(gone) == len(s.args[0]) and (np.diff(s.args[0]) > 0).all()
            cur = [e for i, e in enumerate(cur) if i not in gone]
        elif s.op == "append":
            cur += [(int(i), r.tobytes()) for i, r in zip(s.args[1], s.args[0])]
        out.append(list(cur))
    return out


@pytest.mark.parametrize("name", ALL)
def test_edit_script_bookkeeping(name):
    p, w, steps = lc.PATH_BY_NAME[name], lc.world(name), lc.edit_script(name)
    assert [s.op for s in steps] == ["patch", "patch", "delete", "delete", "delete", "append"]
    for s, want in zip(steps, _replay(w.rows, w.ids, steps)):
        if s.rows is None:
            continue
        assert s.ids.tolist() == [i for i, _ in want] and (np.diff(s.ids) > 0).all()
        assert all(r.tobytes() == b for r, (_, b) in zip(s.rows, want))
        for g in s.dups:
            assert len(g) > 1 and all(s.rows[j].tobytes() == w.qs[0].tobytes() for j in g)
        assert p.proof != 7 or len(s.ids) >= lc.Q8_FLOOR
    pos, new = steps[0].args
    assert len(pos) == len(set(pos.tolist())) == 300 and 0 in pos and p.n - 1 in pos and len(steps[0].dups[0]) == 5
    plant, first_delete = steps[1], steps[2]
    assert plant.warm and plant.rows is None and plant.args[0].tolist() == list(range(p.n - 70, p.n))
    if p.vt in lc.FLOATS:
        x = dg.storage_to_f64(p.vt, plant.args[1])
        with np.errstate(over="ignore"):
            assert (~np.isfinite(x).all(axis=1) | ((x * x).sum(axis=1) > 1e9 * p.dim)).all()
    from_end = int((first_delete.args[0] >= p.n - 96).sum())
    assert from_end > 64 and first_delete.args[0][-1] == p.n - 1 and set(range(7)) <= set(first_delete.args[0].tolist())
    assert set(range(p.n - 70, p.n)) <= set(first_delete.args[0].tolist())        # every planted row leaves - and stays behind the new end
    assert [len(s.ids) % 32 for s in steps[2:5]] == [0, 1, 31]
    assert all(len(s.args[0]) >= 210 for s in steps[2:5])
    assert len(steps[5].args[1]) == 100 and steps[5].ids[-100:].tolist() == steps[5].args[1].tolist()


@pytest.mark.parametrize("name", ALL)
def test_clear_script_bookkeeping(name):
    p, steps = lc.PATH_BY_NAME[name], lc.clear_script(name)
    n1, n2 = lc.clear_sizes(p)
    assert [s.op for s in steps] == ["create", "clear_append"] and steps[0].warm
    (first, first_ids), second = steps[0].args, steps[1]
    assert len(first) == len(first_ids) == n1
    if p.vt in lc.FLOATS:
        x = dg.storage_to_f64(p.vt, first[n2:n2 + 70])
        assert (~np.isfinite(x).all(axis=1) | ((x * x).sum(axis=1) > 1e9 * p.dim)).all()
    assert n2 < n1 and n2 % 32 != 0 and 0.45 < n2 / n1 < 0.55 and (p.proof != 7 or n2 >= lc.Q8_FLOOR)
    assert len(second.ids) == n2 == len(second.rows) and (np.diff(second.ids) > 0).all() and (np.diff(second.ids) > 1).all()
    assert second.rows.tobytes() != lc.world(name).rows[:n2].tobytes()


@pytest.mark.parametrize("name", BATCH)
def test_the_reference_alone_decides_nine_queries_in_ten(orc, name):
    """every compared state of both scripts, the 40-query batch at k = 20 and the ragged one (7 queries, k = 1); the new best row of
    query 1 an append / a re-append brings IS its best row"""
    p, w = lc.PATH_BY_NAME[name], lc.world(name)
    for script in (lc.edit_script(name), lc.clear_script(name)):
        for s in script:
            if s.rows is None:
                continue
            ref = br.batch_references(p.vt, (p.metric,), w.qs, s.rows, orc, kmax=lc.K, duplicates=s.dups)[p.metric]
            assert ref.band_share(lc.K) <= br.BAND_SHARE_CAP, (name, s.op, ref.band_share(lc.K))
            assert ref.band_share(1, nq=7) <= br.BAND_SHARE_CAP, (name, s.op, ref.band_share(1, nq=7))
            if s.op == "append":
                assert s.ids[ref.pos[1, 0]] == 10**7 + 37, (name, ref.pos[1, :3])
            if s.op == "clear_append":
                assert ref.pos[1, 0] == len(s.ids) - 1, (name, ref.pos[1, :3])
            if s.dups:
                assert sorted(ref.pos[0, :len(s.dups[0])].tolist()) == sorted(s.dups[0]), name
