"""The values of a handle across its lifecycle (include/vectorgpu.h: the labels' rules): patch_rows, reserve, trim and clone keep them;
append, delete_rows and clear drop them - has_values() is False and every valued scan is VG_ERR_INVALID; set_values with the wrong
count is refused; three logical shards answer like one corpus for every valued form, also where an interval's rows sit on one shard.

`ask` runs every valued form on one handle; a handle is right when it answers bit for bit like a handle freshly staged from the same
rows, rowids, values and labels, and - uint8, whose distances are exact - like the contract over the handle's own distances."""
import numpy as np
import pytest

import datagen as dg
import labeled_cases as lc
import valued_cases as vc

pytestmark = pytest.mark.gpu

VG_ERR_INVALID = 1
N, NQ = lc.N, 5
SHAPES = [(dg.U8, 64, dg.L2), (dg.F32, 384, dg.L2), (dg.F16, 384, dg.COSINE)]
IDS = ["u8-64", "f32-384", "f16-384"]
RADIUS = {dg.L2: 1e30, dg.COSINE: 1.0}          # the range form's radius: every finite row / about half of them


@pytest.fixture(scope="module")
def pkg():
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    import __graft_entry__ as g
    p = g.load_package()
    if p.device_count() < 1:
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    return p


def _state(vt, dim, n=N, seed=0):
    rows = lc.data(vt, n, dim, 91 + dim + seed)
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    values = (np.arange(n, dtype=np.int64) // 5) * 7 - 2000 + seed               # ascending with repeats, across zero
    labels = np.random.default_rng(92 + seed).integers(0, 40, n).astype(np.uint32)
    return rows, ids, values, labels


def _intervals(values):
    u = np.unique(values)
    return [(None, None), (int(u[len(u) // 3]), int(u[(2 * len(u)) // 3])), (int(u[-1]), None), (-10, 10), (1, 0), (int(u[0]), int(u[1]))]


def _stage(pkg, vt, dim, state, shards=False):
    rows, ids, values, labels = state
    h = pkg.Shards(vt, dim, [0, 0, 0], block_rows=64) if shards else pkg.Corpus(vt, dim)
    third = len(rows) // 3
    h.append(rows[:third], ids[:third])
    h.append(rows[third:], ids[third:])
    h.set_values(values)
    h.set_labels(labels)
    assert h.has_values()
    return h


def _ask(h, metric, qs, values):
    """{(form, interval, query): the answer as a tuple of lists}"""
    out = {}
    ivs = _intervals(values)
    radius = RADIUS[metric]
    for j, (lo, hi) in enumerate(ivs):
        for i in range(NQ):
            q = qs[i]
            ids, d = h.scan_topk_valued(metric, q, 20, lo, hi)
            out[("valued", j, i)] = (ids.tolist(), d.astype(np.float32).view(np.uint32).tolist())
            ids, d = h.scan_topk_valued(metric, q, 64, lo, hi, label=3)
            out[("valued_labeled", j, i)] = (ids.tolist(), d.astype(np.float32).view(np.uint32).tolist())
            for form, res in (("grouped", h.scan_topk_grouped_valued(metric, q, 20, lo, hi)), ("capped", h.scan_topk_capped_valued(metric, q, 20, 2, lo, hi))):
                out[(form, j, i)] = (res[0].tolist(), res[1].astype(np.float32).view(np.uint32).tolist(), res[2].tolist())
        ids, d, m = h.scan_within_valued(metric, qs[0], radius, lo, hi, limit=50)
        out[("within", j, 0)] = (ids.tolist(), d.astype(np.float32).view(np.uint32).tolist(), m)
    los, his = [iv[0] for iv in ivs][:NQ], [iv[1] for iv in ivs][:NQ]
    for name, lab in (("batch", None), ("batch_labeled", np.array([3, 5, 3, 0, 39], dtype=np.uint32))):
        ids, d, cnt = h.scan_topk_batch_valued(metric, qs, los, his, 20, labels=lab)
        for i in range(NQ):
            out[(name, i, i)] = (ids[i, :cnt[i]].tolist(), d[i, :cnt[i]].astype(np.float32).view(np.uint32).tolist())
    return out


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        assert a[key] == b[key], (what, key)


def _fresh_equal(pkg, vt, dim, metric, qs, h, state, what):
    fresh = _stage(pkg, vt, dim, state)
    got = _ask(h, metric, qs, state[2])
    _same(got, _ask(fresh, metric, qs, state[2]), what)
    fresh.close()
    return got


def _valued_calls(h, metric, qs):
    q = qs[0]
    return [lambda: h.scan_topk_valued(metric, q, 20, None, None), lambda: h.scan_topk_valued(metric, q, 20, None, None, label=3),
            lambda: h.scan_topk_grouped_valued(metric, q, 20, None, None), lambda: h.scan_topk_capped_valued(metric, q, 20, 2, None, None),
            lambda: h.scan_within_valued(metric, q, 1e30, None, None), lambda: h.scan_topk_batch_valued(metric, qs, None, None, 20)]


def _dropped(pkg, h, metric, qs, what, labels_too=True):
    assert not h.has_values(), what
    for j, call in enumerate(_valued_calls(h, metric, qs)):
        assert lc.error_code(pkg, call) == VG_ERR_INVALID, (what, j)
    assert h.has_labels() != labels_too, what


@pytest.mark.parametrize("vt,dim,metric", SHAPES, ids=IDS)
def test_patch_reserve_trim_keep_the_values(pkg, vt, dim, metric):
    state = _state(vt, dim)
    rows, ids, values, labels = state
    qs = lc.data(vt, NQ, dim, 93 + dim)
    h = pkg.Corpus(vt, dim, capacity=4 * N)
    h.append(rows, ids)
    h.set_values(values)
    h.set_labels(labels)
    before = _fresh_equal(pkg, vt, dim, metric, qs, h, state, "start")
    if vt == dg.U8:                                              # exact distances: the contract over the handle's own floats
        own = h.scan_distances(metric, qs[1])
        for j, (lo, hi) in enumerate(_intervals(values)):
            want = lc.expected(own, vc.allowed(values, lo, hi), 20, rowids=ids)
            assert before[("valued", j, 1)] == (want[0].tolist(), want[1].view(np.uint32).tolist()), j
    h.trim()
    assert h.has_values()
    _same(_ask(h, metric, qs, values), before, "after trim")
    h.reserve(4 * N)
    assert h.has_values()
    _same(_ask(h, metric, qs, values), before, "after reserve")
    pos = np.array([0, 63, 64, 1500, N - 1], dtype=np.int64)     # patched rows keep their values: the answer follows the new rows
    new_rows = rows.copy()
    new_rows[pos] = lc.data(vt, len(pos), dim, 94 + dim)
    h.patch_rows(pos, new_rows[pos])
    assert h.has_values() and h.has_labels()
    _fresh_equal(pkg, vt, dim, metric, qs, h, (new_rows, ids, values, labels), "after patch_rows")
    # a refused set_values: the count is checked before anything is touched, so the values the handle holds stay
    assert lc.error_code(pkg, lambda: h.set_values(values[:-1])) == VG_ERR_INVALID
    assert lc.error_code(pkg, lambda: h.set_values(np.concatenate([values, values[:1]]))) == VG_ERR_INVALID
    assert h.has_values()
    h.close()


@pytest.mark.parametrize("vt,dim,metric", SHAPES, ids=IDS)
def test_append_delete_clear_drop_the_values(pkg, vt, dim, metric):
    state = _state(vt, dim)
    rows, ids, values, labels = state
    qs = lc.data(vt, NQ, dim, 93 + dim)
    h = _stage(pkg, vt, dim, state)
    gone = np.array([5, 64, 2000], dtype=np.int64)
    h.delete_rows(gone)
    _dropped(pkg, h, metric, qs, "after delete_rows")
    keep = np.setdiff1d(np.arange(N), gone)
    assert lc.error_code(pkg, lambda: h.set_values(values)) == VG_ERR_INVALID          # the old length is refused
    st = (rows[keep], ids[keep], values[keep], labels[keep])
    h.set_values(st[2])
    h.set_labels(st[3])
    _fresh_equal(pkg, vt, dim, metric, qs, h, st, "values set again after delete_rows")
    more = lc.data(vt, 10, dim, 95 + dim)
    h.append(more, np.arange(10, dtype=np.int64) + 10**7)
    _dropped(pkg, h, metric, qs, "after append")
    h.set_values(np.concatenate([st[2], np.full(10, 5, dtype=np.int64)]))
    assert h.has_values() and not h.has_labels()                  # values and labels are set apart
    ids5, _ = h.scan_topk_valued(metric, qs[0], 64, 5, 5)
    assert set(ids5.tolist()) <= set((np.arange(10) + 10**7).tolist()) | set(st[1][st[2] == 5].tolist())
    h.clear()
    assert h.rows == 0
    _dropped(pkg, h, metric, qs, "after clear")
    small = _state(vt, dim, n=1000, seed=1)                      # a smaller re-append lives in the first content's value array
    h.append(small[0], small[1])
    _dropped(pkg, h, metric, qs, "after clear + append")
    h.set_values(small[2])
    h.set_labels(small[3])
    _fresh_equal(pkg, vt, dim, metric, qs, h, small, "clear + smaller append")
    h.close()


@pytest.mark.parametrize("vt,dim,metric", SHAPES, ids=IDS)
def test_clones_carry_the_values_and_are_independent(pkg, vt, dim, metric):
    state = _state(vt, dim)
    rows, ids, values, labels = state
    qs = lc.data(vt, NQ, dim, 93 + dim)
    src = _stage(pkg, vt, dim, state)
    before = _ask(src, metric, qs, values)
    cl = src.clone()
    assert cl.has_values() and cl.has_labels()
    _same(_ask(cl, metric, qs, values), before, "clone")
    other = -values                                              # the clone gets other values: the source does not move
    cl.set_values(other)
    _same(_ask(src, metric, qs, values), before, "source after its clone's values changed")
    _fresh_equal(pkg, vt, dim, metric, qs, cl, (rows, ids, other, labels), "clone with its own values")
    src.clear_values()
    assert not src.has_values() and cl.has_values()
    cl.delete_rows(np.array([1], dtype=np.int64))
    assert not cl.has_values()
    src.set_values(values)
    _same(_ask(src, metric, qs, values), before, "source after its clone was edited")
    src.close()
    cl.close()


@pytest.mark.parametrize("vt,dim,metric", SHAPES, ids=IDS)
def test_three_logical_shards_equal_one_corpus(pkg, vt, dim, metric):
    state = _state(vt, dim)
    rows, ids, values, labels = state
    qs = lc.data(vt, NQ, dim, 93 + dim)
    one = _stage(pkg, vt, dim, state)
    sh = pkg.Shards(vt, dim, [0, 0, 0], block_rows=64)
    for r0 in range(0, N, 1000):
        sh.append(rows[r0:r0 + 1000], ids[r0:r0 + 1000])
    assert not sh.has_values()
    for j, call in enumerate(_valued_calls(sh, metric, qs)):
        assert lc.error_code(pkg, call) == VG_ERR_INVALID, j      # no values
    assert lc.error_code(pkg, lambda: sh.set_values(values[:-1])) == VG_ERR_INVALID
    sh.set_values(values)
    sh.set_labels(labels)
    assert sh.has_values()
    want = _ask(one, metric, qs, values)
    got = _ask(sh, metric, qs, values)
    _same(got, want, "three shards")
    # an interval whose rows sit on one shard only: 60 rows of the first block of 64
    lo, hi = int(values[0]), int(values[59])
    assert hi < int(values[60])
    for i in range(NQ):
        a, b = one.scan_topk_valued(metric, qs[i], 64, lo, hi), sh.scan_topk_valued(metric, qs[i], 64, lo, hi)
        lc.assert_same(b, *a, ctx=("one shard's rows", i))
        assert len(a[0]) == 60 or vt != dg.U8
        g1, g2 = one.scan_topk_grouped_valued(metric, qs[i], 20, lo, hi), sh.scan_topk_grouped_valued(metric, qs[i], 20, lo, hi)
        assert g1[0].tolist() == g2[0].tolist() and g1[2].tolist() == g2[2].tolist(), i
    res1 = one.scan_topk_batch_valued(metric, qs, lo, hi, 20)
    res2 = sh.scan_topk_batch_valued(metric, qs, lo, hi, 20)
    assert all(np.array_equal(x, y) for x, y in zip(res1, res2))
    cl = sh.clone()                                              # Shards.clone carries the values
    assert cl.has_values()
    _same(_ask(cl, metric, qs, values), want, "clone of the shard set")
    cl.close()
    sh.append(lc.data(vt, 10, dim, 96), np.arange(10, dtype=np.int64) + 10**7)      # an append drops the values of the shards it reaches: the set has none
    assert not sh.has_values()
    sh.clear_values()
    assert lc.error_code(pkg, lambda: sh.scan_topk_valued(metric, qs[0], 5, None, None)) == VG_ERR_INVALID
    sh.close()
    one.close()
