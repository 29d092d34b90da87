"""The Hamming / Jaccard matrix-core batches across a corpus' lifecycle: every form after a fresh append in two halves, patch_rows,
delete_rows of a block at the end, clear + a smaller append, an append across the reservation, trim, reserve, clone and a patch of the
clone's source - tests/bits_batch_cases.py has the script (lifecycle), tests/test_bits_batch_cases.py proves without a device that an
answer from the rows before a call, from the rows left behind the new end inside the last 32-row tile, or under the previous mask and
labels would differ.

After every step the full batch answer of 130 pairwise different queries is compared with numpy over the model's rows and explicit,
non-contiguous rowids: ids, order, distance bits, counts, ==.  Every call asserts that its form answered (path 8).  Mask and labels stay
in force over patch, trim, reserve and clone and are gone after delete, append and clear: mask_count() == -1, has_labels() False, the
masked / labeled call refuses; then new ones are set, which differ from the old ones at planted rows."""
import numpy as np
import pytest

import bits_batch_cases as bb

pytestmark = pytest.mark.gpu

NAMES = ("hamming", "jaccard")


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


FORMS = [("plain", 100), ("plain", 200), ("masked", 128), ("masked", 272), ("labeled", 100), ("within", 128), ("within", 512),
         ("within_masked", 128)]
QL = bb.query_labels()


def _ask(pkg, h, name, kind, qs, radii=None, k=bb.K_LIFE, ql=QL, path=True):
    """one batch of a form on `h`, as a list of answers per query; path: assert that the matrix-core form answered"""
    metric = getattr(pkg, name.upper())
    if kind in ("within", "within_masked"):
        got = (h.scan_within_batch_masked if kind == "within_masked" else h.scan_within_batch)(metric, qs, radii)
        assert not path or h.within_batch_last_path() == 8, (name, kind)
        return got
    if kind == "plain":
        ids, dist, cnt = h.scan_topk_batch(metric, qs, k)
        assert not path or h.last_batch_path() == 8, (name, kind)
    elif kind == "masked":
        ids, dist, cnt = h.scan_topk_batch_masked(metric, qs, k)
        assert not path or h.batch_masked_last_path() == 8, (name, kind)
    else:
        ids, dist, cnt = h.scan_topk_batch_labeled(metric, qs, ql[:len(qs)], k)
        assert not path or h.batch_labeled_last_path() == 8, (name, kind)
    return [(ids[i, :cnt[i]], dist[i, :cnt[i]]) for i in range(len(qs))]


def _compare(pkg, h, name, kind, qs, s, ctx, path=True):
    """the handle's batch answer against numpy over the state's rows, rowids, mask and labels"""
    radii = None
    if kind in ("within", "within_masked"):
        radii = bb.lifecycle_radii(bb.batch_distances(name, s.rows, qs), s.allowed if kind == "within_masked" else None)
    want = bb.answers(name, kind, qs, s.rows, s.ids, s.allowed, s.labels, radii)
    got = _ask(pkg, h, name, kind, qs, radii, path=path)
    assert h.rows == len(s.ids), ctx
    m = bb.CASES[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(w) == 2 or g[2] == w[2], (ctx, i)
        m.check(g, w, (ctx, i))


def _set(h, s):
    assert h.set_mask(bits=s.allowed) == int(s.allowed.sum())
    h.set_labels(s.labels)


def _dropped(pkg, h, name, kind, qs):
    """directly after delete / append / clear: neither mask nor labels, the masked / labeled call refuses"""
    assert h.mask_count() == -1 and not h.has_labels()
    metric = getattr(pkg, name.upper())
    if kind == "masked":
        with pytest.raises(pkg.VectorGpuError, match="no row mask set"):
            h.scan_topk_batch_masked(metric, qs, bb.K_LIFE)
    if kind == "within_masked":
        with pytest.raises(pkg.VectorGpuError, match="no row mask set"):
            h.scan_within_batch_masked(metric, qs, [0.0] * len(qs))
    if kind == "labeled":
        with pytest.raises(pkg.VectorGpuError, match="no labels set"):
            h.scan_topk_batch_labeled(metric, qs, QL, bb.K_LIFE)


def _apply(h, s, sharded=False):
    """the state's call; a shard set refuses patch_rows and delete_rows, it reaches these states by clear + append"""
    if s.op == "create" or (sharded and s.op in ("patch", "delete")) or s.op == "clear_append":
        if s.op != "create":
            h.clear()
            assert h.rows == 0 and h.mask_count() == -1 and not h.has_labels()
        half = len(s.ids) // 2
        h.append(s.rows[:half], s.ids[:half])
        h.append(s.rows[half:], s.ids[half:])
        return True
    if s.op == "patch":
        h.patch_rows(*s.args)
    elif s.op == "delete":
        h.delete_rows(*s.args)
    elif s.op == "append":
        h.append(*s.args)
    elif s.op == "trim":
        h.trim()
    elif s.op == "reserve":
        h.reserve(8000)
    return s.dropped


def _script(pkg, monkeypatch, name, kind, dim, make, sharded):
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    qs, states = bb.lifecycle(dim)
    h, clone = make(), None
    try:
        for j, s in enumerate(states):
            ctx = (name, kind, dim, j, s.op)
            if s.op == "clone":
                clone = h.clone()
                assert clone.mask_count() == int(s.allowed.sum()) and clone.has_labels()
                _compare(pkg, clone, name, kind, qs, s, ctx, path=not sharded)
                continue
            if _apply(h, s, sharded):
                _dropped(pkg, h, name, kind, qs)
                _set(h, s)
            assert h.mask_count() == int(s.allowed.sum()) and h.has_labels(), ctx      # kept, or set again
            _compare(pkg, h, name, kind, qs, s, ctx, path=not sharded)
        _compare(pkg, clone, name, kind, qs, states[7], (name, kind, dim, "the clone after its source was patched"), path=not sharded)
    finally:
        h.close()
        if clone is not None:
            clone.close()


@pytest.mark.parametrize("kind,dim", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_lifecycle(pkg, monkeypatch, name, kind, dim):
    _script(pkg, monkeypatch, name, kind, dim, lambda: pkg.Corpus(pkg.U8, dim, capacity=bb.CAPACITY), False)


@pytest.mark.parametrize("name", NAMES)
def test_lifecycle_three_shards(pkg, monkeypatch, name):
    """plain, 100 bytes, 64-row blocks over three shards (a shard handle does not expose its batch path)"""
    _script(pkg, monkeypatch, name, "plain", 100, lambda: pkg.Shards(pkg.U8, 100, [0, 0, 0], block_rows=64), True)


@pytest.mark.parametrize("name", NAMES)
def test_call_sequences_on_one_handle(pkg, monkeypatch, name):
    """calls that reuse the handle's query image, candidate lists, key store and position list with other shapes: k = 32 then 1, 257
    queries then 2, the other metric in between, labeled then plain then masked, a range batch between two top-k batches"""
    monkeypatch.setenv("VG_BATCH_BITS_MIN_QUERIES", "2")
    other = NAMES[1 - NAMES.index(name)]
    rows, qs, pos = bb.planted(100, bb.N0, 257, 9500)
    ids = bb.make_ids(bb.N0)
    rng = np.random.default_rng(9501)
    allowed = rng.random(bb.N0) < 0.6
    labels = rng.integers(0, 5, bb.N0).astype(np.uint32)
    ql = bb.query_labels(257)
    labels[pos[::2]] = ql[::2]
    d = {nm: bb.batch_distances(nm, rows, qs) for nm in NAMES}
    h = pkg.Corpus(pkg.U8, 100)
    h.append(rows, ids)
    _set(h, bb.State(None, None, rows, ids, allowed, labels, False))

    def topk(nm, kind, nq, k):
        got = _ask(pkg, h, nm, kind, qs[:nq], k=k, ql=ql)
        for i in range(nq):
            al = allowed if kind == "masked" else (labels == ql[i]) if kind == "labeled" else None
            bb.CASES[nm].check(got[i], bb.expected(d[nm][i], k, allowed=al, rowids=ids), (nm, kind, nq, k, i))

    def within(nm, kind, nq):
        radii = bb.lifecycle_radii(d[nm][:nq], allowed if kind == "within_masked" else None)
        got = _ask(pkg, h, nm, kind, qs[:nq], radii)
        al = allowed if kind == "within_masked" else None
        bb.check_within(nm, got, [bb.within(d[nm][i], radii[i], allowed=al, rowids=ids) for i in range(nq)], (nm, kind, nq))

    for kind in ("plain", "masked", "labeled"):
        topk(name, kind, 257, 32)
        topk(name, kind, 257, 1)
        topk(name, kind, 2, 20)
        topk(other, kind, 257, 20)
        topk(name, kind, 257, 20)
    for kind in ("labeled", "plain", "masked", "plain"):
        topk(name, kind, 130, 20)
    for wkind in ("within", "within_masked"):
        topk(name, "masked", 257, 20)
        within(name, wkind, 257)
        topk(name, "masked", 130, 5)
        within(other, wkind, 130)
    h.close()
