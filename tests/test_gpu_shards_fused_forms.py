"""Every fused scan form over three shards against one corpus of the same rows: the shard layer only deals rows, mask bits and labels
out and merges the shards' lists back (point 4), through the same kernels over the same floats - so rowids, distances,
labels and counts are compared with ==, no tolerance.

150 f32 rows of 24 floats in blocks of 64 over three logical shards of one device: the shards hold 64, 64 and 22 rows (a ragged last
block).  Labels are position % 7, with label 99 planted on rows 0..9 - shard 0 alone.  The mask allows no row of positions 64..127, so
shard 1 hands back empty lists.  k = 64 exceeds shard 2's 22 rows (short lists) and the 8 labels present (short grouped answers).

The refusals a three-shard handle answers itself (k, per_label, no mask, no labels) are compared word for word; the texts were
recorded before the entry points were folded onto one scaffold."""
import numpy as np
import pytest

import datagen as dg

pytestmark = pytest.mark.gpu

N, DIM, BLOCK = 150, 24, 64
KS = (1, 20, 64)
QUERY_LABELS = (3, 99, 0, 12345, 6)                             # (12345: on no row)
QUERY_SETS = ([99, 2, 5], [], [0, 1, 2, 3, 4, 5, 6], [12345], [99])


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


@pytest.fixture(scope="module")
def world(pkg):
    """(one corpus, three shards) over the same rows, labels and mask; five queries"""
    rng = np.random.default_rng(20)
    rows = rng.standard_normal((N, DIM), dtype=np.float32)
    rows[40] = rows[7]                                          # equal distances on shard 0, and across shards 0 and 2
    rows[140] = rows[7]
    queries = rng.standard_normal((5, DIM), dtype=np.float32)
    labels = (np.arange(N) % 7).astype(np.uint32)
    labels[:10] = 99
    allowed = np.ones(N, dtype=bool)
    allowed[64:128] = False
    allowed[3::11] = False
    one = pkg.Corpus(dg.F32, DIM)
    many = pkg.Shards(dg.F32, DIM, [0, 0, 0], block_rows=BLOCK)
    for h in (one, many):
        h.append(rows)
        h.set_labels(labels)
        assert h.set_mask(bits=allowed) == int(allowed.sum())
    assert [int(n) for n in many.shard_rows()] == [64, 64, 22]
    yield one, many, queries
    one.close()
    many.close()


def _same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (what, g, w)


def _single_forms(k, m):
    """name -> call(handle, query) of every single form; the paged ones return two pages"""
    L2 = dg.L2

    def pages(h, q, masked):
        ids, dist = h.scan_topk_after(L2, q, k, None, masked=masked)
        assert len(ids) > 0
        ids2, dist2 = h.scan_topk_after(L2, q, k, (float(dist[-1]), int(ids[-1])), masked=masked)
        return ids, dist, ids2, dist2

    def key_pages(h, q, masked):
        keys = h.scan_topk_after_keys(L2, q, k, None, masked=masked)
        assert len(keys) > 0
        return keys, h.scan_topk_after_keys(L2, q, k, int(keys[-1]), masked=masked)

    forms = {"masked": lambda h, q: h.scan_topk_masked(L2, q, k)}
    for lab in QUERY_LABELS:
        forms["labeled %d" % lab] = lambda h, q, lab=lab: h.scan_topk_labeled(L2, q, k, lab)
    for ex in (False, True):
        for s in QUERY_SETS[:3]:
            forms["labelset %r exclude=%d" % (s, ex)] = lambda h, q, s=s, ex=ex: h.scan_topk_labelset(L2, q, k, s, exclude=ex)
            forms["grouped labelset %r exclude=%d" % (s, ex)] = lambda h, q, s=s, ex=ex: h.scan_topk_grouped_labelset(L2, q, k, s, exclude=ex)
            forms["capped labelset %r exclude=%d" % (s, ex)] = lambda h, q, s=s, ex=ex: h.scan_topk_capped_labelset(L2, q, k, m, s, exclude=ex)
    for masked in (False, True):
        forms["grouped masked=%d" % masked] = lambda h, q, masked=masked: h.scan_topk_grouped(L2, q, k, masked=masked)
        forms["capped masked=%d" % masked] = lambda h, q, masked=masked: h.scan_topk_capped(L2, q, k, m, masked=masked)
        forms["paged masked=%d" % masked] = lambda h, q, masked=masked: pages(h, q, masked)
        forms["paged keys masked=%d" % masked] = lambda h, q, masked=masked: key_pages(h, q, masked)
    return forms


def _batch_forms(k, m, nq):
    """name -> call(handle, queries) of every batch form"""
    L2 = dg.L2

    def pages(h, qs, masked):
        ids, dist, cnt = h.scan_topk_batch_after(L2, qs, k, None, masked=masked)
        assert cnt.min() > 0
        cur = [(float(dist[i, cnt[i] - 1]), int(ids[i, cnt[i] - 1])) for i in range(nq)]
        return (ids, dist, cnt) + tuple(h.scan_topk_batch_after(L2, qs, k, cur, masked=masked))

    def key_pages(h, qs, masked):
        keys, cnt = h.scan_topk_batch_after_keys(L2, qs, k, None, masked=masked)
        assert cnt.min() > 0
        cur = np.array([keys[i, cnt[i] - 1] for i in range(nq)], dtype=np.uint64)
        return (keys, cnt) + tuple(h.scan_topk_batch_after_keys(L2, qs, k, cur, masked=masked))

    forms = {"batch masked": lambda h, qs: h.scan_topk_batch_masked(L2, qs, k),
             "batch labeled": lambda h, qs: h.scan_topk_batch_labeled(L2, qs, list(QUERY_LABELS[:nq]), k)}
    for ex in (False, True):
        forms["batch labelset exclude=%d" % ex] = lambda h, qs, ex=ex: h.scan_topk_batch_labelset(L2, qs, list(QUERY_SETS[:nq]), k, exclude=ex)
    for masked in (False, True):
        forms["batch grouped masked=%d" % masked] = lambda h, qs, masked=masked: h.scan_topk_batch_grouped(L2, qs, k, masked=masked)
        forms["batch capped masked=%d" % masked] = lambda h, qs, masked=masked: h.scan_topk_batch_capped(L2, qs, k, m, masked=masked)
        forms["batch paged masked=%d" % masked] = lambda h, qs, masked=masked: pages(h, qs, masked)
        forms["batch paged keys masked=%d" % masked] = lambda h, qs, masked=masked: key_pages(h, qs, masked)
    return forms


@pytest.mark.parametrize("k", KS)
def test_three_shards_answer_what_one_corpus_answers(world, k):
    one, many, queries = world
    for m in (1, 3):
        for name, call in _single_forms(k, m).items():
            _same(call(many, queries[0]), call(one, queries[0]), (name, k, m))
        for nq in (1, 5):
            for name, call in _batch_forms(k, m, nq).items():
                _same(call(many, queries[:nq]), call(one, queries[:nq]), (name, k, m, nq))


def test_short_lists_and_short_grouped_answers(world):
    """what the fixture is built to reach, said of the answers themselves"""
    one, many, queries = world
    ids, dist, lab = many.scan_topk_grouped(dg.L2, queries[0], 64)
    assert sorted(lab.tolist()) == [0, 1, 2, 3, 4, 5, 6, 99]   # fewer labels than k
    ids, dist = many.scan_topk_masked(dg.L2, queries[0], 64)
    assert len(ids) == 64 and not ((ids - 1 >= 64) & (ids - 1 < 128)).any()   # nothing of shard 1; shard 2's 22 rows cannot fill a list
    ids, dist = many.scan_topk_labeled(dg.L2, queries[0], 64, 99)
    assert sorted(ids.tolist()) == list(range(1, 11))           # one label on one shard: the other lists are empty


# form -> (call(handle, queries, k, per_label), the name its k / per_label / labels refusals carry, the family word of the k-range
# message, the name "no row mask set" carries or None, needs labels, takes per_label)
def _refusal_forms():
    L2 = dg.L2
    q1 = lambda qs: qs[0]
    S, B = "vg_scan_topk_", "vg_shards_scan_topk_batch_"
    t = {
        "masked": (lambda h, qs, k, m: h.scan_topk_masked(L2, q1(qs), k), S + "masked", "masked", S + "masked", False, False),
        "batch_masked": (lambda h, qs, k, m: h.scan_topk_batch_masked(L2, qs, k), S + "batch_masked", "masked", S + "batch_masked", False, False),
        "labeled": (lambda h, qs, k, m: h.scan_topk_labeled(L2, q1(qs), k, 3), S + "labeled", "labeled", None, True, False),
        "batch_labeled": (lambda h, qs, k, m: h.scan_topk_batch_labeled(L2, qs, [3, 4], k), S + "batch_labeled", "labeled", None, True, False),
        "labelset": (lambda h, qs, k, m: h.scan_topk_labelset(L2, q1(qs), k, [3]), S + "labelset", "label-set", None, True, False),
        "batch_labelset": (lambda h, qs, k, m: h.scan_topk_batch_labelset(L2, qs, [[3], [4]], k), S + "batch_labelset", "label-set", None, True, False),
        "grouped": (lambda h, qs, k, m: h.scan_topk_grouped(L2, q1(qs), k), S + "grouped", "grouped", None, True, False),
        "grouped_masked": (lambda h, qs, k, m: h.scan_topk_grouped(L2, q1(qs), k, masked=True), S + "grouped", "grouped", S + "grouped_masked", True, False),
        "batch_grouped": (lambda h, qs, k, m: h.scan_topk_batch_grouped(L2, qs, k), B + "grouped", "grouped", None, True, False),
        "batch_grouped_masked": (lambda h, qs, k, m: h.scan_topk_batch_grouped(L2, qs, k, masked=True), B + "grouped_masked", "grouped",
                                 B + "grouped_masked", True, False),
        "capped": (lambda h, qs, k, m: h.scan_topk_capped(L2, q1(qs), k, m), S + "capped", "capped", None, True, True),
        "capped_masked": (lambda h, qs, k, m: h.scan_topk_capped(L2, q1(qs), k, m, masked=True), S + "capped", "capped", S + "capped_masked", True, True),
        "batch_capped": (lambda h, qs, k, m: h.scan_topk_batch_capped(L2, qs, k, m), B + "capped", "capped", None, True, True),
        "batch_capped_masked": (lambda h, qs, k, m: h.scan_topk_batch_capped(L2, qs, k, m, masked=True), B + "capped_masked", "capped",
                                B + "capped_masked", True, True),
        "grouped_labelset": (lambda h, qs, k, m: h.scan_topk_grouped_labelset(L2, q1(qs), k, [3]), "vg_shards_scan_topk_grouped_labelset", "label-set",
                             None, True, False),
        "capped_labelset": (lambda h, qs, k, m: h.scan_topk_capped_labelset(L2, q1(qs), k, m, [3]), "vg_shards_scan_topk_capped_labelset", "label-set",
                            None, True, True),
    }
    for masked in (False, True):
        sfx = "_masked" if masked else ""
        t["after" + sfx] = (lambda h, qs, k, m, masked=masked: h.scan_topk_after(L2, q1(qs), k, None, masked=masked), S + "after" + sfx, "paged",
                            S + "after" + sfx if masked else None, False, False)
        t["after" + sfx + "_keys"] = (lambda h, qs, k, m, masked=masked: h.scan_topk_after_keys(L2, q1(qs), k, None, masked=masked), S + "after" + sfx,
                                      "paged", S + "after" + sfx if masked else None, False, False)
        t["batch_after" + sfx] = (lambda h, qs, k, m, masked=masked: h.scan_topk_batch_after(L2, qs, k, None, masked=masked), S + "batch_after" + sfx,
                                  "paged", S + "batch_after" + sfx if masked else None, False, False)
        t["batch_after" + sfx + "_keys"] = (lambda h, qs, k, m, masked=masked: h.scan_topk_batch_after_keys(L2, qs, k, None, masked=masked),
                                            S + "batch_after" + sfx, "paged", S + "batch_after" + sfx if masked else None, False, False)
    return t


def _refused(pkg, call, code, text):
    with pytest.raises(pkg.VectorGpuError) as e:
        call()
    assert str(e.value) == "vectorgpu error %d: %s" % (code, text)


def test_refusals_word_for_word(pkg, world):
    one, many, queries = world
    qs = queries[:2]
    forms = _refusal_forms()
    assert len(forms) == 24
    for name, (call, who, family, mask_who, needs_labels, capped) in forms.items():
        _refused(pkg, lambda: call(many, qs, 0, 2), 1, who + ": k must be at least 1")
        _refused(pkg, lambda: call(many, qs, 65, 2), 5, who + ": k must be in 1..64 (" + family + " scans use the fused list only)")
        if capped:
            _refused(pkg, lambda: call(many, qs, 5, 0), 1, who + ": per_label must be at least 1")
    # a handle of its own: rows, and neither mask nor labels
    bare = pkg.Shards(dg.F32, DIM, [0, 0, 0], block_rows=BLOCK)
    try:
        bare.append(np.zeros((N, DIM), dtype=np.float32))
        for name, (call, who, family, mask_who, needs_labels, capped) in forms.items():
            if mask_who:                                        # (asked for before the labels)
                _refused(pkg, lambda: call(bare, qs, 5, 2), 1, mask_who + ": no row mask set")
        bare.set_mask(bits=np.ones(N, dtype=bool))
        for name, (call, who, family, mask_who, needs_labels, capped) in forms.items():
            if needs_labels:
                _refused(pkg, lambda: call(bare, qs, 5, 2), 1, who + ": no labels set")
    finally:
        bare.close()
