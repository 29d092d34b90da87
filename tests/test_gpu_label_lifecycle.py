"""Labels and the row mask of a handle across its lifecycle: every label-aware scan after patch / delete / append, clear + a smaller
or a larger re-append, clone, trim / reserve, on single corpora and on a 3-shard set - tests/label_lifecycle_cases.py has the paths,
the planted ladders and the scripts, tests/test_label_lifecycle_cases.py proves without a device that every compared answer is decided
by float64 alone and that a stale label, mask bit or row would change it.

The `ask` runs on one handle, with (k, m) in ((20, 3), (64, 5), (20, 1)): scan_topk_labeled for three labels (one absent) and five
queries, scan_topk_batch_labeled for nine queries with mixed labels, scan_topk_grouped / _capped and their batch forms for five
queries (one full pass and a ragged one), each with masked = False and True.  After every compared step the handle answers
  (a) bit for bit - rowids, distance bits, labels, counts - like a handle freshly staged from the model's rows, rowids, labels and
      mask (two fresh handles are compared first);
  (b) like a reference that is not the GPU: uint8 the contract over the oracle's distances, exactly (distance bits and tie order
      included); floats the rowids and labels of the contract over float64 distances, exactly, the distances within the suite's bar
      (test_gpu_scan._check_float_distances) of the oracle's over the returned rows, ascending, and capped_cases._judge_f64.
Directly after delete, append and clear the labels and the mask are gone: has_labels() is False, mask_count() is -1, all twelve
label- or mask-aware calls fail with VG_ERR_INVALID, scan_topk still answers like the oracle, labels of the old length are refused.

f32 x 384 also asks the grouped and capped scans under DOT after the patch and after the first deletion: the patch's +Inf row is
at -Inf there for the even queries and comes first (Runner.dot_side_case).

A refused set_labels (include/vectorgpu.h: n != rows is VG_ERR_INVALID; it does not say what becomes of labels already set): the
length is checked before anything is touched, so the labels the handle holds stay and keep answering.  Pinned here.

Multi-shard sets refuse patch_rows / delete_rows (VG_ERR_UNSUPPORTED), so the shard tests reach the edit script's states by clear +
re-append (a lifecycle of its own: every state differs in size) and apply its append for real."""
import numpy as np
import pytest

import datagen as dg
import label_lifecycle_cases as ll
import labeled_cases as lab
from capped_cases import _judge_f64
from test_gpu_lifecycle import check_scan
from test_gpu_scan import pkg, _check_float_distances          # noqa: F401  (pkg: the module-scoped fixture)

pytestmark = pytest.mark.gpu

VG_ERR_INVALID, VG_ERR_UNSUPPORTED = 1, 5
ALL = [p.name for p in ll.PATHS]
SHARDED = ["f32_384_l2", "u8_64_l2"]
KS = sorted(set(k for k, _ in ll.KMS))


class Runner:
    def __init__(self, pkg, orc, name):
        self.pkg, self.orc, self.p, self.name = pkg, orc, ll.PATH_BY_NAME[name], name
        self.qs = ll.queries(name)
        self.q64 = dg.storage_to_f64(self.p.vt, self.qs)
        self.handles = []

    def close(self):
        for h in self.handles:
            h.close()

    def keep(self, h):
        self.handles.append(h)
        return h

    def make(self, shards=False):
        p = self.p
        return self.keep(self.pkg.Shards(p.vt, p.dim, [0, 0, 0], block_rows=64) if shards else self.pkg.Corpus(p.vt, p.dim))

    def label(self, h, s):
        h.set_labels(s.labels)
        assert h.set_mask(bits=s.allowed) == int(s.allowed.sum())
        assert h.has_labels()

    def stage(self, s, shards=False):
        """a fresh handle of the state's rows (two appends: the second one extends), labels and mask"""
        h = self.make(shards)
        third = len(s.rows) // 3
        h.append(s.rows[:third], s.ids[:third])
        h.append(s.rows[third:], s.ids[third:])
        self.label(h, s)
        return h

    # ------------------------------------------------------------------------------------------------ asking
    def ask(self, h):
        """{(kind, masked, k, m, query, label): (rowids, float32 distances, labels or None)}"""
        p, qs, out = self.p, self.qs, {}
        g5 = np.ascontiguousarray(qs[:ll.NQ_GROUP])

        def rows_of(res, kind, masked, k, m):
            for i in range(res[0].shape[0]):
                c = res[-1][i]
                out[(kind, masked, k, m, i, None)] = (res[0][i, :c].copy(), res[1][i, :c].astype(np.float32), res[2][i, :c].copy())

        for k, m in ll.KMS:
            for i in range(ll.NQ_GROUP):
                for l in ll.ask_labels(self.name, i):
                    ids, d = h.scan_topk_labeled(p.metric, qs[i], k, int(l))
                    out[("labeled", False, k, None, i, int(l))] = (ids, d.astype(np.float32), None)
            for masked in (False, True):
                for i in range(ll.NQ_GROUP):
                    ids, d, gl = h.scan_topk_capped(p.metric, qs[i], k, m, masked=masked)
                    out[("capped", masked, k, m, i, None)] = (ids, d.astype(np.float32), gl)
                rows_of(h.scan_topk_batch_capped(p.metric, g5, k, m, masked=masked), "batch_capped", masked, k, m)
        bl = ll.batch_labels(self.name)
        for k in KS:
            for masked in (False, True):
                for i in range(ll.NQ_GROUP):
                    ids, d, gl = h.scan_topk_grouped(p.metric, qs[i], k, masked=masked)
                    out[("grouped", masked, k, None, i, None)] = (ids, d.astype(np.float32), gl)
                rows_of(h.scan_topk_batch_grouped(p.metric, g5, k, masked=masked), "batch_grouped", masked, k, None)
            ids, d, cnt = h.scan_topk_batch_labeled(p.metric, qs, bl, k)
            for i in range(ll.NQ):
                out[("batch_labeled", False, k, None, i, int(bl[i]))] = (ids[i, :cnt[i]].copy(), d[i, :cnt[i]].astype(np.float32), None)
        return out

    def label_aware_calls(self, h):
        """the twelve calls that read labels or the mask"""
        p, q, qs = self.p, self.qs[0], np.ascontiguousarray(self.qs[:ll.NQ_GROUP])
        l = int(ll.ask_labels(self.name, 0)[0])
        calls = [lambda: h.scan_topk_labeled(p.metric, q, 20, l),
                 lambda: h.scan_topk_batch_labeled(p.metric, qs, np.full(len(qs), l, dtype=np.uint32), 20),
                 lambda: h.scan_topk_masked(p.metric, q, 20), lambda: h.scan_topk_batch_masked(p.metric, qs, 20)]
        for masked in (False, True):
            calls += [lambda masked=masked: h.scan_topk_grouped(p.metric, q, 20, masked=masked),
                      lambda masked=masked: h.scan_topk_capped(p.metric, q, 20, 3, masked=masked),
                      lambda masked=masked: h.scan_topk_batch_grouped(p.metric, qs, 20, masked=masked),
                      lambda masked=masked: h.scan_topk_batch_capped(p.metric, qs, 20, 3, masked=masked)]
        assert len(calls) == 12
        return calls

    # ------------------------------------------------------------------------------------------------ comparing
    def same(self, a, b, what):
        assert a.keys() == b.keys()
        for key in a:
            (ai, ad, al), (bi, bd, bl) = a[key], b[key]
            assert ai.tolist() == bi.tolist(), (self.name, what, key, ai[:6], bi[:6])
            assert len(ad) == len(bd) and dg.same_float_bits(ad, bd), (self.name, what, key, ad[:6], bd[:6])
            assert al is None or al.tolist() == bl.tolist(), (self.name, what, key)

    def check(self, ans, s, what):
        """against the contract over reference distances (ll.distances: float64 / the oracle's)"""
        p, orc = self.p, self.orc
        D = ll.distances(p, orc, s.rows)
        with np.errstate(invalid="ignore"):
            enters = D < np.inf
        for key, (gi, gd, gl) in ans.items():
            kind, masked, k, m, i, label = key
            base = kind.replace("batch_", "")
            ctx = (self.name, what, key)
            pos = ll.answer(base, D[i], s.labels, s.allowed if masked else None, k, m, label)
            assert gi.tolist() == s.ids[pos].tolist(), (ctx, gi[:8], s.ids[pos][:8])
            if gl is not None:
                assert gl.tolist() == s.labels[pos].tolist(), ctx
            if not len(pos):
                continue
            if not ll.is_float(p):
                assert dg.same_float_bits(gd, D[i, pos].astype(np.float32)), (ctx, gd[:6], D[i, pos][:6])
                continue
            want = orc.scan_distances(orc.AVX2, p.metric, p.vt, self.qs[i], s.rows[pos])
            _check_float_distances(gd, want, p.vt, p.metric, self.qs[i], s.rows[pos])
            assert (np.diff(gd) >= 0).all(), ctx
            if base != "labeled":                                # (rows that cannot enter a list count as rows without a label)
                labels = np.where(enters[i], s.labels, ll.NONE).astype(np.uint32)
                _judge_f64((pos + 1, gd.astype(np.float64), gl), np.where(enters[i], D[i], np.inf), labels, p.metric, self.q64[i], k,
                           1 if base == "grouped" else m, ctx, allowed=s.allowed if masked else None)

    def compare(self, h, s, what, twice=False):
        fresh = self.stage(s)
        want = self.ask(fresh)
        if twice:
            again = self.stage(s)
            self.same(self.ask(again), want, what + ": two fresh handles")
            again.close()
        got = self.ask(h)
        self.same(got, want, what)
        self.check(got, s, what)
        assert h.rows == len(s.ids) and h.has_labels() and h.mask_count() == int(s.allowed.sum())
        fresh.close()
        return got

    def ask_dot(self, h):
        """grouped and capped, single and batch, masked and not, under DOT: the keys of `ask`"""
        g5, out = np.ascontiguousarray(self.qs[:ll.NQ_GROUP]), {}
        for k, m in ll.KMS:
            for masked in (False, True):
                bg = h.scan_topk_batch_grouped(dg.DOT, g5, k, masked=masked)
                bc = h.scan_topk_batch_capped(dg.DOT, g5, k, m, masked=masked)
                for i in range(ll.NQ_GROUP):
                    for kind, (ids, d, gl) in (("grouped", h.scan_topk_grouped(dg.DOT, g5[i], k, masked=masked)),
                                               ("capped", h.scan_topk_capped(dg.DOT, g5[i], k, m, masked=masked)),
                                               ("batch_grouped", tuple(a[i, :bg[3][i]] for a in bg[:3])),
                                               ("batch_capped", tuple(a[i, :bc[3][i]] for a in bc[:3]))):
                        out[(kind, masked, k, m, i, None)] = (ids.copy(), d.astype(np.float32), gl.copy())
        return out

    def dot_side_case(self, h, s, what):
        """f32 x 384 after the patch and after a deletion + set_labels: the patched row with +Inf in its last lane is at -Inf under DOT
        for the even queries (it comes first, with its label and the oracle's bits) and at +Inf for the odd ones (never returned).
        Every ladder row of a query ties exactly under DOT (the rung's coordinate meets a 0 of the query).  Bit for bit against a
        fresh handle; rowids, labels, the cap, the mask, the oracle's distances over the returned rows, and capped_cases._judge_f64
        over float64 distances (-Inf stands as -1e30 on both sides there: its bits are compared apart)"""
        p, orc, low = self.p, self.orc, -1.0e30
        fresh = self.stage(s)
        got = self.ask_dot(h)
        self.same(got, self.ask_dot(fresh), what + ": DOT")
        fresh.close()
        D = ll.distances(p, orc, s.rows, metric=dg.DOT)
        (at,) = np.nonzero(np.isinf(s.rows[:, p.dim - 1]))[0]
        with np.errstate(invalid="ignore"):
            enters = D < np.inf
        for key, (gi, gd, gl) in got.items():
            kind, masked, k, m, i, _ = key
            ctx = (self.name, what, "DOT", key)
            cap = 1 if kind.endswith("grouped") else m
            pos = np.searchsorted(s.ids, gi)
            assert (s.ids[pos] == gi).all() and len(set(pos.tolist())) == len(pos) and gl.tolist() == s.labels[pos].tolist(), ctx
            assert enters[i, pos].all() and (gl != ll.NONE).all() and (not masked or s.allowed[pos].all()), ctx
            assert np.unique(gl, return_counts=True)[1].max() <= cap, ctx
            if i % 2 == 0:
                bits = orc.scan_distances(orc.AVX2, dg.DOT, p.vt, self.qs[i], s.rows[at:at + 1])
                assert pos[0] == at and gl[0] == ll.L_SPECIAL and gd[0] == -np.inf and dg.same_float_bits(gd[:1], bits), (ctx, gi[:3], gd[:3])
            else:
                assert D[i, at] == np.inf and at not in pos, ctx
            want = orc.scan_distances(orc.AVX2, dg.DOT, p.vt, self.qs[i], s.rows[pos])
            _check_float_distances(gd, want, p.vt, dg.DOT, self.qs[i], s.rows[pos])
            assert (np.diff(gd) >= 0).all(), ctx
            labels = np.where(enters[i], s.labels, ll.NONE).astype(np.uint32)
            ref = np.where(enters[i], np.maximum(D[i], low), np.inf)
            _judge_f64((pos + 1, np.maximum(gd.astype(np.float64), low), gl), ref, labels, dg.DOT, self.q64[i], k, cap, ctx,
                       allowed=s.allowed if masked else None)

    def check_dropped(self, h, s, old_rows, what):
        """directly after delete / append / clear: no labels, no mask, the plain scan still right"""
        p, pkg = self.p, self.pkg
        assert not h.has_labels() and h.mask_count() == -1, what
        for j, call in enumerate(self.label_aware_calls(h)):
            assert lab.error_code(pkg, call) == VG_ERR_INVALID, (what, j)
        for i in (0, 1):
            got_ids, got_d = h.scan_topk(p.metric, self.qs[i], 20)
            check_scan(self.orc, p.vt, p.metric, self.qs[i], s.rows, s.ids, got_ids, got_d, 20)
        if old_rows != len(s.ids):
            assert lab.error_code(pkg, lambda: h.set_labels(np.zeros(old_rows, dtype=np.uint32))) == VG_ERR_INVALID, what
            assert not h.has_labels()

    def apply(self, h, s, what):
        old = h.rows
        if s.op == "patch":
            h.patch_rows(*s.args)
        elif s.op == "delete":
            h.delete_rows(*s.args)
        elif s.op == "append":
            h.append(*s.args)
        elif s.op == "clear_append":
            h.clear()
            assert h.rows == 0 and not h.has_labels() and h.mask_count() == -1
            h.append(*s.args)
        if s.dropped:
            self.check_dropped(h, s, old, what)
            self.label(h, s)
        else:
            assert h.has_labels() and h.mask_count() == int(s.allowed.sum()), what


@pytest.fixture
def run(pkg, orc, request):
    r = Runner(pkg, orc, request.param)
    yield r
    r.close()


def _start(name):
    return ll.compared_states(name)[0][1]


# ---------------------------------------------------------------------------------------------------- single corpora

@pytest.mark.parametrize("run", ALL, indirect=True)
def test_patch_delete_append_keep_or_drop_labels_and_mask(run):
    """the edit script: the patch keeps labels and mask (ladder rungs move, a NaN and a +Inf row take over a label nobody else
    carries), three deletions (rows mod 64 -> 0, 1, 63) and an append drop them; f32 x 384: the -Inf row under DOT after the patch
    and after the first deletion; then what a refused set_labels leaves behind"""
    start = _start(run.name)
    h = run.stage(start)
    run.compare(h, start, "start", twice=True)
    for i, s in enumerate(ll.edit_script(run.name)):
        what = "step %d (%s)" % (i, s.op)
        run.apply(h, s, what)
        got = run.compare(h, s, what)
        if run.name == "f32_384_l2" and i < 2:                   # the patch planted a row that DOT puts at -Inf; labels kept / set again
            run.dot_side_case(h, s, what)
    code = lab.error_code(run.pkg, lambda: h.set_labels(np.zeros(h.rows + 1, dtype=np.uint32)))
    assert code == VG_ERR_INVALID and h.has_labels()              # refused before anything is touched: the labels stay
    run.same(run.ask(h), got, "after a refused set_labels")


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_clear_then_a_smaller_append_reads_no_stale_label_or_bit(run):
    """the label array and both bitmaps are reused (device_bytes: the working buffers, which hold them, keep their size): the old
    labels right behind the new end all equal the label asked for, the old mask bits there are set"""
    first, s = ll.clear_smaller_script(run.name)
    h = run.stage(first)
    run.ask(h)                                                   # (the label bitmap exists and holds the first content's bits)
    for call in run.label_aware_calls(h)[2:4]:                   # (and the plain masked scans' buffers, which the dropped-state check asks for)
        call()
    h.scan_topk(run.p.metric, run.qs[0], 20)
    before = h.device_bytes()
    run.apply(h, s, "clear + smaller append")
    run.compare(h, s, "clear + smaller append", twice=True)
    after = h.device_bytes()
    # [0] the rows; [2] the working buffers - d_labels, d_label_bits and d_mask among them: nothing was freed or allocated, the
    # smaller content lives in the first content's label array and bitmaps
    assert after[0] == before[0] and after[2] == before[2], (before, after)


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_clear_then_a_larger_append_allocates_labels_and_bitmap_again(run):
    first, s = ll.clear_larger_script(run.name)
    h = run.stage(first)
    run.ask(h)
    before = h.device_bytes()
    run.apply(h, s, "clear + larger append")
    run.compare(h, s, "clear + larger append", twice=True)
    assert h.device_bytes()[2] > before[2], (before, h.device_bytes())       # the working buffers - label array and bitmaps among them - grew


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_clones_carry_labels_and_mask_and_are_independent(run):
    start = _start(run.name)
    patch, dele = ll.edit_script(run.name)[:2]
    src = run.stage(start)
    before = run.compare(src, start, "source", twice=True)
    cl = run.keep(src.clone())
    assert cl.has_labels() and cl.mask_count() == int(start.allowed.sum())
    run.same(run.ask(cl), before, "clone before any edit")
    run.apply(cl, patch, "clone patched")                        # the clone edited: patched, then rows deleted
    run.apply(cl, dele, "clone deleted")
    run.compare(cl, dele, "edited clone")
    run.same(run.ask(src), before, "source after its clone was edited")
    other = run.keep(src.clone())
    run.apply(src, patch, "source patched")                      # the source edited
    run.compare(src, patch, "edited source")
    run.same(run.ask(other), before, "clone after its source was edited")
    src.clear_labels()                                           # one side's labels cleared: the other side stays labeled
    assert not src.has_labels() and other.has_labels() and cl.has_labels()
    run.same(run.ask(other), before, "clone after its source's labels were cleared")
    other.clear_labels()
    src.set_labels(patch.labels)
    assert not other.has_labels() and src.has_labels()


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_trim_and_reserve_keep_labels_and_mask(run):
    start = _start(run.name)
    p = run.p
    h = run.keep(run.pkg.Corpus(p.vt, p.dim, capacity=4 * ll.N))
    h.append(start.rows, start.ids)
    run.label(h, start)
    rows_bytes = h.device_bytes()[0]
    h.trim()
    assert h.device_bytes()[0] < rows_bytes / 2
    got = run.compare(h, start, "after trim", twice=True)
    h.reserve(4 * ll.N)
    assert h.device_bytes()[0] >= rows_bytes
    assert h.has_labels() and h.mask_count() == int(start.allowed.sum())
    run.same(run.ask(h), got, "after reserve")


# ---------------------------------------------------------------------------------------------------- shard sets

@pytest.mark.parametrize("run", SHARDED, indirect=True)
def test_three_shards_follow_the_edit_script(run):
    """three logical shards on device 0, 64-row blocks: every state of the edit script by clear + re-append against a single corpus
    (bit for bit) and the reference, the script's append for real, then a 10-row append that reaches one shard only"""
    pkg, p = run.pkg, run.p
    start = _start(run.name)
    steps = ll.edit_script(run.name)
    sh = run.stage(start, shards=True)
    run.compare(sh, start, "shards: start")
    assert lab.error_code(pkg, lambda: sh.patch_rows(*steps[0].args)) == VG_ERR_UNSUPPORTED
    assert lab.error_code(pkg, lambda: sh.delete_rows(*steps[1].args)) == VG_ERR_UNSUPPORTED
    assert sh.has_labels() and sh.mask_count() == int(start.allowed.sum())
    for i, s in enumerate(steps[:4]):
        restaged = s._replace(op="clear_append", args=(s.rows, s.ids), dropped=True)
        run.apply(sh, restaged, "shards: state %d" % i)
        run.compare(sh, s, "shards: state %d" % i)
    run.apply(sh, steps[4], "shards: append")                    # (rows mod 64 was 63: the 100 rows reach all three shards)
    last = run.compare(sh, steps[4], "shards: append")
    clone = run.keep(sh.clone())                                 # Shards.clone carries labels and mask
    assert clone.has_labels() and clone.mask_count() == sh.mask_count()
    run.same(run.ask(clone), last, "shards: clone")
    # ten more rows fit the open block: one shard loses its labels and its mask, the others keep theirs - the set has neither
    s = steps[4]
    assert len(s.ids) % 64 + 10 <= 64
    more = lab.data(p.vt, 10, p.dim, 77)
    more_ids = np.arange(2 * 10**7, 2 * 10**7 + 10, dtype=np.int64)
    before = sh.shard_rows()
    sh.append(more, more_ids)
    assert sum(a != b for a, b in zip(before, sh.shard_rows())) == 1
    grown = s._replace(rows=np.concatenate([s.rows, more]), ids=np.concatenate([s.ids, more_ids]),
                       labels=np.concatenate([s.labels, np.full(10, ll.L_POOL, dtype=np.uint32)]),
                       allowed=np.concatenate([s.allowed, np.ones(10, dtype=bool)]))
    lib = pkg.lib()
    held = [bool(lib.vg_corpus_has_labels(lib.vg_shards_shard(sh.h, i))) for i in range(3)]
    assert sorted(held) == [False, True, True], held             # the partial drop
    run.check_dropped(sh, grown, len(s.ids), "shards: short append")
    run.label(sh, grown)
    run.compare(sh, grown, "shards: labels set again")
    run.same(run.ask(clone), last, "shards: clone after its source grew")


@pytest.mark.parametrize("run", SHARDED, indirect=True)
def test_three_shards_clear_then_a_smaller_append(run):
    first, s = ll.clear_smaller_script(run.name)
    sh = run.stage(first, shards=True)
    run.ask(sh)
    run.apply(sh, s, "shards: clear + smaller append")
    run.compare(sh, s, "shards: clear + smaller append")


@pytest.mark.parametrize("run", SHARDED, indirect=True)
def test_a_shard_without_rows_holds_labels_of_length_zero(run):
    """100 rows in 64-row blocks: the third shard is empty; the set still counts as labeled and answers like one corpus"""
    start = _start(run.name)
    s = start._replace(rows=start.rows[:100], ids=start.ids[:100], labels=start.labels[:100], allowed=start.allowed[:100])
    sh = run.stage(s, shards=True)
    assert sh.shard_rows() == [64, 36, 0] and sh.has_labels()
    one = run.stage(s)
    got = run.ask(sh)
    run.same(got, run.ask(one), "an empty shard")
    if not ll.is_float(run.p):                                   # (100 rows hold no whole ladder: only the exact paths meet the reference)
        run.check(got, s, "an empty shard")
    clone = run.keep(sh.clone())
    run.same(run.ask(clone), got, "clone of a set with an empty shard")


# ---------------------------------------------------------------------------------------------------- non-finite distances, fresh handles

def _contract(h, metric, qs, dist, labels, allowed, kms):
    """grouped and capped, single and batch, masked and not, against the contract over `dist` - exactly"""
    for k, m in kms:
        for masked in (False, True):
            al = allowed if masked else None
            bg = h.scan_topk_batch_grouped(metric, qs, k, masked=masked)
            bc = h.scan_topk_batch_capped(metric, qs, k, m, masked=masked)
            for i in range(len(qs)):
                for kind, cap, single, batch in (("grouped", 1, h.scan_topk_grouped(metric, qs[i], k, masked=masked), bg),
                                                 ("capped", m, h.scan_topk_capped(metric, qs[i], k, m, masked=masked), bc)):
                    pos = ll.answer("capped", dist[i], labels, al, k, cap)
                    ctx = (kind, masked, k, m, i)
                    for gi, gd, gl in (single, (batch[0][i, :batch[3][i]], batch[1][i, :batch[3][i]], batch[2][i, :batch[3][i]])):
                        assert gi.tolist() == (pos + 1).tolist(), (ctx, gi[:8], pos[:8] + 1)
                        assert gl.tolist() == labels[pos].tolist(), ctx
                        assert dg.same_float_bits(gd, dist[i][pos]), (ctx, gd[:6], dist[i][pos][:6])


@pytest.mark.parametrize("vt", (dg.F32, dg.F16), ids=("f32", "f16"))
def test_non_finite_rows_on_fresh_handles(pkg, orc, vt):
    """small integer values (every dot product is exact in float32): the oracle's distances are the handle's, bit for bit, ties and
    all.  DOT: a label only a NaN row and a +Inf row hold is absent (counts drop), a label whose scan-first row is NaN is represented
    by its best finite row, a -Inf row comes first - and enters a label that is already full at m like any better row.  Cosine: two
    zero-norm rows (distance exactly 1.0) tie by position."""
    n, dim, nq = 1003, 384, 5
    rng = np.random.default_rng(8100 + vt)
    x = rng.integers(-2, 2, (n, dim)).astype(np.float32)
    q = rng.integers(-2, 2, (nq, dim)).astype(np.float32)
    q[:, 3] = 1.0                                                # the coordinate the Inf elements sit at: no 0 * Inf
    labels = rng.integers(0, 30, n).astype(np.uint32)
    labels[rng.random(n) < 0.1] = ll.NONE
    allowed = rng.random(n) < 0.7
    nan_only, inf_only, nan_first, best, neg_inf = 5, 800, 2, 650, 990
    x[nan_only, 7] = np.nan
    x[inf_only, 3] = -np.inf                                     # dot = -Inf: distance +Inf
    labels[[nan_only, inf_only]] = 900                           # f32: a label only non-finite rows hold (f16 skips a NaN lane)
    inf_pair = [300, 901]
    x[inf_pair, 3] = -np.inf
    labels[inf_pair] = 905                                       # both types: a label only +Inf rows hold
    x[nan_first, 9] = np.nan
    x[best] = 3.0 * q[0]
    labels[[nan_first, best]] = 901                              # its scan-first row is NaN, its best row finite
    full = [20, 21, 22, 23]                                      # four good rows of label 902 in front, the -Inf row far behind them
    for j, pos in enumerate(full):
        x[pos] = (2.0 if j < 3 else 1.0) * q[0]
    x[neg_inf, 3] = np.inf                                       # dot = +Inf: distance -Inf
    labels[full + [neg_inf]] = 902
    allowed[[nan_only, inf_only, nan_first, best, neg_inf] + full + inf_pair] = True
    zeros = [10, 700]
    x[zeros] = 0.0
    labels[zeros] = (903, 904)
    allowed[zeros] = True
    rows, qs = dg.to_storage(vt, x), dg.to_storage(vt, q)
    h = pkg.Corpus(vt, dim)
    h.append(rows)
    h.set_labels(labels)
    h.set_mask(bits=allowed)
    dist = [orc.scan_distances(orc.AVX2, dg.DOT, vt, qs[i], rows) for i in range(nq)]
    for i in range(nq):
        assert dg.same_float_bits(h.scan_distances(dg.DOT, qs[i]), dist[i]), i
        assert dist[i][neg_inf] == -np.inf and dist[i][inf_only] == np.inf and (dist[i][inf_pair] == np.inf).all()
    kms = ((20, 3), (64, 5), (20, 1))
    _contract(h, dg.DOT, qs, dist, labels, allowed, kms)
    for masked in (False, True):
        ids, d, gl = h.scan_topk_capped(dg.DOT, qs[0], 64, 3, masked=masked)
        assert ids[0] == neg_inf + 1 and d[0] == -np.inf and gl[0] == 902      # -Inf first, inside a label that four finite rows fill
        assert sorted(ids[gl == 902].tolist()) == [21, 22, neg_inf + 1]        # ... it replaced the worst kept row, like any better row
        assert best + 1 in ids and (vt != dg.F32 or nan_first + 1 not in ids)
        if vt == dg.F32:                                        # (f16 kernels skip a NaN lane: that row is an ordinary row there)
            assert np.isnan(dist[0][nan_only]) and np.isnan(dist[0][nan_first])
            assert 900 not in gl.tolist()
        ids, d, gl = h.scan_topk_grouped(dg.DOT, qs[0], 64, masked=masked)
        present = np.unique(labels[(allowed | (not masked)) & (labels != ll.NONE) & (dist[0] < np.inf)])
        assert len(ids) == len(present) and sorted(gl.tolist()) == present.tolist()      # counts drop with the labels that are gone
        assert ids[0] == neg_inf + 1 and (vt != dg.F32 or 900 not in gl.tolist())
    # the labels that only rows outside every list hold: absent from single, batch and masked answers, the count lower by them
    gone = [905, 900] if vt == dg.F32 else [905]
    for masked in (False, True):
        carried = np.unique(labels[(allowed | (not masked)) & (labels != ll.NONE)])
        assert set(gone) <= set(carried.tolist())
        bg = h.scan_topk_batch_grouped(dg.DOT, qs, 64, masked=masked)
        bc = h.scan_topk_batch_capped(dg.DOT, qs, 64, 5, masked=masked)
        for i in range(nq):
            sg = h.scan_topk_grouped(dg.DOT, qs[i], 64, masked=masked)
            sc = h.scan_topk_capped(dg.DOT, qs[i], 64, 5, masked=masked)
            assert len(sg[0]) == bg[3][i] == len(carried) - len(gone), (masked, i, len(sg[0]), bg[3][i], len(carried))
            for gl in (sg[2], sc[2], bg[2][i, :bg[3][i]], bc[2][i, :bc[3][i]]):
                assert not set(gone) & set(gl.tolist()), (masked, i)
            for ids in (sg[0], sc[0], bg[0][i, :bg[3][i]], bc[0][i, :bc[3][i]]):
                assert not set(p + 1 for p in inf_pair + [inf_only]) & set(ids.tolist()), (masked, i)
    # cosine: the handle's own floats (1 - dot / norms rounds as the kernel rounds), the zero-norm rows at exactly 1.0
    own = [h.scan_distances(dg.COSINE, qs[i]) for i in range(nq)]
    for i in range(nq):
        assert own[i][zeros[0]] == np.float32(1.0) == own[i][zeros[1]]
        _check_float_distances(own[i], orc.scan_distances(orc.AVX2, dg.COSINE, vt, qs[i], rows), vt, dg.COSINE, qs[i], rows)
    _contract(h, dg.COSINE, qs, own, labels, allowed, kms)
    ids, d, gl = h.scan_topk_grouped(dg.COSINE, qs[1], 64)
    at = {int(l): j for j, l in enumerate(gl)}
    assert at[903] < at[904] and ids[at[903]] == 11 and ids[at[904]] == 701 and d[at[903]] == d[at[904]] == 1.0
    h.close()
