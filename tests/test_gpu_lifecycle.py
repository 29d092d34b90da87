"""Edited, cleared, cloned, trimmed and re-reserved corpora against the rows they hold, on every path that reads a derived per-row
copy (norms, row sums and the sign-flipped copy, tile-major copies, the bf16 / int8 / high-nibble shadow copies with their statistics).

The rule of every case: after any lifecycle call a handle answers (a) bit for bit like a handle freshly staged from the surviving
rows on the same path - two fresh handles are compared first, so that bit equality is known to be a fair bar there - and (b) correctly
against a reference that is not the GPU: the oracle's distances and ordered top-k for single scans (floats within the bar of
test_gpu_scan._check_float_distances, uint8 / int8 bit for bit), batch_reference.check_batch - the float64 ranking over all rows - for
batches.  Every case forces its path with environment switches and proves through the handle's diagnostics that the path ran; a case that
cannot prove its path fails.  The scripts are tests/lifecycle_cases.py (checked without a device by tests/test_lifecycle_cases.py)."""
import numpy as np
import pytest

import batch_reference as br
import datagen as dg
import lifecycle_cases as lc
from test_gpu_scan import pkg, _check_float_distances, REL_TOL, _abs_scale          # noqa: F401  (pkg: the module-scoped fixture)

pytestmark = pytest.mark.gpu

ALL = [p.name for p in lc.PATHS]
SCAN_QUERIES = (0, 1, 2)


class Runner:
    """one path of the matrix: makes handles on it, asks them, proves the path, compares answers"""

    def __init__(self, pkg, orc, monkeypatch, name):
        self.pkg, self.orc, self.p, self.w = pkg, orc, lc.PATH_BY_NAME[name], lc.world(name)
        for k in lc.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in self.p.env.items():
            monkeypatch.setenv(k, v)
        pkg.reload_switches()
        self.handles = []

    def make(self, rows, ids, capacity=0):
        c = self.pkg.Corpus(self.p.vt, self.p.dim, capacity=capacity)
        self.handles.append(c)
        if len(rows):
            c.append(rows[:len(rows) // 3], ids[:len(rows) // 3])              # (two appends: the second one extends)
            c.append(rows[len(rows) // 3:], ids[len(rows) // 3:])
        if self.p.scan_filter is not None:
            c.set_scan_filter(self.p.scan_filter)
        return c

    def close(self):
        for c in self.handles:
            c.close()

    def _prove_scan(self, c, evals):
        name = c.kernel_name(self.p.metric)
        assert name.startswith("scan_filter_" + dg.TYPE_NAMES[self.p.vt]) and evals > 0, (self.p.name, name, evals)
        if self.p.proof == "n4":
            assert "_n4_" in name, name
        else:
            assert (("_q8_" in name) == (self.p.env["VG_SCAN_FILTER_SHADOW"] == "int8")), name

    def _prove_batch(self, c):
        assert c.last_batch_path() == self.p.proof, (self.p.name, c.last_batch_path(), c.batch_q8_status())
        if self.p.proof == 7:
            assert c.batch_q8_status() == 0, c.batch_q8_status()

    def warm(self, c):
        """builds the path's derived data over the handle's rows as they are (a small run: rows no bound can judge stay few pairs)"""
        if self.p.kind == "scan":
            c.filter_exact_evals()
            c.scan_topk(self.p.metric, self.w.qs[3], lc.K)
            self._prove_scan(c, c.filter_exact_evals())
        else:
            c.scan_topk_batch(self.p.metric, self.w.qs[:4], lc.K)
            self._prove_batch(c)

    def ask(self, c, ragged=False):
        nq, k = (7, 1) if ragged else (lc.NQ, lc.K)
        if self.p.kind == "scan":
            c.filter_exact_evals()
            out = [c.scan_topk(self.p.metric, self.w.qs[i], k) for i in SCAN_QUERIES]
            self._prove_scan(c, c.filter_exact_evals())
            return out
        out = c.scan_topk_batch(self.p.metric, self.w.qs[:nq], k)
        self._prove_batch(c)
        return out

    def same(self, a, b, what):
        if self.p.kind == "scan":
            for i, ((ai, ad), (bi, bd)) in enumerate(zip(a, b)):
                assert ai.tolist() == bi.tolist() and dg.same_float_bits(ad, bd), (self.p.name, what, i, ai[:5], bi[:5], ad[:5], bd[:5])
            return
        (ai, ad, ac), (bi, bd, bc) = a, b
        assert np.array_equal(ac, bc), (self.p.name, what, "counts", np.nonzero(ac != bc)[0][:5])
        for i in range(len(ac)):
            m = ac[i]
            assert ai[i][:m].tolist() == bi[i][:m].tolist() and dg.same_float_bits(ad[i][:m], bd[i][:m]), \
                (self.p.name, what, i, ai[i][:5], bi[i][:5], ad[i][:5], bd[i][:5])

    def check(self, ans, rows, ids, dups, ragged=False):
        """against the oracle (single scans) / the float64 ranking over all rows (batches)"""
        p, orc = self.p, self.orc
        nq, k = (7, 1) if ragged else (lc.NQ, lc.K)
        if p.kind == "scan":
            for (got_ids, got_d), qi in zip(ans, SCAN_QUERIES):
                check_scan(orc, p.vt, p.metric, self.w.qs[qi], rows, ids, got_ids, got_d, k)
            return
        got_ids, got_d, cnt = ans
        pos1 = np.zeros_like(got_ids)
        for i in range(nq):
            m = cnt[i]
            at = np.searchsorted(ids, got_ids[i][:m])
            assert (at < len(ids)).all() and (ids[at] == got_ids[i][:m]).all(), (p.name, "rowids the corpus does not hold", i)
            pos1[i][:m] = at + 1
        banded = br.check_batch(p.vt, p.metric, k, self.w.qs[:nq], rows, pos1, got_d, cnt, orc, duplicates=dups)
        assert banded <= br.BAND_SHARE_CAP * nq, (p.name, banded)

    def compare(self, c, step, what, twice=False, ragged=False):
        """the handle against a fresh staging of step's rows (and, twice = True, two fresh stagings against each other first)"""
        fresh = self.make(step.rows, step.ids)
        want = self.ask(fresh, ragged)
        if twice:
            again = self.make(step.rows, step.ids)
            self.same(self.ask(again, ragged), want, what + ": two fresh handles")
            again.close()
        got = self.ask(c, ragged)
        self.same(got, want, what)
        self.check(got, step.rows, step.ids, step.dups, ragged)
        assert c.rows == len(step.ids) and c.find_rowid(int(step.ids[len(step.ids) // 2])) == len(step.ids) // 2
        assert c.find_rowid(int(step.ids[-1]) + 1) == -1
        fresh.close()

    def apply(self, c, step):
        if step.op == "patch":
            c.patch_rows(*step.args)
        elif step.op == "delete":
            c.delete_rows(*step.args)
        elif step.op == "append":
            c.append(*step.args)
        elif step.op == "clear_append":
            c.clear()
            assert c.rows == 0
            c.append(*step.args)
        if step.warm:
            self.warm(c)


def check_scan(orc, vt, metric, q, rows, ids, got_ids, got_d, k):
    """one single-scan answer against orc.scan_distances + orc.topk_ordered over the rows the handle should hold"""
    want = orc.scan_distances(orc.AVX2, metric, vt, q, rows)
    oids, odist, opos = orc.topk_ordered(want, ids, k)
    assert len(got_ids) == len(oids), (len(got_ids), len(oids))
    if vt in (dg.U8, dg.I8):
        assert got_ids.tolist() == oids.tolist() and dg.same_float_bits(got_d, odist), (got_ids[:5], oids[:5], got_d[:5], odist[:5])
        return
    at = np.searchsorted(ids, got_ids)
    assert (at < len(ids)).all() and (ids[at] == got_ids).all() and len(set(at.tolist())) == len(at)
    _check_float_distances(got_d.astype(np.float32), want[at], vt, metric, q, rows[at])
    assert (np.diff(got_d) >= 0).all()
    # the same rows in the same places, except where the oracle's own distances lie within the distance bar of each other
    for j in np.nonzero(got_ids != oids)[0]:
        tol = REL_TOL * abs(float(odist[j])) + (REL_TOL * float(_abs_scale(vt, metric, q, rows[at[j]:at[j] + 1])[0]) if metric in (dg.DOT, dg.COSINE) else 0.0)
        assert abs(float(want[at[j]]) - float(odist[j])) <= 2 * tol, (j, got_ids[j], oids[j], want[at[j]], odist[j])


@pytest.fixture
def run(pkg, orc, monkeypatch, request):
    r = Runner(pkg, orc, monkeypatch, request.param)
    yield r
    r.close()


# ---------------------------------------------------------------------------------------------------- the scripts over the path matrix

@pytest.mark.parametrize("run", ALL, indirect=True)
def test_patch_delete_append_equal_a_fresh_corpus(run):
    """script 1-3: 300 scattered rows overwritten (first, last, five copies of a query, NaN / Inf / zero rows), three deletions (front
    run, 200 singles, end run; rows mod 32 -> 0, 1, 31; the first drops 70+ rows of NaN / Inf / 1e18 from the end, so that two whole
    tiles of derived data lie stale behind the new end), then 100 appended rows with a new best row.  The derived data exists - and is
    stale - before every call."""
    steps = lc.edit_script(run.p.name)
    c = run.make(run.w.rows, run.w.ids)
    run.warm(c)
    for i, step in enumerate(steps):
        run.apply(c, step)
        if step.rows is not None:
            run.compare(c, step, "step %d (%s)" % (i, step.op), twice=(i == 0))
    if run.p.kind == "batch":
        run.compare(c, steps[-1], "ragged batch", ragged=True)
        best = c.scan_topk_batch(run.p.metric, run.w.qs[:2], 1)[0]
        assert best[1][0] == 10**7 + 37


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_clear_then_a_smaller_append_equals_a_fresh_corpus(run):
    """script 4: about half as many, different rows after vg_corpus_clear - every derived copy holds the old rows (NaN / Inf / huge ones
    first) behind the new end"""
    create, again = lc.clear_script(run.p.name)
    p = run.p
    c = run.make(*create.args)
    run.warm(c)
    bytes_before = c.device_bytes()
    run.apply(c, again)
    run.compare(c, again, "clear + smaller append", twice=True)
    assert c.device_bytes()[0] == bytes_before[0]                           # (clear keeps the allocation: the old rows ARE behind the end)
    if p.kind == "batch":
        run.compare(c, again, "ragged batch", ragged=True)


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_clones_are_independent_and_carry_rowids_and_switches(run):
    """script 5: a clone made before / after the derived data exists; then the clone edited (the source answers as before, bit for bit)
    and the source edited (the clone answers as before).  Rowids, tie order and scan-filter mode travel; find_rowid works."""
    p, w = run.p, run.w
    patch = lc.edit_script(p.name)[0]
    start = lc.Step("create", (), w.rows, w.ids, (), False)
    src = run.make(w.rows, w.ids)
    early = src.clone()                                                     # before any derived data exists
    run.handles.append(early)
    run.compare(early, start, "clone before derived data", twice=True)
    before = run.ask(src)
    late = src.clone()                                                      # after it exists
    run.handles.append(late)
    run.same(run.ask(late), before, "clone after derived data")
    for cl in (early, late):
        assert cl.rows == p.n and cl.find_rowid(int(w.ids[1234])) == 1234 and cl.find_rowid(11) == -1
        assert run.pkg.lib().vg_corpus_tie_order(cl.h) == run.pkg.TIE_POSITION
    # the clone edited: the source still answers as before
    run.apply(late, patch)
    run.compare(late, patch, "edited clone")
    run.same(run.ask(src), before, "source after its clone was edited")
    # the source edited: the other clone still answers as before
    run.apply(src, patch)
    run.compare(src, patch, "edited source")
    run.same(run.ask(early), before, "clone after its source was edited")
    # tie order and an explicit scan-filter mode travel with a clone
    src.set_tie_order(run.pkg.TIE_REFERENCE)
    src.set_scan_filter(0)
    third = src.clone()
    run.handles.append(third)
    assert run.pkg.lib().vg_corpus_tie_order(third.h) == run.pkg.TIE_REFERENCE
    if p.kind == "scan":
        assert not third.kernel_name(p.metric).startswith("scan_filter"), third.kernel_name(p.metric)
        third.set_scan_filter(1)
        assert third.kernel_name(p.metric).startswith("scan_filter")


@pytest.mark.parametrize("run", ALL, indirect=True)
def test_trim_and_reserve_keep_the_answers(run):
    """script 6: a corpus created far too large, its derived data built (sized by the capacity), trimmed, asked, re-reserved far too
    large, appended to, asked"""
    p, w = run.p, run.w
    start = lc.Step("create", (), w.rows, w.ids, (), False)
    grown = lc.edit_script(p.name)[-1]
    more, more_ids = grown.args
    c = run.make(w.rows, w.ids, capacity=4 * p.n)
    run.warm(c)
    rows_bytes = c.device_bytes()[0]
    c.trim()
    assert c.device_bytes()[0] < rows_bytes / 2, (rows_bytes, c.device_bytes())
    run.compare(c, start, "after trim", twice=True)
    c.reserve(4 * p.n)
    assert c.device_bytes()[0] >= rows_bytes
    run.same(run.ask(c), run.ask(run.make(w.rows, w.ids)), "after reserve")
    c.append(more, more_ids)
    after = lc.Step("append", (), np.concatenate([w.rows, more]), np.concatenate([w.ids, more_ids]), (), False)
    run.compare(c, after, "after reserve + append")
    c.trim()                                                                # (within 25 %: a no-op or not, the answers stay)
    run.compare(c, after, "after the second trim")


def test_nibble_probe_looks_again_after_clear(pkg, orc, monkeypatch):
    """default mode (no scan_filter = 1): a uint8 corpus whose first content the probe found unselective (rows that differ in their low
    nibbles only: one bound for all of them) is cleared and refilled with clustered bytes - the probe must run again and switch the
    filter on; answers equal the oracle's throughout"""
    for k in lc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VG_SCAN_FILTER_MIN_MB", "0")
    pkg.reload_switches()
    dim, n1, n2 = 64, 700_001, (1 << 20) + 333
    rng = np.random.default_rng(5900)
    base = rng.integers(0, 16, dim) * 16
    flat = (base[None, :] + rng.integers(0, 16, (n1, dim))).astype(np.uint8)
    centres = rng.standard_normal((400, dim)).astype(np.float32)
    x = centres[rng.integers(0, 400, n2)] + np.float32(0.05) * rng.standard_normal((n2, dim), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    clustered = np.clip(np.rint((x - x.min()) * (255.0 / (x.max() - x.min()))), 0, 255).astype(np.uint8)
    c = pkg.Corpus(pkg.U8, dim)
    c.append(flat)
    q = flat[77].copy()
    got = c.scan_topk(dg.L2, q, 20)
    check_scan(orc, dg.U8, dg.L2, q, flat, np.arange(1, n1 + 1), got[0], got[1], 20)
    assert c.filter_exact_evals() > 0 and not c.kernel_name(dg.L2).startswith("scan_filter"), c.kernel_name(dg.L2)   # probed: not selective
    c.clear()
    c.append(clustered)
    q = clustered[n2 - 77].copy()
    c.filter_exact_evals()
    got = c.scan_topk(dg.L2, q, 20)
    check_scan(orc, dg.U8, dg.L2, q, clustered, np.arange(1, n2 + 1), got[0], got[1], 20)
    assert c.filter_exact_evals() > 0 and c.kernel_name(dg.L2).startswith("scan_filter_u8"), c.kernel_name(dg.L2)   # probed again: selective
    got = c.scan_topk(dg.L2, clustered[5].copy(), 20)
    check_scan(orc, dg.U8, dg.L2, clustered[5].copy(), clustered, np.arange(1, n2 + 1), got[0], got[1], 20)
    assert c.filter_exact_evals() > 0
    c.close()


# ---------------------------------------------------------------------------------------------------- other scan forms after an edit

FORMS = ("scan_q8_f32", "scan_n4_u8")


def _edited(run, upto=3):
    """a handle with derived data that went through the patch and the first deletion: (handle, the state it should hold)"""
    steps = lc.edit_script(run.p.name)[:upto]
    c = run.make(run.w.rows, run.w.ids)
    run.warm(c)
    for s in steps:
        run.apply(c, s)
    return c, steps[-1]


@pytest.mark.parametrize("run", FORMS, indirect=True)
def test_scan_distances_after_an_edit(run):
    c, st = _edited(run)
    p, q = run.p, run.w.qs[0]
    for metric in (dg.L2, dg.COSINE, dg.DOT):
        got = c.scan_distances(metric, q)
        want = run.orc.scan_distances(run.orc.AVX2, metric, p.vt, q, st.rows)
        if p.vt == dg.F32:
            _check_float_distances(got, want, p.vt, metric, q, st.rows)
        else:
            assert dg.same_float_bits(got, want), metric


@pytest.mark.parametrize("run", FORMS, indirect=True)
def test_scan_within_after_an_edit(run):
    """about 50 rows within the radius (chosen in a gap of the oracle's distances): membership and order before and after the edit; the
    result held before the edit is gone after it"""
    p, w, orc = run.p, run.w, run.orc
    q = w.qs[1]
    c = run.make(w.rows, w.ids)
    run.warm(c)

    def within(rows, ids):
        want = orc.scan_distances(orc.AVX2, p.metric, p.vt, q, rows)
        r, gap = lc.within_radius(want)
        assert gap > 4 * REL_TOL * abs(r) or p.vt != dg.F32, (r, gap)
        got_ids, got_d, matches = c.scan_within(p.metric, q, r)
        inside = np.nonzero(want <= np.float32(r))[0]
        order = inside[np.lexsort((inside, want[inside]))]
        assert matches == len(order) == len(got_ids) and 40 <= matches <= 60, (matches, len(order))
        if p.vt == dg.F32:
            assert sorted(got_ids.tolist()) == sorted(ids[order].tolist())
            at = np.searchsorted(ids, got_ids)
            _check_float_distances(got_d.astype(np.float32), want[at], p.vt, p.metric, q, rows[at])
            assert (np.diff(got_d) >= 0).all()
        else:
            assert got_ids.tolist() == ids[order].tolist() and dg.same_float_bits(got_d, want[order])
        return matches

    held = within(w.rows, w.ids)
    one = np.zeros(1, dtype=np.int64)
    assert pkg_fetch(run.pkg, c, held - 1, one) == 0
    for s in lc.edit_script(p.name)[:3]:
        run.apply(c, s)
        assert pkg_fetch(run.pkg, c, 0, one) != 0, s.op                   # (names positions of the rows as they were)
        if s.rows is not None:
            within(s.rows, s.ids)


def pkg_fetch(pkg, c, first, one):
    return pkg.lib().vg_scan_within_fetch(c.h, first, 1, one.ctypes.data, None)


@pytest.mark.parametrize("run", FORMS, indirect=True)
def test_masked_scan_after_patch_keeps_the_mask_and_after_delete_has_none(run):
    p, w, orc = run.p, run.w, run.orc
    patch, _, dele = lc.edit_script(p.name)[:3]
    c = run.make(w.rows, w.ids)
    run.warm(c)
    allowed = np.arange(0, p.n, 3)
    assert c.set_mask(positions=allowed) == len(allowed)
    q = w.qs[0]

    def masked(rows, ids):
        got_ids, got_d = c.scan_topk_masked(p.metric, q, lc.K)
        check_scan(orc, p.vt, p.metric, q, rows[allowed], ids[allowed], got_ids, got_d, lc.K)

    masked(w.rows, w.ids)
    run.apply(c, patch)
    assert c.mask_count() == len(allowed)
    masked(patch.rows, patch.ids)
    run.apply(c, dele)
    assert c.mask_count() == -1
    with pytest.raises(run.pkg.VectorGpuError):
        c.scan_topk_masked(p.metric, q, lc.K)
    with pytest.raises(run.pkg.VectorGpuError):                             # error cases by return code only
        c.patch_rows(np.array([c.rows], dtype=np.int64), w.rows[:1])
    with pytest.raises(run.pkg.VectorGpuError):
        c.delete_rows(np.array([5, 5], dtype=np.int64))


@pytest.mark.parametrize("run", FORMS, indirect=True)
def test_large_k_select_buffers_sized_before_the_edit(run):
    """k = 100 (radix select over all distances): the selection buffers were sized for the rows held before rows left and arrived"""
    p, w, orc = run.p, run.w, run.orc
    c = run.make(w.rows, w.ids)
    q = w.qs[2]
    c.scan_topk(p.metric, q, 100)
    steps = lc.edit_script(p.name)
    for s in steps:
        run.apply(c, s)
    big = dg.corpus(p.vt, 5000, p.dim, 5950)
    big_ids = np.arange(2 * 10**7, 2 * 10**7 + 5000, dtype=np.int64)
    c.append(big, big_ids)                                                  # (more rows than the buffers were made for)
    rows, ids = np.concatenate([steps[-1].rows, big]), np.concatenate([steps[-1].ids, big_ids])
    got_ids, got_d = c.scan_topk(p.metric, q, 100)
    check_scan(orc, p.vt, p.metric, q, rows, ids, got_ids, got_d, 100)
    fresh = run.make(rows, ids)
    f_ids, f_d = fresh.scan_topk(p.metric, q, 100)
    assert got_ids.tolist() == f_ids.tolist() and dg.same_float_bits(got_d, f_d)


def test_reference_tie_order_after_an_edit(pkg, orc, monkeypatch):
    """tie_order = reference on a tie-heavy uint8 corpus of 140 000 rows (the prefix pass and the candidate emission run): after a
    patch and a deletion the rows and their order are the reference's slot algorithm's over the surviving rows"""
    for k in lc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    pkg.reload_switches()
    n, dim = 140_000, 16
    rows = dg.corpus(dg.U8, n, dim, 5960, low_entropy=True)
    ids = lc.make_ids(n)
    qs = [dg.query(dg.U8, dim, 5961 + i, low_entropy=True) for i in range(3)]
    c = pkg.Corpus(pkg.U8, dim)
    c.append(rows, ids)
    c.set_tie_order(pkg.TIE_REFERENCE)

    def ask(rows, ids, handle):
        for q in qs:
            for metric in (dg.L2, dg.DOT):
                want = orc.scan_distances(orc.AVX2, metric, dg.U8, q, rows)
                rids, rdist = orc.topk_reference(want, ids, lc.K)
                got_ids, got_d = handle.scan_topk(metric, q, lc.K)
                assert got_ids.tolist() == rids.tolist() and dg.same_float_bits(got_d, rdist), (metric, got_ids[:6], rids[:6])

    ask(rows, ids, c)
    m, rng = lc.Model(rows, ids), np.random.default_rng(5962)
    pos = rng.permutation(n)[:300]
    c.patch_rows(*m.patch(pos, dg.corpus(dg.U8, 300, dim, 5963, low_entropy=True)).args)
    ask(m.rows, m.ids, c)
    dele, _ = lc._delete_positions(n, 70, 1, rng)
    c.delete_rows(*m.delete(dele).args)
    assert c.rows >= (1 << 17)
    before = c.tie_stats()
    ask(m.rows, m.ids, c)
    after = c.tie_stats()
    assert after["with_a_tie_among_the_k_plus_1_best"] > before["with_a_tie_among_the_k_plus_1_best"]
    assert after["fused_replays"] > before["fused_replays"] and after["store_mode_replays"] == before["store_mode_replays"], (before, after)
    clone = c.clone()
    ask(m.rows, m.ids, clone)                                               # (the tie order travels with a clone)
    clone.close()
    c.close()


# ---------------------------------------------------------------------------------------------------- shard sets

@pytest.mark.parametrize("vt,dim,metric", ((dg.F32, 100, dg.L2), (dg.U8, 33, dg.L2)))
def test_shards_clear_reappend_and_clone_equal_a_single_corpus(pkg, orc, monkeypatch, vt, dim, metric):
    """three logical shards on device 0, 257-row blocks: clear + a smaller, different re-append, and a clone of the set, against one
    fresh corpus and the oracle"""
    for k in lc.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    pkg.reload_switches()
    n1, n2 = 9_003, 4_503
    first, second = dg.corpus(vt, n1, dim, 5970 + dim), dg.corpus(vt, n2, dim, 5971 + dim)
    ids1, ids2 = lc.make_ids(n1), lc.make_ids(n2, 5, 2)
    qs = dg.corpus(vt, lc.NQ, dim, 5972 + dim)
    second[n2 - 1] = qs[1]
    sh = pkg.Shards(vt, dim, [0, 0, 0], block_rows=257)
    sh.append(first, ids1)
    sh.scan_topk(metric, qs[0], lc.K)
    sh.scan_topk_batch(metric, qs, lc.K)                                     # derived data in every shard
    sh.clear()
    assert sh.rows == 0
    sh.append(second, ids2)
    single = pkg.Corpus(vt, dim)
    single.append(second, ids2)
    clone = sh.clone()

    def ask(h):
        assert h.rows == n2 and h.rowids(n2 - 3, 3).tolist() == ids2[-3:].tolist()
        for i in (0, 1, 2):
            got_ids, got_d = h.scan_topk(metric, qs[i], lc.K)
            s_ids, s_d = single.scan_topk(metric, qs[i], lc.K)
            assert got_ids.tolist() == s_ids.tolist() and dg.same_float_bits(got_d, s_d), i
            check_scan(orc, vt, metric, qs[i], second, ids2, got_ids, got_d, lc.K)
        assert h.scan_topk(metric, qs[1], 1)[0][0] == ids2[-1]
        b_ids, b_d, b_cnt = h.scan_topk_batch(metric, qs, lc.K)
        s_ids, s_d, s_cnt = single.scan_topk_batch(metric, qs, lc.K)
        assert np.array_equal(b_cnt, s_cnt) and np.array_equal(b_ids, s_ids) and dg.same_float_bits(b_d, s_d)
        pos1 = np.searchsorted(ids2, b_ids) + 1
        assert br.check_batch(vt, metric, lc.K, qs, second, pos1, b_d, b_cnt, orc) <= br.BAND_SHARE_CAP * lc.NQ

    ask(sh)
    ask(clone)
    sh.clear()                                                               # the clone owns its rows
    ask(clone)
    sh.trim()
    for h in (sh, clone, single):
        h.close()


@pytest.mark.parametrize("name", ("scan_q8_f32", "batch_i8_u8"))
def test_one_shard_handle_forwards_row_maintenance(pkg, orc, monkeypatch, name):
    r = Runner(pkg, orc, monkeypatch, name)
    p, w = r.p, r.w
    sh = pkg.Shards(p.vt, p.dim, [0])
    sh.append(w.rows, w.ids)
    if p.scan_filter is not None:
        sh.set_scan_filter(p.scan_filter)
    sh.scan_topk(p.metric, w.qs[0], lc.K)
    sh.scan_topk_batch(p.metric, w.qs, lc.K)
    assert sh.find_rowid(int(w.ids[4321])) == 4321 and sh.find_rowid(11) == -1
    for s in lc.edit_script(name)[:3]:
        if s.op == "patch":
            sh.patch_rows(*s.args)
        else:
            sh.delete_rows(*s.args)
        if s.rows is None:
            continue
        assert sh.rows == len(s.ids) and sh.find_rowid(int(s.ids[-1])) == len(s.ids) - 1
        fresh = r.make(s.rows, s.ids)
        for i in SCAN_QUERIES:
            got_ids, got_d = sh.scan_topk(p.metric, w.qs[i], lc.K)
            f_ids, f_d = fresh.scan_topk(p.metric, w.qs[i], lc.K)
            assert got_ids.tolist() == f_ids.tolist() and dg.same_float_bits(got_d, f_d), (s.op, i)
            check_scan(orc, p.vt, p.metric, w.qs[i], s.rows, s.ids, got_ids, got_d, lc.K)
        a, b = sh.scan_topk_batch(p.metric, w.qs, lc.K), fresh.scan_topk_batch(p.metric, w.qs, lc.K)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and dg.same_float_bits(a[1], b[1]), s.op
    with pytest.raises(pkg.VectorGpuError):
        pkg.Shards(p.vt, p.dim, [0, 0]).patch_rows(np.array([0], dtype=np.int64), w.rows[:1])
    sh.close()
    r.close()
