"""Every form of the f16 / bf16 / f32-behind-bf16 matrix-core batch filter (vg_batch_h.hip) against a float64 reference over ALL rows, every
query of every batch (tests/batch_reference.py) - not against the single-query scan, which shares its accumulators and the cached row norms,
and not one form against another, which share one filter.

Each case asserts that the batch took this kernel (last_batch_path() == 3) and that vg_batch_h_plan gives the workgroup form the case is
meant for (expected_form restates the rule), so a routing change cannot empty the matrix.  The worlds and what is planted in them:
tests/batch_half_cases.py.  The cells and the fully checked cases that reach them - 20 003 rows unless said otherwise:

  k-steps (NTB)  row bytes    workgroup form                type / dim                                  cases
  8              <= 256       8 waves; 2 x 4 (nq > 128)     f16, bf16 100; f32 100 (shadow 208 B)       3 batch sizes, 4 metrics at k 20, k 1 / 27 / 32
  16             <= 512       8 waves; 2 x 4 (nq > 128)     f16, bf16 256; f32 192                      the same
  24             <= 768       8 waves; 2 x 4 (nq > 128,     f16, bf16, f32 384                          nq 1, 31, 32, 33, 128, 129, 257 x 4 metrics at k 20,
                              k <= 27); 8 waves at k 32                                                 k 1 / 27 / 32 under two metrics each
  32             <= 1024      8 waves                       f16, bf16, f32 500                          3 batch sizes, 4 metrics at k 20, k 1 / 27 / 32
  48             <= 1536      4 waves (long form)           f16, bf16 768; f32 600 (VG_BATCH_LONG=0)    the same
  64             <= 2048      4 waves (long form), k <= 29  f16, bf16, f32 1000 (VG_BATCH_LONG=0)       the same; k = 32: NOT this kernel - one scan per query
                                                                                                        (path 6: f16, bf16) or the multi-query scan (path 5:
                                                                                                        f32) answers, and is checked the same way

  forms  VG_BATCH_H_WAVES=8, =4, VG_BATCH_TILE_MAJOR=0: x 4 metrics x k 1 / 20 / 27 / 32 at dim 384 (every type; no dot at k = 1, see
         batch_half_cases.K_PAIRS); one metric and k per form on every other cell
  split  VG_BATCH_H_SPLIT=1 (the filter kernel with its ring of 6 / 5 / 4 / 3 / 2 tile buffers + vg_batch_hx_kernel).  Without a pre-pass
         every real pair passes, and a pair region runs over - the fused kernel answers, silently - once a wavefront of 32 queries meets a
         third tile in one partition (see batch_half_cases.FORMS).  Where it does answer, each case asserting so (batch_half_split_off):
           the sparse world, one query group (nq 129; 128 in the 4-wavefront long form): f16, bf16, f32 x all six buckets, plan (8, 1) or
             (4, 1); x 4 metrics x k 1 / 20 / 27 / 32 at dim 384, one metric and k elsewhere
           every tiny world; one query over the small world at dims 384 and 1000 (96 pairs a region)
           the staged world behind its pre-pass (three cases)
         and one case shows the hand-over to the fused kernel: 257 queries over the small world (5 tiles a partition)
  tiny   20 and 33 rows (less than a tile, a tile and a row): counts = min(k, rows that can enter), k 1 / 20 / 32
  sparse 8 259 rows = 259 tiles over 256 partitions: partitions of two tiles, one tile and none
  staged 2 097 187 x 16 bf16 (65 538 tiles: the BOUNDK pre-pass and the staged real passes), nq 40 (growth x 4) and 160 (two query groups:
         doubling), VG_BATCH_STAGES default / 0 / 200, L2 and dot; the duplicate ladder comes back in position order
  append 500 rows behind a checked batch (norms, shadow copy, tile-major copy are extended), then a fresh reference over all rows
  unjudgeable queries (zero, NaN, Inf) in slots 1, 31, 32 of 129
  dot at k = 1: f32 100 and 384, the ~64 queries that have no row at -Inf (half-precision worlds have none: not covered)"""
import numpy as np
import pytest

import datagen as dg
import batch_reference as br
import batch_half_cases as bh
from test_gpu_scan import pkg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

FORM_ENV = {"default": {}, "waves8": {"VG_BATCH_H_WAVES": "8"}, "waves4": {"VG_BATCH_H_WAVES": "4"}, "split": {"VG_BATCH_H_SPLIT": "1"},
            "rowmajor": {"VG_BATCH_TILE_MAJOR": "0"}}
UNSERVED_PATH = {dg.F16: 6, dg.BF16: 6, dg.F32: 5}                  # one scan per query / the multi-query scan (read off last_batch_path(), not guessed)
SWITCHES = ("VG_BATCH_H_WAVES", "VG_BATCH_H_SPLIT", "VG_BATCH_TILE_MAJOR", "VG_BATCH_STAGES", "VG_BATCH_MIN_QUERIES")   # what a case may set


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    bh.close_worlds()


def expected_form(stride, k, nq, form):
    """vg_batch_h_plan restated: (wavefronts per workgroup, workgroups per CU), None where the lists do not fit the LDS at all"""
    ntb = [b for b in (8, 16, 24, 32, 48, 64) if (stride + 31) // 32 <= b][0]
    base = 8 if ntb <= 32 else 4

    def lds(w):
        return 2 * ntb * 1024 + 1024 + w * 32 * 16 + w * 32 * k * 8
    if form == "split":
        return (base, 1)
    if ntb <= 24 and form != "waves8" and 2 * lds(4) + 4096 <= 160 * 1024 and (nq > 128 or form == "waves4"):
        return (4, 2)
    return (base, 1) if lds(base) <= 160 * 1024 else None


def corpus_of(pkg, w):
    if getattr(w, "_corpus", None) is None:
        w._corpus = pkg.Corpus(w.vt, w.dim, capacity=w.n) if w.n > 1_000_000 else pkg.Corpus(w.vt, w.dim)
        w._corpus.append(w.rows)
    return w._corpus


def set_env(mp, w, nq, form="default", extra=None):
    for name in SWITCHES:
        mp.delenv(name, raising=False)
    mp.setenv("VG_BATCH_Q8", "0")                                   # (only reachable from 2^16 rows on; off everywhere: path 3 is what is under test)
    if w.vt == dg.F32:
        mp.setenv("VG_F32_FILTER", "1")
        mp.setenv("VG_BATCH_LONG", "0")                             # (rows of 513 .. 1024 floats: not the K-split kernel)
    if nq < 4:
        mp.setenv("VG_BATCH_MIN_QUERIES", "1")
    for name, v in dict(FORM_ENV[form], **(extra or {})).items():
        mp.setenv(name, v)


def run_case(pkg, orc, mp, w, nq, metric, k, form="default", queries=None, refs=None, unjudged=(), plants=None, extra=None, c=None, rows=None):
    """reference first (and the cap on its weaker check, before any device result exists), then the batch, then every query"""
    qs = w.queries[:nq] if queries is None else queries
    rows = w.rows if rows is None else rows
    ref = (bh.references(w, orc, br) if refs is None else refs)[metric]
    judged = np.ones(nq, dtype=bool)
    judged[list(unjudged)] = False
    share = ref.band_share(k, nq, judged)
    print("band share %.4f  (%s dim %d n %d nq %d %s k %d %s)" % (share, dg.TYPE_NAMES[w.vt], w.dim, rows.shape[0], nq, dg.METRIC_NAMES[metric], k, form))
    assert share <= br.BAND_SHARE_CAP, share
    set_env(mp, w, nq, form, extra)
    c = corpus_of(pkg, w) if c is None else c
    ids, dist, cnt = c.scan_topk_batch(metric, qs, k)
    want_form = expected_form(bh.filter_stride(w.dim), k, nq, form)
    assert pkg.plan_batch_half_form(bh.filter_stride(w.dim), k, nq) == want_form, (pkg.plan_batch_half_form(bh.filter_stride(w.dim), k, nq), want_form)
    if want_form is None:
        assert c.last_batch_path() == UNSERVED_PATH[w.vt], c.last_batch_path()   # 2 KiB rows with k >= 30: no matrix-core kernel, no multi-query kernel
    else:
        assert c.last_batch_path() == 3, c.last_batch_path()
        if form == "split":
            # an overflowed pair region would have re-run the fused kernel, silently.  (This shows that no region ran over, which is all
            # that is visible from here: a corpus that cannot ALLOCATE its pair regions - at most ~34 MB in these cases - also answers
            # through the fused kernel, and leaves the flag alone.)
            assert not c.batch_half_split_off()
    br.check_batch(w.vt, metric, k, qs, rows, ids, dist, cnt, orc, reference=ref)
    if metric != dg.DOT:                                            # a query's own plant is its best row
        for i in (range(nq) if plants is None else plants):
            assert ids[i][0] == w.plant[i] + 1, (i, ids[i][:3], w.plant[i] + 1)
        for i, p in w.second.items():
            if i < nq and k >= 2 and (plants is None or i in plants):
                assert ids[i][1] == p + 1 and dist[i][1] == dist[i][0], (i, ids[i][:3])
    return ids, dist, cnt


def _ids(worlds):
    return ["-".join(dg.TYPE_NAMES[x] if j == 0 else str(x) for j, x in enumerate(v)) for v in worlds]


def _bucket_params():
    return [pytest.param(vt, dim, nq, m, k, id="%s-%d-%d-%s-%d" % (dg.TYPE_NAMES[vt], dim, nq, dg.METRIC_NAMES[m], k))
            for vt, dim in bh.small_worlds() for nq, m, k in bh.bucket_cases(vt, dim)]


def _form_params():
    return [pytest.param(vt, dim, f, nq, m, k, id="%s-%d-%s-%d-%s-%d" % (dg.TYPE_NAMES[vt], dim, f, nq, dg.METRIC_NAMES[m], k))
            for vt, dim in bh.small_worlds() for f, nq, m, k in bh.form_cases(vt, dim)]


def _pinned_forms(vt, dim, nq, k, form, got):
    """the cells the table names, as constants (expected_form is a restatement; these are what the cases are FOR)"""
    if form == "default":
        if dim == 384:
            assert got == ((4, 2) if (nq > 128 and k <= 27) else (8, 1))
        if dim in (768, 1000) or (vt == dg.F32 and dim == 600):
            assert got == ((4, 1) if not (dim == 1000 and k >= 30) else None)
        if dim == 500:
            assert got == (8, 1)
    if form == "waves4" and dim <= 384:
        assert got == ((4, 2) if (dim < 384 or k <= 27) else (8, 1))
    if form == "split":                                             # one workgroup per CU: 8 wavefronts, 4 in the long form
        assert got == ((8, 1) if bh.ntb_of(dim) <= 32 else (4, 1))


@pytest.mark.parametrize("vt,dim,nq,metric,k", _bucket_params())
def test_every_bucket_type_and_batch_size(pkg, orc, monkeypatch, vt, dim, nq, metric, k):
    w = bh.world(vt, dim)
    run_case(pkg, orc, monkeypatch, w, nq, metric, k)
    _pinned_forms(vt, dim, nq, k, "default", pkg.plan_batch_half_form(bh.filter_stride(dim), k, nq))


@pytest.mark.parametrize("vt,dim,form,nq,metric,k", _form_params())
def test_every_form(pkg, orc, monkeypatch, vt, dim, form, nq, metric, k):
    w = bh.world(vt, dim)
    run_case(pkg, orc, monkeypatch, w, nq, metric, k, form=form)
    _pinned_forms(vt, dim, nq, k, form, pkg.plan_batch_half_form(bh.filter_stride(dim), k, nq))


@pytest.mark.parametrize("vt,dim", bh.DOT1_WORLDS, ids=_ids(bh.DOT1_WORLDS))
def test_dot_at_k_1(pkg, orc, monkeypatch, vt, dim):
    """the dot inequality of the filter with a one-entry list, on the queries that have no row at -Inf (batch_half_cases.dot1_queries)"""
    w = bh.world(vt, dim)
    sel = bh.dot1_queries(w)
    refs = bh.references(w, orc, br, w.queries[sel], "dot1", (dg.DOT,))
    run_case(pkg, orc, monkeypatch, w, len(sel), dg.DOT, 1, queries=w.queries[sel], refs=refs)


@pytest.mark.parametrize("metric", (dg.DOT, dg.COSINE, dg.L2), ids=lambda m: dg.METRIC_NAMES[m])
@pytest.mark.parametrize("vt,dim", bh.UNJUDGED_WORLDS, ids=_ids(bh.UNJUDGED_WORLDS))
def test_unjudgeable_queries_leave_their_neighbours_alone(pkg, orc, monkeypatch, vt, dim, metric):
    """a zero query, one with a NaN and one with an Inf element in slots 1, 31 and 32 (both sides of the first wavefront's edge) of 129: every
    pair of theirs passes the filter; their answers follow the oracle, the 126 others are checked like any batch's"""
    w = bh.world(vt, dim)
    qs = bh.unjudgeable_queries(w)
    refs = bh.references(w, orc, br, qs, "unjudgeable", (dg.DOT, dg.COSINE, dg.L2))
    good = [i for i in range(129) if i not in bh.UNJUDGED_SLOTS]
    run_case(pkg, orc, monkeypatch, w, 129, metric, 20, queries=qs, refs=refs, unjudged=bh.UNJUDGED_SLOTS, plants=good)


@pytest.mark.parametrize("vt,dim", bh.APPEND_WORLDS, ids=_ids(bh.APPEND_WORLDS))
def test_a_corpus_appended_to_after_a_batch(pkg, orc, monkeypatch, vt, dim):
    """500 rows behind the ragged last tile of a corpus a batch has already run over: the cached norms, the bf16 shadow copy and the tile-major
    copy are extended.  Among them a new best row (dot) of one query and a second copy of another's plant."""
    w = bh.world(vt, dim)
    nq = bh.APPEND_NQ
    c = pkg.Corpus(vt, dim)
    c.append(w.rows)
    try:
        run_case(pkg, orc, monkeypatch, w, nq, dg.L2, 20, c=c)
        rows, dup = bh.appended(w)
        refs = br.batch_references(vt, (dg.DOT, dg.COSINE, dg.L2), w.queries[:nq], rows, orc, kmax=20, duplicates=dup)
        c.append(rows[w.n:])
        for metric in (dg.DOT, dg.COSINE, dg.L2):
            ids, dist, cnt = run_case(pkg, orc, monkeypatch, w, nq, metric, 20, refs=refs, c=c, rows=rows)
            if metric == dg.DOT:                                    # the appended 30 x query: at the reference's rank, among the first 12
                rank = refs[dg.DOT].pos[bh.APPEND_BEST, :12].tolist().index(w.n + 123)
                assert ids[bh.APPEND_BEST][rank] == w.n + 123 + 1
            if metric == dg.L2:
                assert ids[bh.APPEND_COPY][:2].tolist() == [w.plant[bh.APPEND_COPY] + 1, w.n + 377 + 1] and dist[bh.APPEND_COPY][0] == dist[bh.APPEND_COPY][1]
    finally:
        c.close()


@pytest.mark.parametrize("k", (1, 20, 32))
@pytest.mark.parametrize("vt,dim,n", bh.TINY_WORLDS, ids=_ids(bh.TINY_WORLDS))
def test_tiny_worlds(pkg, orc, monkeypatch, vt, dim, n, k):
    w = bh.world(vt, dim, n)
    refs = bh.references(w, orc, br)
    for metric in bh.ALL_METRICS:
        if (metric, k) == (dg.DOT, 1):                              # (ties at -Inf: see batch_half_cases.K_PAIRS)
            continue
        ids, dist, cnt = run_case(pkg, orc, monkeypatch, w, bh.TINY_NQ, metric, k, refs=refs)
        assert cnt.tolist() == np.minimum(k, refs[metric].enter[:bh.TINY_NQ]).tolist()
        if k == (20 if n == 20 else 32) and metric in (dg.L2, dg.SQUARED_L2):
            assert (cnt < k).all()                                  # fewer rows can enter than the list holds


@pytest.mark.parametrize("metric", bh.ALL_METRICS, ids=lambda m: dg.METRIC_NAMES[m])
@pytest.mark.parametrize("nq,k", ((129, 20), (257, 20), (257, 32)))
@pytest.mark.parametrize("vt,dim", bh.SPARSE_WORLDS, ids=_ids(bh.SPARSE_WORLDS))
def test_sparse_worlds(pkg, orc, monkeypatch, vt, dim, nq, k, metric):
    w = bh.world(vt, dim, bh.N_SPARSE)
    run_case(pkg, orc, monkeypatch, w, nq, metric, k)


def _split_sparse_params():
    return [pytest.param(vt, dim, nq, m, k, id="%s-%d-%d-%s-%d" % (dg.TYPE_NAMES[vt], dim, nq, dg.METRIC_NAMES[m], k))
            for vt, dim in bh.small_worlds() for nq, m, k in bh.split_cases(vt, dim)]


@pytest.mark.parametrize("vt,dim,nq,metric,k", _split_sparse_params())
def test_split_form_every_bucket_and_type(pkg, orc, monkeypatch, vt, dim, nq, metric, k):
    """VG_BATCH_H_SPLIT=1 over the sparse world, one query group: 256 partitions of at most two tiles, so the regions of the wavefronts
    with 32 queries end exactly full and none runs over - the filter kernel of every k-step bucket (its ring of tile buffers, the counted
    wait, the staggered barrier of the 8-wavefront form) and vg_batch_hx_kernel for f16, bf16 and f32 answer, which run_case asserts."""
    w = bh.world(vt, dim, bh.N_SPARSE)
    run_case(pkg, orc, monkeypatch, w, nq, metric, k, form="split")
    _pinned_forms(vt, dim, nq, k, "split", pkg.plan_batch_half_form(bh.filter_stride(dim), k, nq))


@pytest.mark.parametrize("vt,dim,n", bh.TINY_WORLDS, ids=_ids(bh.TINY_WORLDS))
def test_split_form_tiny_worlds(pkg, orc, monkeypatch, vt, dim, n):
    w = bh.world(vt, dim, n)
    refs = bh.references(w, orc, br)
    for metric, k in bh.SPLIT_TINY:
        ids, dist, cnt = run_case(pkg, orc, monkeypatch, w, bh.TINY_NQ, metric, k, form="split", refs=refs)
        assert cnt.tolist() == np.minimum(k, refs[metric].enter[:bh.TINY_NQ]).tolist()
        _pinned_forms(vt, dim, bh.TINY_NQ, k, "split", pkg.plan_batch_half_form(bh.filter_stride(dim), k, bh.TINY_NQ))


def test_split_form_hands_a_corpus_without_a_pre_pass_to_the_fused_kernel(pkg, orc, monkeypatch):
    """VG_BATCH_H_SPLIT=1, 257 queries over 626 tiles: two query groups, 128 partitions of 5 tiles, no pre-pass - the filter kernel's
    thresholds are +Inf, a wavefront of 32 queries fills its region of 2048 pairs with its second tile and runs over with the third, and
    the fused kernel answers this batch and the following ones - silently, but for vg_batch_h_split_off.  The answer is right either way."""
    w = bh.world(dg.BF16, 384)
    c = pkg.Corpus(w.vt, w.dim)
    c.append(w.rows)
    try:
        set_env(monkeypatch, w, 257, "split")
        ref = bh.references(w, orc, br)[dg.L2]
        assert not c.batch_half_split_off()
        ids, dist, cnt = c.scan_topk_batch(dg.L2, w.queries, 20)
        assert c.last_batch_path() == 3 and c.batch_half_split_off()
        br.check_batch(w.vt, dg.L2, 20, w.queries, w.rows, ids, dist, cnt, orc, reference=ref)
    finally:
        c.close()


def _staged_params():
    out = [(nq, stages, m, "default") for nq in (40, 160) for stages in (None, "0", "200") for m in (dg.L2, dg.DOT)]
    return out + [(160, None, dg.L2, "split"), (160, "200", dg.DOT, "split"), (40, None, dg.L2, "split")]


@pytest.mark.parametrize("nq,stages,metric,form", _staged_params(),
                         ids=["%d-%s-%s-%s" % (a, b, dg.METRIC_NAMES[c], d) for a, b, c, d in _staged_params()])
def test_staged_world(pkg, orc, monkeypatch, nq, stages, metric, form):
    """65 538 tiles: the BOUNDK pre-pass, then real passes over growing row ranges, each seeded with the merged lists of the rows before it.
    The 35 copies of query LADDER_Q's best row sit on both sides of every stage bound (see HalfWorld): the first k come back, in position
    order - a stage seed that lost a row of an earlier stage, or met it twice, cannot pass."""
    vt, dim, n = bh.STAGED
    w = bh.world(vt, dim, n)
    refs = bh.references(w, orc, br, metrics=(dg.L2, dg.DOT), kmax=20)
    k = 20
    ids, dist, cnt = run_case(pkg, orc, monkeypatch, w, nq, metric, k, form=form, refs=refs, extra=None if stages is None else {"VG_BATCH_STAGES": stages})
    assert pkg.plan_batch_half_form(bh.filter_stride(dim), k, nq) == ((8, 1) if (nq == 40 or form == "split") else (4, 2))
    got = (ids[bh.LADDER_Q][:cnt[bh.LADDER_Q]] - 1).tolist()
    on_ladder = [p for p in got if p in set(w.ladder)]
    assert on_ladder == w.ladder[:len(on_ladder)], (on_ladder, w.ladder[:k])
    if metric == dg.L2:
        assert got == w.ladder[:k]
