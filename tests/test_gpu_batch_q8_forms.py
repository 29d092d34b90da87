"""Every form of the int8 matrix-core batch filter (vg_batch_q8.hip) against a float64 reference over ALL rows, every query of every batch
(tests/batch_reference.py) - not against another HIP path that shares its exact-evaluation kernel and its cached norms.

Each case asserts that the batch took the int8 filter (last_batch_path() == 7) and that vg_batch_q8_padded_queries() gives the slot count
the case is meant for, so a routing change cannot empty the matrix.  Launcher instantiations (vg_batch_q8_launch's launch_filter) and the
fully checked cases that reach them - rows of 65 603 (dim 200: exactly 65 536) elements-of-`dim`, VG_BATCH_Q8=1:

  form      slots  k-step class (int8 stride)   instantiation          type  dim   nq
  narrow    128    <= 128 B                     launch_q8n_mode<4>     f32   24    4, 16, 127, 128
  narrow    128    <= 256 B                     launch_q8n_mode<8>     f32   200   4, 16, 127, 128        (+ f16 / bf16 dim 100, nq 16)
  narrow    128    <= 384 B                     launch_q8n_mode<12>    f32   384   4, 16, 127, 128, 64 x one query   (+ f16 / bf16 dim 384, nq 16)
  narrow    128    <= 512 B                     launch_q8n_mode<16>    f32   500   4, 16, 127, 128
  256-slot  256    <= 128 B                     launch_q8_mode<4>      f32   24    129, 256
  256-slot  256    <= 256 B                     launch_q8_mode<8>      f32   200   129, 256               (+ f16 / bf16 dim 100, nq 129)
  256-slot  256    <= 384 B                     launch_q8_mode<12>     f32   384   129, 256               (+ f16 / bf16 dim 384, nq 129)
  256-slot  256    <= 512 B                     launch_q8_mode<16>     f32   500   129, 256
  wide      512    <= 128 B                     launch_q8w_mode<4>     f32   24    257, 300, 512
  wide      512    <= 256 B                     launch_q8w_mode<8>     f32   200   257, 300, 512
  wide      512    <= 384 B                     launch_q8w_mode<12>    f32   384   257, 300, 512
  wide      512    <= 512 B                     launch_q8w_mode<16>    f32   500   257, 300, 512
  long-row  256    513 .. 768 B, 2 K-parts      launch_q8l_mode<12,2>  f32   600   5
  long-row  256    769 .. 1024 B, 2 K-parts     launch_q8l_mode<16,2>  f32   1000  5
  long-row  256    1025 .. 1536 B, 3 K-parts    launch_q8l_mode<16,3>  f32   1536  5                      (+ f16 dim 1536)
  long-row  512    the same three               the same three         f32   600, 1000, 1536  257         (+ f16 dim 1536)

(a padded batch of 512 slots over long rows is two 256-query groups of the long-row kernel: it has no wide form.)  Metrics dot, cosine, L2
and squared L2 at k = 20 on every short-row f32 cell, k = 1 and k = 64 under two metrics each; the default policy (no switch, 1 100 003 x
64, nq 4 / 16 / 129 / 300 = narrow<4>, 256-slot<4>, wide<4>), unjudgeable queries, 64 identical queries and a corpus with 7 usable rows
have cases of their own below.

Planted in every corpus (see _World): one exact duplicate of EVERY query at a position of its own (first tile, last ragged tile, tile and
stage boundaries, the rest spread out) - under every metric but dot a query's first rowid is its own plant, so a slot answered with
another query's list cannot pass; second copies of a few plants (ties go by position); coherent-residual duplicates behind grid-exact
competitors (after q8_adversarial_case of test_gpu_filter_bound.py: dropped as soon as the bound's error term is short); the _adversarial
rows of test_gpu_batch_q8.py; rows of magnitude 1e-38 (subnormal shadow scale) and rows just inside / outside the filter's judged window.

Rows are N(0, 1) elements with a decaying spectrum (element e scaled by 1 / (1 + e / 8)) and a magnitude of 1, 2 or 8 per row: iid rows
of 500 elements put every query's 20th and 21st neighbour closer than the suite's own slack too often for the set comparison to apply
(see batch_reference.BAND_SHARE_CAP), under dot - whose slack carries 4 |q|_1 - most of all."""
import ctypes as C

import numpy as np
import pytest

import datagen as dg
import batch_reference as br
from test_gpu_scan import pkg  # noqa: F401  (fixture)
from test_gpu_batch_q8 import _adversarial

pytestmark = pytest.mark.gpu

N_RAGGED, N_EXACT = 65_536 + 67, 65_536
MASTER_NQ = 512
COHERENT = (9, 127, 128, 255, 256, 511)        # queries that are coherent-residual targets: both sides of every form's edge
SECOND_COPIES = (2, 64, 130, 300)              # queries whose plant has a second copy further down
N_COMP = 80
ADV_Q0 = 20                                    # the queries _adversarial's rows are made of: 20 .. 24 (3 x and -1 x a query, a cluster of near-duplicates: cosine ties)
ALL_METRICS = (dg.DOT, dg.COSINE, dg.L2, dg.SQUARED_L2)
JUDGE_LO, JUDGE_HI = np.float32(1.0e-10), np.float32(1.0e10)       # VGQ_JUDGE_LO / VGQ_JUDGE_HI of vg_batch_q8.hip


def coherent_case(dim, n_comp, seed):
    """after q8_adversarial_case (test_gpu_filter_bound.py): every element of the target sits just below an int8 midpoint s (m + 0.5), so the
    residuals are all +s / 2 - coherent; the query is the target.  Competitor j is a grid row s (m - delta_j) with j units taken off its
    elements: grid-exact (its bound is tight), a little worse than the target, and at a distance of its own (no ties among competitors)."""
    rng = np.random.default_rng(seed)
    s = 1.0 / 127.0
    m = rng.integers(10, 100, dim).astype(np.float64)
    target = (s * (m + 0.499)).astype(np.float32)
    target[0] = np.float32(1.0)                                    # sets the scale: max = 127 s
    m[0] = 127.0
    comps = []
    for j in range(n_comp):
        delta = np.zeros(dim)
        delta[1:] = j // (dim - 1) + (np.arange(dim - 1) < j % (dim - 1))
        comps.append((s * (m - delta)).astype(np.float32))
    return target, np.stack(comps)


def spectrum(dim):
    return (1.0 / (1.0 + np.arange(dim) / 8.0)).astype(np.float32)


class _World:
    """one corpus, its 512 master queries (a case takes the first nq), what was planted where, and - lazily - the device corpus and the
    float64 references"""

    def __init__(self, vt, dim, n, seed, nq=MASTER_NQ):
        self.vt, self.dim, self.n = vt, dim, n
        rng = np.random.default_rng(seed)
        w = spectrum(dim)
        rows = rng.standard_normal((n, dim), dtype=np.float32) * w * rng.choice(np.array([1, 1, 1, 2, 8], dtype=np.float32), (n, 1))
        qs = rng.standard_normal((nq, dim), dtype=np.float32) * w
        used = set()
        self.duplicates, self.plant = [], {}

        def take(positions):
            positions = [int(p) for p in np.atleast_1d(positions)]
            assert not used.intersection(positions) and max(positions) < n
            used.update(positions)
            return positions

        take([11, n - 1, 5000, 5001] + list(range(6000, 6009)) + list(range(7000, 7040)))      # _adversarial's
        coherent_at = (n - 5, 3, 8191, 16384, 40_000, 65_500)                                   # last ragged tile, first tile, stage boundaries
        comps = {}
        for ci, i in enumerate(c for c in COHERENT if c < nq):
            qs[i], comps[i] = coherent_case(dim, N_COMP, seed * 31 + i)
        rows = _adversarial(rows, qs[ADV_Q0:], rng)                                             # (its rows are made of queries ADV_Q0 .. + 4)
        if vt == dg.F16:                                                                        # (the largest / smallest norms the type holds)
            rows[6005] = rng.standard_normal(dim).astype(np.float32) * np.float32(1e3)
            rows[6004] = rng.standard_normal(dim).astype(np.float32) * np.float32(1e-4)
        self.plant[ADV_Q0], self.plant[ADV_Q0 + 1] = 11, n - 1
        self.plant[ADV_Q0 + 2] = take(40)[0]                       # ahead of row 5000 = 3 x this query: cosine 0 there too, the tie goes by position
        for ci, i in enumerate(sorted(comps)):
            at = take(20_000 + 97 * ci + 211 * np.arange(N_COMP))                               # competitors: spread over 17 000 rows
            rows[at] = comps[i]
            self.plant[i] = take(coherent_at[ci])[0]
        # rows of magnitude 1e-38 (f16: its own subnormals), and unit rows scaled to both sides of both ends of the judged window
        tiny = np.float32(1e-7 if vt == dg.F16 else 1e-38)
        self.tiny_rows = take([6100, 6101])
        rows[self.tiny_rows] = rng.standard_normal((2, dim)).astype(np.float32) * tiny
        self.window_rows = {}
        if vt != dg.F16:                                                                        # (f16 holds neither 1e-10 nor 1e10)
            for at, scale in zip(take([6102, 6103, 6104, 6105]), (2e-10, 5e-11, 5e9, 2e10)):
                u = rng.standard_normal(dim)
                rows[at] = (u / np.linalg.norm(u) * scale).astype(np.float32)
                self.window_rows[at] = scale
        edges = [0, 1, 2, 4, 5, 31, 32, 33, 8190, 8192, 8193, 16_383, 16_385, 32_767, 32_768, 65_534, N_EXACT, n - 2, n - 3, n - 4, n - 33, n - 34]
        spread = iter([p for p in edges if p < n] + [97 + 127 * j for j in range(nq + 64)])
        for i in range(nq):
            if i in self.plant:
                continue
            p = next(spread)
            while p in used:
                p = next(spread)
            self.plant[i] = take(p)[0]
        second = {}
        for si, i in enumerate(c for c in SECOND_COPIES if c < nq):
            second[i] = take(50_001 + 1000 * si)[0]
        self.rows = dg.to_storage(vt, rows)
        self.queries = dg.to_storage(vt, qs)
        for i, p in self.plant.items():
            self.rows[p] = self.queries[i]
        for i, p in second.items():
            self.rows[p] = self.queries[i]
            assert p > self.plant[i]
            self.duplicates.append([self.plant[i], p])
        self.second = second
        self._refs, self._corpus = {}, None
        self._check_window_rows()

    def _check_window_rows(self):
        """each scaled row lands on the intended side of [VGQ_JUDGE_LO, VGQ_JUDGE_HI] (the kernel tests the row's cached float32 norm)"""
        for at, scale in self.window_rows.items():
            x = dg.storage_to_f64(self.vt, self.rows[at]).astype(np.float32)
            nrm = np.sqrt(np.sum(x * x, dtype=np.float32))
            inside = bool(JUDGE_LO <= nrm <= JUDGE_HI)
            assert inside == (scale in (2e-10, 5e9)) and (abs(float(nrm) / scale - 1.0) < 0.05), (at, scale, nrm)
        for at in self.tiny_rows:
            x = dg.storage_to_f64(self.vt, self.rows[at])
            assert 0.0 < np.abs(x).max() / 127.0 < (6.2e-5 if self.vt == dg.F16 else 1.17e-38)  # (f32 / bf16: the shadow scale max|x| / 127 is subnormal)

    def references(self, orc, queries=None, tag="master", metrics=ALL_METRICS, kmax=64):
        key = (tag, metrics)
        if key not in self._refs:
            self._refs[key] = br.batch_references(self.vt, metrics, self.queries if queries is None else queries, self.rows, orc, kmax=kmax,
                                                  duplicates=self.duplicates)
        return self._refs[key]

    def corpus(self, pkg):
        if self._corpus is None:
            self._corpus = pkg.Corpus(self.vt, self.dim)
            self._corpus.append(self.rows)
        return self._corpus

    def close(self):
        if self._corpus is not None:
            self._corpus.close()
        self._corpus, self._refs = None, {}


_CURRENT = {}
# seeds moved on where the first one left more than 1 query in 10 of some case to the band check (tried on the CPU, reference alone)
SEED_STEP = {(dg.F32, 24): 1, (dg.F32, 200): 10, (dg.F32, 384): 1, (dg.F32, 500): 6, (dg.F16, 384): 1, (dg.BF16, 384): 1}


def world(vt, dim, n=None, nq=MASTER_NQ):
    """the cases of one corpus follow each other: one world at a time is kept (rows, references, the device corpus)"""
    n = (N_EXACT if dim == 200 else N_RAGGED) if n is None else n
    key = (vt, dim, n, nq)
    if key not in _CURRENT:
        for w in _CURRENT.values():
            w.close()
        _CURRENT.clear()
        _CURRENT[key] = _World(vt, dim, n, 9300 + dim + 7 * vt + 10_000 * SEED_STEP.get((vt, dim), 0), nq)
    return _CURRENT[key]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _CURRENT.values():
        w.close()
    _CURRENT.clear()


def q8_stride(dim):
    return (dim + 15) // 16 * 16


def expected_slots(nq, dim):
    """narrow / 256-slot / wide by the batch size; long rows: whole 256-query groups"""
    if q8_stride(dim) <= 512 and nq <= 128:
        return 128
    return (nq + 255) // 256 * 256


def padded_queries(pkg, nq, dim):
    fn = pkg.lib().vg_batch_q8_padded_queries
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_longlong]
    return int(fn(nq, q8_stride(dim)))


def judged_mask(nq, unjudgeable=()):
    m = np.ones(nq, dtype=bool)
    m[list(unjudgeable)] = False
    return m


def run_case(pkg, orc, w, nq, metric, k, queries=None, refs=None, unjudgeable=(), path=7, plants=None):
    """reference first (and the cap on its weaker check, before any device result exists), then the batch, then every query"""
    qs = w.queries[:nq] if queries is None else queries
    ref = (w.references(orc) if refs is None else refs)[metric]
    share = ref.band_share(k, nq, judged_mask(nq, unjudgeable))
    print("band share %.4f  (%s dim %d nq %d %s k %d)" % (share, dg.TYPE_NAMES[w.vt], w.dim, nq, dg.METRIC_NAMES[metric], k))
    assert share <= br.BAND_SHARE_CAP, share
    c = w.corpus(pkg)
    ids, dist, cnt = c.scan_topk_batch(metric, qs, k)
    if path is not None:
        assert c.last_batch_path() == path, (c.last_batch_path(), c.batch_q8_status())
        assert padded_queries(pkg, nq, w.dim) == expected_slots(nq, w.dim)
    banded = br.check_batch(w.vt, metric, k, qs, w.rows, ids, dist, cnt, orc, reference=ref)
    if metric != dg.DOT:                                           # a query's own plant is its best row
        for i in (range(nq) if plants is None else plants):
            assert ids[i][0] == w.plant[i] + 1, (i, ids[i][:3], w.plant[i] + 1)
        for i, p in w.second.items():
            if i < nq and k >= 2 and (plants is None or i in plants):
                assert ids[i][1] == p + 1 and dist[i][1] == dist[i][0], (i, ids[i][:3])
    return ids, dist, cnt, banded


SHORT_DIMS = (24, 200, 384, 500)                                   # the four k-step classes (int8 strides 32, 208, 384, 512 bytes)
SHORT_NQ = (4, 16, 127, 128, 129, 256, 257, 300, 512)


def _short_cases():
    out = []
    for dim in SHORT_DIMS:
        for j, nq in enumerate(SHORT_NQ):
            for metric in ALL_METRICS:
                out.append((dim, nq, metric, 20))
            # k = 1 and k = 64 under two metrics each, alternating with the batch size (every form sees both pairs at every k)
            pair = (dg.L2, dg.DOT) if j % 2 == 0 else (dg.COSINE, dg.SQUARED_L2)
            for k in (1, 64):
                for metric in pair:
                    out.append((dim, nq, metric, k))
    return out


def _id(case):
    return "-".join(dg.METRIC_NAMES[v] if (j == 2) else str(v) for j, v in enumerate(case))


@pytest.mark.parametrize("dim,nq,metric,k", _short_cases(), ids=[_id(c) for c in _short_cases()])
def test_short_rows_f32_every_form_and_kstep_class(pkg, orc, monkeypatch, dim, nq, metric, k):
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    run_case(pkg, orc, world(dg.F32, dim), nq, metric, k)


@pytest.mark.parametrize("metric", ALL_METRICS, ids=lambda m: dg.METRIC_NAMES[m])
@pytest.mark.parametrize("nq", (16, 129))
@pytest.mark.parametrize("dim", (100, 384))
@pytest.mark.parametrize("vt", (dg.F16, dg.BF16), ids=lambda t: dg.TYPE_NAMES[t])
def test_half_precision_corpora(pkg, orc, monkeypatch, vt, dim, nq, metric):
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    run_case(pkg, orc, world(vt, dim, nq=129), nq, metric, 20)


@pytest.mark.parametrize("metric", (dg.COSINE, dg.L2), ids=lambda m: dg.METRIC_NAMES[m])
@pytest.mark.parametrize("nq", (5, 257))
@pytest.mark.parametrize("vt,dim", [(dg.F32, 600), (dg.F32, 1000), (dg.F32, 1536), (dg.F16, 1536)], ids=("f32-600", "f32-1000", "f32-1536", "f16-1536"))
def test_long_rows(pkg, orc, monkeypatch, vt, dim, nq, metric):
    """<12,2>, <16,2>, <16,3>: the K-split kernel, one and two query groups"""
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    run_case(pkg, orc, world(vt, dim, nq=257), nq, metric, 20)


def _unjudgeable(qs32, places):
    """zero, NaN, x 1e25, x 1e-25 at the four slots of every place"""
    out = []
    for at in places:
        qs32[at] = 0.0
        qs32[at + 1, 1] = np.float32(np.nan)
        qs32[at + 2] *= np.float32(1e25)
        qs32[at + 3] *= np.float32(1e-25)
        out += [at, at + 1, at + 2, at + 3]
    return out


@pytest.mark.parametrize("metric", (dg.DOT, dg.COSINE, dg.L2), ids=lambda m: dg.METRIC_NAMES[m])
@pytest.mark.parametrize("nq", (128, 129, 8))
def test_unjudgeable_queries_in_the_middle_and_in_the_last_slot(pkg, orc, monkeypatch, nq, metric):
    """queries the filter cannot judge (zero, NaN, magnitudes outside its window) are answered by single scans: in the middle of a batch, in
    its LAST slots (..., 1e-25 in the very last one), in the narrow form and in the 256-slot form - and a batch of 8 that holds nothing else"""
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    w = world(dg.F32, 200)
    qs = w.queries[:nq].copy()
    bad = _unjudgeable(qs, (0, 4) if nq == 8 else (60, nq - 4))
    assert qs[nq - 1].max() < 1e-20 and (nq != 8 or len(bad) == 8)
    refs = w.references(orc, qs, ("unjudgeable", nq))
    good = [i for i in range(nq) if i not in bad]
    run_case(pkg, orc, w, nq, metric, 20, queries=qs, refs=refs, unjudgeable=bad, plants=good)


def test_a_batch_of_64_identical_queries(pkg, orc, monkeypatch):
    """the sort keys of the slots tie: every one of the 64 lists is the same, and right"""
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    w = world(dg.F32, 384)
    qs = np.repeat(w.queries[7:8], 64, axis=0)
    refs = w.references(orc, qs, "identical")
    for metric in (dg.L2, dg.COSINE, dg.DOT):
        ids, dist, cnt, _ = run_case(pkg, orc, w, 64, metric, 20, queries=qs, refs=refs, plants=())
        assert (ids == ids[0]).all() and dg.same_float_bits(dist, np.repeat(dist[:1], 64, axis=0)) and (cnt == 20).all()
        if metric != dg.DOT:
            assert ids[0][0] == w.plant[7] + 1


def test_fewer_than_k_rows_can_enter_a_list(pkg, orc, monkeypatch):
    """65 600 rows of which all but 7 hold one NaN: every count is 7, exactly those rows; whichever path answered (the filter may hand such
    a batch on).  Afterwards an ordinary batch over a fresh corpus, same process, takes the int8 filter again and passes."""
    monkeypatch.setenv("VG_BATCH_Q8", "1")
    n, dim, nq, k = 65_600, 64, 16, 20
    rng = np.random.default_rng(9477)
    rows = rng.standard_normal((n, dim), dtype=np.float32)
    qs = rng.standard_normal((nq, dim), dtype=np.float32)
    rows[np.arange(n), rng.integers(0, dim, n)] = np.float32(np.nan)
    usable = np.array([0, 31, 32, 8191, 40_000, 65_536, n - 1])
    rows[usable] = rng.standard_normal((7, dim), dtype=np.float32)
    c = pkg.Corpus(pkg.F32, dim)
    c.append(rows)
    for metric in (dg.L2, dg.COSINE, dg.DOT):
        ref = br.batch_references(dg.F32, (metric,), qs, rows, orc, kmax=k)[metric]
        assert ref.enter.tolist() == [7] * nq
        ids, dist, cnt = c.scan_topk_batch(metric, qs, k)
        assert cnt.tolist() == [7] * nq, (metric, cnt, c.last_batch_path(), c.batch_q8_status())
        for i in range(nq):
            assert sorted(ids[i][:7].tolist()) == (usable + 1).tolist(), (metric, i, ids[i])
        br.check_batch(dg.F32, metric, k, qs, rows, ids, dist, cnt, orc, reference=ref)
    c.close()
    run_case(pkg, orc, world(dg.F32, 24), 16, dg.L2, 20)


@pytest.mark.parametrize("nq", (4, 16, 129, 300))
def test_default_policy(pkg, orc, monkeypatch, nq):
    """no switch forced: a corpus the filter scans' policy covers (the shape of test_int8_filter_default_policy_appends_and_unselective_rows)
    sends every batch size through the int8 filter"""
    monkeypatch.delenv("VG_F32_FILTER", raising=False)
    monkeypatch.delenv("VG_BATCH_Q8", raising=False)
    monkeypatch.setenv("VG_SCAN_FILTER_MIN_MB", "0")
    w = world(dg.F32, 64, n=1_100_003, nq=300)
    refs = w.references(orc, metrics=(dg.L2, dg.DOT), kmax=20)
    for metric in (dg.L2, dg.DOT):
        run_case(pkg, orc, w, nq, metric, 20, refs=refs)
