"""Jaccard / Tanimoto distance, the parts that need no device: the constants, jaccard_reference against a bit-by-bit loop (empty
unions included), and the launch-shape plan (pure host logic) - Jaccard takes the shape uint8 L1 takes and is planned for uint8 rows
only."""
import os
import re
import warnings

import numpy as np
import pytest

import jaccard_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def test_constants_agree(pkg):
    header = open(os.path.join(ROOT, "include", "vectorgpu.h")).read()
    assert int(re.search(r"VG_DIST_JACCARD\s*=\s*(\d+)", header).group(1)) == pkg.JACCARD == jc.JACCARD == 7
    assert pkg.TANIMOTO is pkg.JACCARD
    assert int(re.search(r"VG_DIST_HAMMING\s*=\s*(\d+)", header).group(1)) == pkg.HAMMING == jc.HAMMING
    assert int(re.search(r"VG_DIST_L1\s*=\s*(\d+)", header).group(1)) == pkg.L1 == jc.L1


def _jaccard_loop(rows, q):
    out = []
    for r in rows:
        i = sum(bin(int(a) & int(b)).count("1") for a, b in zip(r, q))
        u = sum(bin(int(a) | int(b)).count("1") for a, b in zip(r, q))
        out.append(np.float32(u - i) / np.float32(u) if u else np.float32(0))
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("dim", [1, 2, 9, 128])
def test_reference_against_a_loop(pkg, dim):
    rng = np.random.default_rng(dim)
    rows = jc.random_rows(40, dim, rng)
    rows[3] = 0                                                # an empty row
    rows[5] = 0xFF
    for q in (jc.query(dim, dim + 1, 0.5), np.zeros(dim, dtype=np.uint8), rows[7].copy(), ~rows[7]):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                     # no divide-by-zero / invalid-value warning where the union is empty
            got = pkg.jaccard_reference(rows, q)
            mine = jc.distances(rows, q)
        want = _jaccard_loop(rows, q)
        assert got.dtype == np.float32 and got.shape == (40,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(mine.view(np.uint32), want.view(np.uint32))
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert pkg.jaccard_reference(rows, np.zeros(dim, dtype=np.uint8))[3] == 0          # u == 0
    assert pkg.jaccard_reference(rows, rows[7])[7] == 0
    assert pkg.jaccard_reference(rows, ~rows[5])[5] == 1


def test_reference_refuses_other_dtypes_and_shapes(pkg):
    rows = np.zeros((4, 8), dtype=np.uint8)
    q = np.zeros(8, dtype=np.uint8)
    for bad_rows, bad_q in ((rows.astype(np.int8), q), (rows, q.astype(np.int8)), (rows[0], q), (rows, q[:7]), (rows, q[None, :]),
                            (rows.astype(np.float32), q)):
        with pytest.raises(ValueError, match="jaccard_reference"):
            pkg.jaccard_reference(bad_rows, bad_q)
    assert pkg.jaccard_reference(rows, q).tolist() == [0, 0, 0, 0]


def test_equal_rationals_are_equal_floats():
    """the planted rows of the GPU tests: every (i, u) pair is there as planned and its distance is the float 1/2"""
    for weight, pairs in jc.EQUAL_RATIONALS.items():
        q, rows, pos = jc.equal_rationals(2531, 32, weight, 70 + weight)
        i, u = jc.counts(rows, q)
        assert [(int(a), int(b)) for a, b in zip(i[pos], u[pos])] == [pairs[j % len(pairs)] for j in range(len(pos))]
        assert (jc.distances(rows, q)[pos].view(np.uint32) == 0x3F000000).all()
    q = jc.weighted_query(32, 64, 5)
    rows = jc.shared_kth_value(65, 32, q, 6)
    d = jc.distances(rows, q)
    assert int((d < 0.5).sum()) == 64 and int((d == 0.5).sum()) == 5000 and int((d > 0.5).sum()) == 1000


@pytest.mark.parametrize("dim", jc.ROW_BYTES + jc.WIDE_ROW_BYTES + (jc.LONG_ROW_BYTES,))
def test_plan_scan_shape_is_uint8_l1s(pkg, dim):
    assert pkg.plan_scan_shape(pkg.U8, dim, pkg.JACCARD) == pkg.plan_scan_shape(pkg.U8, dim, pkg.L1)


@pytest.mark.parametrize("vt", ["F32", "F16", "BF16", "I8"])
def test_plan_scan_shape_refuses_other_types(pkg, vt):
    with pytest.raises(pkg.VectorGpuError) as ei:
        pkg.plan_scan_shape(getattr(pkg, vt), 128, pkg.JACCARD)
    assert str(ei.value).startswith("vectorgpu error 5:") and "vg_plan_scan_shape: Jaccard distance needs a uint8 corpus" in str(ei.value)
    with pytest.raises(pkg.VectorGpuError) as ei:              # an unknown metric keeps its refusal
        pkg.plan_scan_shape(getattr(pkg, vt), 128, 99)
    assert str(ei.value).startswith("vectorgpu error 1:") and "bad type / dim / metric" in str(ei.value)


def test_unknown_metric_is_still_invalid(pkg):
    with pytest.raises(pkg.VectorGpuError) as ei:
        pkg.plan_scan_shape(pkg.U8, 128, 99)
    assert str(ei.value).startswith("vectorgpu error 1:")
    with pytest.raises(pkg.VectorGpuError) as ei:
        pkg.plan_scan_shape(pkg.U8, 128, 8)                    # the first number behind Jaccard's
    assert str(ei.value).startswith("vectorgpu error 1:")


def test_the_gpu_tests_row_lengths_cover_the_ladder(pkg):
    """the row lengths of the GPU tests: chunks per lane 1, 2, 3, 4, 6 and 8, a ragged row, and the long-row kernel"""
    dims = jc.ROW_BYTES + jc.WIDE_ROW_BYTES
    shapes = {dim: pkg.plan_scan_shape(pkg.U8, dim, pkg.JACCARD) for dim in dims + (jc.LONG_ROW_BYTES,)}
    assert {u for dim, (lpr, u, lng) in shapes.items() if not lng} >= {1, 2, 3, 4, 6, 8}, shapes
    assert shapes[jc.LONG_ROW_BYTES][2] and not any(shapes[dim][2] for dim in dims), shapes
