"""Hamming distance, the parts that need no device: the constants, pack_bits / hamming_reference against a bit-by-bit loop, and the
launch-shape plan (pure host logic) - Hamming takes the shape uint8 L1 takes and is planned for uint8 rows only."""
import os
import re

import numpy as np
import pytest

import hamming_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def test_constants_agree(pkg):
    header = open(os.path.join(ROOT, "include", "vectorgpu.h")).read()
    assert int(re.search(r"VG_DIST_HAMMING\s*=\s*(\d+)", header).group(1)) == pkg.HAMMING == hc.HAMMING == 6
    assert int(re.search(r"VG_DIST_L1\s*=\s*(\d+)", header).group(1)) == pkg.L1 == hc.L1


def _pack_loop(x):
    n, d = len(x), len(x[0])
    out = np.zeros((n, (d + 7) // 8), dtype=np.uint8)
    for i in range(n):
        for j in range(d):
            if x[i][j] > 0:
                out[i, j // 8] |= 0x80 >> (j % 8)
    return out


def _hamming_loop(rows, q):
    out = []
    for r in rows:
        out.append(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(r, q)))
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("d", [1, 7, 8, 9, 1024])
def test_pack_bits_and_reference_against_a_loop(pkg, d):
    rng = np.random.default_rng(d)
    n = 9
    bools = rng.random((n, d)) < 0.5
    numbers = np.where(bools, rng.random((n, d)) + 0.25, -rng.random((n, d)))        # > 0 exactly where the bit is set; zeros too
    numbers[~bools & (rng.random((n, d)) < 0.3)] = 0.0
    want = _pack_loop(bools.astype(np.int64).tolist())
    for x in (bools, numbers, numbers.astype(np.float32), bools.astype(np.int8) * 3, bools.astype(np.uint8)):
        got = pkg.pack_bits(x)
        assert got.dtype == np.uint8 and got.shape == (n, (d + 7) // 8) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want), (d, x.dtype)
    if d % 8:                                                  # tail bits are zero
        assert not (want[:, -1] & ((1 << (8 - d % 8)) - 1)).any()
    q = want[0] if n else None
    got = pkg.hamming_reference(want, q)
    assert got.dtype == np.float32 and np.array_equal(got, _hamming_loop(want, q))
    assert np.array_equal(got, hc.distances(want, q))
    with pytest.raises(ValueError):
        pkg.pack_bits(np.zeros(8))
    with pytest.raises(ValueError):
        pkg.hamming_reference(want.astype(np.int8), q)


@pytest.mark.parametrize("dim", [1, 16, 32, 64, 100, 128, 256, 768, 1024, 9000])
def test_plan_scan_shape_is_uint8_l1s(pkg, dim):
    assert pkg.plan_scan_shape(pkg.U8, dim, pkg.HAMMING) == pkg.plan_scan_shape(pkg.U8, dim, pkg.L1)


@pytest.mark.parametrize("vt", ["F32", "F16", "BF16", "I8"])
def test_plan_scan_shape_refuses_other_types(pkg, vt):
    with pytest.raises(pkg.VectorGpuError) as ei:
        pkg.plan_scan_shape(getattr(pkg, vt), 128, pkg.HAMMING)
    assert str(ei.value).startswith("vectorgpu error 5:") and "vg_plan_scan_shape: Hamming distance needs a uint8 corpus" in str(ei.value)
    with pytest.raises(pkg.VectorGpuError) as ei:              # an unknown metric keeps its refusal
        pkg.plan_scan_shape(getattr(pkg, vt), 128, 99)
    assert str(ei.value).startswith("vectorgpu error 1:") and "bad type / dim / metric" in str(ei.value)


def test_the_gpu_tests_row_lengths_cover_the_ladder(pkg):
    """the row lengths of the GPU tests: chunks per lane 1, 2, 3, 4, 6 and 8, a ragged row, and the long-row kernel"""
    shapes = {dim: pkg.plan_scan_shape(pkg.U8, dim, pkg.HAMMING) for dim in hc.ROW_BYTES + (hc.LONG_ROW_BYTES,)}
    assert {u for dim, (lpr, u, lng) in shapes.items() if not lng} >= {1, 2, 3, 4, 6, 8}, shapes
    assert shapes[hc.LONG_ROW_BYTES][2] and not any(shapes[dim][2] for dim in hc.ROW_BYTES), shapes
    lpr, u, _ = shapes[100]                                    # 7 chunks: no shape covers them exactly
    assert lpr * u > 7, shapes
