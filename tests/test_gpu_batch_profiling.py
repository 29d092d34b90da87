"""The profiling ring under batches: every call of a matrix-core batch driver (vg_batch_api.hip) claims ONE slot of the ring -
start event behind the query upload, end events behind the launch - so a batch of one slice counts one recorded launch with a
positive scan time and a batch of two slices counts two.  Each driver runs at the smallest shape the other tests reach it with, on
a fresh corpus (its work buffers and derived copies are made by the profiled batch itself), and last_batch_path() pins the driver:
a batch that fell through to another path cannot pass for the one under test.  Random rows and queries: none the filters cannot
judge (those would add a single scan - a slot - each)."""
import numpy as np
import pytest

import datagen as dg
from test_gpu_scan import pkg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# (driver, path, element type, dim, rows, queries of the one-slice batch, floor of VG_BATCH_SLICE, environment)
CASES = [
    pytest.param(7, dg.F32, 64, 65_536, 40, 512, {"VG_BATCH_Q8": "1"}, id="int8-filter"),        # as test_gpu_batch_q8.py: forced, 2048 tiles
    pytest.param(4, dg.F16, 1536, 4133, 70, 256, {}, id="long-rows"),                            # as test_gpu_scan.py's long-row corpus
    pytest.param(2, dg.U8, 64, 3000, 40, 256, {}, id="uint8"),
    pytest.param(3, dg.F16, 64, 3000, 40, 256, {}, id="f16"),
]


@pytest.mark.parametrize("path, vt, dim, n, nq, slice_floor, env", CASES)
def test_one_ring_slot_per_slice_of_a_batch(pkg, monkeypatch, path, vt, dim, n, nq, slice_floor, env):
    for name in ("VG_BATCH_Q8", "VG_BATCH_MFMA", "VG_BATCH_LONG", "VG_BATCH_SLICE", "VG_F32_FILTER", "VG_BATCH_MIN_QUERIES"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    rows = dg.corpus(vt, n, dim, 9100 + path)
    qs = dg.corpus(vt, slice_floor + 1, dim, 9200 + path)
    c = pkg.Corpus(vt, dim)
    c.append(rows)
    k = 5

    c.set_profiling(True)                                     # (also restarts the count)
    _, _, cnt = c.scan_topk_batch(dg.COSINE, qs[:nq], k)
    assert c.last_batch_path() == path, (c.last_batch_path(), c.batch_q8_status())
    assert cnt.tolist() == [k] * nq
    launches, scan_ms, _ = c.profile_mean_ms()
    print("path %d, one slice: %d launches, %.4f ms" % (path, launches, scan_ms))
    assert launches == 1 and scan_ms > 0.0, (launches, scan_ms)

    monkeypatch.setenv("VG_BATCH_SLICE", "1")                 # below the floor: slices of 256 queries (512 for the int8 filter)
    c.set_profiling(True)
    _, _, cnt = c.scan_topk_batch(dg.COSINE, qs, k)           # one more query than a slice
    assert c.last_batch_path() == path, (c.last_batch_path(), c.batch_q8_status())
    assert cnt.tolist() == [k] * (slice_floor + 1)
    launches, scan_ms, _ = c.profile_mean_ms()
    print("path %d, two slices: %d launches, %.4f ms" % (path, launches, scan_ms))
    assert launches == 2 and scan_ms > 0.0, (launches, scan_ms)
    c.close()
