"""CPU-only checks of the paged scans' host side: vg_after_floor against a numpy restatement of the cursor contract
(include/vectorgpu.h), the new symbols exported and bound, and no quiet fall-back without a device.

Contract: the row at scan position p with float distance d is behind the cursor (D, P) - P = rows held with rowid <= the cursor's
rowid - iff d < +Inf and ((double)d > D, or (double)d == D and p >= P).  The kernel admits a key iff key >= floor, key(d, p) =
sortable(d) << 32 | p.  No row holds -0.0 (vg_clamp), so the generated distances never do."""
import ctypes as C

import numpy as np
import pytest

VG_ERR_INVALID = 1
KEY_EMPTY = 0xFFFFFFFFFFFFFFFF
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g._load_build().build_gpu_library()
    return g.load_package()


def _key(d, p):
    b = int(np.float32(d).view(np.uint32))
    s = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
    return (s << 32) | int(p)


def _behind(D, P, d, p):
    """the contract's predicate, in doubles"""
    d = float(np.float32(d))
    D = D + 0.0
    return d < np.inf and (d > D or (d == D and p >= P))


def _floats_around():
    vals = [0.0, 1.0, -1.0, 3.5, -3.5, 1e-45, -1e-45, 1e-38, FLT_MAX, -FLT_MAX, float("-inf"), 0.1, -0.1, 8.0 * 2.0 ** -23, 1e30, -1e30]
    out = []
    for v in vals:
        f = np.float32(v)
        out += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return [x for x in out if not np.isnan(x) and not (x == 0 and np.signbit(x))]


def test_floor_of_named_cursors(pkg):
    held = np.float32(0.1)
    up = np.nextafter(held, np.float32(np.inf))
    mid = (float(held) + float(up)) / 2.0
    assert float(np.float32(mid)) != mid                         # a double that is no float
    cursors = [float(held), mid, -0.0, 0.0, float("-inf"), -1e300, -3.25, float(np.float32(-0.1)), FLT_MAX, 1e-50, -1e-50]
    rows_d = _floats_around() + [held, up]
    for D in cursors:
        for P in (0, 1, 77, 2 ** 32 - 1):
            floor, empty = pkg.after_floor(D, P)
            assert not empty, (D, P)
            for d in rows_d:
                for p in (0, P - 1 if P else 0, P, min(P + 1, 2 ** 32 - 1), 2 ** 32 - 1):
                    want = _behind(D, P, d, p)
                    assert (_key(d, p) >= floor) == want or not float(d) < np.inf, (D, P, float(d), p, hex(floor))
    # -0.0 is 0.0
    assert pkg.after_floor(-0.0, 5) == pkg.after_floor(0.0, 5) == (_key(0.0, 5), False)
    # a held float: exactly its key at P; a midpoint: the next float up at position 0
    assert pkg.after_floor(float(held), 9) == (_key(held, 9), False)
    assert pkg.after_floor(mid, 9) == (_key(up, 0), False)
    # the start cursor admits a -Inf row at position 0
    assert pkg.after_floor(float("-inf"), 0) == (_key(float("-inf"), 0), False)
    assert pkg.after_floor(-1e300, 3) == (_key(-FLT_MAX, 0), False)          # -Inf rows are in FRONT of -1e300
    # nothing can be behind these
    for D in (float("inf"), 1e300, FLT_MAX * (1 + 1e-9)):
        assert pkg.after_floor(D, 0) == (KEY_EMPTY, True)
    assert pkg.after_floor(FLT_MAX, 4) == (_key(FLT_MAX, 4), False)
    with pytest.raises(pkg.VectorGpuError) as ei:
        pkg.after_floor(float("nan"), 0)
    assert "error %d" % VG_ERR_INVALID in str(ei.value)
    assert pkg.lib().vg_after_floor(0.0, 0, None, None) == VG_ERR_INVALID


def test_floor_property_random(pkg):
    rng = np.random.default_rng(20261019)
    n = 10000
    pool = rng.standard_normal(64).astype(np.float32) * np.float32(10)      # few values: (double)d == D happens
    bad = 0
    for i in range(n):
        kind = i % 4
        d = pool[rng.integers(64)] if kind < 3 else np.float32(rng.standard_normal() * 10 ** rng.uniform(-40, 38))
        if kind == 0:
            D = float(pool[rng.integers(64)])                                # a held float
        elif kind == 1:
            a = pool[rng.integers(64)]
            D = (float(a) + float(np.nextafter(a, np.float32(np.inf)))) / 2  # a midpoint double
        else:
            D = float(rng.standard_normal() * 10 ** rng.uniform(-3, 3))
        P = int(rng.integers(0, 2 ** 32)) if i % 3 else int(rng.integers(0, 8))
        p = int(rng.integers(0, 2 ** 32)) if i % 5 else min(max(P + int(rng.integers(-2, 3)), 0), 2 ** 32 - 1)
        if d == 0:
            d = np.float32(0.0)
        floor, empty = pkg.after_floor(D, P)
        assert not empty
        bad += (_key(d, p) >= floor) != _behind(D, P, d, p)
    assert bad == 0


def test_new_symbols_exported_and_bound(pkg):
    lib = pkg.lib()
    names = ["vg_after_floor"]
    for pre in ("vg_scan_topk_", "vg_shards_scan_topk_"):
        for b in ("", "batch_"):
            for m in ("", "_masked"):
                for kform in ("", "_keys"):
                    names.append(pre + b + "after" + m + kform)
    assert len(names) == 17
    for name in names:
        assert hasattr(lib, name), name
        assert name in lib._sig, name
    for cls in (pkg.Corpus, pkg.Shards):
        for meth in ("scan_topk_after", "scan_topk_after_keys", "scan_topk_batch_after", "scan_topk_batch_after_keys"):
            assert callable(getattr(cls, meth))


def test_compute_entry_points_fail_loudly_without_device(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = pkg.lib()
    cnt = C.c_int(7)
    q = np.zeros(8, dtype=np.float32)
    out = np.zeros(64, dtype=np.uint64)
    for name in ("vg_scan_topk_after_keys", "vg_scan_topk_after_masked_keys", "vg_shards_scan_topk_after_keys"):
        rc = getattr(lib, name)(None, 1, q.ctypes.data_as(C.c_void_p), 5, 0, out.ctypes.data_as(C.c_void_p), C.byref(cnt))
        assert rc != 0 and lib.vg_last_error(), name           # no corpus can exist without a device: an error, never an answer
    with pytest.raises(pkg.VectorGpuError):
        pkg.Corpus(pkg.F32, 8)
