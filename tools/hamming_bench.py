#!/usr/bin/env python3
"""Hamming scans against their uint8 L1 twins on the same handle, in ONE process (10M rows of random bytes, k = 20):

  row lengths  128 bytes (1024 bits) and 32 bytes (256 bits)
  (a) single   scan_topk(HAMMING) against scan_topk(L1): the same bytes, loop and epilogue class, one v_sad_u8 per dword in place of
               v_xor + v_bcnt - L1 is code the Hamming change does not touch
  (b) batch    scan_topk_batch(HAMMING) at nq = 4 / 64 / 256 against nq single Hamming scans, per query
  `kernels`: scan + merge kernels summed over the launches of one call, by the corpus' own profiling events; the multi-query scan
  the batch takes records no events, so the batch is compared on the host wall clock (`wall`), which both sides have.  Both come from
  the same timed steps.  Ratios are ratios of the medians; `spread` is min to max over the steps.

Warm-up, then repeated timed steps.  One JSON document on stdout.

    python tools/hamming_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--row-bytes", type=int, nargs="*", default=[128, 32])
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k = args.rows, 20
    out = {"rows": N, "k": k, "steps": args.steps, "warmup": args.warmup, "row_bytes": {}}
    for dim in args.row_bytes:
        c = pkg.Corpus(pkg.U8, dim, capacity=N)
        rng = np.random.default_rng(42 + dim)
        for r0 in range(0, N, 2_000_000):
            c.append(rng.integers(0, 256, (min(2_000_000, N - r0), dim), dtype=np.uint8))
        qs = rng.integers(0, 256, (max(args.nq), dim), dtype=np.uint8)
        q = qs[0]

        def measure(fn):
            """kernel (event) and wall time of the same steps"""
            for _ in range(args.warmup):
                fn()
            kern, wall = [], []
            for _ in range(args.steps):
                c.set_profiling(True)
                t0 = time.perf_counter()
                fn()
                wall.append((time.perf_counter() - t0) * 1e3)
                n, scan, merge = c.profile_mean_ms()
                kern.append(n * (scan + merge))
            c.set_profiling(False)
            st = lambda a, nd: {"min_ms": round(float(np.min(a)), nd), "median_ms": round(float(np.median(a)), nd),
                                "max_ms": round(float(np.max(a)), nd), "spread_ms": round(float(np.max(a) - np.min(a)), nd)}
            return {"kernels": st(kern, 4) if max(kern) > 0 else None, "wall": st(wall, 3)}

        lpr, u, lng = pkg.plan_scan_shape(pkg.U8, dim, pkg.HAMMING)
        per_pass = pkg.batch_masked_plan(c, pkg.HAMMING)[0]     # the multi-query plan every batch form shares
        e = {"bits": 8 * dim, "lanes_per_row": lpr, "chunks_per_lane": u, "queries_per_pass": per_pass,
             "kernel_hamming": c.kernel_name(pkg.HAMMING), "kernel_l1": c.kernel_name(pkg.L1),
             "hbm_floor_ms_at_8TBps": round(N * c_stride(dim) / 8e12 * 1e3, 4)}
        ids, dist = c.scan_topk(pkg.HAMMING, q, k)              # a full, ascending answer before anything is timed
        assert np.all(np.diff(dist) >= 0) and len(ids) == k
        e["single_hamming"] = measure(lambda: c.scan_topk(pkg.HAMMING, q, k))
        e["single_l1"] = measure(lambda: c.scan_topk(pkg.L1, q, k))
        e["hamming_over_l1_kernels"] = round(e["single_hamming"]["kernels"]["median_ms"] / e["single_l1"]["kernels"]["median_ms"], 4)
        e["hamming_minus_l1_kernels_ms"] = round(e["single_hamming"]["kernels"]["median_ms"] - e["single_l1"]["kernels"]["median_ms"], 4)
        e["hamming_over_l1_wall"] = round(e["single_hamming"]["wall"]["median_ms"] / e["single_l1"]["wall"]["median_ms"], 4)
        for nq in args.nq:
            qn = np.ascontiguousarray(qs[:nq])
            bi, bd, bc = c.scan_topk_batch(pkg.HAMMING, qn, k)
            path = c.last_batch_path()
            for i in (0, nq - 1):
                si, sd = c.scan_topk(pkg.HAMMING, qn[i], k)
                assert bi[i, :bc[i]].tolist() == si.tolist() and np.array_equal(bd[i, :bc[i]], sd), (dim, nq, i)
            b = {"batch_path": path, "batch": measure(lambda: c.scan_topk_batch(pkg.HAMMING, qn, k)),
                 "singles": measure(lambda: [c.scan_topk(pkg.HAMMING, qn[i], k) for i in range(nq)])}
            b["batch_per_query_wall_ms"] = round(b["batch"]["wall"]["median_ms"] / nq, 4)
            b["singles_per_query_wall_ms"] = round(b["singles"]["wall"]["median_ms"] / nq, 4)
            b["singles_per_query_kernels_ms"] = round(b["singles"]["kernels"]["median_ms"] / nq, 4)
            b["singles_over_batch_wall"] = round(b["singles"]["wall"]["median_ms"] / b["batch"]["wall"]["median_ms"], 4)
            e["batch_nq_%d" % nq] = b
        out["row_bytes"][str(dim)] = e
        c.close()
    print(json.dumps(out, indent=1))


def c_stride(dim):
    return (dim + 15) // 16 * 16


if __name__ == "__main__":
    main()
