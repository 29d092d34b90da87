#!/usr/bin/env python3
"""Jaccard scans against Hamming and uint8 cosine on the same handle, in ONE process (10M rows of mixed bit density, k = 20):

  row lengths  128 bytes (1024 bits) and 32 bytes (256 bits); a row's bit density is drawn from 1/64, 1/8 and 1/2
  (a) single   scan_topk(JACCARD) against scan_topk(COSINE) - the same loop shape (two integer sums per dword and a query statistic),
               bit counts in place of v_dot4 and one divide in place of two square roots, a product and a divide: Jaccard's median
               is held to cosine's plus cosine's own min-to-max spread - and against scan_topk(HAMMING) (one sum, no divide), which
               is reported, not gated.  Cosine and Hamming are code the Jaccard change does not touch
  (b) batch    scan_topk_batch(JACCARD) at nq = 4 / 64 / 256 against nq single Jaccard scans, per query
  `kernels`: scan + merge kernels summed over the launches of one call, by the corpus' own profiling events; the multi-query scan
  the batch takes records no events, so the batch is compared on the host wall clock (`wall`), which both sides have.  Both come from
  the same timed steps.  Ratios are ratios of the medians; `spread` is min to max over the steps.

Warm-up, then repeated timed steps.  One JSON document on stdout.

    python tools/jaccard_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mixed_rows(rng, n, dim):
    """uint8 [n, dim]: a third of the rows each at bit density 1/2, 1/8 and 1/64 (one, three and six random bytes ANDed)"""
    rows = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    kind = rng.integers(0, 3, n)
    for at_least, rounds in ((1, 2), (2, 3)):
        sel = np.flatnonzero(kind >= at_least)
        for _ in range(rounds):
            rows[sel] &= rng.integers(0, 256, (sel.size, dim), dtype=np.uint8)
    return rows


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
        c.set_scan_filter(0)                                    # cosine on its PLAIN kernel (the nibble filter would serve it from 768 MB): the twin
        rng = np.random.default_rng(42 + dim)
        for r0 in range(0, N, 2_000_000):
            c.append(mixed_rows(rng, min(2_000_000, N - r0), dim))
        qs = mixed_rows(rng, max(args.nq), dim)
        qs[0, 0] |= 1                                           # (whatever density it drew: not an empty query)
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

        lpr, u, lng = pkg.plan_scan_shape(pkg.U8, dim, pkg.JACCARD)
        per_pass = pkg.batch_masked_plan(c, pkg.JACCARD)[0]     # the multi-query plan every batch form shares
        e = {"bits": 8 * dim, "lanes_per_row": lpr, "chunks_per_lane": u, "queries_per_pass": per_pass,
             "kernel_jaccard": c.kernel_name(pkg.JACCARD), "kernel_hamming": c.kernel_name(pkg.HAMMING),
             "kernel_cosine": c.kernel_name(pkg.COSINE), "hbm_floor_ms_at_8TBps": round(N * c_stride(dim) / 8e12 * 1e3, 4)}
        ids, dist = c.scan_topk(pkg.JACCARD, q, k)              # a full, ascending answer in [0, 1] before anything is timed
        assert np.all(np.diff(dist) >= 0) and len(ids) == k and dist[0] >= 0 and dist[-1] <= 1
        e["single_jaccard"] = measure(lambda: c.scan_topk(pkg.JACCARD, q, k))
        e["single_cosine"] = measure(lambda: c.scan_topk(pkg.COSINE, q, k))
        e["single_hamming"] = measure(lambda: c.scan_topk(pkg.HAMMING, q, k))
        jac, cos, ham = (e["single_" + m]["kernels"] for m in ("jaccard", "cosine", "hamming"))
        e["jaccard_minus_cosine_kernels_ms"] = round(jac["median_ms"] - cos["median_ms"], 4)
        e["jaccard_over_cosine_kernels"] = round(jac["median_ms"] / cos["median_ms"], 4)
        e["jaccard_within_cosine_spread"] = bool(jac["median_ms"] - cos["median_ms"] <= cos["spread_ms"])      # the bar
        e["jaccard_minus_hamming_kernels_ms"] = round(jac["median_ms"] - ham["median_ms"], 4)                  # reported, not gated
        e["jaccard_over_hamming_kernels"] = round(jac["median_ms"] / ham["median_ms"], 4)
        for nq in args.nq:
            qn = np.ascontiguousarray(qs[:nq])
            bi, bd, bc = c.scan_topk_batch(pkg.JACCARD, qn, k)
            path = c.last_batch_path()
            for i in (0, nq - 1):
                si, sd = c.scan_topk(pkg.JACCARD, qn[i], k)
                assert bi[i, :bc[i]].tolist() == si.tolist() and np.array_equal(bd[i, :bc[i]], sd), (dim, nq, i)
            b = {"batch_path": path, "batch": measure(lambda: c.scan_topk_batch(pkg.JACCARD, qn, k)),
                 "singles": measure(lambda: [c.scan_topk(pkg.JACCARD, qn[i], k) for i in range(nq)])}
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
