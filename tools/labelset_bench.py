#!/usr/bin/env python3
"""Label-set batch scans against the two ways the code before them answers the same questions, in ONE process (10M x 384 f32, L2, k = 20):

  labels   4096 tenants of equal size, uniformly random rows and run-clustered (every tenant one contiguous run)
  sets     1 / 8 / 64 labels per query, every query its own set (query i: tenants i * s .. i * s + s - 1, modulo the tenants)
  batches  nq = 4, 64, 256
  per (labels, set size, nq), kernels summed over the launches of one batch (the corpus' own profiling events; the bitmap and
  membership kernels are not in the event ring - their cost shows in the wall clock only) and wall clock per batch:
      (s) scan_topk_batch_labelset
      (a) the parent's only answer: per query np.isin on the host + set_mask + scan_topk_masked
      (b) set size 1 only: scan_topk_batch_labeled with the one-label sets, the twin without sets
  s_over_a / s_over_b are ratios of the medians, from the same run.  A shape at which s_over_a (wall) comes out above 1 is one the
  batch form should hand to its fallback.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout.

    python tools/labelset_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from labeled_bench import make_labels  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[4, 64, 256])
    ap.add_argument("--set-sizes", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--tenants", type=int, default=4096)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k, dim, metric = args.rows, 20, 384, pkg.L2
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    rng = np.random.default_rng(42)
    for r0 in range(0, N, 500_000):                             # rows are drawn on the host, half a million at a time
        c.append(rng.standard_normal((min(500_000, N - r0), dim), dtype=np.float32))
    c.set_tie_order(pkg.TIE_POSITION)
    nq_max = max(args.nq)
    qs = rng.standard_normal((nq_max, dim), dtype=np.float32)
    per_pass, lpr, u = pkg.batch_labelset_plan(c, metric)

    def kernel_ms(fn):
        for _ in range(args.warmup):
            fn()
        per = []
        for _ in range(args.steps):
            c.set_profiling(True)
            fn()
            n, scan, merge = c.profile_mean_ms()
            per.append(n * (scan + merge))
        c.set_profiling(False)
        return {"min_ms": round(float(np.min(per)), 4), "median_ms": round(float(np.median(per)), 4), "max_ms": round(float(np.max(per)), 4)}

    def wall_ms(fn):
        for _ in range(args.warmup):
            fn()
        per = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            per.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": round(float(np.min(per)), 3), "median_ms": round(float(np.median(per)), 3)}

    out = {"rows": N, "dim": dim, "k": k, "tenants": args.tenants, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u,
           "steps": args.steps, "warmup": args.warmup, "labels": {}}
    lrng = np.random.default_rng(44)
    for clustered in (False, True):
        name = "clustered" if clustered else "random"
        labels = make_labels(N, args.tenants, clustered, lrng)
        c.set_labels(labels)
        r = {}
        for s in args.set_sizes:
            for nq in args.nq:
                q = np.ascontiguousarray(qs[:nq])
                sets = [((i * s + np.arange(s)) % args.tenants).astype(np.uint32) for i in range(nq)]

                def masked_way():
                    res = []
                    for i in range(nq):
                        c.set_mask(bits=np.isin(labels, sets[i]))
                        res.append(c.scan_topk_masked(metric, q[i], k))
                    return res

                batch = lambda: c.scan_topk_batch_labelset(metric, q, sets, k)
                ids, dist, cnt = batch()
                for i, (si, sd) in enumerate(masked_way()):     # the same rows before anything is timed
                    assert ids[i, :cnt[i]].tolist() == si.tolist(), (name, s, nq, i)
                e = {"s_kernels": kernel_ms(batch), "a_kernels": kernel_ms(masked_way), "s_wall": wall_ms(batch), "a_wall": wall_ms(masked_way)}
                e["s_over_a_kernels"] = round(e["s_kernels"]["median_ms"] / e["a_kernels"]["median_ms"], 4)
                e["s_over_a_wall"] = round(e["s_wall"]["median_ms"] / e["a_wall"]["median_ms"], 4)
                if s == 1:
                    ql = np.array([int(x[0]) for x in sets], dtype=np.uint32)
                    twin = lambda: c.scan_topk_batch_labeled(metric, q, ql, k)
                    e["b_kernels"], e["b_wall"] = kernel_ms(twin), wall_ms(twin)
                    e["s_over_b_kernels"] = round(e["s_kernels"]["median_ms"] / e["b_kernels"]["median_ms"], 4)
                    e["s_over_b_wall"] = round(e["s_wall"]["median_ms"] / e["b_wall"]["median_ms"], 4)
                r["set_%d_nq_%d" % (s, nq)] = e
        out["labels"][name] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
