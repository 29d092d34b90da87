#!/usr/bin/env python3
"""Batch range scans against the only way to ask the same question without them, in ONE process (10M x 384 f32, L2):

  radii    per query: the midpoint behind its 20th and behind its 10 000th smallest distance (about 20 / about 10 000 rows match)
  batches  nq = 4, 16, 64
  per (radius, nq):
    kernels, summed over the launches of one batch (the corpus' own profiling events: set_profiling / profile_mean_ms):
      (w) scan_within_batch                 (a) nq calls of scan_within
    end to end, wall clock per batch:
      (W) scan_within_batch                 (A) nq calls of scan_within
  w_over_a / W_over_A are the ratios of the medians, from the same run.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout.

    python tools/within_batch_bench.py [--rows 10000000] [--steps 10] [--warmup 2]
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, nargs="*", default=[4, 16, 64])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, dim, metric = args.rows, 384, pkg.L2
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        nb = min(1_000_000, N - r0)
        t = torch.randn((nb, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), nb, dim * 4)
        del t
    rng = np.random.default_rng(43)
    nq_max = max(args.nq)
    qs = rng.standard_normal((nq_max, dim), dtype=np.float32)
    per_pass, lpr, u = pkg.within_batch_plan(c, metric)
    ranks = [r for r in (20, 10_000) if r < N]
    radii = {r: [] for r in ranks}
    for i in range(nq_max):                                    # radii from the engine's own distances, query by query
        own = c.scan_distances(metric, qs[i])
        part = np.partition(own, [r - 1 for r in ranks] + [r for r in ranks])
        for r in ranks:
            radii[r].append(0.5 * (float(part[r - 1]) + float(part[r])))

    def kernel_ms(fn):
        """kernel milliseconds of ONE call of fn, summed over its launches (mean per launch x launches)"""
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

    out = {"rows": N, "dim": dim, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u,
           "single_kernel": c.kernel_name(metric), "steps": args.steps, "warmup": args.warmup, "radii": {}}
    for rank in ranks:
        r = {}
        for nq in args.nq:
            q = np.ascontiguousarray(qs[:nq])
            rr = radii[rank][:nq]
            singles = lambda: [c.scan_within(metric, q[i], rr[i]) for i in range(nq)]
            batch = lambda: c.scan_within_batch(metric, q, rr)
            got = batch()
            for i, (si, sd, sm) in enumerate(singles()):        # the same rows before anything is timed
                assert got[i][0].tolist() == si.tolist() and got[i][2] == sm, (rank, nq, i)
            e = {"matches_per_query": float(np.mean([x[2] for x in got])), "launches": c.within_batch_last_launches(),
                 "w_batch_within_kernels": kernel_ms(batch), "a_single_within_kernels": kernel_ms(singles),
                 "W_batch_within": wall_ms(batch), "A_single_within": wall_ms(singles)}
            e["w_over_a"] = round(e["w_batch_within_kernels"]["median_ms"] / e["a_single_within_kernels"]["median_ms"], 4)
            e["W_over_A"] = round(e["W_batch_within"]["median_ms"] / e["A_single_within"]["median_ms"], 4)
            r["nq_%d" % nq] = e
        out["radii"]["about_%d_rows" % rank] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
