#!/usr/bin/env python3
"""Range scans against the scans they sit next to, in ONE process on ONE 10M x 384 f32 corpus (L2):

  kernels, timed with the corpus' own profiling events (set_profiling / profile_mean_ms):
    (a) the plain top-20 kernel          (b) the store-mode kernel (all N distances written)
    (c) the within kernel at radii matching about 20, 10 000 and 1 000 000 rows
  end to end, wall clock:
    (d) scan_within                      (e) scan_distances + a numpy filter and sort

(a) and (b) are the yardsticks for (c) - from the same run.  Warm-up, then repeated timed steps; min / median are printed.

    python tools/within_bench.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5]
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
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, dim = args.rows, args.dim
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        nb = min(1_000_000, N - r0)
        t = torch.randn((nb, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), nb, dim * 4)
        del t
    c.set_scan_filter(0)                      # (a) is the PLAIN top-k kernel, the one the within kernel is an instantiation of
    q = np.random.default_rng(43).standard_normal(dim, dtype=np.float32)
    own = c.scan_distances(pkg.L2, q)
    targets = [m for m in (20, 10_000, 1_000_000) if m < N]
    part = np.partition(own, [m - 1 for m in targets])
    radii = {m: float(part[m - 1]) for m in targets}

    def kernel_ms(fn):
        for _ in range(args.warmup):
            fn()
        per = []
        for _ in range(args.steps):
            c.set_profiling(True)
            fn()
            n, scan, merge = c.profile_mean_ms()
            per.append(scan)
        c.set_profiling(False)
        return {"min_ms": round(float(np.min(per)), 4), "median_ms": round(float(np.median(per)), 4), "launches_per_call": n}

    def wall_ms(fn):
        for _ in range(args.warmup):
            fn()
        per = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            fn()
            per.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": round(float(np.min(per)), 3), "median_ms": round(float(np.median(per)), 3)}

    def filtered(radius):
        d = c.scan_distances(pkg.L2, q)
        pos = np.nonzero(d <= radius)[0]
        order = np.lexsort((pos, d[pos]))
        return pos[order] + 1, d[pos][order]

    out = {"rows": N, "dim": dim, "kernel": c.kernel_name(pkg.L2), "steps": args.steps, "warmup": args.warmup}
    out["a_topk20_kernel"] = kernel_ms(lambda: c.scan_topk(pkg.L2, q, 20))
    out["b_store_mode_kernel"] = kernel_ms(lambda: c.scan_distances(pkg.L2, q))
    for m in targets:
        r = radii[m]
        ids, dist, matches = c.scan_within(pkg.L2, q, r)
        fids, fdist = filtered(r)
        assert ids.tolist() == fids.tolist() and np.array_equal(dist, fdist.astype(np.float64))
        out["c_within_kernel_%d" % m] = dict(kernel_ms(lambda: c.scan_within(pkg.L2, q, r)), matches=matches)
        out["d_scan_within_%d" % m] = wall_ms(lambda: c.scan_within(pkg.L2, q, r))
        out["e_scan_distances_numpy_%d" % m] = wall_ms(lambda: filtered(r))
        out["e_over_d_%d" % m] = round(out["e_scan_distances_numpy_%d" % m]["median_ms"] / out["d_scan_within_%d" % m]["median_ms"], 2)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
