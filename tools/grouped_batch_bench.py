#!/usr/bin/env python3
"""Grouped batch scans against the two things they can be compared with, in ONE process over ONE corpus (k = 20):

  corpus   10M x 384 f32, L2 (--rows / --dim to change it), random labels of about 100 rows each
  (g) scan_topk_batch_grouped, nq queries        the grouped form of the multi-query scan
  (a) nq scan_topk_grouped calls, same handle    the only answer before the batch form (its code is unchanged)
  (b) scan_topk_batch_masked, all-allowed mask   the twin without labels, at the same nq
  nq = 4, 64, 256

  kernel time: the corpus' own profiling events (set_profiling / profile_mean_ms: scan kernel + merge kernel, mean per launch times
  the launches of the call), medians of --steps steps behind --warmup warm-up calls.  No ratio is fixed in advance: per_query_ms
  and the two ratios are what this run measured.

One JSON document on stdout.

    python tools/grouped_batch_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="+", default=[4, 64, 256])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, dim, k, metric = args.rows, args.dim, 20, pkg.L2
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        nb = min(1_000_000, N - r0)
        t = torch.randn((nb, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), nb, dim * 4)
        del t
    c.set_tie_order(pkg.TIE_POSITION)
    c.set_scan_filter(0)
    rng = np.random.default_rng(43)
    labels = rng.integers(0, max(1, N // 100), N).astype(np.uint32)
    c.set_labels(labels)
    c.set_mask(bits=np.ones(N, dtype=bool))

    def kernel_ms(fn, steps):
        for _ in range(min(args.warmup, steps)):
            fn()
        tot = []
        for _ in range(steps):
            c.set_profiling(True)
            fn()
            launches, s, m = c.profile_mean_ms()
            tot.append(launches * (s + m))
        c.set_profiling(False)
        tot = np.array(tot)
        return {"min_ms": round(float(tot.min()), 4), "median_ms": round(float(np.median(tot)), 4), "max_ms": round(float(tot.max()), 4)}

    out = {"rows": N, "dim": dim, "k": k, "steps": args.steps, "warmup": args.warmup,
           "plan_grouped": pkg.batch_grouped_plan(c, metric), "plan_masked": pkg.batch_masked_plan(c, metric), "runs": []}
    for nq in args.nq:
        qs = rng.standard_normal((nq, dim), dtype=np.float32)
        batch = c.scan_topk_batch_grouped(metric, qs, k)
        one = c.scan_topk_grouped(metric, qs[0], k)             # the same labels as the single form before anything is timed
        assert batch[2][0, :batch[3][0]].tolist() == one[2].tolist(), nq

        def singles():
            for i in range(nq):
                c.scan_topk_grouped(metric, qs[i], k)

        run = {"nq": nq,
               "g_batch_grouped": kernel_ms(lambda: c.scan_topk_batch_grouped(metric, qs, k), args.steps),
               "a_single_grouped_calls": kernel_ms(singles, args.steps if nq <= 64 else max(3, args.steps // 4)),
               "b_batch_masked_all_allowed": kernel_ms(lambda: c.scan_topk_batch_masked(metric, qs, k), args.steps)}
        for name in ("g_batch_grouped", "a_single_grouped_calls", "b_batch_masked_all_allowed"):
            run[name]["per_query_ms"] = round(run[name]["median_ms"] / nq, 4)
        run["g_over_a"] = round(run["g_batch_grouped"]["median_ms"] / run["a_single_grouped_calls"]["median_ms"], 4)
        run["g_over_b"] = round(run["g_batch_grouped"]["median_ms"] / run["b_batch_masked_all_allowed"]["median_ms"], 4)
        out["runs"].append(run)
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
