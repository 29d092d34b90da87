#!/usr/bin/env python3
"""Capped batch scans against the two things they can be compared with, in ONE process over ONE corpus (k = 20, m = 3):

  corpus   10M x 384 f32, L2 (--rows / --dim to change it), two label layouts in turn:
             random   random labels of about 100 rows each
             hot      the same, with one label on the 1 000 rows nearest to query 0 (a top-64-then-cap sees that label only)
  (c) scan_topk_batch_capped, nq queries         the capped form of the multi-query scan
  (a) nq scan_topk_capped calls, same handle     the only exact answer before the batch form (its code is unchanged)
  (b) scan_topk_batch_grouped, nq queries        the twin whose lists hold one row per label
  nq = 4, 64, 256 - the first nq of one set of queries, so query 0 is the same in every run

  kernel time: the corpus' own profiling events (set_profiling / profile_mean_ms: scan kernel + merge kernel, mean per launch times
  the launches of the call), min / median / max of --steps steps behind --warmup warm-up calls.  No ratio is fixed in advance:
  per_query_ms and the two ratios are what this run measured; c_outside_a_spread says whether the capped batch's slowest step per
  query is below the fastest step of (a) per query.

One JSON document on stdout.

    python tools/capped_batch_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
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
    ap.add_argument("--per-label", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="+", default=[4, 64, 256])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, dim, k, m, metric = args.rows, args.dim, 20, args.per_label, pkg.L2
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
    random_labels = rng.integers(2, max(3, N // 100), N).astype(np.uint32)
    all_qs = rng.standard_normal((max(args.nq), dim), dtype=np.float32)
    d0 = c.scan_distances(metric, all_qs[0])
    hot_labels = random_labels.copy()
    hot_labels[np.lexsort((np.arange(N), d0))[:1000]] = 1
    del d0

    def kernel_ms(fn, steps):
        for _ in range(min(args.warmup, steps)):
            fn()
        tot = []
        for _ in range(steps):
            c.set_profiling(True)
            fn()
            launches, s, mg = c.profile_mean_ms()
            tot.append(launches * (s + mg))
        c.set_profiling(False)
        tot = np.array(tot)
        return {"min_ms": round(float(tot.min()), 4), "median_ms": round(float(np.median(tot)), 4), "max_ms": round(float(tot.max()), 4)}

    out = {"rows": N, "dim": dim, "k": k, "per_label": m, "steps": args.steps, "warmup": args.warmup,
           "plan_capped": pkg.batch_capped_plan(c, metric), "plan_grouped": pkg.batch_grouped_plan(c, metric), "runs": []}
    for layout, labels in (("random", random_labels), ("hot", hot_labels)):
        c.set_labels(labels)
        for nq in args.nq:
            qs = np.ascontiguousarray(all_qs[:nq])
            batch = c.scan_topk_batch_capped(metric, qs, k, m)
            one = c.scan_topk_capped(metric, qs[0], k, m)       # the same labels as the single form before anything is timed
            assert batch[2][0, :batch[3][0]].tolist() == one[2].tolist(), (layout, nq)
            if layout == "hot":
                assert one[2].tolist()[:m] == [1] * m and 1 not in one[2].tolist()[m:], (layout, nq)

            def singles():
                for i in range(nq):
                    c.scan_topk_capped(metric, qs[i], k, m)

            run = {"layout": layout, "nq": nq,
                   "c_batch_capped": kernel_ms(lambda: c.scan_topk_batch_capped(metric, qs, k, m), args.steps),
                   "a_single_capped_calls": kernel_ms(singles, args.steps),
                   "b_batch_grouped": kernel_ms(lambda: c.scan_topk_batch_grouped(metric, qs, k), args.steps)}
            for name in ("c_batch_capped", "a_single_capped_calls", "b_batch_grouped"):
                run[name]["per_query_ms"] = round(run[name]["median_ms"] / nq, 4)
            run["c_over_a"] = round(run["c_batch_capped"]["median_ms"] / run["a_single_capped_calls"]["median_ms"], 4)
            run["c_over_b"] = round(run["c_batch_capped"]["median_ms"] / run["b_batch_grouped"]["median_ms"], 4)
            run["c_outside_a_spread"] = bool(run["c_batch_capped"]["max_ms"] < run["a_single_capped_calls"]["min_ms"])
            run["c_median_above_b_max"] = bool(run["c_batch_capped"]["median_ms"] > run["b_batch_grouped"]["max_ms"])
            out["runs"].append(run)
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
