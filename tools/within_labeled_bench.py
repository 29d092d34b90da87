#!/usr/bin/env python3
"""Labeled batch range scans against the two ways to ask the same question without them, in ONE process (10M x 384 f32, L2):

  labels   16 / 256 / 4096 tenants of equal size, uniformly random rows and run-clustered (every tenant one contiguous run)
  batches  nq = 4, 16, 64, two query mixes: "own" - every query its own label (tenant i % tenants) - and "one" - all queries tenant 0
  radii    per query: the midpoint behind the 20th smallest distance among the rows of ITS label
  per (labels, mix, nq):
    kernels, summed over the launches of one call (the corpus' own profiling events: set_profiling / profile_mean_ms; the bitmap
    kernel of a single labeled range scan is not in the event ring - its cost shows in the wall clock only):
      (l) scan_within_batch_labeled         (s) nq calls of scan_within_labeled on the same handle
      (u) scan_within_batch over ALL rows with the same radii
    end to end, wall clock per call:
      (L) scan_within_batch_labeled         (S) nq calls of scan_within_labeled - the fallback of the batch form
      (U) scan_within_batch + the other tenants' rows thrown away on the host
  l_over_s / l_over_u / L_over_S / L_over_U are the ratios of the medians, from the same run.  Nothing is asserted about a timing.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout: run it on an MI355X, keep the output as
profiles/within_labeled_bench_10Mx384_f32_l2.json and put the figures into the README and DESIGN.md 3.21.

    python tools/within_labeled_bench.py [--rows 10000000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RANK = 20                                                      # matches per query among the rows of its label


def make_labels(n, tenants, clustered, rng):
    """equal-sized tenants: a random permutation of (row % tenants), or one contiguous run per tenant"""
    if clustered:
        return (np.arange(n, dtype=np.int64) * tenants // n).astype(np.uint32)
    lab = (np.arange(n, dtype=np.int64) % tenants).astype(np.uint32)
    rng.shuffle(lab)
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, nargs="*", default=[4, 16, 64])
    ap.add_argument("--tenants", type=int, nargs="*", default=[16, 256, 4096])
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
    own = [c.scan_distances(metric, qs[i]) for i in range(nq_max)]      # radii from the engine's own distances
    per_pass, lpr, u = pkg.within_batch_labeled_plan(c, metric)

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

    out = {"rows": N, "dim": dim, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u, "matches_per_query": RANK,
           "single_kernel": c.kernel_name(metric), "steps": args.steps, "warmup": args.warmup, "labels": {}}
    lrng = np.random.default_rng(44)
    for tenants in args.tenants:
        if N // tenants <= RANK:
            continue
        for clustered in (False, True):
            name = "%s_%d" % ("clustered" if clustered else "random", tenants)
            labels = make_labels(N, tenants, clustered, lrng)
            c.set_labels(labels)
            r = {"rows_per_tenant": N // tenants}
            for mix in ("own", "one"):
                for nq in args.nq:
                    q = np.ascontiguousarray(qs[:nq])
                    ql = np.array([(i % tenants) if mix == "own" else 0 for i in range(nq)], dtype=np.uint32)
                    radii = []
                    for i in range(nq):
                        part = np.partition(own[i][labels == ql[i]], [RANK - 1, RANK])
                        radii.append(0.5 * (float(part[RANK - 1]) + float(part[RANK])))

                    batch = lambda: c.scan_within_batch_labeled(metric, q, ql, radii)
                    singles = lambda: [c.scan_within_labeled(metric, q[i], radii[i], int(ql[i])) for i in range(nq)]
                    unlabeled = lambda: c.scan_within_batch(metric, q, radii)

                    def host_filtered():
                        return [(ids[labels[ids - 1] == ql[i]], dist[labels[ids - 1] == ql[i]]) for i, (ids, dist, _) in enumerate(unlabeled())]

                    got = batch()                                       # the same rows before anything is timed
                    for i, (ui, ud) in enumerate(host_filtered()):
                        assert got[i][0].tolist() == ui.tolist() and got[i][2] == len(ui), (name, mix, nq, i)
                    e = {"matches_per_query": float(np.mean([x[2] for x in got])), "matches_per_query_all_rows": float(np.mean([x[2] for x in unlabeled()])),
                         "launches_batch": c.within_batch_last_launches(),
                         "l_batch_labeled_kernels": kernel_ms(batch), "s_single_labeled_kernels": kernel_ms(singles),
                         "u_batch_all_rows_kernels": kernel_ms(unlabeled),
                         "L_batch_labeled": wall_ms(batch), "S_single_labeled": wall_ms(singles), "U_batch_all_rows_host_filter": wall_ms(host_filtered)}
                    e["l_over_s"] = round(e["l_batch_labeled_kernels"]["median_ms"] / e["s_single_labeled_kernels"]["median_ms"], 4)
                    e["l_over_u"] = round(e["l_batch_labeled_kernels"]["median_ms"] / e["u_batch_all_rows_kernels"]["median_ms"], 4)
                    e["L_over_S"] = round(e["L_batch_labeled"]["median_ms"] / e["S_single_labeled"]["median_ms"], 4)
                    e["L_over_U"] = round(e["L_batch_labeled"]["median_ms"] / e["U_batch_all_rows_host_filter"]["median_ms"], 4)
                    r["%s_nq_%d" % (mix, nq)] = e
            out["labels"][name] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
