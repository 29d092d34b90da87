#!/usr/bin/env python3
"""Grouped scans against the plain top-k scan and against the only way the code before them answers the same question, in ONE
process over ONE corpus (k = 20):

  corpus   10M x 384 f32, L2 (--rows / --dim to change it)
  (p) scan_topk                          the parent's plain fused top-k: the figure the others are compared with
  (r) scan_topk_grouped, random labels   about 100 rows per label, uniformly random
  (h) scan_topk_grouped, one hot label   the nearest 1 000 rows of the query carry one label, every other row a random one
  (d) scan_distances + numpy group-by    every distance to the host, then the three-step contract in numpy

  kernels: the corpus' own profiling events (set_profiling / profile_mean_ms: scan kernel and merge kernel, mean per launch);
  wall: perf_counter around the call.  r_over_p / h_over_p: ratios of the kernel medians from this run.

Warm-up, then repeated timed steps; min / median / max are printed.  One JSON document on stdout.

    python tools/grouped_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def group_by(dist, labels, k):
    """the contract in numpy over all distances: what a caller without the grouped scan has to do"""
    pos = np.nonzero(dist < np.inf)[0]
    pos = pos[np.lexsort((pos, dist[pos]))]
    _, first = np.unique(labels[pos], return_index=True)
    return pos[np.sort(first)][:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=3)
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
    c.set_scan_filter(0)                                        # the plain kernel on both sides, not the int8 filter scan
    rng = np.random.default_rng(43)
    q = rng.standard_normal(dim, dtype=np.float32)
    dist = c.scan_distances(metric, q)
    random_labels = rng.integers(0, max(1, N // 100), N).astype(np.uint32)
    hot_labels = random_labels.copy()
    hot_labels[np.argsort(dist, kind="stable")[:1000]] = np.uint32(N)      # a label no random row carries

    def kernel_ms(fn):
        for _ in range(args.warmup):
            fn()
        scan, merge = [], []
        for _ in range(args.steps):
            c.set_profiling(True)
            fn()
            _, s, m = c.profile_mean_ms()
            scan.append(s); merge.append(m)
        c.set_profiling(False)
        tot = np.array(scan) + np.array(merge)
        return {"scan_median_ms": round(float(np.median(scan)), 4), "merge_median_ms": round(float(np.median(merge)), 4),
                "min_ms": round(float(tot.min()), 4), "median_ms": round(float(np.median(tot)), 4), "max_ms": round(float(tot.max()), 4)}

    def wall_ms(fn, steps):
        for _ in range(min(args.warmup, steps)):
            fn()
        per = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            per.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": round(float(np.min(per)), 3), "median_ms": round(float(np.median(per)), 3), "max_ms": round(float(np.max(per)), 3)}

    plain = lambda: c.scan_topk(metric, q, k)
    grouped = lambda: c.scan_topk_grouped(metric, q, k)
    out = {"rows": N, "dim": dim, "k": k, "steps": args.steps, "warmup": args.warmup, "kernel": c.kernel_name(metric)}
    out["p_plain_topk"] = {"kernels": kernel_ms(plain), "wall": wall_ms(plain, args.steps)}
    for name, labels in (("r_grouped_random_labels", random_labels), ("h_grouped_hot_label", hot_labels)):
        c.set_labels(labels)
        ids, d, lab = grouped()
        want = group_by(dist, labels, k)                        # the same rows before anything is timed
        assert (ids - 1).tolist() == want.tolist() and lab.tolist() == labels[want].tolist(), name
        out[name] = {"kernels": kernel_ms(grouped), "wall": wall_ms(grouped, args.steps), "groups": int(len(ids))}
    host = lambda: group_by(c.scan_distances(metric, q), random_labels, k)
    out["d_distances_plus_numpy_group_by"] = {"wall": wall_ms(host, args.host_steps)}
    pk = out["p_plain_topk"]["kernels"]["median_ms"]
    out["r_over_p"] = round(out["r_grouped_random_labels"]["kernels"]["median_ms"] / pk, 4)
    out["h_over_p"] = round(out["h_grouped_hot_label"]["kernels"]["median_ms"] / pk, 4)
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
