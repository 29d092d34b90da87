#!/usr/bin/env python3
"""Capped scans against the plain top-k scan, the grouped scan and the only exact answer the code before them has, in ONE process over
ONE corpus (k = 20):

  corpus   10M x 384 f32, L2 (--rows / --dim to change it); labels: random (about 100 rows per label) and hot (the nearest 1 000 rows
           of the query carry one label, every other row a random one)
  (a) scan_topk                          the plain fused top-k
  (b) scan_topk_grouped                  the yardstick: the same kernels with a list of one row per label
  (c) scan_topk_capped, per_label = 1    the same work as (b), through the capped routine
  (d) scan_topk_capped, per_label = 3    up to two more in-label replacements per accept
  (e) scan_topk_after paging + host cap  hot labels only: pages of 64 rows, capped on the host until k rows are kept (wall time and
                                         the number of passes over the corpus)

  kernels: the corpus' own profiling events (set_profiling / profile_mean_ms: scan kernel and merge kernel, mean per launch);
  wall: perf_counter around the call.  c_over_b / d_over_b: ratios of the kernel medians from this run; b_spread = (b)'s max - min.

Warm-up, then repeated timed steps; min / median / max are printed.  One JSON document on stdout.

    python tools/capped_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def capped(dist, labels, k, m):
    """the contract in numpy over all distances (every row labeled): the rows a capped scan must return"""
    pos = np.nonzero(dist < np.inf)[0]
    pos = pos[np.lexsort((pos, dist[pos]))][:4096]              # (k rows are kept long before 4 096 rows are walked here)
    kept, out = {}, []
    for p in pos.tolist():
        lab = int(labels[p])
        if kept.get(lab, 0) < m:
            kept[lab] = kept.get(lab, 0) + 1
            out.append(p)
            if len(out) == k:
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
    c.set_scan_filter(0)                                        # the plain kernel on every side, not the int8 filter scan
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

    def paged(labels, m):
        """pages of 64 rows behind a (distance, rowid) cursor, capped on the host: (positions kept, passes over the corpus)"""
        kept, out, after, passes = {}, [], None, 0
        while len(out) < k:
            ids, d = c.scan_topk_after(metric, q, 64, after)
            passes += 1
            if len(ids) == 0:
                break
            for i in ids.tolist():
                lab = int(labels[i - 1])
                if kept.get(lab, 0) < m:
                    kept[lab] = kept.get(lab, 0) + 1
                    out.append(i - 1)
                    if len(out) == k:
                        break
            after = (float(d[-1]), int(ids[-1]))
        return out, passes

    measure = lambda fn: {"kernels": kernel_ms(fn), "wall": wall_ms(fn, args.steps)}
    out = {"rows": N, "dim": dim, "k": k, "steps": args.steps, "warmup": args.warmup, "kernel": c.kernel_name(metric)}
    out["a_plain_topk"] = measure(lambda: c.scan_topk(metric, q, k))
    for name, labels in (("random_labels", random_labels), ("hot_label", hot_labels)):
        c.set_labels(labels)
        for m in (1, 3):                                        # the same rows before anything is timed
            ids, d, lab = c.scan_topk_capped(metric, q, k, m)
            want = capped(dist, labels, k, m)
            assert (ids - 1).tolist() == want and lab.tolist() == labels[want].tolist(), (name, m)
        ids, d, lab = c.scan_topk_grouped(metric, q, k)
        assert (ids - 1).tolist() == capped(dist, labels, k, 1), name
        r = {"b_grouped": measure(lambda: c.scan_topk_grouped(metric, q, k)),
             "c_capped_m1": measure(lambda: c.scan_topk_capped(metric, q, k, 1)),
             "d_capped_m3": measure(lambda: c.scan_topk_capped(metric, q, k, 3))}
        b = r["b_grouped"]["kernels"]
        r["b_spread_ms"] = round(b["max_ms"] - b["min_ms"], 4)
        r["c_over_b"] = round(r["c_capped_m1"]["kernels"]["median_ms"] / b["median_ms"], 4)
        r["d_over_b"] = round(r["d_capped_m3"]["kernels"]["median_ms"] / b["median_ms"], 4)
        out[name] = r
    got, passes = paged(hot_labels, 3)                          # (e): the hot labels are still set
    assert got == capped(dist, hot_labels, k, 3)
    out["hot_label"]["e_paging_loop_host_cap_m3"] = {"wall": wall_ms(lambda: paged(hot_labels, 3), args.steps), "passes": passes}
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
