#!/usr/bin/env python3
"""Value-range scans against their twins on the same handle, in ONE process (10M x 384 f32, L2, k = 20):

  values       one int64 per row: `sorted` = the scan position (time-ordered inserts: the rows of a window are contiguous and whole
               batches of rows outside it are skipped) and `random` = a permutation of the positions (no batch is skipped)
  selectivity  the window [lo, hi] holds 100 % / 10 % / 1 % of the rows
  per (values, selectivity), same run:
      (v) scan_topk_valued(lo, hi)
      (m) scan_topk_masked with the identical bitmap preset - the twin: the difference is the bitmap kernel
      (p) plain scan_topk
  and at 10 %, every query its own window (shifted through the rows): scan_topk_batch_valued at nq = 4 / 64 / 256 against nq single
  scan_topk_valued calls.
  `kernels`: scan + merge kernels summed over the launches of one call, by the corpus' own profiling events (the bitmap and membership
  kernels are not in the event ring - their cost shows in the wall clock only); `wall`: host wall clock per call.  Both come from the
  same timed steps.  Ratios are ratios of the medians.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout.

    python tools/valued_bench.py [--rows 10000000] [--steps 20] [--warmup 3]
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
    ap.add_argument("--percent", type=float, nargs="*", default=[100.0, 10.0, 1.0])
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
    per_pass, lpr, u = pkg.batch_valued_plan(c, metric)

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
        st = lambda a, nd: {"min_ms": round(float(np.min(a)), nd), "median_ms": round(float(np.median(a)), nd), "max_ms": round(float(np.max(a)), nd)}
        return {"kernels": st(kern, 4), "wall": st(wall, 3)}

    ratio = lambda a, b, what: round(a[what]["median_ms"] / b[what]["median_ms"], 4)
    out = {"rows": N, "dim": dim, "k": k, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u,
           "steps": args.steps, "warmup": args.warmup, "values": {}}
    for order in ("sorted", "random"):
        values = np.arange(N, dtype=np.int64) if order == "sorted" else np.random.default_rng(43).permutation(N).astype(np.int64)
        c.set_values(values)
        r = {}
        for pct in args.percent:
            m = max(1, int(round(N * pct / 100.0)))
            lo = (N - m) // 2
            hi = lo + m - 1
            allow = (values >= lo) & (values <= hi)
            assert int(allow.sum()) == m
            c.set_mask(bits=allow)
            q = qs[0]
            v_ids, _ = c.scan_topk_valued(metric, q, k, lo, hi)
            m_ids, _ = c.scan_topk_masked(metric, q, k)
            assert v_ids.tolist() == m_ids.tolist(), (order, pct)            # the same rows before anything is timed
            e = {"allowed_rows": m,
                 "valued": measure(lambda: c.scan_topk_valued(metric, q, k, lo, hi)),
                 "masked_twin": measure(lambda: c.scan_topk_masked(metric, q, k)),
                 "plain": measure(lambda: c.scan_topk(metric, q, k))}
            for what in ("kernels", "wall"):
                e["valued_over_masked_" + what] = ratio(e["valued"], e["masked_twin"], what)
                e["valued_over_plain_" + what] = ratio(e["valued"], e["plain"], what)
            e["bitmap_kernel_wall_ms"] = round(e["valued"]["wall"]["median_ms"] - e["masked_twin"]["wall"]["median_ms"], 3)
            r["percent_%g" % pct] = e
        # the batch at 10 %: every query its own window
        m = N // 10
        for nq in args.nq:
            qn = np.ascontiguousarray(qs[:nq])
            los = [int((i * (N - m)) // max(nq - 1, 1)) for i in range(nq)]
            his = [x + m - 1 for x in los]
            ids, _, cnt = c.scan_topk_batch_valued(metric, qn, los, his, k)
            for i in (0, nq - 1):
                s_ids, _ = c.scan_topk_valued(metric, qn[i], k, los[i], his[i])
                assert ids[i, :cnt[i]].tolist() == s_ids.tolist(), (order, nq, i)
            e = {"batch": measure(lambda: c.scan_topk_batch_valued(metric, qn, los, his, k)),
                 "singles": measure(lambda: [c.scan_topk_valued(metric, qn[i], k, los[i], his[i]) for i in range(nq)])}
            for what in ("kernels", "wall"):
                e["batch_over_singles_" + what] = ratio(e["batch"], e["singles"], what)
            r["batch_10pct_nq_%d" % nq] = e
        out["values"][order] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
