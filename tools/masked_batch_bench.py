#!/usr/bin/env python3
"""Masked batch scans against the ways to ask the same question without them, in ONE process per corpus (k = 20):

  corpus   --corpus f32: 10M x 384 f32 (L2), --corpus u8: 10M x 768 uint8 (L2); one corpus per run (run the tool twice)
  masks    densities 1, 1/10, 1/100, 1/1000 of uniformly random rows, and the same counts as tenant-clustered runs of 4096 rows
  batches  nq = 4, 16, 64
  per (mask, nq):
    kernels, summed over the launches of one batch (the corpus' own profiling events: set_profiling / profile_mean_ms):
      (m) scan_topk_batch_masked            (a) nq calls of scan_topk_masked - the only way to answer the question without (m)
    end to end, wall clock per batch:
      (M) scan_topk_batch_masked            (A) nq calls of scan_topk_masked       (B) the UNMASKED scan_topk_batch, for orientation only
  m_over_a / M_over_A are the ratios of the medians, from the same run.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout.

    python tools/masked_batch_bench.py --corpus f32 [--rows 10000000] [--steps 10] [--warmup 2]
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
    ap.add_argument("--corpus", choices=("f32", "u8"), default="f32")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, nargs="*", default=[4, 16, 64])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k = args.rows, 20
    f32 = args.corpus == "f32"
    vt, dim, metric = (pkg.F32, 384, pkg.L2) if f32 else (pkg.U8, 768, pkg.L2)
    c = pkg.Corpus(vt, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        nb = min(1_000_000, N - r0)
        if f32:
            t = torch.randn((nb, dim), generator=gen, device="cuda", dtype=torch.float32)
        else:
            t = torch.randint(0, 256, (nb, dim), generator=gen, device="cuda", dtype=torch.uint8)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), nb, dim * (4 if f32 else 1))
        del t
    c.set_tie_order(pkg.TIE_POSITION)
    rng = np.random.default_rng(43)
    nq_max = max(args.nq)
    qs = rng.standard_normal((nq_max, dim), dtype=np.float32) if f32 else rng.integers(0, 256, (nq_max, dim)).astype(np.uint8)
    per_pass, lpr, u = pkg.batch_masked_plan(c, metric)

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

    mrng = np.random.default_rng(44)
    masks = [("density_1", np.ones(N, dtype=bool))]
    for den in (10, 100, 1000):
        allowed = mrng.random(N) < 1.0 / den
        masks.append(("random_1_%d" % den, allowed))
        runs = np.zeros(N, dtype=bool)
        starts = mrng.choice(max(1, N // 4096), size=max(1, int(allowed.sum()) // 4096), replace=False) * 4096
        for s in starts:
            runs[s:s + 4096] = True
        masks.append(("clustered_1_%d" % den, runs))

    out = {"corpus": args.corpus, "rows": N, "dim": dim, "k": k, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u,
           "single_kernel": c.kernel_name(metric), "steps": args.steps, "warmup": args.warmup, "masks": {}}
    for name, allowed in masks:
        c.set_mask(bits=allowed)
        r = {"allowed_rows": int(allowed.sum())}
        for nq in args.nq:
            q = np.ascontiguousarray(qs[:nq])
            singles = lambda: [c.scan_topk_masked(metric, q[i], k) for i in range(nq)]
            batch = lambda: c.scan_topk_batch_masked(metric, q, k)
            ids, dist, cnt = batch()
            for i, (si, sd) in enumerate(singles()):            # the same rows before anything is timed
                assert ids[i, :cnt[i]].tolist() == si.tolist(), (name, nq, i)
            e = {"m_batch_masked_kernels": kernel_ms(batch), "a_single_masked_kernels": kernel_ms(singles),
                 "M_batch_masked": wall_ms(batch), "A_single_masked": wall_ms(singles),
                 "B_unmasked_batch": wall_ms(lambda: c.scan_topk_batch(metric, q, k))}
            e["m_over_a"] = round(e["m_batch_masked_kernels"]["median_ms"] / e["a_single_masked_kernels"]["median_ms"], 4)
            e["M_over_A"] = round(e["M_batch_masked"]["median_ms"] / e["A_single_masked"]["median_ms"], 4)
            r["nq_%d" % nq] = e
        out["masks"][name] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
