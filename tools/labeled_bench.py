#!/usr/bin/env python3
"""Labeled batch scans against the only way the code before them answers the same question, in ONE process per corpus (k = 20):

  corpus   --corpus f32: 10M x 384 f32 (L2), --corpus u8: 10M x 768 uint8 (L2); one corpus per run (run the tool twice)
  labels   16 / 256 / 4096 tenants of equal size, uniformly random rows and run-clustered (every tenant one contiguous run)
  batches  nq = 4, 16, 64, two query mixes: "own" - every query its own label (tenant i % tenants) - and "one" - all queries tenant 0
  per (labels, mix, nq):
    kernels, summed over the launches of one batch (the corpus' own profiling events: set_profiling / profile_mean_ms; the bitmap
    kernel of the single labeled scan is not in the event ring - its cost shows in the wall clock only):
      (l) scan_topk_batch_labeled           (a) per query set_mask(tenant) + scan_topk_masked
    end to end, wall clock per batch:
      (L) scan_topk_batch_labeled           (F) nq calls of scan_topk_labeled - the fallback of the batch form
      (A) per query set_mask(bits = labels == tenant, built on the host as a caller has to) + scan_topk_masked
  l_over_a / L_over_A / L_over_F are the ratios of the medians, from the same run.  L_over_F > 1 marks a shape the batch form should
  hand to its fallback.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout.

    python tools/labeled_bench.py --corpus f32 [--rows 10000000] [--steps 10] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_labels(n, tenants, clustered, rng):
    """equal-sized tenants: a random permutation of (row % tenants), or one contiguous run per tenant"""
    if clustered:
        return (np.arange(n, dtype=np.int64) * tenants // n).astype(np.uint32)
    lab = (np.arange(n, dtype=np.int64) % tenants).astype(np.uint32)
    rng.shuffle(lab)
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=("f32", "u8"), default="f32")
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
    per_pass, lpr, u = pkg.batch_labeled_plan(c, metric)

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

    out = {"corpus": args.corpus, "rows": N, "dim": dim, "k": k, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u,
           "steps": args.steps, "warmup": args.warmup, "labels": {}}
    lrng = np.random.default_rng(44)
    for tenants in args.tenants:
        for clustered in (False, True):
            name = "%s_%d" % ("clustered" if clustered else "random", tenants)
            labels = make_labels(N, tenants, clustered, lrng)
            c.set_labels(labels)
            r = {"rows_per_tenant": N // tenants}
            for mix in ("own", "one"):
                for nq in args.nq:
                    q = np.ascontiguousarray(qs[:nq])
                    ql = np.array([(i % tenants) if mix == "own" else 0 for i in range(nq)], dtype=np.uint32)

                    def masked_way():
                        res = []
                        for i in range(nq):
                            c.set_mask(bits=labels == ql[i])
                            res.append(c.scan_topk_masked(metric, q[i], k))
                        return res

                    batch = lambda: c.scan_topk_batch_labeled(metric, q, ql, k)
                    singles = lambda: [c.scan_topk_labeled(metric, q[i], k, int(ql[i])) for i in range(nq)]
                    ids, dist, cnt = batch()
                    for i, (si, sd) in enumerate(masked_way()):         # the same rows before anything is timed
                        assert ids[i, :cnt[i]].tolist() == si.tolist(), (name, mix, nq, i)
                    e = {"l_batch_labeled_kernels": kernel_ms(batch), "a_set_mask_plus_masked_kernels": kernel_ms(masked_way),
                         "L_batch_labeled": wall_ms(batch), "F_single_labeled": wall_ms(singles), "A_set_mask_plus_masked": wall_ms(masked_way)}
                    e["l_over_a"] = round(e["l_batch_labeled_kernels"]["median_ms"] / e["a_set_mask_plus_masked_kernels"]["median_ms"], 4)
                    e["L_over_A"] = round(e["L_batch_labeled"]["median_ms"] / e["A_set_mask_plus_masked"]["median_ms"], 4)
                    e["L_over_F"] = round(e["L_batch_labeled"]["median_ms"] / e["F_single_labeled"]["median_ms"], 4)
                    r["%s_nq_%d" % (mix, nq)] = e
            out["labels"][name] = r
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
