#!/usr/bin/env python3
"""Masked range scans against the only way to ask the same question without them, in ONE process (10M x 384 f32, L2):

  masks    100 %, 10 % scattered (uniformly random rows), 10 % clustered and 1 % clustered (runs of 4096 consecutive rows)
  radii    per query and mask: the midpoint behind its 20th and behind its 10 000th smallest ALLOWED distance
  forms    the single form (one query) and nq = 16
  per (mask, radius, form):
    kernels, summed over the launches of one call (the corpus' own profiling events: set_profiling / profile_mean_ms):
      (m) scan_within_masked / scan_within_batch_masked      (u) scan_within / scan_within_batch with the same radii
    end to end, wall clock per call:
      (M) the masked form                                    (U) the unmasked form + the foreign rows thrown away on the host
  m_over_u / M_over_U are the ratios of the medians, from the same run.  Nothing is asserted about a timing.

Warm-up, then repeated timed steps; min / median are printed.  One JSON document on stdout: run it on an MI355X, keep the output under
profiles/ and put the figures into DESIGN.md 3.12.

    python tools/within_masked_bench.py [--rows 10000000] [--steps 10] [--warmup 2] [--nq 16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RUN = 4096                                                     # rows per run of a clustered mask


def masks(n, rng):
    out = {"all": np.ones(n, dtype=bool), "scattered_10pct": rng.random(n) < 0.10}
    for name, p in (("clustered_10pct", 0.10), ("clustered_1pct", 0.01)):
        runs = (n + RUN - 1) // RUN
        on = np.zeros(runs, dtype=bool)
        on[rng.choice(runs, size=max(1, int(round(p * runs))), replace=False)] = True
        out[name] = np.repeat(on, RUN)[:n]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, default=16)
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
    qs = rng.standard_normal((args.nq, dim), dtype=np.float32)
    own = [c.scan_distances(metric, qs[i]) for i in range(args.nq)]      # radii from the engine's own distances
    per_pass, lpr, u = pkg.within_batch_masked_plan(c, metric)

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

    out = {"rows": N, "dim": dim, "queries_per_pass": per_pass, "lanes_per_row": lpr, "chunks_per_lane": u, "nq": args.nq,
           "single_kernel": c.kernel_name(metric), "steps": args.steps, "warmup": args.warmup, "masks": {}}
    for name, allowed in masks(N, rng).items():
        t0 = time.perf_counter()
        n_allowed = c.set_mask(bits=allowed)
        entry = {"allowed_rows": int(n_allowed), "set_mask_ms": round((time.perf_counter() - t0) * 1e3, 3), "radii": {}}
        for rank in (20, 10_000):
            if rank >= n_allowed:
                continue
            radii = []
            for i in range(args.nq):
                part = np.partition(own[i][allowed], [rank - 1, rank])
                radii.append(0.5 * (float(part[rank - 1]) + float(part[rank])))
            single_m = lambda: c.scan_within_masked(metric, qs[0], radii[0])
            single_u = lambda: c.scan_within(metric, qs[0], radii[0])
            batch_m = lambda: c.scan_within_batch_masked(metric, qs, radii)
            batch_u = lambda: c.scan_within_batch(metric, qs, radii)

            def host_filtered(res):
                return [(ids[allowed[ids - 1]], dist[allowed[ids - 1]]) for ids, dist, _ in res]

            # the same rows before anything is timed
            gi, gd, gm = single_m()
            (ui, ud), = host_filtered([single_u()])
            assert gi.tolist() == ui.tolist() and gm == len(ui), (name, rank)
            got = batch_m()
            for i, (ui, ud) in enumerate(host_filtered(batch_u())):
                assert got[i][0].tolist() == ui.tolist(), (name, rank, i)
            e = {"allowed_matches_single": int(gm), "matches_overall_single": int(single_u()[2]),
                 "allowed_matches_per_query": float(np.mean([x[2] for x in got])), "launches_batch": c.within_batch_last_launches(),
                 "m_single_masked_kernels": kernel_ms(single_m), "u_single_unmasked_kernels": kernel_ms(single_u),
                 "M_single_masked": wall_ms(single_m), "U_single_unmasked_host_filter": wall_ms(lambda: host_filtered([single_u()])),
                 "m_batch_masked_kernels": kernel_ms(batch_m), "u_batch_unmasked_kernels": kernel_ms(batch_u),
                 "M_batch_masked": wall_ms(batch_m), "U_batch_unmasked_host_filter": wall_ms(lambda: host_filtered(batch_u()))}
            for form in ("single", "batch"):
                e["m_over_u_" + form] = round(e["m_%s_masked_kernels" % form]["median_ms"] / e["u_%s_unmasked_kernels" % form]["median_ms"], 4)
                e["M_over_U_" + form] = round(e["M_%s_masked" % form]["median_ms"] / e["U_%s_unmasked_host_filter" % form]["median_ms"], 4)
            entry["radii"]["about_%d_allowed_rows" % rank] = e
        out["masks"][name] = entry
    c.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
