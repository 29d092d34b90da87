#!/usr/bin/env python3
"""Masked Hamming / Jaccard batch RANGE scans: the gathering matrix-core form (vg_batch_bits_within.hip GATHER, within_batch_last_path()
== 8) against the masked multi-query range scan (path 5) on ONE handle, in ONE process (10M rows; Hamming over random bytes, Jaccard
over the mixed-density rows of tools/jaccard_bench.py):

  row lengths  32 bytes (256 bits) and 128 bytes (1024 bits) - rows beyond 128 bytes keep path 5 under a mask
  nq           128, 256, 1024 (below 128 queries the form is not taken whatever the switch says)
  masks        100 %, a random 10 %, a random 1 %, and 10 % as one contiguous run of rows (tools/bits_batch_masked_bench.py's)
  radii        each query's own 20th smallest distance among the ALLOWED rows (scan_topk_batch_masked): a query matches about 20 rows;
               what the queries of a cell really matched is in the output (`matches_per_query`)
  The two paths ALTERNATE step by step on the same build: VG_BATCH_BITS_MIN_QUERIES=2 takes the matrix cores, =0 switches them off - the
  masked multi-query range scan is then the code every such batch ran before.  Before anything is timed both paths' ids, distance bits
  and `matches` are compared (==).  `wall`: host wall clock of scan_within_batch_masked, results fetched, both paths; medians, and
  min-to-max spreads.
  `threshold`: the smallest measured nq from which on (it and every larger one) the matrix cores are faster in EVERY cell by more than
  both paths' spreads; 0 (switched off) when none qualifies.

    python tools/bits_within_masked_bench.py [--rows 10000000] [--steps 10] [--warmup 2] > profiles/bits_within_masked_bench_10M_u8.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bits_batch_masked_bench import make_mask        # noqa: E402
from jaccard_bench import mixed_rows                # noqa: E402

SWITCH = "VG_BATCH_BITS_MIN_QUERIES"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, nargs="*", default=[128, 256, 1024])
    ap.add_argument("--row-bytes", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--metrics", nargs="*", default=["hamming", "jaccard"])
    ap.add_argument("--masks", nargs="*", default=["all", "random10", "random1", "run10"])
    ap.add_argument("--target", type=int, default=20)
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N = args.rows
    out = {"rows": N, "steps": args.steps, "warmup": args.warmup, "target_matches": args.target, "cases": {}}
    st = lambda a: {"min_ms": round(float(np.min(a)), 3), "median_ms": round(float(np.median(a)), 3),
                    "max_ms": round(float(np.max(a)), 3), "spread_ms": round(float(np.max(a) - np.min(a)), 3)}
    wins = {nq: True for nq in args.nq}
    makers = {"hamming": (pkg.HAMMING, lambda rng, n, dim: rng.integers(0, 256, (n, dim), dtype=np.uint8)), "jaccard": (pkg.JACCARD, mixed_rows)}
    for name in args.metrics:
        metric, make = makers[name]
        for dim in args.row_bytes:
            os.environ[SWITCH] = "2"
            c = pkg.Corpus(pkg.U8, dim, capacity=N)
            rng = np.random.default_rng(42 + dim)
            for r0 in range(0, N, 2_000_000):
                c.append(make(rng, min(2_000_000, N - r0), dim))
            qs = make(rng, max(args.nq), dim)
            qs[:, 0] |= 1                                       # (no empty query)
            for kind in args.masks:
                allowed = make_mask(kind, N, rng)
                e = {"allowed_rows": int(allowed.sum())}
                c.set_mask(bits=allowed)
                os.environ[SWITCH] = "2"
                radius = c.scan_topk_batch_masked(metric, qs, args.target)[1][:, args.target - 1].copy()
                for nq in args.nq:
                    qn, rn = np.ascontiguousarray(qs[:nq]), radius[:nq]

                    def run(switch):
                        os.environ[SWITCH] = switch             # (the package re-reads the switches at every call)
                        t0 = time.perf_counter()
                        r = c.scan_within_batch_masked(metric, qn, rn)
                        return r, (time.perf_counter() - t0) * 1e3, c.within_batch_last_path(), c.within_batch_last_launches()

                    new, _, npath, nlaunch = run("2")
                    old, _, mpath, mlaunch = run("0")
                    assert (npath, mpath) == (8, 5), (npath, mpath)
                    for a, b in zip(new, old):
                        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (name, dim, kind, nq)
                    for _ in range(args.warmup):
                        run("2"); run("0")
                    wall_new, wall_multi = [], []
                    for _ in range(args.steps):
                        wall_new.append(run("2")[1])
                        wall_multi.append(run("0")[1])
                    b = {"matches_per_query": round(float(np.mean([x[2] for x in new])), 1),
                         "matrix_cores": {"wall": st(wall_new), "launches": nlaunch}, "multi_query": {"wall": st(wall_multi), "launches": mlaunch}}
                    gain = b["multi_query"]["wall"]["median_ms"] - b["matrix_cores"]["wall"]["median_ms"]
                    b["multi_over_matrix_wall"] = round(b["multi_query"]["wall"]["median_ms"] / b["matrix_cores"]["wall"]["median_ms"], 3)
                    b["faster_by_more_than_both_spreads"] = bool(gain > max(b["multi_query"]["wall"]["spread_ms"], b["matrix_cores"]["wall"]["spread_ms"]))
                    wins[nq] = wins[nq] and b["faster_by_more_than_both_spreads"]
                    e["nq_%d" % nq] = b
                    print(name, dim, kind, nq, b["matrix_cores"]["wall"]["median_ms"], b["multi_query"]["wall"]["median_ms"], file=sys.stderr, flush=True)
                out["cases"]["%s_%d_bytes_%s" % (name, dim, kind)] = e
            c.close()
    order = sorted(wins)
    ok = [nq for i, nq in enumerate(order) if all(wins[m] for m in order[i:])]      # (it and every larger measured batch)
    out["threshold"] = ok[0] if ok else 0
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
