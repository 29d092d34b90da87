#!/usr/bin/env python3
"""Labeled Hamming / Jaccard batches: the labeled matrix-core form (vg_batch_bits.hip LABELED, batch_labeled_last_path() == 8) against the
labeled multi-query scan (path 5) on ONE handle, in ONE process (10M rows, k = 20; Hamming over random bytes, Jaccard over the
mixed-density rows of tools/jaccard_bench.py):

  row lengths  32 bytes (256 bits) and 128 bytes (1024 bits)
  nq           16, 32, 64, 256, 1024
  row labels   16 / 256 / 4096 equal tenants, spread randomly (`random`) or in contiguous runs of rows (`runs`)
  query labels every query its own - cycling through the tenants - (`own`), or all queries one tenant (`one`)
  The two paths ALTERNATE step by step on the same build: VG_BATCH_BITS_MIN_QUERIES=2 takes the matrix cores, =0 switches them off - the
  multi-query scan is then the code every such batch ran before.  Before anything is timed both paths' ids, counts and distance bits
  are compared (==).
  `wall`: host wall clock of scan_topk_batch_labeled with the results fetched, both paths, medians with min-to-max spreads.
  `threshold`: the smallest measured nq from which on (it and every larger one) the matrix cores are faster in EVERY measured cell by
  more than both paths' min-to-max spreads; 0 (switched off) when none qualifies.  `losing_cells`: per nq, the cells that do not.

    python tools/bits_batch_labeled_bench.py [--rows 10000000] [--steps 10] [--warmup 2] > profiles/bits_batch_labeled_bench_10M_u8_k20.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from jaccard_bench import mixed_rows                # noqa: E402

SWITCH = "VG_BATCH_BITS_MIN_QUERIES"


def make_labels(tenants, spread, n, rng):
    if spread == "runs":
        return (np.arange(n, dtype=np.int64) * tenants // n).astype(np.uint32)
    return rng.permutation(np.arange(n, dtype=np.int64) % tenants).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nq", type=int, nargs="*", default=[16, 32, 64, 256, 1024])
    ap.add_argument("--row-bytes", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--metrics", nargs="*", default=["hamming", "jaccard"])
    ap.add_argument("--tenants", type=int, nargs="*", default=[16, 256, 4096])
    ap.add_argument("--spreads", nargs="*", default=["random", "runs"])
    ap.add_argument("--query-labels", nargs="*", default=["own", "one"])
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k = args.rows, 20
    out = {"rows": N, "k": k, "steps": args.steps, "warmup": args.warmup, "cases": {}}
    st = lambda a, nd: {"min_ms": round(float(np.min(a)), nd), "median_ms": round(float(np.median(a)), nd),
                        "max_ms": round(float(np.max(a)), nd), "spread_ms": round(float(np.max(a) - np.min(a)), nd)}
    losing = {nq: [] for nq in args.nq}
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

            def run(qn, ql, switch):
                os.environ[SWITCH] = switch                     # (the package re-reads the switches at every call)
                t0 = time.perf_counter()
                r = c.scan_topk_batch_labeled(metric, qn, ql, k)
                return r, (time.perf_counter() - t0) * 1e3, c.batch_labeled_last_path()

            for tenants in args.tenants:
                for spread in args.spreads:
                    c.set_labels(make_labels(tenants, spread, N, rng))
                    for qmode in args.query_labels:
                        cell = "%s_%d_bytes_%d_%s_%s" % (name, dim, tenants, spread, qmode)
                        e = {}
                        for nq in args.nq:
                            qn = np.ascontiguousarray(qs[:nq])
                            ql = (np.arange(nq) % tenants if qmode == "own" else np.full(nq, tenants // 2)).astype(np.uint32)
                            (ni, nd, nc), _, npath = run(qn, ql, "2")
                            (mi, md, mc), _, mpath = run(qn, ql, "0")
                            assert (npath, mpath) == (8, 5), (npath, mpath)
                            assert np.array_equal(nc, mc) and np.array_equal(ni, mi) and nd.tobytes() == md.tobytes(), (cell, nq)
                            for _ in range(args.warmup):
                                run(qn, ql, "2"); run(qn, ql, "0")
                            wall_new, wall_multi = [], []
                            for _ in range(args.steps):
                                wall_new.append(run(qn, ql, "2")[1])
                                wall_multi.append(run(qn, ql, "0")[1])
                            b = {"matrix_cores": {"wall": st(wall_new, 3)}, "multi_query": {"wall": st(wall_multi, 3)}}
                            gain = b["multi_query"]["wall"]["median_ms"] - b["matrix_cores"]["wall"]["median_ms"]
                            b["multi_over_matrix_wall"] = round(b["multi_query"]["wall"]["median_ms"] / b["matrix_cores"]["wall"]["median_ms"], 3)
                            b["faster_by_more_than_both_spreads"] = bool(gain > max(b["multi_query"]["wall"]["spread_ms"], b["matrix_cores"]["wall"]["spread_ms"]))
                            if not b["faster_by_more_than_both_spreads"]:
                                losing[nq].append(cell)
                            e["nq_%d" % nq] = b
                        out["cases"][cell] = e
                        print("%s: done" % cell, file=sys.stderr, flush=True)
            c.close()
    out["losing_cells"] = {str(nq): losing[nq] for nq in args.nq}
    out["threshold"] = next((nq for i, nq in enumerate(sorted(args.nq)) if not any(losing[m] for m in sorted(args.nq)[i:])), 0)   # (it and every larger measured batch)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
