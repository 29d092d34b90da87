#!/usr/bin/env python3
"""Masked Hamming / Jaccard batches: the gathering matrix-core form (vg_batch_bits.hip / vg_batch_bitsl.hip GATHER, batch_masked_last_path() == 8) against the
masked multi-query scan (path 5) on ONE handle, in ONE process (10M rows, k = 20; Hamming over random bytes, Jaccard over the
mixed-density rows of tools/jaccard_bench.py):

  row lengths  32 bytes (256 bits) and 128 bytes (1024 bits); --row-bytes 256 512 [192 384]: the long-row form's ladder steps
  nq           16, 32, 64, 256, 1024
  masks        100 %, a random 10 %, a random 1 %, and 10 % as one contiguous run of rows
  The two paths ALTERNATE step by step on the same build: VG_BATCH_BITS_MIN_QUERIES=2 takes the matrix cores, =0 switches them off - the
  multi-query scan is then the code every such batch ran before.  Before anything is timed both paths' ids, counts and distance bits
  are compared (==).
  `wall`: host wall clock of scan_topk_batch_masked, both paths, medians with min-to-max spreads.  `kernels`: the matrix-core path's
  launches (pre-pass, stages, merges) by the corpus' own profiling events.
  `position_list_ms`: what the first matrix-core batch behind a set_mask takes longer than the median one (16 queries; the build of
  the position list), median of 5.
  `threshold`: the smallest measured nq from which on (it and every larger one) the matrix cores are faster in EVERY measured cell by
  more than both paths' min-to-max spreads; 0 (switched off) when none qualifies.  `threshold_by_row_bytes`: the same rule over the
  cells of one row length - the long-row form ships a default per ladder step.

    python tools/bits_batch_masked_bench.py [--rows 10000000] [--steps 20] [--warmup 3] > profiles/bits_batch_masked_bench_10M_u8_k20.json
    python tools/bits_batch_masked_bench.py --row-bytes 192 256 384 512 > profiles/bits_batch_masked_long_bench_10M_u8_k20.json
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


def make_mask(kind, n, rng):
    a = np.zeros(n, dtype=bool)
    if kind == "all":
        a[:] = True
    elif kind == "run10":
        a[n // 3:n // 3 + n // 10] = True
    else:
        a[rng.random(n) < {"random10": 0.10, "random1": 0.01}[kind]] = True
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[16, 32, 64, 256, 1024])
    ap.add_argument("--row-bytes", type=int, nargs="*", default=[32, 128])
    ap.add_argument("--metrics", nargs="*", default=["hamming", "jaccard"])
    ap.add_argument("--masks", nargs="*", default=["all", "random10", "random1", "run10"])
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k = args.rows, 20
    out = {"rows": N, "k": k, "steps": args.steps, "warmup": args.warmup, "cases": {}}
    st = lambda a, nd: {"min_ms": round(float(np.min(a)), nd), "median_ms": round(float(np.median(a)), nd),
                        "max_ms": round(float(np.max(a)), nd), "spread_ms": round(float(np.max(a) - np.min(a)), nd)}
    wins = {nq: True for nq in args.nq}
    wins_dim = {dim: {nq: True for nq in args.nq} for dim in args.row_bytes}
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

            def run(qn, switch):
                os.environ[SWITCH] = switch                     # (the package re-reads the switches at every call)
                t0 = time.perf_counter()
                r = c.scan_topk_batch_masked(metric, qn, k)
                return r, (time.perf_counter() - t0) * 1e3, c.batch_masked_last_path()

            for kind in args.masks:
                allowed = make_mask(kind, N, rng)
                e = {"allowed_rows": int(allowed.sum())}
                c.set_mask(bits=allowed)
                for nq in args.nq:
                    qn = np.ascontiguousarray(qs[:nq])
                    (ni, nd, nc), _, npath = run(qn, "2")
                    (mi, md, mc), _, mpath = run(qn, "0")
                    assert (npath, mpath) == (8, 5), (npath, mpath)
                    assert np.array_equal(nc, mc) and np.array_equal(ni, mi) and nd.tobytes() == md.tobytes(), (name, dim, kind, nq)
                    for _ in range(args.warmup):
                        run(qn, "2"); run(qn, "0")
                    wall_new, wall_multi, kern = [], [], []
                    for _ in range(args.steps):
                        c.set_profiling(True)
                        wall_new.append(run(qn, "2")[1])
                        n, scan, merge = c.profile_mean_ms()
                        kern.append(n * (scan + merge))
                        c.set_profiling(False)
                        wall_multi.append(run(qn, "0")[1])
                    b = {"matrix_cores": {"wall": st(wall_new, 3), "kernels": st(kern, 4)}, "multi_query": {"wall": st(wall_multi, 3)}}
                    gain = b["multi_query"]["wall"]["median_ms"] - b["matrix_cores"]["wall"]["median_ms"]
                    b["multi_over_matrix_wall"] = round(b["multi_query"]["wall"]["median_ms"] / b["matrix_cores"]["wall"]["median_ms"], 3)
                    b["faster_by_more_than_both_spreads"] = bool(gain > max(b["multi_query"]["wall"]["spread_ms"], b["matrix_cores"]["wall"]["spread_ms"]))
                    wins[nq] = wins[nq] and b["faster_by_more_than_both_spreads"]
                    wins_dim[dim][nq] = wins_dim[dim][nq] and b["faster_by_more_than_both_spreads"]
                    e["nq_%d" % nq] = b
                # the one-off cost of the position list: the first matrix-core batch behind set_mask against the median one
                q16 = np.ascontiguousarray(qs[:16])
                steady = float(np.median([run(q16, "2")[1] for _ in range(5)]))
                first = []
                for _ in range(5):
                    c.set_mask(bits=allowed)
                    first.append(run(q16, "2")[1] - steady)
                e["position_list_ms"] = st(first, 3)
                out["cases"]["%s_%d_bytes_%s" % (name, dim, kind)] = e
                print("%s %d bytes, mask %s: done" % (name, dim, kind), file=sys.stderr, flush=True)
            c.close()
    first_ok = lambda w: next((nq for i, nq in enumerate(sorted(args.nq)) if all(w[m] for m in sorted(args.nq)[i:])), 0)      # (it and every larger measured batch)
    out["threshold"] = first_ok(wins)
    out["threshold_by_row_bytes"] = {str(dim): first_ok(wins_dim[dim]) for dim in args.row_bytes}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
