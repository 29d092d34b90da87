#!/usr/bin/env python3
"""Hamming / Jaccard batches: the integer matrix cores (vg_batch_bits.hip, path 8) against the multi-query scan (path 5) on ONE handle,
in ONE process (10M rows, k = 20; Hamming over random bytes, Jaccard over the mixed-density rows of tools/jaccard_bench.py):

  row lengths  32 bytes (256 bits) and 128 bytes (1024 bits)
  nq           16, 32, 64, 128, 256, 1024
  The two paths ALTERNATE step by step on the same build: VG_BATCH_BITS_MIN_QUERIES=2 takes the matrix cores, =0 switches them off - the
  multi-query scan is then the code every such batch ran before, instruction for instruction.  Before anything is timed both paths'
  ids and distance bits are compared (==).
  `wall`: host wall clock of scan_topk_batch, both paths.  `kernels`: the matrix-core path's launches (pre-pass, stages, merges) by the
  corpus' own profiling events; the multi-query scan records none.  `mfma_peak_frac`: 2 * nq * rows * bits int8 operations over the
  kernel time, against the int8 MFMA ceiling bench.py uses (bench_common.I8_MFMA_PEAK_TOPS).
  `threshold`: the smallest measured nq at which the matrix cores are faster at BOTH row lengths and BOTH metrics by more than the
  multi-query path's own min-to-max spread in this run; never below 10; 0 (switched off) when no nq up to 256 qualifies.

    python tools/bits_batch_bench.py [--rows 10000000] [--steps 20] [--warmup 3] > profiles/bits_batch_bench_10M_u8_k20.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_common import I8_MFMA_PEAK_TOPS          # noqa: E402
from jaccard_bench import mixed_rows                # noqa: E402

SWITCH = "VG_BATCH_BITS_MIN_QUERIES"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, nargs="*", default=[16, 32, 64, 128, 256, 1024])
    ap.add_argument("--row-bytes", type=int, nargs="*", default=[32, 128])
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, k = args.rows, 20
    out = {"rows": N, "k": k, "steps": args.steps, "warmup": args.warmup, "int8_peak_tops": I8_MFMA_PEAK_TOPS, "cases": {}}
    st = lambda a, nd: {"min_ms": round(float(np.min(a)), nd), "median_ms": round(float(np.median(a)), nd),
                        "max_ms": round(float(np.max(a)), nd), "spread_ms": round(float(np.max(a) - np.min(a)), nd)}
    wins = {nq: True for nq in args.nq}
    for name, metric, make in (("hamming", pkg.HAMMING, lambda rng, n, dim: rng.integers(0, 256, (n, dim), dtype=np.uint8)),
                               ("jaccard", pkg.JACCARD, mixed_rows)):
        for dim in args.row_bytes:
            os.environ[SWITCH] = "2"
            c = pkg.Corpus(pkg.U8, dim, capacity=N)
            rng = np.random.default_rng(42 + dim)
            for r0 in range(0, N, 2_000_000):
                c.append(make(rng, min(2_000_000, N - r0), dim))
            qs = make(rng, max(args.nq), dim)
            qs[:, 0] |= 1                                       # (no empty query)
            e = {}
            for nq in args.nq:
                qn = np.ascontiguousarray(qs[:nq])

                def run(switch):
                    os.environ[SWITCH] = switch                 # (the package re-reads the switches at every call)
                    t0 = time.perf_counter()
                    r = c.scan_topk_batch(metric, qn, k)
                    return r, (time.perf_counter() - t0) * 1e3, c.last_batch_path()

                (ni, nd, nc), _, npath = run("2")
                (mi, md, mc), _, mpath = run("0")
                assert (npath, mpath) == (8, 5), (npath, mpath)
                assert np.array_equal(nc, mc) and np.array_equal(ni, mi) and nd.tobytes() == md.tobytes(), (name, dim, nq)
                for _ in range(args.warmup):
                    run("2"); run("0")
                wall_new, wall_multi, kern = [], [], []
                for _ in range(args.steps):
                    c.set_profiling(True)
                    wall_new.append(run("2")[1])
                    n, scan, merge = c.profile_mean_ms()
                    kern.append(n * (scan + merge))
                    c.set_profiling(False)
                    wall_multi.append(run("0")[1])
                b = {"matrix_cores": {"wall": st(wall_new, 3), "kernels": st(kern, 4)}, "multi_query": {"wall": st(wall_multi, 3)}}
                b["multi_over_matrix_wall"] = round(b["multi_query"]["wall"]["median_ms"] / b["matrix_cores"]["wall"]["median_ms"], 3)
                b["matrix_per_query_wall_ms"] = round(b["matrix_cores"]["wall"]["median_ms"] / nq, 5)
                b["multi_per_query_wall_ms"] = round(b["multi_query"]["wall"]["median_ms"] / nq, 5)
                tops = 2.0 * nq * N * 8 * dim / (b["matrix_cores"]["kernels"]["median_ms"] * 1e-3) / 1e12
                b["mfma_tops"] = round(tops, 1)
                b["mfma_peak_frac"] = round(tops / I8_MFMA_PEAK_TOPS, 4)
                b["faster_by_more_than_multi_spread"] = bool(
                    b["multi_query"]["wall"]["median_ms"] - b["matrix_cores"]["wall"]["median_ms"] > b["multi_query"]["wall"]["spread_ms"])
                wins[nq] = wins[nq] and b["faster_by_more_than_multi_spread"]
                e["nq_%d" % nq] = b
            out["cases"]["%s_%d_bytes" % (name, dim)] = e
            c.close()
    upto = [nq for nq in sorted(args.nq) if nq <= 256]
    ok = [nq for i, nq in enumerate(upto) if all(wins[m] for m in upto[i:])]      # (it and every larger measured batch)
    out["threshold"] = max(10, ok[0]) if ok else 0
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
