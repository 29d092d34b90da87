#!/usr/bin/env python3
"""Masked scans against the scans they sit next to, in ONE process on ONE 10M x 384 f32 corpus (L2, k = 20):

  per mask - densities 1, 1/10, 1/100, 1/1000 of uniformly random rows, and the count of 1/100 as contiguous runs of 4096 rows:
    kernels, timed with the corpus' own profiling events (set_profiling / profile_mean_ms):
      (a) the plain top-20 kernel, in the same run          (b) the masked kernel
    end to end, wall clock:
      (c) scan_topk_masked (the mask already set)           (d) scan_distances + numpy mask + argpartition: the way without masked scans
    setting the mask, wall clock:
      (e) set_mask(rowids=...)                              (f) set_mask(bits=...)
  through SQL (--sql-rows, default 200 000 rows, a file-less database): vector_full_scan_filtered with a TEXT filter, the filter
  statement alone, and the stream statement it replaces.

(a) is the yardstick for (b) - from the same run.  Warm-up, then repeated timed steps; min / median are printed.

    python tools/masked_bench.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--sql-rows 200000]
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
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sql-rows", type=int, default=200_000)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import __graft_entry__ as g
    pkg = g.load_package()
    N, dim, k = args.rows, args.dim, 20
    c = pkg.Corpus(pkg.F32, dim, capacity=N)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(42)
    for r0 in range(0, N, 1_000_000):
        nb = min(1_000_000, N - r0)
        t = torch.randn((nb, dim), generator=gen, device="cuda", dtype=torch.float32)
        torch.cuda.synchronize()
        c.append_device(t.data_ptr(), nb, dim * 4)
        del t
    c.set_scan_filter(0)                      # (a) is the PLAIN top-k kernel, the one the masked kernel is an instantiation of
    c.set_tie_order(pkg.TIE_POSITION)
    q = np.random.default_rng(43).standard_normal(dim, dtype=np.float32)

    def kernel_ms(fn):
        for _ in range(args.warmup):
            fn()
        per = []
        for _ in range(args.steps):
            c.set_profiling(True)
            fn()
            n, scan, merge = c.profile_mean_ms()
            per.append(scan)
        c.set_profiling(False)
        return {"min_ms": round(float(np.min(per)), 4), "median_ms": round(float(np.median(per)), 4), "max_ms": round(float(np.max(per)), 4)}

    def wall_ms(fn, steps=None):
        for _ in range(args.warmup if steps is None else 1):
            fn()
        per = []
        for _ in range(steps or args.steps):
            t0 = time.perf_counter()
            fn()
            per.append((time.perf_counter() - t0) * 1e3)
        return {"min_ms": round(float(np.min(per)), 3), "median_ms": round(float(np.median(per)), 3)}

    def host_way(allowed):
        d = c.scan_distances(pkg.L2, q)
        pos = np.nonzero(allowed & (d < np.inf))[0]
        dd = d[pos]
        if len(pos) > k:
            kth = np.partition(dd, k - 1)[k - 1]
            keep = dd <= kth
            pos, dd = pos[keep], dd[keep]
        order = np.lexsort((pos, dd))[:k]
        return pos[order] + 1, dd[order]

    rng = np.random.default_rng(44)
    masks = [("density_1", np.ones(N, dtype=bool))]
    for den in (10, 100, 1000):
        masks.append(("density_1_%d" % den, rng.random(N) < 1.0 / den))
    runs = np.zeros(N, dtype=bool)
    want = int(masks[2][1].sum())
    starts = rng.choice(max(1, N // 4096), size=max(1, want // 4096), replace=False) * 4096
    for s in starts:
        runs[s:s + 4096] = True
    masks.append(("clustered_runs_of_4096", runs))

    out = {"rows": N, "dim": dim, "k": k, "kernel": c.kernel_name(pkg.L2), "steps": args.steps, "warmup": args.warmup, "masks": {}}
    for name, allowed in masks:
        r = {"allowed_rows": int(allowed.sum())}
        ids = np.nonzero(allowed)[0].astype(np.int64) + 1
        r["e_set_mask_rowids"] = wall_ms(lambda: c.set_mask(rowids=ids), steps=3)
        r["f_set_mask_bits"] = wall_ms(lambda: c.set_mask(bits=allowed), steps=3)
        gi, gd = c.scan_topk_masked(pkg.L2, q, k)
        hi, hd = host_way(allowed)
        assert gi.tolist() == hi.tolist() and np.array_equal(gd, hd.astype(np.float64)), name
        r["a_plain_topk_kernel"] = kernel_ms(lambda: c.scan_topk(pkg.L2, q, k))
        r["b_masked_kernel"] = kernel_ms(lambda: c.scan_topk_masked(pkg.L2, q, k))
        r["b_over_a_median"] = round(r["b_masked_kernel"]["median_ms"] / r["a_plain_topk_kernel"]["median_ms"], 4)
        r["c_scan_topk_masked"] = wall_ms(lambda: c.scan_topk_masked(pkg.L2, q, k))
        r["d_scan_distances_numpy"] = wall_ms(lambda: host_way(allowed), steps=max(3, args.steps // 5))
        r["d_over_c"] = round(r["d_scan_distances_numpy"]["median_ms"] / r["c_scan_topk_masked"]["median_ms"], 2)
        out["masks"][name] = r
    c.close()

    # ---- through SQL: the filter statement's own cost is SQLite's and is reported apart
    import sqlite3
    b = g._load_build()
    ext = b.build_extension()[:-3]
    n = args.sql_rows
    rows = np.random.default_rng(45).standard_normal((n, dim), dtype=np.float32)
    db = sqlite3.connect(":memory:", isolation_level=None)
    db.enable_load_extension(True)
    db.load_extension(ext)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", ((i + 1, (i * 7919) % 100, rows[i].tobytes()) for i in range(n)))
    db.execute("COMMIT")
    db.execute("CREATE INDEX t_tenant ON t(tenant)")
    db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2')" % dim)
    qb = q.tobytes()
    flt = "SELECT id FROM t WHERE tenant = 7"
    sql = {"rows": n, "filter": flt, "filter_rows": db.execute("SELECT count(*) FROM (%s)" % flt).fetchone()[0]}
    filtered = lambda: db.execute("SELECT id, distance FROM vector_full_scan_filtered('t','v',?,?,?)", (qb, k, flt)).fetchall()
    stream = lambda: db.execute("SELECT id, distance FROM vector_full_scan_stream('t','v',?) WHERE id IN (%s) ORDER BY distance, id LIMIT ?" % flt, (qb, k)).fetchall()
    assert filtered() == stream()
    sql["vector_full_scan_filtered"] = wall_ms(filtered)
    sql["filter_statement_alone"] = wall_ms(lambda: db.execute(flt).fetchall())
    sql["unfiltered_vector_full_scan"] = wall_ms(lambda: db.execute("SELECT id, distance FROM vector_full_scan('t','v',?,?)", (qb, k)).fetchall())
    sql["stream_where_id_in_order_limit"] = wall_ms(stream, steps=max(3, args.steps // 5))
    out["sql"] = sql
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
