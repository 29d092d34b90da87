#!/usr/bin/env python3
"""Paged scans against the scans they sit next to, in ONE process on ONE 10M x 384 f32 corpus (L2, k = 20):

  per page depth - the page behind 0, 1, 10, 100 and 1000 pages of 20 rows (cursors taken from a host sort of scan_distances):
    kernels, timed with the corpus' own profiling events (set_profiling / profile_mean_ms):
      (a) the plain top-20 kernel, in the same run          (b) the paged kernel (scan_topk_after)
      (c) the paged masked kernel under a 1/10 mask (scan_topk_after masked=True), against (d) the masked kernel without a cursor
    end to end, wall clock:
      (e) scan_topk_after                                   (f) the way without paged scans: scan_topk with k = (depth + 1) * 20 and a
                                                                cut on the host - the radix-select path beyond 64 results
  a batch - nq = 16 queries, a cursor each at mixed depths: scan_topk_batch_after against 16 single paged scans, wall clock;
  through SQL (--sql-rows, default 200 000 rows, a file-less database): a ten-page loop of vector_full_scan_after against the
  LIMIT 20 OFFSET m statement over the stream function it replaces.

(a) is the yardstick for (b), (d) for (c) - from the same run.  Warm-up, then repeated timed steps; min / median are printed.

    python tools/after_bench.py [--rows 10000000] [--dim 384] [--steps 30] [--warmup 5] [--sql-rows 200000]
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
    c.set_scan_filter(0)                      # (a) is the PLAIN top-k kernel, the one the paged kernel is an instantiation of
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

    d = c.scan_distances(pkg.L2, q)
    pos = np.nonzero(d < np.inf)[0]
    order = pos[np.lexsort((pos, d[pos]))]
    allowed = np.random.default_rng(44).random(N) < 0.1
    order_m = order[allowed[order]]

    def cursor(o, depth):
        if depth == 0:
            return None
        p = o[depth * k - 1]
        return (float(d[p]), int(p) + 1)

    out = {"rows": N, "dim": dim, "k": k, "kernel": c.kernel_name(pkg.L2), "steps": args.steps, "warmup": args.warmup, "depths": {}}
    c.set_mask(bits=allowed)
    for depth in (0, 1, 10, 100, 1000):
        if (depth + 1) * k > len(order_m):
            continue
        cur, cur_m = cursor(order, depth), cursor(order_m, depth)
        gi, gd = c.scan_topk_after(pkg.L2, q, k, after=cur)
        assert gi.tolist() == (order[depth * k:(depth + 1) * k] + 1).tolist(), depth
        gi, gd = c.scan_topk_after(pkg.L2, q, k, after=cur_m, masked=True)
        assert gi.tolist() == (order_m[depth * k:(depth + 1) * k] + 1).tolist(), depth
        r = {}
        r["a_plain_topk_kernel"] = kernel_ms(lambda: c.scan_topk(pkg.L2, q, k))
        r["b_paged_kernel"] = kernel_ms(lambda: c.scan_topk_after(pkg.L2, q, k, after=cur))
        r["b_over_a_median"] = round(r["b_paged_kernel"]["median_ms"] / r["a_plain_topk_kernel"]["median_ms"], 4)
        r["d_masked_kernel"] = kernel_ms(lambda: c.scan_topk_masked(pkg.L2, q, k))
        r["c_paged_masked_kernel"] = kernel_ms(lambda: c.scan_topk_after(pkg.L2, q, k, after=cur_m, masked=True))
        r["c_over_d_median"] = round(r["c_paged_masked_kernel"]["median_ms"] / r["d_masked_kernel"]["median_ms"], 4)
        r["e_scan_topk_after"] = wall_ms(lambda: c.scan_topk_after(pkg.L2, q, k, after=cur))
        r["f_topk_of_everything_in_front"] = wall_ms(lambda: c.scan_topk(pkg.L2, q, (depth + 1) * k)[0][depth * k:], steps=max(3, args.steps // 5))
        r["f_over_e"] = round(r["f_topk_of_everything_in_front"]["median_ms"] / r["e_scan_topk_after"]["median_ms"], 2)
        out["depths"]["page_%d" % depth] = r

    nq = 16
    qs = np.random.default_rng(45).standard_normal((nq, dim), dtype=np.float32)
    cursors = []
    for i in range(nq):
        after = None
        for _ in range(i % 4):
            gi, gd = c.scan_topk_after(pkg.L2, qs[i], k, after=after)
            after = (float(gd[-1]), int(gi[-1]))
        cursors.append(after)
    out["batch_16"] = {"plan": pkg.batch_masked_plan(c, pkg.L2),
                       "scan_topk_batch_after": wall_ms(lambda: c.scan_topk_batch_after(pkg.L2, qs, k, after=cursors)),
                       "sixteen_single_paged_scans": wall_ms(lambda: [c.scan_topk_after(pkg.L2, qs[i], k, after=cursors[i]) for i in range(nq)])}
    c.close()

    # ---- through SQL: a ten-page loop against the LIMIT / OFFSET statements it replaces
    import sqlite3
    b = g._load_build()
    ext = b.build_extension()[:-3]
    n = args.sql_rows
    rows = np.random.default_rng(46).standard_normal((n, dim), dtype=np.float32)
    db = sqlite3.connect(":memory:", isolation_level=None)
    db.enable_load_extension(True)
    db.load_extension(ext)
    db.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, tenant INTEGER, v BLOB)")
    db.execute("BEGIN")
    db.executemany("INSERT INTO t(id, tenant, v) VALUES (?, ?, ?)", ((i + 1, (i * 7919) % 100, rows[i].tobytes()) for i in range(n)))
    db.execute("COMMIT")
    db.execute("SELECT vector_init('t', 'v', 'type=FLOAT32,dimension=%d,distance=L2')" % dim)
    qb = q.tobytes()

    def paged():
        res, after = [], (None, None)
        for _ in range(10):
            page = db.execute("SELECT id, distance FROM vector_full_scan_after('t','v',?,?,?,?)", (qb, k) + after).fetchall()
            res += page
            after = (page[-1][1], page[-1][0])
        return res

    def offset():
        res = []
        for m in range(10):
            res += db.execute("SELECT id, distance FROM vector_full_scan_stream('t','v',?) WHERE distance < 9e999 ORDER BY distance, id LIMIT ? OFFSET ?",
                              (qb, k, m * k)).fetchall()
        return res

    assert paged() == offset()
    out["sql"] = {"rows": n, "ten_pages_vector_full_scan_after": wall_ms(paged),
                  "ten_pages_stream_order_limit_offset": wall_ms(offset, steps=max(3, args.steps // 5))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
