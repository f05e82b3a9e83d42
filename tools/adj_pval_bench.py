#!/usr/bin/env python3
"""Device time of the p-value correction (seekr_amd.consumers.adjust_pvalues / skr_adjust_pvalues) on 50 000^2 float32
matrices, symmetric (1.25e9 tests, upper triangle) and not (2.5e9 tests), plus adj_pval(DataFrame) end to end at
8 000^2 next to the numpy restatement (tests/adj_rule.py) and hommel at its 2^22-test limit.

Device time: the ctx's HIP-event profile scopes (symmetry test, gather, sort, scan, write-back) after one warm-up call,
and the wall time of the call with the stream synchronised.  Algorithmic bytes: what each phase must move at least
(see DESIGN §4), over the time, against the 6.29 TB/s measured HBM peak.

    python tools/adj_pval_bench.py [--n 50000] [--out profiles/adj_pval_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from seekr_amd import _lib, consumers  # noqa: E402

HBM = 6.29e12
SCOPES = ["pvals_symmetric", "triu_flatten", "adjust_gather", "adjust_sort", "adjust_scan", "adjust_mapback",
          "adjust_elementwise"]


def hashed(rows, cols, symmetric):
    """float32 p-values in [0, 1) from a hash of (row, col) — of (min, max) when symmetric: 2^24 distinct values."""
    i = rows[:, None].astype(np.uint64)
    j = cols[None, :].astype(np.uint64)
    if symmetric:
        i, j = np.minimum(i, j), np.maximum(i, j)
    h = (i * np.uint64(0x9E3779B1) + j * np.uint64(0x85EBCA77) + np.uint64(0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))


def device_matrix(ctx, n, symmetric, stripe=2000):
    d = ctx.empty(n, n)
    cols = np.arange(n)
    for r0 in range(0, n, stripe):
        d.upload(hashed(np.arange(r0, min(n, r0 + stripe)), cols, symmetric), row0=r0)
    ctx.sync()
    return d


def timed(ctx, fn):
    ctx.prof_reset()
    ctx.sync()
    t0 = time.perf_counter()
    res = fn()
    ctx.sync()
    wall = time.perf_counter() - t0
    scopes = {}
    for s in SCOPES:
        ms, cnt = ctx.prof_query(s)
        if cnt:
            scopes[s] = round(ms, 3)
    return res, wall * 1e3, scopes


def algorithmic_bytes(n_rows, symmetric, method, sort_passes):
    cells = n_rows * n_rows
    n = n_rows * (n_rows - 1) // 2 if symmetric else cells
    b = {}
    if symmetric:
        b["symmetry"] = cells * 4
    if method == "bonferroni":
        b["elementwise"] = (n * 4) + cells * (8 if symmetric else 4)
        return n, b
    if symmetric:
        b["gather"] = 2 * n * 4
    b["key_bits"] = n * 4
    b["sort"] = sort_passes * 3 * n * 4
    b["scan"] = 2 * n * 4 + n * 8
    b["mapback"] = n * 4 + n * 8 + cells * 8
    return n, b


def run_big(ctx, n_rows, symmetric, methods, log):
    d = device_matrix(ctx, n_rows, symmetric)
    out = []
    if symmetric:
        (flag, ms, sc) = timed(ctx, lambda: consumers.pvals_symmetric(d))
        assert flag
        log({"case": "symmetry_test", "n": n_rows, "wall_ms": round(ms, 3), "scopes": sc})
    for m in methods:
        r = consumers.adjust_pvalues(d, m, 0.05, symmetric=symmetric)  # warm-up (workspace allocation)
        r.free()
        r, ms, sc = timed(ctx, lambda: consumers.adjust_pvalues(d, m, 0.05, symmetric=symmetric))
        r.free()
        n, b = algorithmic_bytes(n_rows, symmetric, m, 4)
        dev_ms = sum(sc.values())
        rec = {"case": "%s_%d" % ("symmetric" if symmetric else "full", n_rows), "method": m, "tests": n,
               "wall_ms": round(ms, 3), "device_ms": round(dev_ms, 3), "scopes": sc,
               "tests_per_s": round(n / (ms / 1e3), 1), "alg_bytes": sum(b.values()), "alg_bytes_parts": b,
               "alg_floor_ms": round(sum(b.values()) / HBM * 1e3, 3),
               "hbm_fraction_of_wall": round(sum(b.values()) / (ms / 1e3) / HBM, 4)}
        log(rec)
        out.append(rec)
    d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--frame", type=int, default=8000)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--skip-hommel", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    ctx.prof_enable(True)
    records = []

    def log(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    methods = ["bonferroni", "holm", "fdr_bh", "fdr_tsbky"]
    if not args.skip_big:
        run_big(ctx, args.n, True, methods, log)
        run_big(ctx, args.n, False, methods, log)
    # end to end: DataFrame in, DataFrame out, at frame^2, next to the numpy restatement in the same run
    import pandas as pd
    import adj_rule
    v = hashed(np.arange(args.frame), np.arange(args.frame), True)
    names = ["t%d" % i for i in range(args.frame)]
    df = pd.DataFrame(v, index=names, columns=names)
    from seekr_amd.adj_pval import adj_pval
    for m in ("fdr_bh", "holm"):
        with contextlib.redirect_stdout(io.StringIO()):
            adj_pval(df, m)
            t0 = time.perf_counter()
            res = adj_pval(df, m)
            t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, want = adj_rule.adj_frame(v, True, m)
        t_np = time.perf_counter() - t0
        same = bool(np.array_equal(res.to_numpy(), want, equal_nan=True))
        log({"case": "adj_pval_dataframe_%d" % args.frame, "method": m, "device_end_to_end_s": round(t_dev, 4),
             "numpy_restatement_s": round(t_np, 4), "equal": same})
    if not args.skip_hommel:
        h = hashed(np.arange(2048), np.arange(2048), False) ** 3
        d = ctx.from_numpy(h)
        r = consumers.adjust_pvalues(d, "hommel", symmetric=False)
        r.free()
        r, ms, sc = timed(ctx, lambda: consumers.adjust_pvalues(d, "hommel", symmetric=False))
        r.free()
        log({"case": "hommel_limit", "tests": int(h.size), "wall_ms": round(ms, 3), "scopes": sc})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
