"""The distribution of r without r, measured: the histogram kernels on one stripe of real r values, the sweeps that stand
on them at the benchmark's size, and the route through the whole matrix where it still fits.  One process, one GPU.

    python tools/distribution_bench.py [--rows 50000] [--small-rows 20000] [--runs 9] [--out profiles/distribution_bench.json]

1  kernels  One [8 192, rows] stripe of r (k = 6 profiles of synthetic sequences, as tools/neighbors_bench.py makes them)
   stays in its buffer; each arm is one call on it, device time from the library's event timers (HIP events around the
   launch), median / fastest / slowest of --runs after a warm-up, the arms alternating:
     select_count      skr_select_cells_ge with all outputs NULL: one read of the block over the same tiling (the yardstick)
     key_pass1         skr_hist_key_digits, 12 bits, every cell (the descent's first pass), plain LDS atomics
     key_pass1_match   the same with SEEKR_DIST_MATCH=1 (two ballot rounds before the atomics)
     key_pass2         10 bits under the 8 most populated 12-bit prefixes (a pass further down)
     edges_200         skr_hist_edges, 200 equal bins over [-1, 1]
     edges_200_match   the same with SEEKR_DIST_MATCH=1
     edges_4096        4 096 equal bins (the deepest bisection)
   with bytes/s of the block over the time and that rate over the device-to-device copy rate measured here.
2  sweeps   rows x 4 096 operands, stripes of 8 192 rows: wall time (host clock around work that ends in a device
   synchronise) of r_order_statistics for 1 and 8 ranks and of r_histogram with 200 bins against `plain`, one sweep of the
   same contractions into the same buffer with nothing done to the blocks.
3  route    at --small-rows, where r fits: the whole r, triu_values, download, np.partition for one quantile — against
   r_quantiles; seconds and peak device memory above what the operand itself takes (the device's own figure, taken while
   the buffers are held, beside the bytes the shapes give).
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib, consumers, distribution  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402

STRIPE = 8192


def copy_bandwidth_gbs(ctx):
    """Bytes moved per second by a device-to-device copy of 1 GiB (read + write), median of 7 after a warm-up."""
    rows, cols = 65536, 4096
    src, dst = ctx.zeros(rows, cols), ctx.zeros(rows, cols)
    ctx.sync()
    ts = []
    for _ in range(8):
        t0 = time.perf_counter()
        _lib.peer_copy_rows(dst, 0, src, 0, rows)  # on the communication stream
        done = _lib.Event(ctx, comm=True)
        done.wait_on(ctx)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
        done.free()
    src.free()
    dst.free()
    return 2.0 * rows * cols * 4 / statistics.median(ts[1:]) / 1e9


def operand(ctx, n, length=2000, k=6):
    blob, offsets = synthetic_ascii(1, n, length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), k)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()
    return z


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def set_match(ctx, on):
    os.environ["SEEKR_DIST_MATCH"] = "1" if on else "0"
    ctx.reload_knobs()


def kernels(ctx, z, runs, copy_gbs):
    rows = min(STRIPE, z.rows)
    buf = ctx.empty(rows, z.rows)
    _lib.pearson_gemm_op(ctx, z.view(0, rows), z, buf)
    ctx.sync()
    block_bytes = rows * z.rows * 4
    top, nan = np.zeros((1, 4096), np.uint64), np.zeros(1, np.uint64)
    distribution.hist_key_block(buf, 20, 12, [0], 0, top, nan)
    prefixes = sorted(np.argsort(top[0])[::-1][:8].tolist())
    e200, e4096 = distribution.make_edges(None, 200, (-1, 1)), distribution.make_edges(None, 4096, (-1, 1))

    def key(shift, bits, pref, pbits):
        hist, n = np.zeros((len(pref), 1 << bits), np.uint64), np.zeros(1, np.uint64)
        return lambda: distribution.hist_key_block(buf, shift, bits, pref, pbits, hist, n)

    def edges(table):
        hist, extra = np.zeros(len(table) - 1, np.uint64), np.zeros(3, np.uint64)
        return lambda: distribution.hist_edges_block(buf, table, hist, extra)

    arms = {  # name: (scope of the event timer, match knob, call)
        "select_count": ("cells_count", False, lambda: consumers.select_cells(buf, 0.0, None)),
        "key_pass1": ("hist_key_digits", False, key(20, 12, [0], 0)),
        "key_pass1_match": ("hist_key_digits", True, key(20, 12, [0], 0)),
        "key_pass2": ("hist_key_digits", False, key(10, 10, prefixes, 12)),
        "edges_200": ("hist_edges", False, edges(e200)),
        "edges_200_match": ("hist_edges", True, edges(e200)),
        "edges_4096": ("hist_edges", False, edges(e4096)),
    }
    ms = {name: [] for name in arms}
    ctx.prof_enable(True)
    for rep in range(runs + 1):  # the arms alternate; the first round warms up
        for name, (scope, match, call) in arms.items():
            set_match(ctx, match)
            ctx.prof_reset()
            call()
            ctx.sync()
            if rep:
                ms[name].append(ctx.prof_query(scope)[0])
    ctx.prof_enable(False)
    set_match(ctx, False)
    out = {"block": [rows, z.rows], "block_bytes": block_bytes, "nonzero_bins_pass1": int((top[0] > 0).sum()),
           "bins_holding_99_percent_pass1": int(np.searchsorted(np.cumsum(np.sort(top[0])[::-1]), 0.99 * top[0].sum()) + 1),
           "prefixes_pass2": prefixes, "arms": {}}
    base = statistics.median(ms["select_count"])
    for name in arms:
        row = summary(ms[name])
        row["gbs"] = round(block_bytes / row["median_ms"] / 1e6, 1)
        row["gbs_over_copy_gbs"] = round(row["gbs"] / copy_gbs, 3)
        row["over_select_count"] = round(row["median_ms"] / base, 3)
        out["arms"][name] = row
        print(json.dumps({name: row}), flush=True)
    buf.free()
    return out


def sweeps(ctx, z, runs):
    n = z.rows
    m = distribution.n_cells(z)
    ranks1, ranks8 = [m // 2], [int(m * q) for q in (0.001, 0.01, 0.1, 0.25, 0.5, 0.75, 0.99, 0.999)]
    edges = distribution.make_edges(None, 200, (-1, 1))
    sweep = consumers.Sweep(z, None, STRIPE)
    arms = {
        "plain": lambda: sweep.run(lambda buf, **where: None),
        "order_statistics_1": lambda: distribution.r_order_statistics(z, ranks=ranks1, stripe_rows=STRIPE),
        "order_statistics_8": lambda: distribution.r_order_statistics(z, ranks=ranks8, stripe_rows=STRIPE),
        "histogram_200": lambda: distribution.r_histogram(z, edges=edges, stripe_rows=STRIPE),
    }
    ms = {name: [] for name in arms}
    for rep in range(runs + 1):
        for name, call in arms.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    sweep.free()
    out = {"rows": n, "cols": z.cols, "cells": m, "stripe_rows": STRIPE, "arms": {}}
    base = statistics.median(ms["plain"])
    for name in arms:
        row = summary(ms[name])
        row["over_plain"] = round(row["median_ms"] / base, 3)
        out["arms"][name] = row
        print(json.dumps({name: row}), flush=True)
    # what one pass adds to the contraction that feeds it
    out["pass_over_contraction"] = round((out["arms"]["histogram_200"]["median_ms"] - base) / base, 3)
    out["key_pass_over_contraction"] = round((out["arms"]["order_statistics_1"]["median_ms"] / 3 - base) / base, 3)
    return out


def route(ctx, z, runs):
    n = z.rows
    q = 0.999

    def used():
        free, total = ctx.mem_info()
        return total - free

    def whole_matrix(peak):
        r = ctx.empty(n, n)
        _lib.pearson_gemm_op(ctx, z, z, r, symmetric=True)
        v = consumers.triu_values(r, 1)
        ctx.sync()
        peak.append(used())
        host = np.array(v.to_numpy()).reshape(-1)
        r.free()
        v.free()
        host = host[~np.isnan(host)]
        rank = distribution.quantile_rank(q, len(host))
        return np.partition(host, rank)[rank]

    def no_matrix(peak):
        sweep = consumers.Sweep(z, None, STRIPE)
        try:
            values, _, _ = distribution._order_statistics(sweep, lambda m: [distribution.quantile_rank(q, m)])
            ctx.sync()
            peak.append(used())
        finally:
            sweep.free()
        return values[0]

    ctx.sync()
    floor = used()
    out = {"rows": n, "q": q}
    got = {}
    out["bytes_by_shapes"] = {"whole_matrix": n * n * 4 + n * (n - 1) // 2 * 4, "no_matrix": min(STRIPE, n) * n * 4}
    for name, call in (("no_matrix", no_matrix), ("whole_matrix", whole_matrix)):
        ts, peak = [], []
        for rep in range(runs + 1):
            ctx.sync()
            t0 = time.perf_counter()
            got[name] = call(peak)
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        row = summary(ts)
        row["peak_device_bytes_above_operand"] = int(max(peak) - floor)
        out[name] = row
        print(json.dumps({name: row}), flush=True)
    out["same_value"] = bool(np.float32(got["whole_matrix"]).view(np.uint32) == np.float32(got["no_matrix"]).view(np.uint32))
    out["value"] = float(got["no_matrix"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--small-rows", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "runs": args.runs, "copy_gbs": round(copy_bandwidth_gbs(ctx), 1)}
    z = operand(ctx, args.rows)
    res["kernels"] = kernels(ctx, z, args.runs, res["copy_gbs"])
    res["sweeps"] = sweeps(ctx, z, args.runs)
    z.free()
    z = operand(ctx, args.small_rows)
    res["route"] = route(ctx, z, max(2, args.runs // 3))
    z.free()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
