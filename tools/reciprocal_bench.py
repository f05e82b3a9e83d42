"""Column top-k, one sweep for both directions, and the k-NN graph beside the thresholded one.  One process, one GPU.

    python tools/reciprocal_bench.py [--arms abc] [--block-rows 8192] [--block-cols 50000] [--set-rows 50000 20000]
                                     [--leiden-rows 100000] [--dense-rows 20000] [--runs 9] [--out profiles/reciprocal_bench.json]

  a  one [--block-rows, --block-cols] block of real r (synthetic transcripts, k = 6), at k = 10 and k = kmax of the column
     kernel: skr_topk_merge_cols beside skr_topk_merge_rows on the same block, both beside skr_select_cells_ge without
     outputs at a cutoff nothing passes (the plain read, twice: it counts, finds nothing and stops) and beside the
     contraction that made the block.
  b  --set-rows rows of 4 096 columns, k = 10: consumers.pearson_topk_both beside pearson_topk(a, b) + pearson_topk(b, a);
     the device memory each needs beyond the operands (from the shapes of its buffers).
  c  --leiden-rows rows, k = 15: reciprocal.knn_graph (union and mutual): seconds and edges, and leiden.communities on it;
     beside the thresholded graph of tools/leiden_bench.py's dense case (--dense-rows rows at cutoff 0), made in this run.
Every time is the median of --runs runs with the fastest and the slowest, the arms alternating within a run."""
import argparse
import json
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from seekr_amd import _lib, consumers, leiden, reciprocal  # noqa: E402
from seekr_amd import pearson as pearson_mod  # noqa: E402
from seekr_amd.synthetic import synthetic_ascii  # noqa: E402


def operand(ctx, n, seed=1, length=2000, k=6):
    """tools/leiden_bench.py's operand: n synthetic transcripts, k-mer counts, Log2.post, prepared for the contraction."""
    blob, offsets = synthetic_ascii(seed, n, length)
    x = _lib.count_per_kb(ctx, _lib.PackedSeqs.from_buffer(ctx, blob, offsets), k)
    _lib.normalize(ctx, x, "Log2.post", 1, None, 1, None)
    z, _ = _lib.operand_fill(ctx, x, None, pearson_mod._precision_for(np.dtype(np.float32), True))
    x.free()
    return z


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def alternating(ctx, arms, runs):
    """{name: summary} of the callables in `arms`, one after another within each of `runs` rounds (after one warm-up)."""
    times = {name: [] for name in arms}
    for run in range(runs + 1):
        for name, fn in arms.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            if run:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(ms) for name, ms in times.items()}


def arm_block(ctx, rows, cols, runs):
    kmax = _lib.topk_merge_cols_limits()[0]
    za, zb = operand(ctx, rows), operand(ctx, cols, seed=2)
    r = ctx.empty(rows, cols)
    _lib.pearson_gemm_op(ctx, za, zb, r)
    out = {"rows": rows, "cols": cols, "bytes": rows * cols * 4, "kmax_cols": kmax, "k": {}}
    for k in (10, kmax):
        ridx, rval = ctx.empty(rows, k, np.uint32), ctx.empty(rows, k, np.float32)
        cidx, cval = ctx.empty(cols, k, np.uint32), ctx.empty(cols, k, np.float32)
        arms = {
            "contraction": lambda: _lib.pearson_gemm_op(ctx, za, zb, r),
            "select_cells_count_only": lambda: consumers.select_cells(r, 3.0, None),
            "merge_rows": lambda: _lib.topk_merge_rows(ctx, r, ridx, rval, k, first=True, exclude_diag=False),
            "merge_cols": lambda: _lib.topk_merge_cols(ctx, r, cidx, cval, k, first=True, exclude_diag=False),
        }
        res = alternating(ctx, arms, runs)
        res["merge_cols_gb_s"] = round(out["bytes"] / res["merge_cols"]["median_ms"] / 1e6, 1)
        res["merge_rows_gb_s"] = round(out["bytes"] / res["merge_rows"]["median_ms"] / 1e6, 1)
        res["merge_cols_over_merge_rows"] = round(res["merge_cols"]["median_ms"] / res["merge_rows"]["median_ms"], 3)
        res["merge_cols_over_contraction"] = round(res["merge_cols"]["median_ms"] / res["contraction"]["median_ms"], 3)
        out["k"][str(k)] = res
        for m in (ridx, rval, cidx, cval):
            m.free()
        print(json.dumps({"block_k": k, **res}), flush=True)
    for m in (r, za, zb):
        m.free()
    return out


def arm_two_sets(ctx, n1, n2, runs, k=10, stripe_rows=8192):
    za, zb = operand(ctx, n1), operand(ctx, n2, seed=2)
    got = {}

    def one_sweep():
        got["both"] = consumers.pearson_topk_both(za, zb, k=k, stripe_rows=stripe_rows)

    def two_sweeps():
        got["two"] = consumers.pearson_topk(za, zb, k=k, stripe_rows=stripe_rows) + consumers.pearson_topk(zb, za, k=k, stripe_rows=stripe_rows)

    res = alternating(ctx, {"one_sweep": one_sweep, "two_sweeps": two_sweeps}, runs)
    both, two = got["both"], got["two"]
    lists = lambda n: n * k * 8  # noqa: E731
    res.update({
        "rows": [n1, n2], "k": k, "stripe_rows": stripe_rows,
        "one_sweep_over_two_sweeps": round(res["one_sweep"]["median_ms"] / res["two_sweeps"]["median_ms"], 3),
        # beyond the operands: the block buffer, a stripe's row lists and (one sweep) the resident column lists
        "one_sweep_device_bytes": min(stripe_rows, n1) * n2 * 4 + lists(min(stripe_rows, n1)) + lists(n2),
        "two_sweeps_device_bytes": max(min(stripe_rows, n1) * n2, min(stripe_rows, n2) * n1) * 4 + lists(min(stripe_rows, max(n1, n2))),
        "row_lists_same_bytes": bool(np.array_equal(both[0], two[0]) and np.array_equal(both[1].view(np.uint32), two[1].view(np.uint32))),
        "col_lists_same_indices_as_second_sweep": bool(np.array_equal(both[2], two[2])),
        "col_values_with_other_bits_than_second_sweep": int((both[3].view(np.uint32) != two[3].view(np.uint32)).sum()),
    })
    za.free()
    zb.free()
    print(json.dumps({"two_sets": res}), flush=True)
    return res


def timed_leiden(rows, cols, vals, n):
    t0 = time.perf_counter()
    _, q, info = leiden.communities(rows, cols, vals, n)
    return {"communities_s": round(time.perf_counter() - t0, 4), "quality": q, **info}


def arm_leiden(ctx, n, dense_n, runs, k=15):
    z = operand(ctx, n)
    leiden.communities(np.array([0], np.uint32), np.array([1], np.uint32), np.array([1.0], np.float32), 2)  # loads the kernels
    out = {"rows": n, "k": k}
    graphs = {}
    arms = {mode: (lambda mode=mode: graphs.__setitem__(mode, reciprocal.knn_graph(z, k, mode=mode))) for mode in ("union", "mutual")}
    times = alternating(ctx, arms, max(1, runs // 3))
    for mode in ("union", "mutual"):
        rows, cols, vals = graphs[mode]
        deg = np.bincount(np.concatenate([rows, cols]), minlength=n)
        out[mode] = {"knn_graph": times[mode], "edges": int(len(vals)), "largest_degree": int(deg.max()), "nodes_without_edge": int((deg == 0).sum()),
                     **timed_leiden(rows, cols, vals, n)}
        print(json.dumps({mode: out[mode]}), flush=True)
    z.free()
    if dense_n:
        z = operand(ctx, dense_n)
        t0 = time.perf_counter()
        rows, cols, vals = consumers.pearson_edges(z, 0.0, upper_only=True)
        edges_s = time.perf_counter() - t0
        keep = vals > 0
        rows, cols, vals = rows[keep].astype(np.uint32), cols[keep].astype(np.uint32), vals[keep].astype(np.float32)
        out["thresholded_cutoff_0"] = {"rows": dense_n, "pearson_edges_s": round(edges_s, 4), "edges": int(len(vals)), **timed_leiden(rows, cols, vals, dense_n)}
        del rows, cols, vals
        t0 = time.perf_counter()
        rows, cols, vals = reciprocal.knn_graph(z, k, mode="union")
        out["knn_union_same_rows"] = {"rows": dense_n, "knn_graph_s": round(time.perf_counter() - t0, 4), "edges": int(len(vals)),
                                      **timed_leiden(rows, cols, vals, dense_n)}
        z.free()
        print(json.dumps({key: out[key] for key in ("thresholded_cutoff_0", "knn_union_same_rows")}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--block-rows", type=int, default=8192)
    ap.add_argument("--block-cols", type=int, default=50000)
    ap.add_argument("--set-rows", type=int, nargs=2, default=[50000, 20000])
    ap.add_argument("--leiden-rows", type=int, default=100000)
    ap.add_argument("--dense-rows", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.default_context()
    res = {"box": socket.gethostname(), "runs": args.runs, "cols_limits": _lib.topk_merge_cols_limits()}
    if "a" in args.arms:
        res["block"] = arm_block(ctx, args.block_rows, args.block_cols, args.runs)
    if "b" in args.arms:
        res["two_sets"] = arm_two_sets(ctx, args.set_rows[0], args.set_rows[1], args.runs)
    if "c" in args.arms:
        res["leiden"] = arm_leiden(ctx, args.leiden_rows, args.dense_rows, args.runs)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
